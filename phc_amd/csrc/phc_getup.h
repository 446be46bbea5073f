// phc_getup.h -- per-env pieces of the device form of HumanoidImGetup._reset_envs (phc_getup_assign, csrc/phc_getup.hip; contract: include/phc_amd.h) and the
// per-step uniforms of cycle_motion / far starts (phc_task_draws).  The rules are those of phc_amd/env/tasks/humanoid_im_getup.py:79-110 (reference:
// humanoid_im_getup.py:131-196); the numbers are this file's own: counter-based hashes (phc_rng.h) instead of torch.bernoulli / torch.randperm.
// PHC_HD: tests/getup_shim.cpp and tests/getup_asan_main.cpp build everything here for the CPU, getup_assign_host included -- the whole launch as plain loops,
// which the kernel must equal bit for bit.
//
// One launch, for every env i with reset_buf[i] != 0:
//   release   avail[assign[i]] = 0.  An env that never held a fall state has assign[i] == 0 and releases slot 0, and an env whose last episode was not a FALL
//             one releases the slot it held before that -- whoever holds it now.  Both are the reference's behaviour (fall_id_assignments starts as zeros and
//             is never cleared) and the torch path's, and are kept.  An assign[i] outside [0, N) releases nothing.
//   draw      u = getup_draws(key, env_offset + i, k[i]); k[i] += 1.
//   decide    RECOVERY (2) when u[0] < p_recovery and terminate_buf[i] == 1, else FALL (3) when u[1] < p_fall, else NORMAL (1): torch.bernoulli(p) == 1,
//             p = 0 never, p = 1 always (u < 1).
//   slots     the FALL envs are ranked in env order, r = 0 .. n_f - 1; the slots free after ALL releases are listed in slot order, free[0 .. F - 1]; FALL env r
//             takes pick = free[getup_perm(pkey, F, r)], where pkey = getup_perm_key(key, *launch_count, F): a bijection of [0, F) that depends on the key,
//             the launch's count and F alone.  The permutation is a four-round balanced Feistel network over 2 h bits, h the smallest with 4^h >= F, walked
//             in cycles until the value falls below F (fewer than four walks on average); its round function is splitmix64 of (pkey, round, half).
//             n_f <= F holds whenever every held slot has one holder; should the arrays say otherwise (a restored state), the FALL envs of rank >= F become
//             NORMAL ones: nothing is read or written out of range, and the result still is a function of the inputs alone.
//   teleport  root_states[i] = fall_root[pick], dof_pos[i] = fall_dof_pos[pick], dof_vel[i] = 0; avail[pick] = 1, assign[i] = pick.
//   counters  recovery_counter[i] = recovery_steps for FALL and RECOVERY envs.
//   publish   kind[i] (0 for an env that is not done); normal_flag[i] = kind[i] == 1 (what phc_im_reset_done reads in place of reset_buf); fall_list[r] = the
//             FALL env of rank r, every other entry N (what phc_refresh_body_state_masked reads).
#pragma once
#include "phc_rng.h"
#include "../../include/phc_amd.h"

namespace phc {

constexpr int GETUP_BLOCK = 1024;                 // threads of the launch's one workgroup == envs per scan tile
constexpr int GETUP_MAX_ENVS = 1 << 20;           // PHC_EUNSUPPORTED above (1024 tiles)
constexpr int GETUP_NOT_DONE = 0, GETUP_NORMAL = 1, GETUP_RECOVERY = 2, GETUP_FALL = 3;

// The two uniforms of draw `k` of env `global_env`: recovery, fall.  Keyed like push_draws (phc_push.h): the draw's counter 2 k + j is folded into the stream key.
PHC_HD void getup_draws(uint64_t key, uint32_t global_env, uint32_t k, float u[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
        u[j] = hash_u01(splitmix64(key ^ (((uint64_t)k * 2u + (uint64_t)j) * 0x9E6C63D0876A9A47ull)), global_env);
}

// The three uniforms of draw `k` of env `global_env` for phc_task_draws: cycle_phase, offset_rand[0], offset_rand[1].
PHC_HD void task_draws(uint64_t key, uint32_t global_env, uint32_t k, float u[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
        u[j] = hash_u01(splitmix64(key ^ (((uint64_t)k * 3u + (uint64_t)j) * 0x9E6C63D0876A9A47ull)), global_env);
}

// One env of phc_task_draws: the kernel's lane, and the host build's loop body.
PHC_HD void task_draws_env(uint64_t key, int64_t env_offset, int32_t* k, float* cycle_phase, float* offset_rand, int64_t env) {
    const uint32_t kk = (uint32_t)k[env];
    float u[3];
    task_draws(key, (uint32_t)(env_offset + env), kk, u);
    if (cycle_phase) cycle_phase[env] = u[0];
    if (offset_rand) { offset_rand[env * 2] = u[1]; offset_rand[env * 2 + 1] = u[2]; }
    k[env] = (int32_t)(kk + 1u);
}

// torch.bernoulli(p_recovery) == 1 & terminated, else torch.bernoulli(p_fall) == 1, else normal
PHC_HD int getup_decide(const float u[2], float p_recovery, float p_fall, int64_t terminate) {
    if (u[0] < p_recovery && terminate == 1) return GETUP_RECOVERY;
    return u[1] < p_fall ? GETUP_FALL : GETUP_NORMAL;
}

// The permutation key of one launch: (stream key, launch count, F).
PHC_HD uint64_t getup_perm_key(uint64_t key, uint64_t count, uint32_t F) {
    return splitmix64(splitmix64(key ^ (count * 0xD1342543DE82EF95ull)) ^ ((uint64_t)F * 0x9E6C63D0876A9A47ull));
}
// pi(r) for r in [0, F): cycle-walking Feistel (see the head of the file).
PHC_HD uint32_t getup_perm(uint64_t pkey, uint32_t F, uint32_t r) {
    if (F <= 1u) return 0u;
    int h = 1;
    while ((1u << (2 * h)) < F) ++h;
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = r;
    do {
        uint32_t l = x >> h, rr = x & mask;
        for (uint32_t round = 0; round < 4u; ++round) {
            const uint32_t f = (uint32_t)(splitmix64(pkey ^ (((uint64_t)(round + 1u) << 32) | (uint64_t)rr)) >> 32) & mask;
            const uint32_t t = l ^ f;
            l = rr; rr = t;
        }
        x = (l << h) | rr;
    } while (x >= F);
    return x;
}

// Phase 1 of the launch for one env: release, draw (or take `u_given`), decide, the RECOVERY counter, kind / normal_flag / the fall list's filler.
PHC_HD int getup_env_decide(const phc_getup_args_t& a, int64_t i, float p_recovery, float p_fall, const float* u_given) {
    int kind = GETUP_NOT_DONE;
    if (a.reset_buf[i] != 0) {
        const int64_t held = a.assign[i];
        if ((uint64_t)held < (uint64_t)a.num_envs) a.avail[held] = 0;
        float u[2];
        if (u_given) { u[0] = u_given[0]; u[1] = u_given[1]; }
        else {
            const uint32_t k = (uint32_t)a.k[i];
            getup_draws(a.key, (uint32_t)(a.env_offset + i), k, u);
            a.k[i] = (int32_t)(k + 1u);
        }
        kind = getup_decide(u, p_recovery, p_fall, a.terminate_buf[i]);
        if (kind == GETUP_RECOVERY) a.recovery_counter[i] = a.recovery_steps;
    }
    a.kind[i] = kind;
    a.normal_flag[i] = kind == GETUP_NORMAL;
    a.fall_list[i] = a.num_envs;
    return kind;
}

// Phase 3 for the FALL env of rank r (fall_list[r] and free_list[0 .. F) are complete): its slot and counter, or the demotion of a rank the pool cannot serve.
// `p` = pi(r).
PHC_HD void getup_env_pick(const phc_getup_args_t& a, int64_t r, int64_t F, int64_t p) {
    const int64_t i = a.fall_list[r];
    if (r < F && (uint64_t)p < (uint64_t)F) {
        const int64_t pick = a.free_list[p];
        a.assign[i] = pick;
        a.avail[pick] = 1;
        a.recovery_counter[i] = a.recovery_steps;
    } else {
        a.kind[i] = GETUP_NORMAL;
        a.normal_flag[i] = 1;
        a.fall_list[r] = a.num_envs;
    }
}

// Phase 4: element c of the teleported row of the FALL env of rank r (13 root floats, then num_dof joint positions; the velocities are zeroed).
PHC_HD void getup_env_teleport(const phc_getup_args_t& a, int64_t r, int c) {
    const int64_t i = a.fall_list[r];
    if (i >= a.num_envs) return;   // (demoted)
    const int64_t pick = a.assign[i];
    if (c < 13) a.root_states[i * 13 + c] = a.fall_root[pick * 13 + c];
    else {
        const int d = c - 13;
        float* s = a.dof_state + (i * a.num_dof + d) * 2;
        s[0] = a.fall_dof_pos[pick * a.num_dof + d];
        s[1] = 0.f;
    }
}

// The whole launch on the host, in the order the kernel's phases keep.  u_given [N, 2] / perm_given [F]: the tests' explicit uniforms and permutation
// (nullable: drawn / computed as the kernel does; with u_given the per-env counters stay, with either the launch count still moves on).
inline void getup_assign_host(const phc_getup_args_t& a, const float* u_given, const int32_t* perm_given) {
    const int64_t N = a.num_envs;
    const uint64_t count = (uint64_t)*a.launch_count;
    const float p_recovery = a.prob[0], p_fall = a.prob[1];
    for (int64_t i = 0; i < N; ++i) getup_env_decide(a, i, p_recovery, p_fall, u_given ? u_given + 2 * i : nullptr);
    int64_t F = 0, n_f = 0;
    for (int64_t i = 0; i < N; ++i) {
        if (a.avail[i] == 0) a.free_list[F++] = (int32_t)i;
        if (a.kind[i] == GETUP_FALL) a.fall_list[n_f++] = i;
    }
    const uint64_t pkey = getup_perm_key(a.key, count, (uint32_t)F);
    for (int64_t r = 0; r < n_f; ++r) getup_env_pick(a, r, F, r < F ? (perm_given ? (int64_t)perm_given[r] : (int64_t)getup_perm(pkey, (uint32_t)F, (uint32_t)r)) : -1);
    for (int64_t r = 0; r < n_f; ++r)
        for (int c = 0; c < 13 + a.num_dof; ++c) getup_env_teleport(a, r, c);
    *a.launch_count = (int64_t)(count + 1u);
}

// The argument checks of phc_getup_assign (host side; include/phc_amd.h lists them): 0, PHC_EINVAL or PHC_EUNSUPPORTED.  A function of its own so that the tests
// can ask it about arguments they must never hand to a launch.
inline int32_t getup_args_check(const phc_getup_args_t* a) {
    if (!a || !a->prob || !a->reset_buf || !a->terminate_buf || !a->fall_root || !a->fall_dof_pos || !a->root_states || !a->dof_state || !a->avail || !a->assign
        || !a->recovery_counter || !a->k || !a->launch_count || !a->kind || !a->normal_flag || !a->fall_list || !a->free_list) return PHC_EINVAL;
    if (a->num_envs < 0 || a->num_dof < 1 || a->recovery_steps < 0) return PHC_EINVAL;
    if (a->env_offset < 0 || a->env_offset + (int64_t)a->num_envs > (int64_t)1 << 32) return PHC_EINVAL;
    return a->num_envs > GETUP_MAX_ENVS ? PHC_EUNSUPPORTED : 0;
}
inline int32_t task_draws_check(int32_t num_envs, int64_t env_offset, const int32_t* k) {
    if (num_envs < 0 || !k) return PHC_EINVAL;
    return env_offset < 0 || env_offset + (int64_t)num_envs > (int64_t)1 << 32 ? PHC_EINVAL : 0;
}

}  // namespace phc
