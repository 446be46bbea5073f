// phc_obs_aug.h -- per-lane code of phc_obs_augment (env.fut_tracks_dropout + env.add_obs_noise) and phc_occl_advance (env.occl_training) under
// `+env.task_rng=device` (csrc/phc_obs_aug.hip; contract: include/phc_amd.h).  The rules are those of HumanoidIm._fut_dropout / _add_obs_noise /
// _update_occl_training (phc_amd/env/tasks/humanoid_im.py; reference: humanoid_im.py:824-830, :710-711, :1081-1092); the numbers are this file's own:
// counter-based hashes (phc_rng.h) instead of torch.rand / torch.randn / torch.bernoulli / torch.randint.
// PHC_HD: tests/obs_aug_shim.cpp and tests/obs_aug_asan_main.cpp build everything here for the CPU, obs_augment_host and occl_advance_host included -- the
// whole launches as plain loops.  Integers (counters, dropout decisions, count, mask) and every stored 0.0f are bit-equal between the two builds; a noised
// element differs by the device's logf / sinf / cosf / sqrtf alone (no contraction, no fast-math on either side).
//
// Draws.  A draw is a function of (key, env_offset + env, k[env], index, which) alone:
//   u = hash_u01(splitmix64(key ^ (counter * 0x9E6C63D0876A9A47)), env_offset + env),  counter = ((k << 16 | index) << 1) | which,
//   index < 2^16, which in {0, 1}: no two (k, index, which) share a counter (k < 2^32: counter < 2^49).
// Index space of one phc_obs_augment call on a row: column pairs j = 0 .. P - 1, P = (num_obs + 1) / 2, then the dropout samples P + t, t = 0 .. T - 1.
//   Limits: num_obs <= 65536 (P <= 32768) and T <= 1024, so P + T < 2^16; PHC_EUNSUPPORTED above.
// Index space of phc_occl_advance: the bodies j = 0 .. J - 1, J <= 64.
//
// Normal pair of column pair j.  a = u(j, 0), b = u(j, 1), multiples of 2^-24.  u1 = 1 - a (exact, in (0, 1]); r = sqrtf(-2 logf(u1)) (<= 5.77 at
//   u1 = 2^-24); theta = 2 pi b; z0 = r cosf(theta) -> column 2 j, z1 = r sinf(theta) -> column 2 j + 1 where it exists.
//
// Row rule of phc_obs_augment, for a selected row, in the reference's order (dropout, then noise):
//   1. T > 1 and dropout_p > 0: for each t with u(P + t, 0) < dropout_p, 0.0f into columns so + t W .. so + (t + 1) W - 1, W = (num_obs - so) / T;
//   2. noise_std > 0: every column c becomes obs[c] + noise_std * z[c] (the zeroed ones included);
//   3. k[env] += 1.
//   An unselected row is untouched and its counter stays.  Selection: all rows (row_flag and env_ids null), row_flag [N] (non-zero = selected) or
//   env_ids [n] (distinct ids in [0, N); an id outside selects nothing).
//
// One env i of phc_occl_advance, for j = 0 .. J - 1 (u = u(j, 0), v = u(j, 1)):
//   start = (j != 0) && u < prob;  span = min(span_lo + floor(v * (span_hi - span_lo)), span_hi - 1);
//   count[i, j] = max((start ? span : count[i, j]) - 1, 0);
//   mask[i, j] = !(9 <= j && j < 24) -- humanoid_im.py:1091-1092 overwrites the mask it has just derived from the counts, and so does
//   _update_occl_training here: the schedule therefore never reaches the mask, as in the reference;
//   then k[i] += 1, for every env.
#pragma once
#include "phc_rng.h"
#include "../../include/phc_amd.h"

namespace phc {

constexpr int OBS_AUG_BLOCK = 256;                // threads of a row's workgroup == column pairs per pass
constexpr int OBS_AUG_MAX_OBS = 65536;            // PHC_EUNSUPPORTED above
constexpr int OBS_AUG_MAX_SAMPLES = 1024;         // PHC_EUNSUPPORTED above (the row's dropout decisions live in LDS)
constexpr int OCCL_MAX_BODIES = 64;               // PHC_EUNSUPPORTED above

PHC_HD float aug_u01(uint64_t key, uint32_t global_env, uint32_t k, uint32_t index, uint32_t which) {
    const uint64_t counter = ((((uint64_t)k << 16) | (uint64_t)index) << 1) | (uint64_t)which;
    return hash_u01(splitmix64(key ^ (counter * 0x9E6C63D0876A9A47ull)), global_env);
}

// Box-Muller on two uniforms that are multiples of 2^-24 in [0, 1)
PHC_HD void aug_box_muller(float a, float b, float* z0, float* z1) {
    const float u1 = 1.0f - a;
    const float r = sqrtf(-2.0f * logf(u1));
    const float theta = 6.28318530717958647692f * b;
    *z0 = r * cosf(theta);
    *z1 = r * sinf(theta);
}

PHC_HD void aug_normal_pair(uint64_t key, uint32_t global_env, uint32_t k, uint32_t j, float* z0, float* z1) {
    aug_box_muller(aug_u01(key, global_env, k, j, 0u), aug_u01(key, global_env, k, j, 1u), z0, z1);
}

// W of the row rule's step 1, or 0 where that step stores nothing (T <= 1, dropout_p == 0, an empty tail)
PHC_HD int obs_aug_width(const phc_obs_aug_args_t& a) {
    return a.num_samples > 1 && a.dropout_p > 0.f ? (a.num_obs - a.self_obs_size) / a.num_samples : 0;
}

// Is reference sample t of this row dropped?
PHC_HD bool obs_aug_dropped(const phc_obs_aug_args_t& a, uint32_t global_env, uint32_t k, int t) {
    const uint32_t P = (uint32_t)(a.num_obs + 1) / 2u;
    return aug_u01(a.key, global_env, k, P + (uint32_t)t, 0u) < a.dropout_p;
}

// The new value of column c: `v` what the row holds, `drop` [T] the row's dropout decisions (null: none), z the column's normal.
PHC_HD float obs_aug_value(const phc_obs_aug_args_t& a, const uint8_t* drop, int W, int c, float v, float z) {
    if (drop && c >= a.self_obs_size && drop[(c - a.self_obs_size) / W]) v = 0.0f;
    return a.noise_std > 0.f ? v + a.noise_std * z : v;
}

// Column pair j of a selected row, by 4-byte accesses (the kernel also has an 8-byte form for rows that start on an 8-byte boundary).  A column that neither
// rule changes is not written.
PHC_HD void obs_aug_pair(const phc_obs_aug_args_t& a, float* row, const uint8_t* drop, int W, uint32_t global_env, uint32_t k, int j) {
    float z0 = 0.f, z1 = 0.f;
    if (a.noise_std > 0.f) aug_normal_pair(a.key, global_env, k, (uint32_t)j, &z0, &z1);
    else if (!drop) return;
    const int c = 2 * j;
    row[c] = obs_aug_value(a, drop, W, c, row[c], z0);
    if (c + 1 < a.num_obs) row[c + 1] = obs_aug_value(a, drop, W, c + 1, row[c + 1], z1);
}

// The env of selection slot s (a row of the grid): s itself, or env_ids[s]; -1 = not selected.
PHC_HD int64_t obs_aug_env_of(const phc_obs_aug_args_t& a, int64_t s) {
    if (a.env_ids) {
        const int64_t e = a.env_ids[s];
        return (uint64_t)e < (uint64_t)a.num_envs ? e : -1;
    }
    return (a.row_flag && a.row_flag[s] == 0) ? -1 : s;
}
PHC_HD int64_t obs_aug_slots(const phc_obs_aug_args_t& a) { return a.env_ids ? a.n_ids : (int64_t)a.num_envs; }

// The whole launch on the host, in the kernel's order: per selected row the dropout decisions, the column pairs, the counter.
inline void obs_augment_host(const phc_obs_aug_args_t& a) {
    const int P = (a.num_obs + 1) / 2, W = obs_aug_width(a);
    uint8_t drop[OBS_AUG_MAX_SAMPLES];
    for (int64_t s = 0; s < obs_aug_slots(a); ++s) {
        const int64_t env = obs_aug_env_of(a, s);
        if (env < 0) continue;
        const uint32_t k = (uint32_t)a.k[env], ge = (uint32_t)(a.env_offset + env);
        for (int t = 0; W > 0 && t < a.num_samples; ++t) drop[t] = obs_aug_dropped(a, ge, k, t);
        float* row = a.obs + env * (int64_t)a.num_obs;
        for (int j = 0; j < P; ++j) obs_aug_pair(a, row, W > 0 ? drop : nullptr, W, ge, k, j);
        a.k[env] = (int32_t)(k + 1u);
    }
}

// One env of phc_occl_advance: the kernel's lane, and the host build's loop body.
PHC_HD void occl_advance_env(int J, uint64_t key, int64_t env_offset, int32_t* k, float prob, int32_t span_lo, int32_t span_hi, int64_t* count, uint8_t* mask,
                             int64_t env) {
    const uint32_t kk = (uint32_t)k[env], ge = (uint32_t)(env_offset + env);
    const float width = (float)((int64_t)span_hi - (int64_t)span_lo);
    for (int j = 0; j < J; ++j) {
        const float u = aug_u01(key, ge, kk, (uint32_t)j, 0u), v = aug_u01(key, ge, kk, (uint32_t)j, 1u);
        const bool start = j != 0 && u < prob;
        int64_t span = (int64_t)span_lo + (int64_t)floorf(v * width);
        if (span > (int64_t)span_hi - 1) span = (int64_t)span_hi - 1;
        const int64_t c = (start ? span : count[env * J + j]) - 1;
        count[env * J + j] = c > 0 ? c : 0;
        mask[env * J + j] = !(9 <= j && j < 24);
    }
    k[env] = (int32_t)(kk + 1u);
}

inline void occl_advance_host(int32_t num_envs, int32_t J, uint64_t key, int64_t env_offset, int32_t* k, float prob, int32_t span_lo, int32_t span_hi,
                              int64_t* count, uint8_t* mask) {
    for (int64_t e = 0; e < num_envs; ++e) occl_advance_env(J, key, env_offset, k, prob, span_lo, span_hi, count, mask, e);
}

// The argument checks (host side; include/phc_amd.h lists them): 0, PHC_EINVAL or PHC_EUNSUPPORTED.  Functions of their own so that the tests can ask them
// about arguments they must never hand to a launch.
inline bool aug_offset_ok(int64_t env_offset, int64_t num_envs) { return env_offset >= 0 && env_offset + num_envs <= (int64_t)1 << 32; }
inline int32_t obs_augment_check(const phc_obs_aug_args_t* a) {
    if (!a || !a->obs || !a->k) return PHC_EINVAL;
    if (a->num_envs < 0 || a->num_obs < 0 || a->num_samples < 0 || a->n_ids < 0) return PHC_EINVAL;
    if (a->self_obs_size < 0 || a->self_obs_size > a->num_obs) return PHC_EINVAL;
    if (a->num_samples >= 1 && (a->num_obs - a->self_obs_size) % a->num_samples != 0) return PHC_EINVAL;
    if ((a->row_flag && a->env_ids) || (!a->env_ids && a->n_ids != 0) || a->n_ids > a->num_envs) return PHC_EINVAL;   // (distinct ids: n <= N)
    if (!aug_offset_ok(a->env_offset, a->num_envs)) return PHC_EINVAL;
    if (!(a->dropout_p >= 0.f && a->dropout_p <= 1.f) || !(a->noise_std >= 0.f)) return PHC_EINVAL;
    return a->num_obs > OBS_AUG_MAX_OBS || a->num_samples > OBS_AUG_MAX_SAMPLES ? PHC_EUNSUPPORTED : 0;
}
inline int32_t occl_advance_check(int32_t num_envs, int32_t J, int64_t env_offset, const int32_t* k, float prob, int32_t span_lo, int32_t span_hi,
                                  const int64_t* count, const uint8_t* mask) {
    if (!k || !count || !mask || num_envs < 0 || J < 0) return PHC_EINVAL;
    if (!aug_offset_ok(env_offset, num_envs)) return PHC_EINVAL;
    if (!(prob >= 0.f && prob <= 1.f) || span_hi <= span_lo) return PHC_EINVAL;
    return J > OCCL_MAX_BODIES ? PHC_EUNSUPPORTED : 0;
}

}  // namespace phc
