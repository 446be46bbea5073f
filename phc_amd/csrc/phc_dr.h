// phc_dr.h -- per-lane pieces of domain randomisation (contract: include/phc_amd.h): the torque-noise draw and the PD-target shift of the DR instantiations of
// the stepper's kernel (phc_sim_step_dr, csrc/phc_sim_dr.hip), and one env of phc_dr_advance (csrc/phc_dr.hip): control delay and velocity push.
// PHC_HD: tests/dr_shim.cpp builds all of it for the CPU.
#pragma once
#include <math.h>
#include "phc_rng.h"
#include "../../include/phc_amd.h"

namespace phc {

// The streams of one key: a draw's own counter is folded into the stream key the way the push schedule folds its launch counter (phc_push.h), each stream
// behind its own salt, so that the torque noise, the delay and the push of one (key, env, k) are unrelated.
#define PHC_DR_SALT_NOISE 0x6A09E667F3BCC909ull
#define PHC_DR_SALT_DELAY 0xBB67AE8584CAA73Bull
#define PHC_DR_SALT_PUSH  0x3C6EF372FE94F82Bull
PHC_HD uint64_t dr_fold(uint64_t key, uint64_t salt, uint64_t counter) { return splitmix64((key + salt) ^ (counter * 0x9E6C63D0876A9A47ull)); }

// ---- torque noise ("rfi"): u in [-1, 1) of env-step k, simulate call `call`, at index (env_offset + env) D + dof ----
PHC_HD uint64_t dr_noise_key(uint64_t key, uint32_t k, uint32_t call) { return dr_fold(key, PHC_DR_SALT_NOISE, ((uint64_t)k << 32) | (uint64_t)call); }
PHC_HD float dr_noise_u(uint64_t key, uint32_t k, uint32_t call, uint32_t index) { return 2.0f * hash_u01(dr_noise_key(key, k, call), index) - 1.0f; }
// A torque n added in front of the effort clip is the PD target raised by n / kp: clip(kp (t + n / kp - q) - kd qd) = clip(kp (t - q) - kd qd + n).
// `gain` = amp / kp, 0 where kp == 0.
PHC_HD float dr_noise_gain(float amp, float kp) { return kp != 0.f ? amp / kp : 0.f; }
PHC_HD float dr_target_shift(float target, float u, float gain) { return target + u * gain; }

// ---- control delay ----
PHC_HD int dr_delay_of(int lo, int hi, float u) {
    const int span = hi - lo;
    const int d = (int)floorf(u * (float)(span + 1));
    return lo + (d < span ? d : span);
}
PHC_HD float dr_delay_u(uint64_t key, uint32_t global_env, uint32_t k) { return hash_u01(dr_fold(key, PHC_DR_SALT_DELAY, k), global_env); }
// ---- velocity push: the two draws in [-1, 1) of launch k ----
PHC_HD float dr_push_u(uint64_t key, uint32_t global_env, uint32_t k, int axis) {
    return 2.0f * hash_u01(dr_fold(key, PHC_DR_SALT_PUSH, (uint64_t)k * 2u + (uint64_t)axis), global_env) - 1.0f;
}

// One env of phc_dr_advance: the kernel's lane, and the host build's loop body.  The ring [Q, N, D]: the action of launch k sits in row k mod Q, so row
// (k - delay) mod Q is what a queue that shifts every step, takes the new action at slot 0 and is read at slot `delay` hands out; rows zeroed at a reset are
// read as zeros until the env has written them again.
PHC_HD void dr_env(const phc_dr_args_t& a, int64_t env) {
    const uint32_t k = (uint32_t)a.k[env];
    const bool just_reset = a.progress_buf != nullptr && a.progress_buf[env] == 0;
    const bool reset = k == 0u || just_reset;
    const uint32_t genv = (uint32_t)(a.env_offset + env);
    const int D = a.num_dof;
    const int64_t N = a.num_envs;
    const float* act = a.actions + env * D;
    float* out = a.delayed_actions + env * D;
    if (a.delay_hi > 0) {
        const uint32_t Q = (uint32_t)a.delay_hi + 1u;
        int delay = a.delay[env];
        if (reset) {
            for (uint32_t q = 0; q < Q; ++q) {
                float* row = a.action_queue + ((int64_t)q * N + env) * D;
                for (int d = 0; d < D; ++d) row[d] = 0.f;
            }
            delay = dr_delay_of(a.delay_lo, a.delay_hi, dr_delay_u(a.key, genv, k));
            a.delay[env] = delay;
        }
        if (delay < 0) delay = 0;   // (a restored or foreign state: never outside the ring)
        if (delay > a.delay_hi) delay = a.delay_hi;
        float* in_row = a.action_queue + ((int64_t)(k % Q) * N + env) * D;
        for (int d = 0; d < D; ++d) in_row[d] = act[d];
        const float* out_row = a.action_queue + ((int64_t)((k % Q + Q - (uint32_t)delay) % Q) * N + env) * D;
        for (int d = 0; d < D; ++d) out[d] = out_row[d];
    } else {
        for (int d = 0; d < D; ++d) out[d] = act[d];
        a.delay[env] = 0;
    }
    if (a.push_interval > 0 && k > 0u && k % (uint32_t)a.push_interval == 0u && !just_reset) {
        float* r = a.root_states + env * 13;
        r[7] = dr_push_u(a.key, genv, k, 0) * a.max_push_vel_xy;
        r[8] = dr_push_u(a.key, genv, k, 1) * a.max_push_vel_xy;
    }
    a.k[env] = (int32_t)(k + 1u);
}

// The argument checks of phc_dr_advance (host side; include/phc_amd.h lists them): 0 or PHC_EINVAL.
inline int32_t dr_args_check(const phc_dr_args_t* a) {
    if (!a || !a->actions || !a->delayed_actions || !a->delay || !a->k) return PHC_EINVAL;
    if (a->num_envs < 0 || a->num_dof < 1) return PHC_EINVAL;
    if (a->delay_lo < 0 || a->delay_hi < a->delay_lo || a->delay_hi > 1023) return PHC_EINVAL;
    if (a->delay_hi > 0 && !a->action_queue) return PHC_EINVAL;
    if (a->push_interval < 0 || (a->push_interval > 0 && !a->root_states)) return PHC_EINVAL;
    if (!(a->max_push_vel_xy >= 0.f && a->max_push_vel_xy <= 3.0e38f)) return PHC_EINVAL;
    if (a->env_offset < 0 || a->env_offset + (int64_t)a->num_envs > (int64_t)1 << 32) return PHC_EINVAL;
    return 0;
}

}  // namespace phc
