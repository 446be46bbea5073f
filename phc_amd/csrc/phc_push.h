// phc_push.h -- per-lane pieces of the device push schedule (phc_push_advance, csrc/phc_push.hip; contract: include/phc_amd.h): the five draws of an
// env step and the schedule's transition for one env, which restates PushSchedule.advance (phc_amd/perturb.py) line for line.
// PHC_HD: tests/push_shim.cpp builds both for the CPU.
#pragma once
#include <math.h>
#include "phc_rng.h"
#include "../../include/phc_amd.h"

namespace phc {

// The five uniforms of launch `k` of env `global_env`: pause, magnitude, azimuth, height, body.  The draw's own counter 5 k + i is folded into the
// stream key the way the reset launch folds its call counter (phc_kernels.hip k_im_reset), the env id is hashed under that key.
PHC_HD void push_draws(uint64_t key, uint32_t global_env, uint32_t k, float u[5]) {
#pragma unroll
    for (int i = 0; i < 5; ++i)
        u[i] = hash_u01(splitmix64(key ^ (((uint64_t)k * 5u + (uint64_t)i) * 0x9E6C63D0876A9A47ull)), global_env);
}

// What of phc_push_args_t the transition reads.
struct PushParams {
    int pause_lo, pause_hi, duration, direction, num_listed;
    float force_lo, force_hi;
    const int32_t* bodies;   // [num_listed] the rows of force[env] a push may act on
};
PHC_HD PushParams push_params(const phc_push_args_t& a) {
    PushParams p;
    p.pause_lo = a.pause_lo; p.pause_hi = a.pause_hi; p.duration = a.duration; p.direction = a.direction; p.num_listed = a.num_listed;
    p.force_lo = a.force_lo; p.force_hi = a.force_hi; p.bodies = a.bodies;
    return p;
}

// One env's state, and what the launch has to do to the env's rows of the force buffer.
struct PushState {
    int remaining, countdown, body, started;   // `body`: the row of force[env] that holds a force (-1: none)
    int clear_row, write_row;                  // outputs of push_lane: the row to zero / to fill with f (-1: none)
    float f[3];
};

// PushSchedule._pause
PHC_HD int push_pause(const PushParams& p, float u0) {
    const int span = p.pause_hi - p.pause_lo;
    const int d = (int)floorf(u0 * (float)(span + 1));
    return p.pause_lo + (d < span ? d : span);
}

// PushSchedule.advance for one env (p.bodies is read only where a push starts).
PHC_HD void push_lane(const PushParams& p, PushState& s, const float u[5], bool reset) {
    s.clear_row = s.write_row = -1;
    const int pause = push_pause(p, u[0]);
    if (reset) { s.remaining = 0; s.countdown = pause; }
    const bool start = s.remaining == 0 && s.countdown <= 0;
    if (start) s.remaining = p.duration;
    const bool active = s.remaining > 0;
    if (s.body >= 0 && (start || !active)) { s.clear_row = s.body; s.body = -1; }   // force = where(start, new, force) * active
    if (start) {
        const float mag = p.force_lo + u[1] * (p.force_hi - p.force_lo);
        const float az = u[2] * 6.283185307179586f;
        float z = 0.f, r = 1.f;
        if (p.direction != 0) {
            z = 2.0f * u[3] - 1.0f;
            const float q = 1.0f - z * z;
            r = sqrtf(q > 0.f ? q : 0.f);
        }
        s.f[0] = r * cosf(az) * mag; s.f[1] = r * sinf(az) * mag; s.f[2] = z * mag;
        const int j = (int)floorf(u[4] * (float)p.num_listed);
        s.body = s.write_row = p.bodies[j < p.num_listed - 1 ? j : p.num_listed - 1];
        s.started += 1;
    }
    const bool ended = active && s.remaining == 1;
    s.remaining = s.remaining > 1 ? s.remaining - 1 : 0;
    s.countdown = ended ? pause : (active ? s.countdown : s.countdown - 1);
}

// One env of a launch with its draws given: state in, transition, the (at most two) rows of force[env], state out.
PHC_HD void push_env_given(const phc_push_args_t& a, int64_t env, const float u[5], bool reset) {
    PushState s;
    s.remaining = a.remaining[env]; s.countdown = a.countdown[env]; s.body = a.body[env]; s.started = a.started[env];
    push_lane(push_params(a), s, u, reset);
    float* f = a.force + env * (int64_t)a.num_bodies * 3;
    // (rows come from device memory -- the listed bodies, a restored state: one outside the env's block is dropped, never written)
    if ((unsigned)s.clear_row < (unsigned)a.num_bodies) { f[s.clear_row * 3 + 0] = 0.f; f[s.clear_row * 3 + 1] = 0.f; f[s.clear_row * 3 + 2] = 0.f; }
    if ((unsigned)s.write_row < (unsigned)a.num_bodies) { f[s.write_row * 3 + 0] = s.f[0]; f[s.write_row * 3 + 1] = s.f[1]; f[s.write_row * 3 + 2] = s.f[2]; }
    a.remaining[env] = s.remaining; a.countdown[env] = s.countdown; a.body[env] = s.body; a.started[env] = s.started;
}

// One env of phc_push_advance: the kernel's lane, and the host build's loop body.
PHC_HD void push_env(const phc_push_args_t& a, int64_t env) {
    const uint32_t k = (uint32_t)a.k[env];
    const bool reset = k == 0u || (a.progress_buf != nullptr && a.progress_buf[env] == 0);
    float u[5];
    push_draws(a.key, (uint32_t)(a.env_offset + env), k, u);
    push_env_given(a, env, u, reset);
    a.k[env] = (int32_t)(k + 1u);
}

// The argument checks of phc_push_advance (host side; include/phc_amd.h lists them): 0 or PHC_EINVAL.  A function of its own so that the tests can ask
// it about arguments they must never hand to a launch.
inline int32_t push_args_check(const phc_push_args_t* a) {
    if (!a || !a->bodies || !a->remaining || !a->countdown || !a->body || !a->k || !a->started || !a->force) return PHC_EINVAL;
    if (a->num_envs < 0 || a->num_bodies < 1 || a->num_bodies > PHC_MAX_BODIES || a->num_listed < 1 || a->num_listed > PHC_MAX_BODIES) return PHC_EINVAL;
    if (a->pause_lo < 0 || a->pause_hi < a->pause_lo || a->pause_hi > (1 << 24) || a->duration < 1 || (a->direction != 0 && a->direction != 1)) return PHC_EINVAL;
    if (!(a->force_lo >= 0.f && a->force_hi >= a->force_lo && a->force_hi < INFINITY)) return PHC_EINVAL;
    if (a->env_offset < 0 || a->env_offset + (int64_t)a->num_envs > (int64_t)1 << 32) return PHC_EINVAL;
    return 0;
}

}  // namespace phc
