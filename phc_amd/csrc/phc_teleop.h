// phc_teleop.h -- per-lane code of phc_teleop_rewards (contract: include/phc_amd.h; kernel: csrc/phc_teleop.hip): HumanoidTeleop's regularisation rewards, their
// per-env state and the recovery window after a velocity push (reference: phc/env/tasks/humanoid_teleop.py:95-101,167-307).
// A group of G lanes per env.  teleop_rows_lane / teleop_feet_lane: lane l's share -- the DoFs l, l + G, ... of the [N, D] rows (coalesced), foot l -- as partial sums;
// the caller sums every field over the group (device: csrc/phc_group.h; host: teleop_group_sum_host below, the same butterfly in the same order, so the two
// builds add the same numbers in the same order); teleop_finish: scaling, columns, rew_buf and the recovery counter.
// PHC_HD: tests/teleop_shim.cpp builds all of it for the CPU.  The reference-motion lookup is phc_task.h's / phc_im.h's (frame_ref, motion_time, ref_body).
#pragma once
#include <math.h>
#include "phc_im.h"

namespace phc {

#define PHC_TELEOP_G 32   // lanes per env
#define PHC_TELEOP_BIT(t) (1u << (t))
#define PHC_TELEOP_FEET_FORCE_TERMS (PHC_TELEOP_BIT(PHC_TELEOP_SLIPPAGE) | PHC_TELEOP_BIT(PHC_TELEOP_FEET_CONTACT_FORCES) | PHC_TELEOP_BIT(PHC_TELEOP_STUMBLE) \
                                     | PHC_TELEOP_BIT(PHC_TELEOP_FEET_AIR_TIME))

// One lane's partial value of every term (a term that is off stays 0); after the group sums: the env's values.  `stumble` is a count of feet.
struct TeleopSums { float v[PHC_TELEOP_NUM_TERMS]; };

PHC_HD bool teleop_on(const phc_teleop_args_t& a, int term) { return (a.term_mask & PHC_TELEOP_BIT(term)) != 0u; }

// quat_rotate_inverse(q, (0, 0, -1)) of the reference's quaternion library (isaacgym torch_utils), operation by operation: a - b + c with
// a = v (2 w^2 - 1), b = cross(q_xyz, v) w 2, c = q_xyz dot(q_xyz, v) 2; only x and y are needed.
PHC_HD float teleop_gravity_xy_norm(Q4 q) {
    PHC_NO_CONTRACT
    const V3 v = v3(0.f, 0.f, -1.f), qv = v3(q.x, q.y, q.z);
    const float s = 2.0f * (q.w * q.w) - 1.0f;
    const V3 cr = cross(qv, v);
    const float d = dot(qv, v);
    const float gx = v.x * s - cr.x * q.w * 2.0f + qv.x * d * 2.0f;
    const float gy = v.y * s - cr.y * q.w * 2.0f + qv.y * d * 2.0f;
    return sqrtf(gx * gx + gy * gy);
}

// [|ref root v_xy| > 0.1] at the imitation reward's lookup time of this step (humanoid_teleop.py:298 reads what the previous observation pass stored), in two
// halves: the env's clock and its clip's table entries -- loads that depend on nothing, requested at the kernel's top next to the row loads -- and the lookup.
struct TeleopClock { int64_t progress; float start, start_off; FrameTab tab; };
PHC_HD TeleopClock teleop_clock(const phc_motion_lib_t& lib, const phc_teleop_args_t& a, int64_t env) {
    TeleopClock c;
    const bool gated = a.recovery_counter != nullptr && a.recovery_counter[env] > 0;   // post-physics wrote progress - 1 back for these
    c.progress = a.progress_buf[env] + (gated ? 1 : 0);
    c.start = a.motion_start_times[env];
    c.start_off = a.motion_start_times_offset[env];
    c.tab = frame_tab(lib, a.sampled_motion_ids ? a.sampled_motion_ids[env] : env);
    return c;
}
PHC_HD float teleop_ref_moving(const phc_motion_lib_t& lib, const phc_teleop_args_t& a, const TeleopClock& c) {
    PHC_NO_CONTRACT
    const float t = motion_time(c.progress, a.dt, c.start, c.start_off);
    const V3 vel = ref_body(lib, frame_ref(c.tab, t), 0).vel;
    return sqrtf(vel.x * vel.x + vel.y * vel.y) > 0.1f ? 1.0f : 0.0f;
}

// Lane `lane` of env `env`, the DoF rows: its partial sums of the six row terms (the other terms 0), and its DoFs of last_actions / last_dof_vel.
PHC_HD TeleopSums teleop_rows_lane(const phc_teleop_args_t& a, int64_t env, int lane) {
    PHC_NO_CONTRACT
    TeleopSums s;
    for (int t = 0; t < PHC_TELEOP_NUM_TERMS; ++t) s.v[t] = 0.f;
    const int D = a.num_dof;
    const bool on_lim = teleop_on(a, PHC_TELEOP_DOF_POS_LIMITS), on_tlim = teleop_on(a, PHC_TELEOP_TORQUE_LIMITS), on_tau = teleop_on(a, PHC_TELEOP_TORQUES);
    const bool on_vel = teleop_on(a, PHC_TELEOP_DOF_VEL), on_acc = teleop_on(a, PHC_TELEOP_DOF_ACC), on_rate = teleop_on(a, PHC_TELEOP_ACTION_RATE);
    const bool need_qd = on_vel || on_acc || a.last_dof_vel != nullptr, need_tau = on_tlim || on_tau, need_act = on_rate || a.last_actions != nullptr;
    for (int d = lane; d < D; d += PHC_TELEOP_G) {
        const int64_t i = env * D + d;
        // every load of the element first: they are independent
        float q = 0.f, qd = 0.f, tau = 0.f, act = 0.f, last_qd = 0.f, last_act = 0.f, lo = 0.f, hi = 0.f, tl = 0.f;
        if (on_lim) { q = a.dof_state[2 * i]; lo = a.dof_limits_lower[d]; hi = a.dof_limits_upper[d]; }
        if (need_qd) qd = a.dof_state[2 * i + 1];
        if (need_tau) tau = a.dof_force[i];
        if (on_tlim) tl = a.torque_limits[d];
        if (need_act) act = a.actions[i];
        if (on_acc) last_qd = a.last_dof_vel[i];
        if (on_rate) last_act = a.last_actions[i];
        if (on_lim) {   // -(q - lo).clip(max=0) + (q - hi).clip(min=0)
            float out = -fminf(q - lo, 0.f);
            out += fmaxf(q - hi, 0.f);
            s.v[PHC_TELEOP_DOF_POS_LIMITS] += out;
        }
        if (on_tlim) s.v[PHC_TELEOP_TORQUE_LIMITS] += fmaxf(fabsf(tau) - tl, 0.f);
        if (on_tau) s.v[PHC_TELEOP_TORQUES] += tau * tau;
        if (on_vel) s.v[PHC_TELEOP_DOF_VEL] += qd * qd;
        if (on_acc) { const float acc = (last_qd - qd) / a.dt; s.v[PHC_TELEOP_DOF_ACC] += acc * acc; }
        if (on_rate) { const float da = last_act - act; s.v[PHC_TELEOP_ACTION_RATE] += da * da; }
        if (a.last_dof_vel) a.last_dof_vel[i] = qd;
        if (a.last_actions) a.last_actions[i] = act;
    }
    return s;
}

// Lane `lane` of env `env`, the feet: foot `lane`'s share of the five feet terms into `s`, and its entries of feet_air_time / last_contacts.
PHC_HD void teleop_feet_lane(const phc_teleop_args_t& a, int64_t env, int lane, TeleopSums& s) {
    PHC_NO_CONTRACT
    if (lane < a.num_feet) {
        const int body = a.feet[lane];
        const int64_t b = env * a.num_bodies + body;
        V3 F = v3(0.f, 0.f, 0.f);
        if (a.term_mask & PHC_TELEOP_FEET_FORCE_TERMS) F = ld3(a.contact_force + b * 3);
        const float Fn = norm(F);
        if (teleop_on(a, PHC_TELEOP_SLIPPAGE)) s.v[PHC_TELEOP_SLIPPAGE] = norm(ld3(a.rigid_body_state + b * 13 + 7)) * (Fn > 1.0f ? 1.0f : 0.0f);
        if (teleop_on(a, PHC_TELEOP_FEET_CONTACT_FORCES)) s.v[PHC_TELEOP_FEET_CONTACT_FORCES] = fmaxf(Fn - a.max_contact_force, 0.f);
        if (teleop_on(a, PHC_TELEOP_STUMBLE)) s.v[PHC_TELEOP_STUMBLE] = sqrtf(F.x * F.x + F.y * F.y) > 5.0f * fabsf(F.z) ? 1.0f : 0.0f;
        if (teleop_on(a, PHC_TELEOP_FEET_AIR_TIME)) {   // humanoid_teleop.py:289-300, statement by statement
            const int64_t f = env * a.num_feet + lane;
            const bool contact = F.z > 1.0f;
            const bool filt = contact || a.last_contacts[f] != 0;
            a.last_contacts[f] = contact ? 1 : 0;
            float air = a.feet_air_time[f];
            const bool first = air > 0.f && filt;
            air += a.dt;
            s.v[PHC_TELEOP_FEET_AIR_TIME] = (air - 0.25f) * (first ? 1.0f : 0.0f);
            a.feet_air_time[f] = filt ? 0.f : air;
        }
        if (teleop_on(a, PHC_TELEOP_FEET_ORI) && lane < 2) s.v[PHC_TELEOP_FEET_ORI] = teleop_gravity_xy_norm(ld4(a.rigid_body_state + b * 13 + 3));
    }
}

// The env's reward before this launch, for the lane that adds to it (requested at the kernel's top: the last link of the chain is then a store).
PHC_HD float teleop_rew_in(const phc_teleop_args_t& a, int64_t env, int lane) { return lane == 0 && a.term_mask != 0u ? a.rew_buf[env] : 0.f; }

// After the group sums, every lane of the group with the env's `s`; `moving` = teleop_ref_moving (1 when the air-time term is off), `rew_in` = teleop_rew_in.
PHC_HD void teleop_finish(const phc_teleop_args_t& a, int64_t env, int lane, TeleopSums s, float moving, float rew_in) {
    PHC_NO_CONTRACT
    int R = 0;
    for (int t = 0; t < PHC_TELEOP_NUM_TERMS; ++t) R += teleop_on(a, t) ? 1 : 0;
    const int C = a.num_im_cols;
    float* row = a.reward_raw + env * (int64_t)(C + R);
    if (lane < C) row[lane] = a.reward_im[env * (int64_t)C + lane];
    if (lane != 0) return;
    s.v[PHC_TELEOP_STUMBLE] = s.v[PHC_TELEOP_STUMBLE] > 0.f ? 1.0f : 0.0f;   // torch.any over the feet
    s.v[PHC_TELEOP_FEET_AIR_TIME] *= moving;
    if (R > 0) {
        float rew = rew_in;
        for (int r = 0; r < R; ++r) {   // humanoid_teleop.py:242-246: rew = term * scale; rew_buf += rew; a column each
            const int t = a.order[r];
            float term = 0.f;   // (a select chain: the sums stay in registers)
            for (int u = 0; u < PHC_TELEOP_NUM_TERMS; ++u) term = t == u ? s.v[u] : term;
            const float v = term * a.scale[t];
            rew += v;
            row[C + r] = v;
        }
        a.rew_buf[env] = rew;
    }
    if (a.push_interval > 0) {   // the next step's phc_dr_advance pushes this env (phc_dr.h: k > 0, k % push_interval == 0) unless it is reset before
        const uint32_t k = (uint32_t)a.dr_k[env];
        if (k > 0u && k % (uint32_t)a.push_interval == 0u) a.recovery_counter[env] = a.recovery_steps + 1;
    }
}

// The group sum of csrc/phc_group.h on the host, v[G] in place: xor 1, xor 2, mirror within 8, mirror within 16, xor 16 -- the same additions in the same order.
inline void teleop_group_sum_host(float* v) {
    float w[PHC_TELEOP_G];
    const int G = PHC_TELEOP_G;
    for (int step = 0; step < 5; ++step) {
        for (int i = 0; i < G; ++i) {
            const int j = step == 0 ? (i ^ 1) : step == 1 ? (i ^ 2) : step == 2 ? ((i & ~7) | (7 - (i & 7))) : step == 3 ? ((i & ~15) | (15 - (i & 15))) : (i ^ 16);
            w[i] = v[i] + v[j];
        }
        for (int i = 0; i < G; ++i) v[i] = w[i];
    }
}

// One env on the host: what a lane group of the kernel does.
inline void teleop_env_host(const phc_motion_lib_t& lib, const phc_teleop_args_t& a, int64_t env) {
    const bool air = teleop_on(a, PHC_TELEOP_FEET_AIR_TIME);
    const float moving = air ? teleop_ref_moving(lib, a, teleop_clock(lib, a, env)) : 1.0f, rew_in = teleop_rew_in(a, env, 0);
    TeleopSums lanes[PHC_TELEOP_G], s;
    for (int l = 0; l < PHC_TELEOP_G; ++l) {
        lanes[l] = teleop_rows_lane(a, env, l);
        teleop_feet_lane(a, env, l, lanes[l]);
    }
    for (int t = 0; t < PHC_TELEOP_NUM_TERMS; ++t) {
        float v[PHC_TELEOP_G];
        for (int l = 0; l < PHC_TELEOP_G; ++l) v[l] = lanes[l].v[t];
        teleop_group_sum_host(v);
        s.v[t] = v[0];
    }
    for (int l = 0; l < PHC_TELEOP_G; ++l) teleop_finish(a, env, l, s, moving, l == 0 ? rew_in : 0.f);
}

// The argument checks of phc_teleop_rewards (host side; include/phc_amd.h lists them): 0 or PHC_EINVAL.
inline int32_t teleop_args_check(const phc_motion_lib_t* lib, const phc_teleop_args_t* a) {
    if (!a || !a->rew_buf || !a->reward_raw) return PHC_EINVAL;
    if (a->num_envs < 0 || a->num_dof < 1 || a->num_feet < 0 || a->num_feet > PHC_TELEOP_MAX_FEET) return PHC_EINVAL;
    if (a->num_im_cols < 0 || a->num_im_cols > 8 || (a->num_im_cols > 0 && !a->reward_im)) return PHC_EINVAL;
    if (a->term_mask >> PHC_TELEOP_NUM_TERMS) return PHC_EINVAL;
    if (!(a->dt > 0.f && a->dt <= 3.0e38f) || a->push_interval < 0 || a->recovery_steps < 0) return PHC_EINVAL;
    uint32_t seen = 0u;
    int R = 0;
    for (int t = 0; t < PHC_TELEOP_NUM_TERMS; ++t) R += (a->term_mask >> t) & 1u;
    for (int r = 0; r < R; ++r) {
        const int t = a->order[r];
        if (t < 0 || t >= PHC_TELEOP_NUM_TERMS || !((a->term_mask >> t) & 1u) || ((seen >> t) & 1u)) return PHC_EINVAL;
        seen |= 1u << t;
    }
    const auto on = [&](int t) { return ((a->term_mask >> t) & 1u) != 0u; };
    if (a->num_feet > 0) {
        if (a->num_bodies < 1 || a->num_bodies > PHC_MAX_BODIES) return PHC_EINVAL;
        for (int f = 0; f < a->num_feet; ++f)
            if (a->feet[f] < 0 || a->feet[f] >= a->num_bodies) return PHC_EINVAL;
    }
    if (on(PHC_TELEOP_FEET_ORI) && a->num_feet < 2) return PHC_EINVAL;
    if ((on(PHC_TELEOP_DOF_POS_LIMITS) || on(PHC_TELEOP_DOF_VEL) || on(PHC_TELEOP_DOF_ACC) || a->last_dof_vel) && !a->dof_state) return PHC_EINVAL;
    if (on(PHC_TELEOP_DOF_POS_LIMITS) && (!a->dof_limits_lower || !a->dof_limits_upper)) return PHC_EINVAL;
    if ((on(PHC_TELEOP_TORQUE_LIMITS) || on(PHC_TELEOP_TORQUES)) && !a->dof_force) return PHC_EINVAL;
    if (on(PHC_TELEOP_TORQUE_LIMITS) && !a->torque_limits) return PHC_EINVAL;
    if (on(PHC_TELEOP_DOF_ACC) && !a->last_dof_vel) return PHC_EINVAL;
    if ((on(PHC_TELEOP_ACTION_RATE) || a->last_actions) && !a->actions) return PHC_EINVAL;
    if (on(PHC_TELEOP_ACTION_RATE) && !a->last_actions) return PHC_EINVAL;
    if ((a->term_mask & PHC_TELEOP_FEET_FORCE_TERMS) && a->num_feet > 0 && !a->contact_force) return PHC_EINVAL;
    if ((on(PHC_TELEOP_SLIPPAGE) || on(PHC_TELEOP_FEET_ORI)) && a->num_feet > 0 && !a->rigid_body_state) return PHC_EINVAL;
    if (on(PHC_TELEOP_FEET_AIR_TIME)) {
        if (!lib || !lib->frames || !lib->motion_lengths || !lib->motion_dt || !lib->motion_num_frames || !lib->length_starts) return PHC_EINVAL;
        if (!a->progress_buf || !a->motion_start_times || !a->motion_start_times_offset) return PHC_EINVAL;
        if (a->num_feet > 0 && (!a->feet_air_time || !a->last_contacts)) return PHC_EINVAL;
    }
    if (a->push_interval > 0 && (!a->dr_k || !a->recovery_counter)) return PHC_EINVAL;
    return 0;
}

}  // namespace phc
