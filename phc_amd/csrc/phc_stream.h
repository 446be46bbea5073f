// phc_stream.h -- per-lane code of phc_stream_track (contract: include/phc_amd.h; kernel: csrc/phc_stream.hip): tracking of streamed keypoints, the per-step
// work of HumanoidImDemo / HumanoidImMCPDemo (reference: phc/env/tasks/humanoid_im_mcp_demo.py:252-321).
// A group of G lanes per env, lanes along the bodies (body j = lane + G r in round r).  stream_limb_lane: lane k's limb pair, summed over the group by the
// caller (device: csrc/phc_group.h; host: teleop_group_sum_host, the same butterfly in the same order); stream_advance_lane: body j's new sample, its ring
// slot, the filtered value at the newest sample, frame matrix and velocity; stream_head_advance: the env's ring counters; stream_obs_lane: gating, the
// obs_v 7 task observation and the lane's share of track_err; stream_finish: the env's flags and track_err.
// PHC_HD: tests/stream_shim.cpp builds all of it for the CPU.  Gating and observation are phc_im.h's / phc_task.h's (zero_out_far_ref, task_obs_lane).
#pragma once
#include <math.h>
#include "phc_im.h"
#include "phc_teleop.h"   // teleop_group_sum_host: the host form of phc_group.h's sum

namespace phc {

#define PHC_STREAM_G 32        // lanes per env
#define PHC_STREAM_ROUNDS 2    // PHC_MAX_BODIES / PHC_STREAM_G

struct StreamRef { V3 pos, vel; };
// The env's ring position before this launch (every lane reads the same three values).
struct StreamHead { int head, count, prev; };

PHC_HD StreamHead stream_head(const phc_stream_args_t& a, int64_t env) {
    StreamHead h;
    h.head = a.head[env]; h.count = a.count[env]; h.prev = a.has_prev[env] != 0 ? 1 : 0;
    // the counters are the caller's memory: whatever they hold, every ring access stays inside the env's ring
    h.head = h.head < 0 ? 0 : (h.head >= a.window ? a.window - 1 : h.head);
    h.count = h.count < 0 ? 0 : (h.count > a.window ? a.window : h.count);
    return h;
}

// staged keypoint of body j of env `env`
PHC_HD V3 stream_frame(const phc_stream_args_t& a, int nb, int64_t env, int j) {
    const int64_t row = a.frame_rows == 1 ? 0 : env;
    int src = a.perm ? a.perm[j] : j;
    src = src < 0 ? 0 : (src >= nb ? nb - 1 : src);   // (a table entry outside the frame reads inside it)
    return ld3(a.frames + (row * nb + src) * 3);
}

// Lane k < num_pairs: |p_parent - p_child| / length of pair k (the root cancels); 0 for the other lanes.  The caller sums over the group.
PHC_HD float stream_limb_lane(const phc_stream_args_t& a, int nb, int64_t env, int lane) {
    PHC_NO_CONTRACT
    if (!a.limb_scale || lane >= a.num_pairs) return 0.f;
    const V3 d = stream_frame(a, nb, env, a.pair_parent[lane]) - stream_frame(a, nb, env, a.pair_child[lane]);
    return norm(d) / a.pair_length[lane];
}
// the group's sum of stream_limb_lane -> the scale the root-relative keypoints are divided by
PHC_HD float stream_scale(const phc_stream_args_t& a, float limb_sum) { return a.limb_scale ? limb_sum / (float)a.num_pairs : 1.0f; }

// Body j of env `env`, mode ADVANCE: steps (1) - (5) of the contract.  Loads first (the frame, the L - 1 older ring samples of the body and of the root, the
// fold rows, the previous reference), then the stores (ring slot, cur_ref, cur_vel).  `root_lane`: this lane also writes the root ring's slot.
PHC_HD StreamRef stream_advance_lane(const phc_stream_args_t& a, int nb, int64_t env, int j, const StreamHead& h, float scale, bool root_lane) {
    PHC_NO_CONTRACT
    const int W = a.window, FW = a.fold_window;
    const int L = h.count + 1 < W ? h.count + 1 : W;
    const V3 p0 = stream_frame(a, nb, env, 0), pj = stream_frame(a, nb, env, j);
    const V3 prev = ld3(a.cur_ref + (env * nb + j) * 3);
    V3 q;   // root-relative, limb-scaled: one rounding
    q.x = (float)(((double)pj.x - (double)p0.x) / (double)scale);
    q.y = (float)(((double)pj.y - (double)p0.y) / (double)scale);
    q.z = (float)(((double)pj.z - (double)p0.z) / (double)scale);
    const double* fb = a.fold + ((int64_t)3 * FW + (L - 1)) * FW;                       // bodies
    const double* fx = a.fold + ((int64_t)0 * FW + (L - 1)) * FW;                       // root translation, per axis
    const double* fy = a.fold + ((int64_t)1 * FW + (L - 1)) * FW;
    const double* fz = a.fold + ((int64_t)2 * FW + (L - 1)) * FW;
    const float* rb = a.ring_body + env * (int64_t)W * nb * 3;
    const float* rr = a.ring_root + env * (int64_t)W * 3;
    double bx = 0.0, by = 0.0, bz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    for (int k = 0; k < L - 1; ++k) {   // oldest first; sample k sits L - 1 - k slots behind the new one
        int slot = h.head - (L - 1 - k);
        slot += slot < 0 ? W : 0;
        const V3 s = ld3(rb + ((int64_t)slot * nb + j) * 3), t = ld3(rr + slot * 3);
        const double w = fb[k];
        bx += w * (double)s.x; by += w * (double)s.y; bz += w * (double)s.z;
        tx += fx[k] * (double)t.x; ty += fy[k] * (double)t.y; tz += fz[k] * (double)t.z;
    }
    const double wn = fb[L - 1];
    bx += wn * (double)q.x; by += wn * (double)q.y; bz += wn * (double)q.z;
    tx += fx[L - 1] * (double)p0.x; ty += fy[L - 1] * (double)p0.y; tz += fz[L - 1] * (double)p0.z;
    const double gx = bx + tx, gy = by + ty, gz = bz + tz;
    const float* M = a.frame_mat;
    const double rx = (double)M[0] * gx + (double)M[1] * gy + (double)M[2] * gz;
    const double ry = (double)M[3] * gx + (double)M[4] * gy + (double)M[5] * gz;
    const double rz = (double)M[6] * gx + (double)M[7] * gy + (double)M[8] * gz;
    StreamRef r;
    r.pos = v3((float)rx, (float)ry, (float)rz);
    r.vel = v3(0.f, 0.f, 0.f);
    if (h.prev) {
        const double dt = (double)a.dt;
        r.vel = v3((float)((rx - (double)prev.x) / dt), (float)((ry - (double)prev.y) / dt), (float)((rz - (double)prev.z) / dt));
    }
    st3(a.ring_body + env * (int64_t)W * nb * 3 + ((int64_t)h.head * nb + j) * 3, q);
    if (root_lane) st3(a.ring_root + env * (int64_t)W * 3 + h.head * 3, p0);
    st3(a.cur_ref + (env * nb + j) * 3, r.pos);
    st3(a.cur_vel + (env * nb + j) * 3, r.vel);
    return r;
}

// mode OBSERVE: the reference as the last ADVANCE left it
PHC_HD StreamRef stream_load_lane(const phc_stream_args_t& a, int nb, int64_t env, int j) {
    StreamRef r;
    r.pos = ld3(a.cur_ref + (env * nb + j) * 3);
    r.vel = ld3(a.cur_vel + (env * nb + j) * 3);
    return r;
}

// The env's ring counters after an ADVANCE (one lane of the group).
PHC_HD void stream_head_advance(const phc_stream_args_t& a, int64_t env, const StreamHead& h) {
    const int W = a.window;
    a.head[env] = h.head + 1 < W ? h.head + 1 : 0;
    a.count[env] = h.count + 1 < W ? h.count + 1 : W;
    a.has_prev[env] = 1;
}

// Body j: gating (humanoid_im_mcp_demo.py:296-306) and the obs_v 7 task observation of a tracked body; returns its share of track_err.  `prm` carries the
// stream's distances (stream_params); `ref_root`: the reference of the body in track slot 0.
PHC_HD float stream_obs_lane(const phc_im_params_t& prm, const phc_stream_args_t& a, int nb, int64_t env, int j, const StreamRef& ref, V3 ref_root) {
    const int slot = prm.track_slot[j];
    if (slot < 0) return 0.f;
    const BodyState body = load_body(a.rigid_body_state, env, nb, j), root = load_body(a.rigid_body_state, env, nb, 0);
    const Q4 hroot = obs_root_rot(prm, root.rot);
    const Q4 hinv = calc_heading_quat_inv(hroot), h = calc_heading_quat(hroot);
    BodyState rt = body, rroot = root;
    rt.pos = ref.pos; rt.vel = ref.vel;
    rroot.pos = ref_root;
    if (prm.zero_out_far) zero_out_far_ref(prm, slot, body, root, rroot, &rt);
    task_obs_lane(prm, slot, body, root, rt, hinv, h, a.obs_buf + env * (int64_t)(prm.num_self_obs + prm.num_task_obs) + prm.num_self_obs);
    return norm(body.pos - ref.pos);
}

// After the group sum of the shares (one lane of the group).
PHC_HD void stream_finish(const phc_im_params_t& prm, const phc_stream_args_t& a, int64_t env, float err_sum) {
    a.track_err[env] = err_sum / (float)prm.num_track_bodies;
    if (a.reset_buf) a.reset_buf[env] = 0;           // humanoid_im_mcp_demo.py:319-321
    if (a.terminate_buf) a.terminate_buf[env] = 0;
}

// prm with the stream's own distances: what the kernel takes by value
inline phc_im_params_t stream_params(const phc_im_params_t& prm, const phc_stream_args_t& a) {
    phc_im_params_t p = prm;
    p.close_distance = a.close_distance;
    p.far_distance = a.far_distance;
    return p;
}

// One env on the host: what a lane group of the kernel does.
inline void stream_env_host(int nb, const phc_im_params_t& prm, const phc_stream_args_t& a, int64_t env) {
    const int G = PHC_STREAM_G;
    StreamRef ref[PHC_STREAM_ROUNDS * PHC_STREAM_G];
    float v[PHC_STREAM_G];
    if (a.mode == PHC_STREAM_ADVANCE) {
        const StreamHead h = stream_head(a, env);
        for (int l = 0; l < G; ++l) v[l] = stream_limb_lane(a, nb, env, l);
        teleop_group_sum_host(v);
        const float scale = stream_scale(a, v[0]);
        for (int j = 0; j < nb; ++j) ref[j] = stream_advance_lane(a, nb, env, j, h, scale, j == 0);
        stream_head_advance(a, env, h);
    } else {
        for (int j = 0; j < nb; ++j) ref[j] = stream_load_lane(a, nb, env, j);
    }
    const V3 ref_root = ref[a.track_root_body].pos;
    for (int l = 0; l < G; ++l) {
        v[l] = 0.f;
        for (int r = 0; r < PHC_STREAM_ROUNDS; ++r)
            if (l + G * r < nb) v[l] += stream_obs_lane(prm, a, nb, env, l + G * r, ref[l + G * r], ref_root);
    }
    teleop_group_sum_host(v);
    stream_finish(prm, a, env, v[0]);
}

// The argument checks of phc_stream_track (host side; include/phc_amd.h lists them): 0, PHC_EINVAL or PHC_EUNSUPPORTED.
inline int32_t stream_args_check(const phc_model_t* model, const phc_im_params_t* prm, const phc_stream_args_t* a) {
    if (!model || !prm || !a || !prm->track_slot || !a->cur_ref || !a->cur_vel || !a->rigid_body_state || !a->obs_buf || !a->track_err) return PHC_EINVAL;
    const int nb = model->num_bodies;
    if (a->num_envs < 0 || nb < 1 || nb > PHC_MAX_BODIES || prm->num_track_bodies < 1 || prm->num_track_bodies > nb) return PHC_EINVAL;
    if (a->track_root_body < 0 || a->track_root_body >= nb) return PHC_EINVAL;
    if (a->mode != PHC_STREAM_ADVANCE && a->mode != PHC_STREAM_OBSERVE) return PHC_EINVAL;
    if (a->mode == PHC_STREAM_ADVANCE) {
        if (a->window < 1 || a->window > PHC_STREAM_MAX_WINDOW || a->fold_window < a->window) return PHC_EINVAL;
        if (!a->frames || !a->fold || !a->ring_body || !a->ring_root || !a->head || !a->count || !a->has_prev) return PHC_EINVAL;
        if (a->frame_rows != 1 && a->frame_rows != a->num_envs) return PHC_EINVAL;
        if (a->num_pairs < (a->limb_scale ? 1 : 0) || a->num_pairs > PHC_STREAM_MAX_PAIRS) return PHC_EINVAL;
        for (int k = 0; k < a->num_pairs; ++k) {
            if (a->pair_parent[k] < 0 || a->pair_parent[k] >= nb || a->pair_child[k] < 0 || a->pair_child[k] >= nb) return PHC_EINVAL;
            if (!(a->pair_length[k] > 0.f && a->pair_length[k] <= 3.0e38f)) return PHC_EINVAL;
        }
        if (!(a->dt > 0.f && a->dt <= 3.0e38f)) return PHC_EINVAL;
    }
    if (prm->obs_v != 7 || prm->num_traj_samples > 1) return PHC_EUNSUPPORTED;
    return 0;
}

}  // namespace phc
