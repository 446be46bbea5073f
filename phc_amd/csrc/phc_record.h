// phc_record.h -- per-lane code of phc_motion_record (csrc/phc_record.hip; contract, row layout and row rule: include/phc_amd.h): the simulated motion of every
// env, appended frame by frame to a caller-owned block on the device, in a form phc_amd/motion_record.py turns into a clip library.  What the reference does
// by hand with three to five .cpu().clone() copies per env step (base_task.py:242-246,405-440, humanoid.py:445-453, humanoid_im.py:401-466,
// humanoid_amp.py:827-873) is one launch here and one host copy per batch.
// PHC_HD: tests/record_shim.cpp and tests/record_asan_main.cpp build everything here for the CPU, motion_record_host included -- the whole launch as plain
// loops over (env, lane).  Headers, counters and every copied float are bit-equal between the two builds; the root's exp map (acosf, sqrt, the division of
// quat_to_angle_axis) and the revolute rows' axis x angle products differ by the device's elementary functions alone (no contraction, no fast-math).
//
// Thread mapping: a group of G lanes per env (G = 32 up to 32 bodies including the extended ones, two envs per wavefront; 64 above), lane j = body j, as in the
// env kernels.  A lane's share of the row (record_lane): its body's quaternion, its pose_aa row, the columns lane, lane + G, .. of dof_pos and ref_body_pos,
// and -- the first lanes -- the root position, the two root velocities and the time.
//
// Hazards, and how each is settled:
//   counter race   len[i] / closed[i] / seg[i] decide where (and whether) every lane of env i stores, and are updated in the same launch.  An env's row stays
//                  inside ONE wavefront (G divides 64 and groups do not straddle wavefronts); every lane reads the counters (record_decide: one vector load
//                  per counter, the same address across the group) IN FRONT OF a wavefront-scope ordering point, and lane 0 alone updates them BEHIND it
//                  (record_commit).  Lane 0's store needs the loaded value, so the load instruction -- which is every lane's load -- has returned before the
//                  store issues; no other wavefront or workgroup ever reads env i's counters.  (A flat element-per-thread grid, in which another workgroup
//                  may read the already bumped len[i], is the arrangement this avoids.)
//   alignment      W is odd for the SMPL family (247), so rows start at any multiple of 4 bytes, and so do the quaternions in rigid_body_state (13 floats per
//                  body) and the dof_pos rows (69 / 37 floats).  The one 16-byte access is the store of a lane's quaternion, taken only where the address is a
//                  multiple of 16 (uniform over the group: the lanes' addresses are 16 bytes apart); every other access, and that store elsewhere, is 4 bytes
//                  wide.  `frames` itself needs 4-byte alignment only.
//   argument check motion_record_check runs before any device access and reads host memory alone (the two structs; never a table or an array).
#pragma once
#include <math.h>
#include "phc_task.h"
#include "phc_aba.h"

namespace phc {

constexpr int RECORD_BLOCK = 256;   // threads per workgroup: 8 / 4 env groups

PHC_HD int record_width(int nb, int ne, int nd, int flags) { return 3 + 4 * nb + 3 * (nb + ne) + nd + 7 + ((flags & PHC_RECORD_REF) ? 3 * nb : 0); }
PHC_HD int record_group(int nb, int ne) { return nb + ne > 32 ? 64 : 32; }
// column offsets of a row
PHC_HD int rec_o_quat() { return 3; }
PHC_HD int rec_o_aa(int nb) { return 3 + 4 * nb; }
PHC_HD int rec_o_dof(int nb, int ne) { return 3 + 4 * nb + 3 * (nb + ne); }
PHC_HD int rec_o_vel(int nb, int ne, int nd) { return rec_o_dof(nb, ne) + nd; }
PHC_HD int rec_o_time(int nb, int ne, int nd) { return rec_o_vel(nb, ne, nd) + 6; }
PHC_HD int rec_o_ref(int nb, int ne, int nd) { return rec_o_time(nb, ne, nd) + 1; }

// Steps 1 and 2 of the row rule, read side: f = the row to write, or -1 (refused); `drop`: the refusal counts; `dead`: the env is closed (nothing happens at all).
struct RecDecision { int f; int seg; bool drop, dead; };
PHC_HD RecDecision record_decide(const phc_motion_record_args_t& a, int64_t env) {
    RecDecision d;
    const int len = a.len[env], closed = a.closed[env];
    d.seg = a.seg[env];
    int room = a.cap;
    if (a.limit) { const int l = a.limit[env]; room = l < room ? l : room; }
    d.dead = closed != 0;
    d.drop = !d.dead && len >= room;
    d.f = (d.dead || d.drop) ? -1 : len;
    return d;
}

// a lane's quaternion: one 16-byte store where the address allows (device build), four 4-byte stores elsewhere
PHC_HD void rec_store_quat(float* p, Q4 q) {
#if defined(__HIP_DEVICE_COMPILE__)
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) { *reinterpret_cast<float4*>(p) = make_float4(q.x, q.y, q.z, q.w); return; }
#endif
    p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
}

// pose_aa row of body j (j < NB + E)
PHC_HD V3 record_pose_aa(const phc_model_t& m, const phc_motion_record_args_t& a, int64_t env, int j) {
    if (j == 0) return quat_to_exp_map(ld4(a.root_states + env * 13 + 3));
    if (j >= a.num_bodies) return v3(0.f, 0.f, 0.f);           // extended bodies do not rotate (fit_smpl_motion.py:165)
    const int jt = model_tab(m, 2, j), ds = model_tab(m, 3, j);
    const float* q = a.dof_state + (env * a.num_dof) * 2;
    if (jt == PHC_JT_SPHERICAL && ds >= 0 && ds + 3 <= a.num_dof) return v3(q[2 * ds], q[2 * ds + 2], q[2 * ds + 4]);
    if (jt == PHC_JT_REVOLUTE && ds >= 0 && ds < a.num_dof) {
        const float* f = model_body(m, j);
        return v3(f[25], f[26], f[27]) * q[2 * ds];
    }
    return v3(0.f, 0.f, 0.f);
}

// Lane `lane` of env's group of G lanes: its share of row f (0 <= f < cap).
PHC_HD void record_lane(const phc_model_t& m, const phc_motion_record_args_t& a, int64_t env, int f, int lane, int G) {
    const int nb = a.num_bodies, ne = a.num_ext, nd = a.num_dof;
    float* row = a.frames + (env * a.cap + f) * (int64_t)a.width;
    const float* root = a.root_states + env * 13;
    if (lane < nb) rec_store_quat(row + rec_o_quat() + 4 * lane, ld4(a.rigid_body_state + (env * nb + lane) * 13 + 3));
    if (lane < nb + ne) st3(row + rec_o_aa(nb) + 3 * lane, record_pose_aa(m, a, env, lane));
    const float* q = a.dof_state + (env * nd) * 2;
    float* dof = row + rec_o_dof(nb, ne);
    for (int c = lane; c < nd; c += G) dof[c] = q[2 * c];
    if (lane < 3) row[lane] = root[lane];
    if (lane < 6) row[rec_o_vel(nb, ne, nd) + lane] = root[7 + lane];
    if (lane == 0)
        row[rec_o_time(nb, ne, nd)] = motion_time(a.progress_buf[env], a.dt, a.motion_start_times[env], a.motion_start_times_offset[env]);
    if (a.flags & PHC_RECORD_REF) {
        const float* r = a.ref_body_pos + env * (int64_t)(nb * 3);
        float* o = row + rec_o_ref(nb, ne, nd);
        for (int c = lane; c < nb * 3; c += G) o[c] = r[c];
    }
}

// Lane 0 behind the ordering point: the header row (step 2), the counters (steps 1 - 3).
PHC_HD void record_commit(const phc_motion_record_args_t& a, int64_t env, const RecDecision& d) {
    if (d.dead) return;
    const bool seed = (a.flags & PHC_RECORD_SEED) != 0;
    const int flag = (!seed && a.flag[env] != 0) ? 1 : 0;
    if (d.f >= 0) {
        int32_t* h = a.header + (env * a.cap + d.f) * 4;
        h[0] = d.seg; h[1] = (int32_t)a.progress_buf[env]; h[2] = (int32_t)a.motion_ids[env]; h[3] = flag;
        a.len[env] = d.f + 1;
    } else if (d.drop) {
        a.dropped[env] += 1;
    }
    if (flag) {
        if (a.flags & PHC_RECORD_ONE_SEGMENT) a.closed[env] = 1;
        else a.seg[env] = d.seg + 1;
    }
}

// The whole launch on the host, in the kernel's order: per env the decision, the lanes' shares, lane 0's commit.
inline void motion_record_host(const phc_model_t& m, const phc_motion_record_args_t& a) {
    const int G = record_group(a.num_bodies, a.num_ext);
    for (int64_t env = 0; env < a.num_envs; ++env) {
        const RecDecision d = record_decide(a, env);
        if (d.f >= 0)
            for (int lane = 0; lane < G; ++lane) record_lane(m, a, env, d.f, lane, G);
        record_commit(a, env, d);
    }
}

// The argument check (host side; include/phc_amd.h lists it): 0, PHC_EINVAL or PHC_EUNSUPPORTED.  Reads the two structs alone.
inline int32_t motion_record_check(const phc_model_t* m, const phc_motion_record_args_t* a) {
    if (!m || !a || !m->ints || !m->floats) return PHC_EINVAL;
    if (a->num_envs < 1 || a->num_bodies < 1 || a->num_dof < 1 || a->cap < 1 || a->num_ext < 0) return PHC_EINVAL;
    if (a->flags & ~(PHC_RECORD_REF | PHC_RECORD_SEED | PHC_RECORD_ONE_SEGMENT)) return PHC_EINVAL;
    if (!a->root_states || !a->dof_state || !a->rigid_body_state || !a->progress_buf || !a->flag || !a->motion_ids || !a->motion_start_times ||
        !a->motion_start_times_offset || !a->frames || !a->header || !a->len || !a->seg || !a->closed || !a->dropped) return PHC_EINVAL;
    if ((a->flags & PHC_RECORD_REF) && !a->ref_body_pos) return PHC_EINVAL;
    if (!(a->dt > 0.f) || !isfinite(a->dt)) return PHC_EINVAL;
    if ((int64_t)a->num_bodies + a->num_ext > PHC_MAX_BODIES) return PHC_EUNSUPPORTED;
    if (a->num_bodies != m->num_bodies || a->num_dof != m->num_dof || a->num_dof > 3 * PHC_MAX_BODIES) return PHC_EINVAL;
    if (a->width != record_width(a->num_bodies, a->num_ext, a->num_dof, a->flags)) return PHC_EINVAL;
    return 0;
}

}  // namespace phc
