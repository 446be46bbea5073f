// phc_clip_real.h -- per-lane pieces of the device clip processing for the robots (phc_clip_process_real, csrc/phc_clip_real.hip; contract: include/phc_amd.h):
// the height fix, `robot_fk` / `process_clip_real` (phc_amd/motion_lib.py) and the fp32 packing of the revolute record, restated operation by operation in
// fp64.  Every sum and product is written in the order of the numpy statement; numpy's 3x3 `matmul` leaves its own order (and whether it fuses) open, so the
// host build differs from `process_clip_real` by a few fp64 ulps -- far below the one fp32 rounding of the stores.  The velocities and the filter are
// phc_clip.h's: the scratch rows keep its [F, 6 NB] layout.
// PHC_HD: tests/clip_real_shim.cpp builds all of it for the CPU.
#pragma once
#include "phc_clip.h"

namespace phc {

struct Mat3d { double m[9]; };   // row-major

// the revolute record (abi.frame_stride_for(NB, E, 1)): gts 3(NB+E) | grs 4(NB+E) | gvs 3NB | gavs 3NB | dof_pos NB-1 | dvs NB-1 | pad to a multiple of 4
PHC_HD int clip_real_pad_begin(int NB, int E) { return 7 * (NB + E) + 6 * NB + 2 * (NB - 1); }
PHC_HD int clip_real_stride(int NB, int E) { return (clip_real_pad_begin(NB, E) + 3) / 4 * 4; }
PHC_HD int clip_real_frames_per_block(int NB, int E) {
    const int n = CLIP_LDS_BYTES / (clip_real_stride(NB, E) * 4 + 4);
    return n > 16 ? 16 : n;    // H1 (20 + 3, 320 floats): 16 frames; G1 (38 + 1, 576 floats): 14; 64 bodies: 7 or 8
}

// scratch: [F, 6 NB] f64 (phc_clip.h's rows: the fp64 positions 3 NB, then the raw angular velocities 3 NB), [U] f64 clip_dz, [F] i32 frame -> clip
PHC_HD int64_t clip_real_scratch_bytes(int64_t F, int NB, int U) { return F * 6 * NB * 8 + (int64_t)U * 8 + (F * 4 + 7) / 8 * 8; }
PHC_HD double* clip_real_dz(const phc_clip_real_args_t& a) { return (double*)a.scratch + a.num_frames * 6 * a.num_bodies; }
PHC_HD int32_t* clip_real_frame_clip(const phc_clip_real_args_t& a) { return (int32_t*)(clip_real_dz(a) + a.num_clips); }

// _quat_xyzw_to_mat(_aa_to_quat_xyzw(aa)): the norm and the quaternion's squared length summed left to right, the series branch below 1e-6 rad
PHC_HD Mat3d clip_real_aa_to_mat(const double* aa) {
    const double ang = sqrt(aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]);
    const double half = 0.5 * ang;
    const double k = fabs(ang) < 1e-6 ? 0.5 - ang * ang / 48.0 : sin(half) / ang;
    const double x = aa[0] * k, y = aa[1] * k, z = aa[2] * k, w = cos(half);
    const double two_s = 2.0 / (x * x + y * y + z * z + w * w);
    Mat3d r;
    r.m[0] = 1 - two_s * (y * y + z * z); r.m[1] = two_s * (x * y - z * w);     r.m[2] = two_s * (x * z + y * w);
    r.m[3] = two_s * (x * y + z * w);     r.m[4] = 1 - two_s * (x * x + z * z); r.m[5] = two_s * (y * z - x * w);
    r.m[6] = two_s * (x * z - y * w);     r.m[7] = two_s * (y * z + x * w);     r.m[8] = 1 - two_s * (x * x + y * y);
    return r;
}

PHC_HD Mat3d clip_real_matmul(const Mat3d& a, const Mat3d& b) {
    Mat3d r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
    return r;
}

// _mat_to_quat_xyzw: the four candidates, the first of the largest q_abs taken as is (no sign standardisation)
PHC_HD Quatd clip_real_mat_to_quat(const Mat3d& M) {
    const double m00 = M.m[0], m01 = M.m[1], m02 = M.m[2], m10 = M.m[3], m11 = M.m[4], m12 = M.m[5], m20 = M.m[6], m21 = M.m[7], m22 = M.m[8];
    const double e0 = 1 + m00 + m11 + m22, e1 = 1 + m00 - m11 - m22, e2 = 1 - m00 + m11 - m22, e3 = 1 - m00 - m11 + m22;
    const double a0 = sqrt(e0 > 0.0 ? e0 : 0.0), a1 = sqrt(e1 > 0.0 ? e1 : 0.0), a2 = sqrt(e2 > 0.0 ? e2 : 0.0), a3 = sqrt(e3 > 0.0 ? e3 : 0.0);
    int best = 0;
    double ab = a0;
    if (a1 > ab) { best = 1; ab = a1; }
    if (a2 > ab) { best = 2; ab = a2; }
    if (a3 > ab) { best = 3; ab = a3; }
    const double d = 2.0 * (ab > 0.1 ? ab : 0.1);
    double w, x, y, z;   // the candidate's row is wxyz
    if (best == 0)      { w = a0 * a0;   x = m21 - m12; y = m02 - m20; z = m10 - m01; }
    else if (best == 1) { w = m21 - m12; x = a1 * a1;   y = m10 + m01; z = m02 + m20; }
    else if (best == 2) { w = m02 - m20; x = m10 + m01; y = a2 * a2;   z = m12 + m21; }
    else                { w = m10 - m01; x = m20 + m02; y = m21 + m12; z = a3 * a3; }
    Quatd q; q.x = x / d; q.y = y / d; q.z = z / d; q.w = w / d;
    return q;
}

// The ancestor set of body j (j included) as one 64-bit word.  parents comes from device memory: a parent outside [0, k) ends the walk (a root).
PHC_HD uint64_t clip_real_chain(const int32_t* parents, int J, int j) {
    uint64_t chain = 0;
    for (int k = j, n = 0; n < J; ++n) {
        chain |= (uint64_t)1 << k;
        const int p = parents[k];
        if (p < 0 || p >= k) break;
        k = p;
    }
    return chain;
}

// robot_fk for one (frame, body): the lane walks its ancestor set in index order -- parents precede their children, so that is the host's order -- and
// needs nothing another lane computes.  The chain's first body is the root: wmat = pm, wpos = trans - (0, 0, dz).
PHC_HD void clip_real_fk(const phc_clip_real_args_t& a, int64_t f, uint64_t chain, double dz, bool want_pos, double wpos[3], Mat3d& wmat) {
    const int J = a.num_bodies + a.num_ext;
    const double* pose = a.pose_aa + f * J * 3;
    bool first = true;
    while (chain) {
        const int k = __builtin_ctzll(chain);
        chain &= chain - 1;
        const Mat3d pm = clip_real_aa_to_mat(pose + 3 * k);
        if (first) {
            wmat = pm;
            if (want_pos) { wpos[0] = a.trans[f * 3 + 0]; wpos[1] = a.trans[f * 3 + 1]; wpos[2] = a.trans[f * 3 + 2] - dz; }
            first = false;
        } else {
            if (want_pos) {
                const double* off = a.offsets + 3 * k;
                const double r0 = wmat.m[0] * off[0] + wmat.m[1] * off[1] + wmat.m[2] * off[2];
                const double r1 = wmat.m[3] * off[0] + wmat.m[4] * off[1] + wmat.m[5] * off[2];
                const double r2 = wmat.m[6] * off[0] + wmat.m[7] * off[1] + wmat.m[8] * off[2];
                wpos[0] = r0 + wpos[0]; wpos[1] = r1 + wpos[1]; wpos[2] = r2 + wpos[2];
            }
            Mat3d rest;
            for (int i = 0; i < 9; ++i) rest.m[i] = a.rest_mat[9 * k + i];
            wmat = clip_real_matmul(wmat, clip_real_matmul(rest, pm));
        }
    }
}

// Clip c's frame range, frame time and height shift.  clip_start is device memory: whatever it holds, the range stays inside [0, F) and around f.
struct ClipRealSpan { int64_t t0, t1; double dt, dz; };
PHC_HD ClipRealSpan clip_real_span(const phc_clip_real_args_t& a, int c, int64_t f) {
    ClipRealSpan s;
    s.t0 = a.clip_start[c]; s.t1 = a.clip_start[c + 1];
    s.t0 = s.t0 < 0 ? 0 : (s.t0 > f ? f : s.t0);
    s.t1 = s.t1 > a.num_frames ? a.num_frames : (s.t1 < f + 1 ? f + 1 : s.t1);
    s.dt = a.clip_dt[c];
    s.dz = a.fix_height ? clip_real_dz(a)[c] : 0.0;
    return s;
}

// ---- height fix: z of the lowest contact point in the clip's first frame ----
// what the FK of the first frame leaves per simulated body: wpos z and the third row of wmat
PHC_HD void clip_real_height_body(const phc_clip_real_args_t& a, int64_t f0, int j, double out[4]) {
    double wpos[3];
    Mat3d wmat;
    clip_real_fk(a, f0, clip_real_chain(a.parents, a.num_bodies + a.num_ext, j), 0.0, true, wpos, wmat);
    out[0] = wpos[2]; out[1] = wmat.m[6]; out[2] = wmat.m[7]; out[3] = wmat.m[8];
}
// contact point k: wpos_z + wmat[2, :] . contact_pos - radius (the body index comes from device memory: bounded to the simulated bodies)
PHC_HD double clip_real_contact_z(const phc_clip_real_args_t& a, const double* body4, int k) {
    int b = a.contact_body[k];
    b = b < 0 ? 0 : (b >= a.num_bodies ? a.num_bodies - 1 : b);
    const double* r = body4 + 4 * b;
    const double* p = a.contact_pos + 3 * k;
    return r[0] + (r[1] * p[0] + r[2] * p[1] + r[3] * p[2]) - a.contact_radius[k];
}
PHC_HD int64_t clip_real_first_frame(const phc_clip_real_args_t& a, int c) {
    const int64_t t = a.clip_start[c];
    return t < 0 ? 0 : (t > a.num_frames - 1 ? a.num_frames - 1 : t);
}

// ---- the bodies launch ----
// What one (frame, body) lane produces.  Bodies NB .. NB+E-1 (extended) have position and rotation only.
struct ClipRealBody {
    double gts[3];
    Quatd grs;
    double gav[3];       // raw angular velocity (0 in the clip's last frame)
    double dof_pos, dvs; // bodies 1 .. NB-1
};

PHC_HD double clip_real_row_sum(const double* pose, int J, int64_t f, int j) {
    const double* p = pose + (f * J + j) * 3;
    return p[0] + p[1] + p[2];
}

PHC_HD void clip_real_body(const phc_clip_real_args_t& a, int64_t f, int j, const ClipRealSpan& s, ClipRealBody& o) {
    const int NB = a.num_bodies, J = NB + a.num_ext;
    const uint64_t chain = clip_real_chain(a.parents, J, j);
    Mat3d wmat;
    clip_real_fk(a, f, chain, s.dz, true, o.gts, wmat);
    o.grs = clip_real_mat_to_quat(wmat);
    o.gav[0] = o.gav[1] = o.gav[2] = 0.0;
    o.dof_pos = o.dvs = 0.0;
    if (j >= NB) return;
    // _angular_velocity: axis * angle of g[t+1] * conj(g[t]) over dt; the lane walks its chain for frame f + 1 too
    if (f + 1 < s.t1) {
        double unused[3];
        Mat3d wnext;
        clip_real_fk(a, f + 1, chain, 0.0, false, unused, wnext);
        const Quatd dq = clip_pos_unit(clip_qmul(clip_real_mat_to_quat(wnext), clip_qconj(o.grs)));
        double c = 2.0 * (dq.w * dq.w) - 1.0;
        c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        const double ang = acos(c);
        const double n = sqrt(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z);
        const double d = n > 1e-9 ? n : 1e-9;
        o.gav[0] = dq.x / d * ang / s.dt; o.gav[1] = dq.y / d * ang / s.dt; o.gav[2] = dq.z / d * ang / s.dt;
    }
    if (j >= 1) {
        // dof_pos = pose.sum(-1); dvs = (dof_pos[t+1] - dof_pos[t]) / dt, the clip's last frame takes the difference T-3 -> T-2 (dv[-2:-1])
        o.dof_pos = clip_real_row_sum(a.pose_aa, J, f, j);
        int64_t ta = f + 1 < s.t1 ? f : s.t1 - 3;
        ta = ta < s.t0 ? s.t0 : ta;                       // (a clip has at least 3 frames: phc_amd/motion_lib.py refuses shorter ones)
        const int64_t tb = ta + 1 < s.t1 ? ta + 1 : ta;
        o.dvs = (clip_real_row_sum(a.pose_aa, J, tb, j) - clip_real_row_sum(a.pose_aa, J, ta, j)) / s.dt;
    }
}

// The bodies launch's stores for one lane: the fp32 fields into `rec` (one record; the kernel's is in LDS), the fp64 position and raw angular velocity of a
// simulated body into the frame's scratch row.
PHC_HD void clip_real_body_store(const ClipRealBody& o, int NB, int E, int j, float* rec, double* row) {
    const int J = NB + E;
    rec[3 * j + 0] = (float)o.gts[0]; rec[3 * j + 1] = (float)o.gts[1]; rec[3 * j + 2] = (float)o.gts[2];
    float* grs = rec + 3 * J + 4 * j;
    grs[0] = (float)o.grs.x; grs[1] = (float)o.grs.y; grs[2] = (float)o.grs.z; grs[3] = (float)o.grs.w;
    if (j >= NB) return;
    if (j >= 1) {
        rec[7 * J + 6 * NB + (j - 1)] = (float)o.dof_pos;
        rec[7 * J + 6 * NB + (NB - 1) + (j - 1)] = (float)o.dvs;
    }
    row[3 * j + 0] = o.gts[0]; row[3 * j + 1] = o.gts[1]; row[3 * j + 2] = o.gts[2];
    row[3 * NB + 3 * j + 0] = o.gav[0]; row[3 * NB + 3 * j + 1] = o.gav[1]; row[3 * NB + 3 * j + 2] = o.gav[2];
}

// The argument checks of phc_clip_process_real (host side; include/phc_amd.h lists them): 0, PHC_EINVAL or PHC_EUNSUPPORTED.  A function of its own so that
// the tests can ask it about arguments they must never hand to a launch.
inline int32_t clip_real_args_check(const phc_clip_real_args_t* a) {
    if (!a || !a->parents || !a->offsets || !a->rest_mat || !a->pose_aa || !a->trans || !a->clip_start || !a->clip_dt || !a->scratch || !a->frames) return PHC_EINVAL;
    if (a->num_clips < 1 || a->num_bodies < 1 || a->num_ext < 0) return PHC_EINVAL;
    if (a->fix_height && (a->num_contacts < 1 || !a->contact_body || !a->contact_pos || !a->contact_radius)) return PHC_EINVAL;
    if ((int64_t)a->num_bodies + a->num_ext > CLIP_MAX_BODIES) return PHC_EUNSUPPORTED;
    if (a->num_frames < 3 * (int64_t)a->num_clips) return PHC_EINVAL;   // (every clip has at least three frames)
    if (a->frame_stride != clip_real_stride(a->num_bodies, a->num_ext)) return PHC_EINVAL;
    // grid.x of the launches: U blocks, ceil(F / frames per block) tiles, ceil(6 NB F / 256) blocks of velocity lanes
    if (a->num_frames > ((int64_t)0x7fffffff * CLIP_BLOCK) / (6 * a->num_bodies)) return PHC_EUNSUPPORTED;
    if (a->num_frames > (int64_t)0x7fffffff * clip_real_frames_per_block(a->num_bodies, a->num_ext)) return PHC_EUNSUPPORTED;
    if (a->scratch_bytes < clip_real_scratch_bytes(a->num_frames, a->num_bodies, a->num_clips)) return PHC_EINVAL;
    if ((((uintptr_t)a->offsets | (uintptr_t)a->rest_mat | (uintptr_t)a->pose_aa | (uintptr_t)a->trans | (uintptr_t)a->clip_start | (uintptr_t)a->clip_dt |
          (uintptr_t)a->scratch) & 7) != 0)
        return PHC_EINVAL;
    if ((((uintptr_t)a->parents | (uintptr_t)a->frames) & 3) != 0) return PHC_EINVAL;
    if (a->fix_height && ((((uintptr_t)a->contact_pos | (uintptr_t)a->contact_radius) & 7) != 0 || ((uintptr_t)a->contact_body & 3) != 0)) return PHC_EINVAL;
    return 0;
}

}  // namespace phc
