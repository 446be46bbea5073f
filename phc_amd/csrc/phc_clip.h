// phc_clip.h -- per-lane pieces of the device clip processing (phc_clip_process, csrc/phc_clip.hip; contract: include/phc_amd.h): forward kinematics,
// finite-difference velocities and the gaussian filter of `process_clip` (phc_amd/motion_lib.py), restated operation by operation in fp64 -- the order of
// every sum and product is numpy's / scipy's, so the host build differs from `process_clip` by the math library's last bits only.
// PHC_HD: tests/clip_shim.cpp builds all of it for the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include "phc_math.h"
#include "../../include/phc_amd.h"

namespace phc {

constexpr int CLIP_MAX_BODIES = PHC_MAX_BODIES;   // the ancestor set of a body is one 64-bit word
constexpr int CLIP_RADIUS = 8;                    // gaussian_filter1d(sigma = 2): radius = int(4 sigma + 0.5)
constexpr int CLIP_BLOCK = 256;                   // threads per block of both launches
constexpr int CLIP_LDS_BYTES = 32 * 1024;         // record tile of the first launch: at most this much LDS per block

struct Quatd { double x, y, z, w; };
struct ClipWeights { double w[CLIP_RADIUS + 1]; };   // w[i] = weight of offset -(RADIUS - i) and of +(RADIUS - i); w[RADIUS] the centre

// the spherical record (abi.frame_stride_for(J, 0, 3)): gts 3J | grs 4J | gvs 3J | gavs 3J | lrs 4J | dvs 3(J-1) | pad to a multiple of 4
PHC_HD int clip_stride(int J) { return 20 * J; }   // 20 J - 3 floats of fields and 3 of padding
PHC_HD int clip_pad_begin(int J) { return 20 * J - 3; }
PHC_HD int clip_frames_per_block(int J) {
    const int n = CLIP_LDS_BYTES / (clip_stride(J) * 4 + 4);
    return n > 16 ? 16 : n;    // J = 24: 16 frames (30 KB); J = 64: 6 frames
}

// scratch: [F, 6J] f64 (per frame: the fp64 positions 3J, then the raw angular velocities 3J), then [F] i32 frame -> clip
PHC_HD int64_t clip_scratch_bytes(int64_t F, int J) { return F * 6 * J * 8 + (F * 4 + 7) / 8 * 8; }

// _q_mul: numpy evaluates each sum left to right
PHC_HD Quatd clip_qmul(const Quatd& a, const Quatd& b) {
    Quatd r;
    r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
    r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
    r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
    r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
    return r;
}
PHC_HD Quatd clip_qconj(const Quatd& a) { Quatd r; r.x = -a.x; r.y = -a.y; r.z = -a.z; r.w = a.w; return r; }

// _q_pos_unit
PHC_HD Quatd clip_pos_unit(Quatd q) {
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double n = sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    const double d = n > 1e-9 ? n : 1e-9;
    q.x /= d; q.y /= d; q.z /= d; q.w /= d;
    return q;
}

// _q_rot: v + w t + qv x t with t = 2 (qv x v)
PHC_HD void clip_qrot(const Quatd& q, const double v[3], double out[3]) {
    const double t0 = 2.0 * (q.y * v[2] - q.z * v[1]), t1 = 2.0 * (q.z * v[0] - q.x * v[2]), t2 = 2.0 * (q.x * v[1] - q.y * v[0]);
    out[0] = v[0] + q.w * t0 + (q.y * t2 - q.z * t1);
    out[1] = v[1] + q.w * t1 + (q.z * t0 - q.x * t2);
    out[2] = v[2] + q.w * t2 + (q.x * t1 - q.y * t0);
}

PHC_HD Quatd clip_load_quat(const double* quat, int64_t f, int J, int j) {
    const double* p = quat + (f * J + j) * 4;
    Quatd q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3];
    return q;
}

// lrs[f, j]: the root's given rotation, else pos_unit(conj(g[parent]) * g[j])
PHC_HD Quatd clip_local_rot(const double* quat, int64_t f, int J, int j, int p) {
    const Quatd g = clip_load_quat(quat, f, J, j);
    return p < 0 ? g : clip_pos_unit(clip_qmul(clip_qconj(clip_load_quat(quat, f, J, p)), g));
}

// _gaussian_kernel1d(sigma = 2, order 0, radius 8): exp(-x^2 / 8) over their sum, the sum in numpy's order for 17 contiguous doubles (eight running
// sums over the first sixteen, folded pairwise, then the last element)
PHC_HD ClipWeights clip_gauss_weights() {
    double phi[2 * CLIP_RADIUS + 1];
    for (int i = 0; i <= 2 * CLIP_RADIUS; ++i) {
        const double x = (double)(i - CLIP_RADIUS);
        phi[i] = exp(-0.125 * (x * x));
    }
    double r[8];
    for (int i = 0; i < 8; ++i) r[i] = phi[i] + phi[8 + i];
    const double sum = (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) + phi[16];
    ClipWeights w;
    for (int i = 0; i <= CLIP_RADIUS; ++i) w.w[i] = phi[i] / sum;
    return w;
}

// the clip that holds frame f: the last c with clip_start[c] <= f (clip_start is ascending, clip_start[0] = 0, clip_start[U] = F)
PHC_HD int clip_of_frame(const int64_t* clip_start, int num_clips, int64_t f) {
    int lo = 0, hi = num_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (clip_start[mid] <= f) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Clip c's frame range, tree and frame time.  The arrays are device memory filled by the caller: whatever they hold, the range stays inside [0, F) and
// around f, and the tree inside [0, num_trees).
struct ClipSpan { int64_t t0, t1; int tree; double dt; };
PHC_HD ClipSpan clip_span(const phc_clip_args_t& a, int c, int64_t f) {
    ClipSpan s;
    s.t0 = a.clip_start[c]; s.t1 = a.clip_start[c + 1];
    s.t0 = s.t0 < 0 ? 0 : (s.t0 > f ? f : s.t0);
    s.t1 = s.t1 > a.num_frames ? a.num_frames : (s.t1 < f + 1 ? f + 1 : s.t1);
    const int t = a.clip_tree[c];
    s.tree = t < 0 ? 0 : (t >= a.num_trees ? a.num_trees - 1 : t);
    s.dt = a.clip_dt[c];
    return s;
}

// What one (frame, body) lane of the first launch produces.
struct ClipBody {
    double gts[3];   // world position (FK with the normalised local rotations)
    Quatd grs;       // the given global rotation
    Quatd lrs;       // local rotation
    double gav[3];   // raw angular velocity (0 in the clip's last frame)
    double dvs[3];   // joint velocity (bodies with a parent; the clip's last frame repeats the one before)
};

// Frame f (of the clip with span s) of body j.  The lane walks its own ancestor chain from the root in index order -- parents
// precede their children, so that is the host's order -- and so needs nothing another lane computes.  Every index read from device memory is bounded:
// a parent outside [0, j) ends the walk, frames outside the clip are never read.
PHC_HD void clip_body(const phc_clip_args_t& a, int64_t f, int j, const ClipSpan& s, ClipBody& o) {
    const int J = a.num_bodies;
    const int64_t t0 = s.t0, t1 = s.t1;
    const int tree = s.tree;
    const double dt = s.dt;
    uint64_t chain = 0;
    for (int k = j, n = 0; n < J; ++n) {
        chain |= (uint64_t)1 << k;
        const int p = a.parents[k];
        if (p < 0 || p >= k) break;
        k = p;
    }
    const int par = a.parents[j];
    const int pj = (par >= 0 && par < j) ? par : -1;
    const double* lt = a.local_translation + (int64_t)tree * J * 3;
    Quatd g_prev = {0.0, 0.0, 0.0, 1.0}, grot = g_prev;
    double pos[3] = {0.0, 0.0, 0.0};
    bool first = true;
    while (chain) {
        const int k = __builtin_ctzll(chain);
        chain &= chain - 1;
        const Quatd g = clip_load_quat(a.quat, f, J, k);
        if (first) {
            grot = g;   // (the root's rotation is taken as given, not normalised)
            pos[0] = a.trans[f * 3 + 0]; pos[1] = a.trans[f * 3 + 1]; pos[2] = a.trans[f * 3 + 2];
            first = false;
        } else {
            const Quatd l = clip_pos_unit(clip_qmul(clip_qconj(g_prev), g));
            const double off[3] = {lt[k * 3 + 0], lt[k * 3 + 1], lt[k * 3 + 2]};
            double r[3];
            clip_qrot(grot, off, r);
            pos[0] = r[0] + pos[0]; pos[1] = r[1] + pos[1]; pos[2] = r[2] + pos[2];
            grot = clip_pos_unit(clip_qmul(grot, l));
        }
        g_prev = g;
    }
    o.gts[0] = pos[0]; o.gts[1] = pos[1]; o.gts[2] = pos[2];
    o.grs = g_prev;   // (the chain ends in j)
    o.lrs = clip_local_rot(a.quat, f, J, j, pj);
    // angular velocity: axis * angle of g[t+1] * conj(g[t]) over dt
    o.gav[0] = o.gav[1] = o.gav[2] = 0.0;
    if (f + 1 < t1) {
        const Quatd dq = clip_pos_unit(clip_qmul(clip_load_quat(a.quat, f + 1, J, j), clip_qconj(o.grs)));
        double c = 2.0 * (dq.w * dq.w) - 1.0;
        c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        const double ang = acos(c);
        const double n = sqrt(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z);
        const double d = n > 1e-9 ? n : 1e-9;
        o.gav[0] = dq.x / d * ang / dt; o.gav[1] = dq.y / d * ang / dt; o.gav[2] = dq.z / d * ang / dt;
    }
    // joint velocity: quat_to_angle_axis of conj(lrs[t]) * lrs[t+1] over dt
    o.dvs[0] = o.dvs[1] = o.dvs[2] = 0.0;
    if (t1 - t0 >= 2) {
        const int64_t ta = f + 1 < t1 ? f : f - 1;
        const Quatd la = ta == f ? o.lrs : clip_local_rot(a.quat, ta, J, j, pj);
        const Quatd lb = ta == f ? clip_local_rot(a.quat, ta + 1, J, j, pj) : o.lrs;
        const Quatd d = clip_qmul(clip_qconj(la), lb);
        const double s2 = 1.0 - d.w * d.w;
        const double sin_t = sqrt(s2 > 0.0 ? s2 : 0.0);
        const double wc = d.w < -1.0 ? -1.0 : (d.w > 1.0 ? 1.0 : d.w);
        double angle = 2.0 * acos(wc);
        angle = atan2(sin(angle), cos(angle));
        if (sin_t > 1e-5) {   // (otherwise: axis (0, 0, 1), angle 0)
            o.dvs[0] = d.x / sin_t * angle / dt; o.dvs[1] = d.y / sin_t * angle / dt; o.dvs[2] = d.z / sin_t * angle / dt;
        }
    }
}

// The first launch's stores for one lane: the fp32 fields into `rec` (one record; the kernel's is in LDS), the fp64 position and raw angular velocity
// into the frame's scratch row.
PHC_HD void clip_body_store(const ClipBody& o, int J, int j, float* rec, double* row) {
    rec[3 * j + 0] = (float)o.gts[0]; rec[3 * j + 1] = (float)o.gts[1]; rec[3 * j + 2] = (float)o.gts[2];
    float* grs = rec + 3 * J + 4 * j;
    grs[0] = (float)o.grs.x; grs[1] = (float)o.grs.y; grs[2] = (float)o.grs.z; grs[3] = (float)o.grs.w;
    float* lrs = rec + 13 * J + 4 * j;
    lrs[0] = (float)o.lrs.x; lrs[1] = (float)o.lrs.y; lrs[2] = (float)o.lrs.z; lrs[3] = (float)o.lrs.w;
    if (j > 0) {
        float* dvs = rec + 17 * J + 3 * (j - 1);
        dvs[0] = (float)o.dvs[0]; dvs[1] = (float)o.dvs[1]; dvs[2] = (float)o.dvs[2];
    }
    row[3 * j + 0] = o.gts[0]; row[3 * j + 1] = o.gts[1]; row[3 * j + 2] = o.gts[2];
    row[3 * J + 3 * j + 0] = o.gav[0]; row[3 * J + 3 * j + 1] = o.gav[1]; row[3 * J + 3 * j + 2] = o.gav[2];
}

// The unfiltered velocity column r (0 .. 3J-1 linear: np.gradient(gts) / dt; 3J .. 6J-1 angular) at frame t of the clip [t0, t1).
PHC_HD double clip_raw_velocity(const double* scratch, int J, int r, int64_t t, int64_t t0, int64_t t1, double dt) {
    if (r >= 3 * J) return scratch[t * 6 * J + r];
    if (t1 - t0 < 2) return 0.0;
    const int64_t lo = t > t0 ? t - 1 : t, hi = t + 1 < t1 ? t + 1 : t;
    double g = scratch[hi * 6 * J + r] - scratch[lo * 6 * J + r];
    if (hi - lo == 2) g = g / 2.0;
    return g / dt;
}

// gaussian_filter1d(raw, 2, mode="nearest") at frame t: scipy's correlate1d for symmetric weights -- the centre first, then the pairs from the outermost
// inwards; `nearest` clamps the index to the clip's own first and last frame.
PHC_HD double clip_filtered_velocity(const double* scratch, const ClipWeights& w, int J, int r, int64_t t, int64_t t0, int64_t t1, double dt) {
    double acc = clip_raw_velocity(scratch, J, r, t, t0, t1, dt) * w.w[CLIP_RADIUS];
    for (int i = 0; i < CLIP_RADIUS; ++i) {
        const int64_t off = CLIP_RADIUS - i;
        const int64_t ta = t - off < t0 ? t0 : t - off, tb = t + off > t1 - 1 ? t1 - 1 : t + off;
        acc += (clip_raw_velocity(scratch, J, r, ta, t0, t1, dt) + clip_raw_velocity(scratch, J, r, tb, t0, t1, dt)) * w.w[i];
    }
    return acc;
}

// The argument checks of phc_clip_process (host side; include/phc_amd.h lists them): 0, PHC_EINVAL or PHC_EUNSUPPORTED.  A function of its own so that
// the tests can ask it about arguments they must never hand to a launch.
inline int32_t clip_args_check(const phc_clip_args_t* a) {
    if (!a || !a->parents || !a->local_translation || !a->clip_tree || !a->clip_start || !a->clip_dt || !a->quat || !a->trans || !a->scratch || !a->frames)
        return PHC_EINVAL;
    if (a->num_clips < 1 || a->num_bodies < 1 || a->num_trees < 1) return PHC_EINVAL;
    if (a->num_bodies > CLIP_MAX_BODIES) return PHC_EUNSUPPORTED;
    if (a->num_frames < 2 * (int64_t)a->num_clips) return PHC_EINVAL;   // (every clip has at least two frames)
    if (a->frame_stride != clip_stride(a->num_bodies)) return PHC_EINVAL;
    // grid.x of the two launches: ceil(F / frames per block) tiles, ceil(6 J F / 256) blocks of velocity lanes
    if (a->num_frames > ((int64_t)0x7fffffff * CLIP_BLOCK) / (6 * a->num_bodies)) return PHC_EUNSUPPORTED;
    if (a->num_frames > (int64_t)0x7fffffff * clip_frames_per_block(a->num_bodies)) return PHC_EUNSUPPORTED;
    if (a->scratch_bytes < clip_scratch_bytes(a->num_frames, a->num_bodies)) return PHC_EINVAL;
    if ((((uintptr_t)a->local_translation | (uintptr_t)a->clip_start | (uintptr_t)a->clip_dt | (uintptr_t)a->quat | (uintptr_t)a->trans | (uintptr_t)a->scratch) & 7) != 0)
        return PHC_EINVAL;
    if ((((uintptr_t)a->parents | (uintptr_t)a->clip_tree | (uintptr_t)a->frames) & 3) != 0) return PHC_EINVAL;
    return 0;
}

}  // namespace phc
