// phc_fit.h -- per-lane pieces of the device retargeting fit (phc_fit_iterate, csrc/phc_fit.hip; contract: include/phc_amd.h): one trip of the loop of
// `fit_clip` (phc_amd/utils/fit_robot_motion.py) -- forward kinematics, the L1 keypoint loss with its analytic gradient, Adam, the clamp and the 5-tap
// gaussian -- in fp32, stated once for the kernels and for the host build.
// PHC_HD: tests/fit_shim.cpp builds all of it for the CPU and loops over the lanes in the kernels' order.
//
// A frame's group runs three stages with a barrier between them; what crosses lanes goes through two small arrays (LDS in the kernel):
//   A  lane b (one per body): its own ancestor chain from the root -> world position p_b and the body's rotation in its parent's frame L_b (both published),
//      and its world rotation R_b;
//   B  lane m (one per matched entry): u_m = (p - g) / |p - g| (published), |p - g|;
//   C  lane j: the gradient of its own parameter from the published (p, L, u), Adam and the clamp; the group's butterfly sums u, |p - g| and dof^2.
// A joint's lever arms are built in the joint's own frame by walking from the matched body up to the joint (d <- offset_k + L_k d), not as differences of
// world positions: a matched body that sits on the joint's axis then gives an exact 0, as autograd's product with the offset's zero components does, where a
// difference of world positions leaves ~1e-11 of rounding -- which Adam's division by sqrt(v) + 1e-8 would turn into a drift of 1e-5 rad per step.
#pragma once
#include <math.h>
#include <stdint.h>
#include "phc_math.h"
#include "../../include/phc_amd.h"

namespace phc {

constexpr int FIT_BLOCK = 256;                      // threads per block of every launch
constexpr int FIT_MAX_BODIES = PHC_MAX_BODIES;      // the ancestor set of a body is one 64-bit word
constexpr int FIT_MAX_MATCHED = PHC_FIT_MAX_MATCHED;// the matched entries of a joint's subtree are one 32-bit word
constexpr int FIT_SUMS = 5;                         // per frame / tile / clip: sum_m u (3), sum_m |p - g|, sum_j dof^2
constexpr int FIT_TAPS = 5;

PHC_HD int fit_group(int nbe) { return nbe > 32 ? 64 : 32; }                    // lanes per frame
PHC_HD int fit_tile_frames(int nbe) { return FIT_BLOCK / fit_group(nbe); }      // frames per tile: 8 or 4
PHC_HD int64_t fit_max_tiles(int64_t F, int C, int nbe) { return F / fit_tile_frames(nbe) + C; }   // sum_c ceil(T_c / TF) <= F / TF + C
PHC_HD int64_t fit_align16(int64_t n) { return (n + 15) / 16 * 16; }

// scratch: tile_start [C + 1] i32 | coef [C, 2] f32 | partial [max tiles, 5] f32 | clamped [F, NB + E] f32 (rows of ND floats are used)
struct FitScratch { int32_t* tile_start; float* coef; float* partial; float* clamped; };
PHC_HD int64_t fit_scratch_bytes(int64_t F, int C, int nbe) {
    return fit_align16(((int64_t)C + 1) * 4) + fit_align16((int64_t)C * 8) + fit_align16(fit_max_tiles(F, C, nbe) * FIT_SUMS * 4) + fit_align16(F * nbe * 4);
}
PHC_HD FitScratch fit_scratch(const phc_fit_args_t& a) {
    const int nbe = a.num_bodies + a.num_ext;
    char* p = (char*)a.scratch;
    FitScratch s;
    s.tile_start = (int32_t*)p; p += fit_align16(((int64_t)a.num_clips + 1) * 4);
    s.coef = (float*)p;         p += fit_align16((int64_t)a.num_clips * 8);
    s.partial = (float*)p;      p += fit_align16(fit_max_tiles(a.num_frames, a.num_clips, nbe) * FIT_SUMS * 4);
    s.clamped = (float*)p;
    return s;
}

// Clip c's frames, bounded whatever the device array holds: 0 <= t0 <= t1 <= F.
struct FitSpan { int64_t t0, t1; };
PHC_HD FitSpan fit_span(const phc_fit_args_t& a, int c) {
    FitSpan s;
    s.t0 = a.clip_start[c]; s.t1 = a.clip_start[c + 1];
    s.t0 = s.t0 < 0 ? 0 : (s.t0 > a.num_frames ? a.num_frames : s.t0);
    s.t1 = s.t1 < s.t0 ? s.t0 : (s.t1 > a.num_frames ? a.num_frames : s.t1);
    return s;
}
PHC_HD int32_t fit_clip_tiles(const FitSpan& s, int tf) { return (int32_t)((s.t1 - s.t0 + tf - 1) / tf); }

// the clip that holds tile `tile`: the last c with tile_start[c] <= tile (ascending; tile_start[0] = 0), or -1 past the last tile
PHC_HD int fit_clip_of_tile(const int32_t* tile_start, int num_clips, int32_t tile) {
    if (tile >= tile_start[num_clips]) return -1;
    int lo = 0, hi = num_clips - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tile_start[mid] <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// torch.optim.Adam's two scalars of step k (python floats there: fp64), as the fp32 operands of its tensor statements
struct FitCoef { float step_size, bc2_sqrt; };
PHC_HD FitCoef fit_coef(double lr, int32_t k) {
    FitCoef c;
    c.step_size = (float)(lr / (1.0 - pow(0.9, (double)k)));
    c.bc2_sqrt = (float)sqrt(1.0 - pow(0.999, (double)k));
    return c;
}

// exp_avg.lerp_(g, 1 - b1); exp_avg_sq.mul_(b2).addcmul_(g, g, value = 1 - b2); denom = sqrt(v) / bc2_sqrt + eps; p.addcdiv_(m, denom, value = -step_size)
PHC_HD float fit_adam(float p, float g, float* m, float* v, const FitCoef& c) {
    const float mn = *m + (float)(1.0 - 0.9) * (g - *m);
    const float vn = *v * 0.999f + (float)(1.0 - 0.999) * g * g;
    *m = mn; *v = vn;
    const float denom = sqrtf(vn) / c.bc2_sqrt + 1e-8f;
    return p + (-c.step_size) * (mn / denom);
}

// The coefficients of the exponential map at rotation vector r, t = |r|: A = sin t / t, B = (1 - cos t) / t^2 (as 2 sin^2(t / 2) / t^2: the difference
// 1 - cos t has no correct bit left in fp32 below t ~ 3e-4, and B carries the first-order term of the Jacobian), C = (t - sin t) / t^3;
// for t^2 < 1e-8 their series (_aa_to_mat's branch): A = 1 - t^2 / 6, B = 1 / 2 - t^2 / 24, C = 1 / 6 - t^2 / 120.
struct FitExp { float A, B, C; };
PHC_HD FitExp fit_exp_coef(const float r[3], bool want_c) {
    const float t2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    FitExp e;
    if (t2 < 1e-8f) {
        e.A = 1.0f - t2 / 6.0f; e.B = 0.5f - t2 / 24.0f; e.C = 1.0f / 6.0f - t2 / 120.0f;
    } else {
        const float t = sqrtf(t2), sn = sinf(t), sh = sinf(0.5f * t);
        e.A = sn / t; e.B = 2.0f * (sh * sh) / t2; e.C = want_c ? (t - sn) / (t2 * t) : 0.0f;
    }
    return e;
}

// Rodrigues: R = I + A [r]x + B [r]x^2, row-major
PHC_HD void fit_rodrigues(const float r[3], float R[9]) {
    const FitExp e = fit_exp_coef(r, false);
    const float x = r[0], y = r[1], z = r[2];
    R[0] = 1.0f - e.B * (y * y + z * z); R[1] = e.B * (x * y) - e.A * z;       R[2] = e.B * (x * z) + e.A * y;
    R[3] = e.B * (x * y) + e.A * z;       R[4] = 1.0f - e.B * (x * x + z * z); R[5] = e.B * (y * z) - e.A * x;
    R[6] = e.B * (x * z) - e.A * y;       R[7] = e.B * (y * z) + e.A * x;       R[8] = 1.0f - e.B * (x * x + y * y);
}
PHC_HD void fit_matmul(const float a[9], const float b[9], float o[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
PHC_HD void fit_matvec(const float a[9], const float v[3], float o[3]) {
    for (int i = 0; i < 3; ++i) o[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
}
PHC_HD void fit_cross(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// Stage A.  Frame f of clip c, body b: world position, world rotation R and the rotation in the parent's frame L = rest_b Rodrigues(axis_b dof_b) (rest_b for
// an extended body, which does not rotate; the root's L is not used).  The lane walks its ancestor chain from the root in index order, as clip_body does; a
// parent outside [0, k) ends the walk.
PHC_HD void fit_body(const phc_fit_args_t& a, int64_t f, int c, int b, float pos[3], float R[9], float L[9]) {
    const int NB = a.num_bodies, NBE = a.num_bodies + a.num_ext, ND = NB - 1;
    uint64_t chain = 0;
    for (int k = b, n = 0; n < NBE; ++n) {
        chain |= (uint64_t)1 << k;
        const int p = a.parents[k];
        if (p < 0 || p >= k) break;
        k = p;
    }
    for (int i = 0; i < 9; ++i) R[i] = L[i] = (i % 4 == 0) ? 1.f : 0.f;
    pos[0] = pos[1] = pos[2] = 0.f;
    bool first = true;
    while (chain) {
        const int k = __builtin_ctzll(chain);
        chain &= chain - 1;
        if (first) {
            const float r[3] = {a.root_rot[f * 3 + 0], a.root_rot[f * 3 + 1], a.root_rot[f * 3 + 2]};
            fit_rodrigues(r, R);
            for (int i = 0; i < 3; ++i) pos[i] = a.root_trans_offset[f * 3 + i] + a.root_off[(int64_t)c * 3 + i];
            first = false;
            continue;
        }
        const float off[3] = {a.offsets[k * 3 + 0], a.offsets[k * 3 + 1], a.offsets[k * 3 + 2]};
        float ro[3];
        fit_matvec(R, off, ro);
        for (int i = 0; i < 3; ++i) pos[i] = ro[i] + pos[i];
        float Rn[9];
        for (int i = 0; i < 9; ++i) L[i] = a.rest[k * 9 + i];
        if (k < NB) {
            const float q = a.dof[f * ND + (k - 1)];
            const float aa[3] = {a.axis[(k - 1) * 3 + 0] * q, a.axis[(k - 1) * 3 + 1] * q, a.axis[(k - 1) * 3 + 2] * q};
            float Rj[9], rest[9];
            for (int i = 0; i < 9; ++i) rest[i] = L[i];
            fit_rodrigues(aa, Rj);
            fit_matmul(rest, Rj, L);
        }
        fit_matmul(R, L, Rn);
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
    }
}

PHC_HD int fit_clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// Stage B.  Matched entry m of frame f: u = (p - g) / |p - g| (0 where the residual is exactly 0: torch's norm backward), n = |p - g|.
// `frame_pos`: the frame's published positions [NB + E, 3].
PHC_HD void fit_residual(const phc_fit_args_t& a, int64_t f, int m, const float* frame_pos, float u[3], float* n) {
    const int M = a.num_matched;
    const int mb = fit_clampi(a.match_body[m], a.num_bodies + a.num_ext), slot = fit_clampi(a.match_slot[m], M);
    const float* g = a.target + (f * M + slot) * 3;
    const float r[3] = {frame_pos[mb * 3 + 0] - g[0], frame_pos[mb * 3 + 1] - g[1], frame_pos[mb * 3 + 2] - g[2]};
    const float d = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    *n = d;
    for (int i = 0; i < 3; ++i) u[i] = d > 0.f ? r[i] / d : 0.f;
}

// Stage C, the sum the root lane owns: sum over the matched entries of `mask`, in entry order, of (p_m - p) x u_m in the world.
// `frame_u`: the frame's published u [M, 3].
PHC_HD void fit_torque(const phc_fit_args_t& a, uint32_t mask, const float p[3], const float* frame_pos, const float* frame_u, float tau[3]) {
    tau[0] = tau[1] = tau[2] = 0.f;
    while (mask) {
        const int m = __builtin_ctz(mask);
        mask &= mask - 1;
        const int mb = fit_clampi(a.match_body[m], a.num_bodies + a.num_ext);
        const float d[3] = {frame_pos[mb * 3 + 0] - p[0], frame_pos[mb * 3 + 1] - p[1], frame_pos[mb * 3 + 2] - p[2]};
        float x[3];
        fit_cross(d, frame_u + m * 3, x);
        tau[0] += x[0]; tau[1] += x[1]; tau[2] += x[2];
    }
}
PHC_HD uint32_t fit_all_matched(int M) { return M >= 32 ? 0xffffffffu : ((1u << M) - 1u); }

// Stage C, the sum joint lane j owns, in the joint's own frame: sum over the matched entries of `mask`, in entry order, of d x (R_j^T u_m), d the way from
// the joint's origin to the matched body: from the body up to the joint, d <- offset_k + L_k d.  `frame_L`: the frame's published L [NB + E, 9].
PHC_HD void fit_joint_torque(const phc_fit_args_t& a, uint32_t mask, int j, const float R[9], const float* frame_L, const float* frame_u, float tau[3]) {
    const int NBE = a.num_bodies + a.num_ext;
    tau[0] = tau[1] = tau[2] = 0.f;
    while (mask) {
        const int m = __builtin_ctz(mask);
        mask &= mask - 1;
        float d[3] = {0.f, 0.f, 0.f};
        for (int k = fit_clampi(a.match_body[m], NBE), n = 0; n < NBE && k > j; ++n) {
            float ld[3];
            fit_matvec(frame_L + k * 9, d, ld);
            for (int i = 0; i < 3; ++i) d[i] = a.offsets[k * 3 + i] + ld[i];
            const int p = a.parents[k];
            if (p < 0 || p >= k) break;
            k = p;
        }
        const float* u = frame_u + m * 3;
        const float ul[3] = {R[0] * u[0] + R[3] * u[1] + R[6] * u[2], R[1] * u[0] + R[4] * u[1] + R[7] * u[2], R[2] * u[0] + R[5] * u[1] + R[8] * u[2]};
        float x[3];
        fit_cross(d, ul, x);
        tau[0] += x[0]; tau[1] += x[1]; tau[2] += x[2];
    }
}

// Stage C for joint lane j (1 <= j < NB) of frame f in a clip of T frames: gradient (the joint's axis is the same in its own frame before and after its own
// rotation), Adam, clamp; the clamped angle goes to the scratch row (the smoothing reads it in the next launch).  Returns dof^2 (the regulariser's term of
// the loss, at the angle the trip started from).
PHC_HD float fit_joint_step(const phc_fit_args_t& a, int64_t f, int j, int64_t T, const FitCoef& co, const float R[9], const float* frame_L,
                            const float* frame_u, float* clamped) {
    const int ND = a.num_bodies - 1, M = a.num_matched;
    float tau[3];
    fit_joint_torque(a, a.subtree[j] & fit_all_matched(M), j, R, frame_L, frame_u, tau);
    const float* ax = a.axis + (j - 1) * 3;
    const int64_t i = f * ND + (j - 1);
    const float q = a.dof[i];
    const float g = (ax[0] * tau[0] + ax[1] * tau[1] + ax[2] * tau[2]) / (float)(T * M) + (0.02f * q) / (float)(T * ND);
    float qn = fit_adam(q, g, a.dof_m + i, a.dof_v + i, co);
    const float lo = a.range[(j - 1) * 2 + 0], hi = a.range[(j - 1) * 2 + 1];
    qn = qn < lo ? lo : qn;
    qn = qn > hi ? hi : qn;
    clamped[i] = qn;
    return q * q;
}

// Stage C for the root lane: d loss / d r = J_l(r)^T tau / (T M) with tau = sum_m (p_m - p_root) x u_m and J_l^T = I - B [r]x + C [r]x^2; Adam.
PHC_HD void fit_root_step(const phc_fit_args_t& a, int64_t f, int64_t T, const FitCoef& co, const float p[3], const float* frame_pos, const float* frame_u) {
    const int M = a.num_matched;
    float tau[3], rt[3], rrt[3];
    fit_torque(a, fit_all_matched(M), p, frame_pos, frame_u, tau);
    const float r[3] = {a.root_rot[f * 3 + 0], a.root_rot[f * 3 + 1], a.root_rot[f * 3 + 2]};
    const FitExp e = fit_exp_coef(r, true);
    fit_cross(r, tau, rt);
    fit_cross(r, rt, rrt);
    for (int i = 0; i < 3; ++i) {
        const float g = (tau[i] - e.B * rt[i] + e.C * rrt[i]) / (float)(T * M);
        a.root_rot[f * 3 + i] = fit_adam(r[i], g, a.root_rot_m + f * 3 + i, a.root_rot_v + f * 3 + i, co);
    }
}

// The normalised 5-tap gaussian (sigma 0.75), offsets -2 .. 2
struct FitTaps { float w[FIT_TAPS]; };
inline FitTaps fit_taps() {
    double k[FIT_TAPS], s = 0.0;
    for (int i = 0; i < FIT_TAPS; ++i) { const double x = (i - FIT_TAPS / 2) / 0.75; k[i] = exp(-0.5 * x * x); s += k[i]; }
    FitTaps t;
    for (int i = 0; i < FIT_TAPS; ++i) t.w[i] = (float)(k[i] / s);
    return t;
}
// Step 5 for (frame t, joint d) of the clip [t0, t1): replicate padding clamps the index to the clip's own first and last frame.
PHC_HD float fit_smooth(const float* clamped, const FitTaps& w, int ND, int d, int64_t t, int64_t t0, int64_t t1) {
    float acc = 0.f;
    for (int i = 0; i < FIT_TAPS; ++i) {
        int64_t s = t + i - FIT_TAPS / 2;
        s = s < t0 ? t0 : (s > t1 - 1 ? t1 - 1 : s);
        acc += w.w[i] * clamped[s * ND + d];
    }
    return acc;
}

// The second launch's lane for clip c, component i (0 .. 2: root_off's Adam step; 3: the loss): the clip's tile partials added in tile order.
PHC_HD float fit_clip_sum(const float* partial, int32_t tile0, int32_t tiles, int64_t num_tiles, int i) {
    float s = 0.f;
    if (tile0 < 0) return s;   // (a table from a clip_start that breaks the contract: nothing outside `partial` is read)
    for (int32_t k = 0; k < tiles && (int64_t)tile0 + k < num_tiles; ++k) s += partial[((int64_t)tile0 + k) * FIT_SUMS + i];
    return s;
}
PHC_HD void fit_clip_lane(const phc_fit_args_t& a, const FitScratch& s, int c, int i, int64_t num_tiles) {
    const FitSpan sp = fit_span(a, c);
    const int64_t T = sp.t1 - sp.t0;
    if (T < 1) return;
    const int tf = fit_tile_frames(a.num_bodies + a.num_ext), M = a.num_matched, ND = a.num_bodies - 1;
    const int32_t tile0 = s.tile_start[c], tiles = fit_clip_tiles(sp, tf);
    if (i < 3) {
        const FitCoef co = {s.coef[c * 2 + 0], s.coef[c * 2 + 1]};
        const float g = fit_clip_sum(s.partial, tile0, tiles, num_tiles, i) / (float)(T * M);
        const int64_t k = (int64_t)c * 3 + i;
        a.root_off[k] = fit_adam(a.root_off[k], g, a.root_off_m + k, a.root_off_v + k, co);
    } else {
        const float n = fit_clip_sum(s.partial, tile0, tiles, num_tiles, 3), q = fit_clip_sum(s.partial, tile0, tiles, num_tiles, 4);
        a.loss[c] = n / (float)(T * M) + (ND > 0 ? 0.01f * (q / (float)(T * ND)) : 0.f);
    }
}
// ... and, after the four lanes above, the clip's step counter and the scalars of its next step
PHC_HD void fit_clip_advance(const phc_fit_args_t& a, const FitScratch& s, int c) {
    const int32_t k = a.step[c] + 1;
    a.step[c] = k;
    const FitCoef co = fit_coef(a.lr, k + 1);
    s.coef[c * 2 + 0] = co.step_size; s.coef[c * 2 + 1] = co.bc2_sqrt;
}

// group_sum (phc_group.h) on the host: the butterfly's partners are lane ^ 1, ^ 2, ^ 7 (row_half_mirror), ^ 15 (row_mirror), ^ 16, ^ 32; every lane ends
// with the same bits (an addition commutes), so lane 0's value stands for the group.
inline float fit_group_sum_host(const float* lanes, int G) {
    float v[64], w[64];
    for (int i = 0; i < G; ++i) v[i] = lanes[i];
    const int masks[6] = {1, 2, 7, 15, 16, 32};
    for (int s = 0; s < 6 && (s < 4 || masks[s] < G); ++s) {
        for (int i = 0; i < G; ++i) w[i] = v[i] + v[i ^ masks[s]];
        for (int i = 0; i < G; ++i) v[i] = w[i];
    }
    return v[0];
}

// The argument checks of phc_fit_iterate (host side; include/phc_amd.h lists them): 0, PHC_EINVAL or PHC_EUNSUPPORTED.  A function of its own so that the
// tests can ask it about arguments they must never hand to a launch.  *tiles_out: the grid of the two per-trip launches.
inline int32_t check_fit(const phc_fit_args_t* a, int32_t iterations, int64_t* tiles_out) {
    if (!a || iterations < 0) return PHC_EINVAL;
    const void* ptrs[] = {a->parents, a->offsets, a->rest, a->axis, a->range, a->match_body, a->match_slot, a->subtree, a->clip_start, a->clip_start_host,
                          a->target, a->root_trans_offset, a->dof, a->dof_m, a->dof_v, a->root_rot, a->root_rot_m, a->root_rot_v, a->root_off, a->root_off_m,
                          a->root_off_v, a->step, a->loss, a->scratch};
    uintptr_t bits = 0;
    for (const void* p : ptrs) {
        if (!p) return PHC_EINVAL;
        bits |= (uintptr_t)p;
    }
    if (a->num_clips < 1 || a->num_bodies < 1 || a->num_ext < 0 || a->num_matched < 1 || a->num_frames < 1) return PHC_EINVAL;
    if ((int64_t)a->num_bodies + a->num_ext > FIT_MAX_BODIES) return PHC_EUNSUPPORTED;
    if (a->num_matched > FIT_MAX_MATCHED) return PHC_EUNSUPPORTED;
    if (!(a->lr == a->lr)) return PHC_EINVAL;
    if ((bits & 3) != 0 || (((uintptr_t)a->clip_start | (uintptr_t)a->clip_start_host) & 7) != 0 || ((uintptr_t)a->scratch & 15) != 0) return PHC_EINVAL;
    const int nbe = a->num_bodies + a->num_ext, tf = fit_tile_frames(nbe);
    if (a->clip_start_host[0] != 0 || a->clip_start_host[a->num_clips] != a->num_frames) return PHC_EINVAL;
    int64_t tiles = 0;
    for (int c = 0; c < a->num_clips; ++c) {
        const int64_t T = a->clip_start_host[c + 1] - a->clip_start_host[c];
        if (T < 1 || a->clip_start_host[c + 1] > a->num_frames) return PHC_EINVAL;
        tiles += (T + tf - 1) / tf;
    }
    if (tiles > 0x7fffffff) return PHC_EUNSUPPORTED;
    if (a->scratch_bytes < fit_scratch_bytes(a->num_frames, a->num_clips, nbe)) return PHC_EINVAL;
    if (tiles_out) *tiles_out = tiles;
    return 0;
}

}  // namespace phc
