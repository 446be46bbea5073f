// phc_fit_sph.hip -- phc_fit_sph_iterate: trips of the spherical-joint keypoint fit (phc_amd/utils/fit_keypoints.py) for concatenated clips (contract:
// include/phc_amd.h; per-lane code: phc_fit_sph.h over phc_fit.h).  fp32, built with -ffp-contract=off and without fast-math.
//
// k_fit_setup (phc_fit.hip, once per call): the tile table and Adam's two scalars of every clip's next step.
// k_fit_sph_frames (per trip): a block is one tile of 8 frames, a group of 32 lanes one frame, a lane one body.  Stage A1: the lane's own exponential ->
// its rotation in the parent's frame into LDS (one sin / cos pair per lane; the chain walk then multiplies published matrices, where an exponential per
// ancestor would cost up to nine per lane on the SMPL tree).  Stage A2: the ancestor chain -> world position into LDS.  Stage B: lane m -> u_m into LDS.
// Stage C: lane 0 the root rotation vector's step, lane j joint j's three components: gradient, Adam, clamp into the scratch row.  The frame's sums are
// butterflies over the group; five lanes add the tile's frames in order and store the tile's partial.
// k_fit_sph_finish (per trip): a block is one tile again: the 5-tap filter over the 3 (NB - 1) columns from the scratch rows into dof; the block of a clip's
// first tile also adds the clip's partials in tile order (root_off's Adam step, the loss) and advances the clip's step.
// Nothing is exchanged between blocks inside a launch; no atomics.
#include <hip/hip_runtime.h>
#include "phc_fit_sph.h"
#include "phc_group.h"

using namespace phc;

namespace phc {
hipError_t fit_launch_setup(const phc_fit_args_t& a, int tf, hipStream_t st);   // phc_fit.hip
}

constexpr int SPH_G = 32, SPH_TF = FIT_BLOCK / SPH_G;

__global__ __launch_bounds__(FIT_BLOCK) void k_fit_sph_frames(phc_fit_args_t a) {
    __shared__ float s_pos[SPH_TF][SPH_G * 3];          // (lane strides of 3 and 9 floats: no bank conflict)
    __shared__ float s_L[SPH_TF][SPH_G * 9];
    __shared__ float s_u[SPH_TF][FIT_MAX_MATCHED * 3];
    __shared__ float s_sum[SPH_TF][FIT_SUMS];
    const FitScratch s = fit_scratch(a);
    const int32_t tile = (int32_t)blockIdx.x;
    const int c = fit_clip_of_tile(s.tile_start, a.num_clips, tile);
    if (c < 0) return;                                  // (the whole block)
    const FitSpan sp = fit_span(a, c);
    const int fl = (int)threadIdx.x / SPH_G, b = (int)threadIdx.x % SPH_G;
    const int NB = a.num_bodies;
    const int64_t f = sp.t0 + ((int64_t)(tile - s.tile_start[c]) * SPH_TF + fl), T = sp.t1 - sp.t0;
    const bool live = f >= sp.t0 && f < sp.t1;
    float pos[3] = {0.f, 0.f, 0.f}, R[9];
    if (live && b < NB) {
        float L[9];
        fit_sph_local(a, f, b, L);
#pragma unroll
        for (int i = 0; i < 9; ++i) s_L[fl][b * 9 + i] = L[i];
    }
    __syncthreads();
    if (live && b < NB) {
        fit_sph_chain(a, f, c, b, s_L[fl], pos, R);
        s_pos[fl][b * 3 + 0] = pos[0]; s_pos[fl][b * 3 + 1] = pos[1]; s_pos[fl][b * 3 + 2] = pos[2];
    }
    __syncthreads();
    float v[FIT_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (live && b < a.num_matched) {
        fit_residual(a, f, b, s_pos[fl], v, &v[3]);
        s_u[fl][b * 3 + 0] = v[0]; s_u[fl][b * 3 + 1] = v[1]; s_u[fl][b * 3 + 2] = v[2];
    }
    __syncthreads();
    if (live) {
        const FitCoef co = {s.coef[c * 2 + 0], s.coef[c * 2 + 1]};
        if (b == 0) fit_root_step(a, f, T, co, pos, s_pos[fl], s_u[fl]);
        else if (b < NB) v[4] = fit_sph_joint_step(a, f, b, T, co, R, s_L[fl], s_u[fl], s.clamped);
    }
#pragma unroll
    for (int i = 0; i < FIT_SUMS; ++i) {
        v[i] = group_sum<SPH_G>(v[i]);
        if (b == 0) s_sum[fl][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < FIT_SUMS) {
        float acc = 0.f;
        for (int k = 0; k < SPH_TF; ++k) acc += s_sum[k][threadIdx.x];
        s.partial[(int64_t)tile * FIT_SUMS + threadIdx.x] = acc;
    }
}

__global__ __launch_bounds__(FIT_BLOCK) void k_fit_sph_finish(phc_fit_args_t a, FitTaps w, int64_t num_tiles) {
    const FitScratch s = fit_scratch(a);
    const int32_t tile = (int32_t)blockIdx.x;
    const int c = fit_clip_of_tile(s.tile_start, a.num_clips, tile);
    if (c < 0) return;
    const FitSpan sp = fit_span(a, c);
    const int ND = fit_sph_nd(a.num_bodies);
    const int32_t first = s.tile_start[c];
    const int64_t t_lo = sp.t0 + (int64_t)(tile - first) * SPH_TF;
    int64_t nf = sp.t1 - t_lo;
    nf = t_lo < sp.t0 ? 0 : (nf > SPH_TF ? SPH_TF : nf);
    for (int i = (int)threadIdx.x; i < (int)nf * ND; i += FIT_BLOCK) {
        const int fl = i / ND, d = i - fl * ND;
        a.dof[(t_lo + fl) * ND + d] = fit_smooth(s.clamped, w, ND, d, t_lo + fl, sp.t0, sp.t1);
    }
    if (tile == first) {
        if (threadIdx.x < 4) fit_sph_clip_lane(a, s, c, (int)threadIdx.x, num_tiles);
        __syncthreads();
        if (threadIdx.x == 0) fit_clip_advance(a, s, c);
    }
}

extern "C" int64_t phc_fit_sph_scratch_bytes(int64_t num_frames, int32_t num_clips, int32_t num_bodies) {
    if (num_frames < 0 || num_clips < 1 || num_bodies < 1 || num_bodies > FIT_SPH_MAX_BODIES) return PHC_EINVAL;
    return fit_sph_scratch_bytes(num_frames, num_clips, num_bodies);
}

extern "C" int32_t phc_fit_sph_iterate(const phc_fit_args_t* a, int32_t iterations, void* stream) {
    int64_t tiles = 0;
    const int32_t rc = check_fit_sph(a, iterations, &tiles);
    if (rc) return rc;
    if (iterations == 0) return 0;
    const FitTaps w = fit_taps();
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = fit_launch_setup(*a, SPH_TF, st);
    if (e != hipSuccess) return (int32_t)e;
    for (int32_t it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(k_fit_sph_frames, dim3((unsigned)tiles), dim3(FIT_BLOCK), 0, st, *a);
        e = hipGetLastError();
        if (e != hipSuccess) return (int32_t)e;
        hipLaunchKernelGGL(k_fit_sph_finish, dim3((unsigned)tiles), dim3(FIT_BLOCK), 0, st, *a, w, tiles);
        e = hipGetLastError();
        if (e != hipSuccess) return (int32_t)e;
    }
    return 0;
}
