// phc_fit.hip -- phc_fit_iterate: trips of `fit_clip`'s loop (phc_amd/utils/fit_robot_motion.py) for concatenated clips (contract: include/phc_amd.h;
// per-lane code: phc_fit.h).  fp32, built with -ffp-contract=off and without fast-math.
//
// k_fit_setup (once per call, one block): the tile table -- clip c owns tiles tile_start[c] .. tile_start[c + 1] - 1, each of TF frames of that clip
// alone -- and Adam's two scalars of every clip's next step.
// k_fit_frames<G> (per trip): a block is one tile, a group of G lanes one frame, a lane one body.  Stage A: the lane's ancestor chain -> its world position
// and its rotation in the parent's frame into LDS.  Stage B: lane m -> u_m into LDS.  Stage C: lane 0 the root rotation vector's gradient and Adam step, lane j joint j's gradient, Adam step and
// clamp (into the scratch row: the smoothing needs the neighbour frames, which other blocks own).  The frame's sums of u, |p - g| and dof^2 are butterflies
// over the group; five lanes add the tile's frames in order and store the tile's partial.  Latency-bound: a chain of dependent 3x3 products per lane.
// k_fit_finish (per trip): a block is one tile again: the 5-tap filter from the scratch rows into dof; the block of a clip's first tile also adds the
// clip's partials in tile order (root_off's Adam step, the loss) and advances the clip's step.
// Nothing is exchanged between blocks inside a launch; no atomics.
#include <hip/hip_runtime.h>
#include "phc_fit.h"
#include "phc_group.h"

using namespace phc;

__global__ __launch_bounds__(FIT_BLOCK) void k_fit_setup(phc_fit_args_t a, int tf) {
    __shared__ int32_t s_n[FIT_BLOCK];
    __shared__ int32_t s_carry;
    const FitScratch s = fit_scratch(a);
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int c0 = 0; c0 < a.num_clips; c0 += FIT_BLOCK) {
        const int c = c0 + (int)threadIdx.x;
        int32_t n = 0;
        if (c < a.num_clips) {
            n = fit_clip_tiles(fit_span(a, c), tf);
            const FitCoef co = fit_coef(a.lr, a.step[c] + 1);
            s.coef[c * 2 + 0] = co.step_size; s.coef[c * 2 + 1] = co.bc2_sqrt;
        }
        s_n[threadIdx.x] = n;
        __syncthreads();
        if (threadIdx.x == 0) {
            int32_t run = s_carry;
            for (int i = 0; i < FIT_BLOCK; ++i) { const int32_t t = s_n[i]; s_n[i] = run; run += t; }
            s_carry = run;
        }
        __syncthreads();
        if (c < a.num_clips) s.tile_start[c] = s_n[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) s.tile_start[a.num_clips] = s_carry;
}

// k_fit_setup for the fits of other translation units (phc_fit_sph.hip): the same launch, the same table.
namespace phc {
hipError_t fit_launch_setup(const phc_fit_args_t& a, int tf, hipStream_t st) {
    hipLaunchKernelGGL(k_fit_setup, dim3(1), dim3(FIT_BLOCK), 0, st, a, tf);
    return hipGetLastError();
}
}  // namespace phc

template <int G>
__global__ __launch_bounds__(FIT_BLOCK) void k_fit_frames(phc_fit_args_t a) {
    constexpr int TF = FIT_BLOCK / G;
    __shared__ float s_pos[TF][G * 3];                  // (lane strides of 3 and 9 floats: no bank conflict)
    __shared__ float s_L[TF][G * 9];
    __shared__ float s_u[TF][FIT_MAX_MATCHED * 3];
    __shared__ float s_sum[TF][FIT_SUMS];
    const FitScratch s = fit_scratch(a);
    const int32_t tile = (int32_t)blockIdx.x;
    const int c = fit_clip_of_tile(s.tile_start, a.num_clips, tile);
    if (c < 0) return;                                  // (the whole block)
    const FitSpan sp = fit_span(a, c);
    const int fl = (int)threadIdx.x / G, b = (int)threadIdx.x % G;
    const int NB = a.num_bodies, NBE = a.num_bodies + a.num_ext;
    const int64_t f = sp.t0 + ((int64_t)(tile - s.tile_start[c]) * TF + fl), T = sp.t1 - sp.t0;
    const bool live = f >= sp.t0 && f < sp.t1;
    float pos[3] = {0.f, 0.f, 0.f}, R[9], L[9];
    if (live && b < NBE) {
        fit_body(a, f, c, b, pos, R, L);
        s_pos[fl][b * 3 + 0] = pos[0]; s_pos[fl][b * 3 + 1] = pos[1]; s_pos[fl][b * 3 + 2] = pos[2];
#pragma unroll
        for (int i = 0; i < 9; ++i) s_L[fl][b * 9 + i] = L[i];
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
        else if (b < NB) v[4] = fit_joint_step(a, f, b, T, co, R, s_L[fl], s_u[fl], s.clamped);
    }
#pragma unroll
    for (int i = 0; i < FIT_SUMS; ++i) {
        v[i] = group_sum<G>(v[i]);
        if (b == 0) s_sum[fl][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x < FIT_SUMS) {
        float acc = 0.f;
        for (int k = 0; k < TF; ++k) acc += s_sum[k][threadIdx.x];
        s.partial[(int64_t)tile * FIT_SUMS + threadIdx.x] = acc;
    }
}

__global__ __launch_bounds__(FIT_BLOCK) void k_fit_finish(phc_fit_args_t a, FitTaps w, int tf, int64_t num_tiles) {
    const FitScratch s = fit_scratch(a);
    const int32_t tile = (int32_t)blockIdx.x;
    const int c = fit_clip_of_tile(s.tile_start, a.num_clips, tile);
    if (c < 0) return;
    const FitSpan sp = fit_span(a, c);
    const int ND = a.num_bodies - 1;
    const int32_t first = s.tile_start[c];
    const int64_t t_lo = sp.t0 + (int64_t)(tile - first) * tf;
    int64_t nf = sp.t1 - t_lo;
    nf = t_lo < sp.t0 ? 0 : (nf > tf ? tf : nf);
    for (int i = (int)threadIdx.x; i < (int)nf * ND; i += FIT_BLOCK) {
        const int fl = i / ND, d = i - fl * ND;
        a.dof[(t_lo + fl) * ND + d] = fit_smooth(s.clamped, w, ND, d, t_lo + fl, sp.t0, sp.t1);
    }
    if (tile == first) {
        if (threadIdx.x < 4) fit_clip_lane(a, s, c, (int)threadIdx.x, num_tiles);
        __syncthreads();
        if (threadIdx.x == 0) fit_clip_advance(a, s, c);
    }
}

extern "C" int64_t phc_fit_scratch_bytes(int64_t num_frames, int32_t num_clips, int32_t num_bodies_ext) {
    if (num_frames < 0 || num_clips < 1 || num_bodies_ext < 1 || num_bodies_ext > FIT_MAX_BODIES) return PHC_EINVAL;
    return fit_scratch_bytes(num_frames, num_clips, num_bodies_ext);
}

extern "C" int32_t phc_fit_iterate(const phc_fit_args_t* a, int32_t iterations, void* stream) {
    int64_t tiles = 0;
    const int32_t rc = check_fit(a, iterations, &tiles);
    if (rc) return rc;
    if (iterations == 0) return 0;
    const int nbe = a->num_bodies + a->num_ext, tf = fit_tile_frames(nbe);
    const FitTaps w = fit_taps();
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_fit_setup, dim3(1), dim3(FIT_BLOCK), 0, st, *a, tf);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int32_t)e;
    for (int32_t it = 0; it < iterations; ++it) {
        if (fit_group(nbe) == 32) hipLaunchKernelGGL(k_fit_frames<32>, dim3((unsigned)tiles), dim3(FIT_BLOCK), 0, st, *a);
        else hipLaunchKernelGGL(k_fit_frames<64>, dim3((unsigned)tiles), dim3(FIT_BLOCK), 0, st, *a);
        e = hipGetLastError();
        if (e != hipSuccess) return (int32_t)e;
        hipLaunchKernelGGL(k_fit_finish, dim3((unsigned)tiles), dim3(FIT_BLOCK), 0, st, *a, w, tf, tiles);
        e = hipGetLastError();
        if (e != hipSuccess) return (int32_t)e;
    }
    return 0;
}
