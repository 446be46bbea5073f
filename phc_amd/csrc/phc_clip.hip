// phc_clip.hip -- phc_clip_process: `process_clip` (phc_amd/motion_lib.py) for concatenated clips in two launches (contract: include/phc_amd.h; per-lane
// code: phc_clip.h).  fp64 throughout, one rounding at the fp32 store; built with -ffp-contract=off and without fast-math.
//
// k_clip_bodies: a block owns a tile of `fpb` consecutive frames (16 for the 24 SMPL bodies).  One lane per frame finds the frame's clip (binary search
// over clip_start) and records it; then one lane per (frame, body) runs clip_body -- its ancestor chain from the root, its own neighbour frame for the
// two finite differences -- and writes its fp32 fields into the LDS image of the tile's records; the block then copies the image out with lane i on
// float i of a record (the velocity columns, which the second launch owns, are skipped).  The fp64 positions and raw angular velocities go to the
// scratch rows.  Latency-bound: a chain of dependent fp64 divisions and square roots per lane, 96 B in and 80 B out per lane.
// k_clip_filter: one lane per velocity float of a record (6 J consecutive floats); the 17 taps read the scratch rows of the lane's clip, lane i on
// double i of a row.  The rows of 18 neighbouring frames are re-read from L2.
#include <hip/hip_runtime.h>
#include "phc_clip.h"

using namespace phc;

__global__ __launch_bounds__(CLIP_BLOCK) void k_clip_bodies(phc_clip_args_t a, int fpb) {
    extern __shared__ float s_rec[];                // [fpb, stride] the tile's records, then [fpb] i32 the frames' clips
    const int J = a.num_bodies, stride = a.frame_stride;
    int* s_clip = (int*)(s_rec + fpb * stride);
    const int64_t f0 = (int64_t)blockIdx.x * fpb;
    const int nf = (int)(a.num_frames - f0 < fpb ? a.num_frames - f0 : fpb);
    double* rows = (double*)a.scratch;
    int32_t* frame_clip = (int32_t*)(rows + a.num_frames * 6 * J);
    for (int i = threadIdx.x; i < nf; i += CLIP_BLOCK) {
        const int c = clip_of_frame(a.clip_start, a.num_clips, f0 + i);
        s_clip[i] = c;
        frame_clip[f0 + i] = c;
    }
    for (int i = threadIdx.x; i < nf * 3; i += CLIP_BLOCK) s_rec[(i / 3) * stride + clip_pad_begin(J) + i % 3] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < nf * J; i += CLIP_BLOCK) {
        const int fl = i / J, j = i - fl * J;
        const int64_t f = f0 + fl;
        ClipBody o;
        clip_body(a, f, j, clip_span(a, s_clip[fl], f), o);
        clip_body_store(o, J, j, s_rec + fl * stride, rows + f * 6 * J);
    }
    __syncthreads();
    const int W = stride - 6 * J;                   // gts | grs, then lrs | dvs | pad
    for (int i = threadIdx.x; i < nf * W; i += CLIP_BLOCK) {
        const int fl = i / W, r = i - fl * W;
        const int col = r < 7 * J ? r : r + 6 * J;
        a.frames[(f0 + fl) * stride + col] = s_rec[fl * stride + col];
    }
}

__global__ __launch_bounds__(CLIP_BLOCK) void k_clip_filter(phc_clip_args_t a, ClipWeights w) {
    const int J = a.num_bodies, W = 6 * J;
    const int64_t idx = (int64_t)blockIdx.x * CLIP_BLOCK + threadIdx.x;
    if (idx >= a.num_frames * W) return;
    const int64_t f = idx / W;
    const int r = (int)(idx - f * W);
    const double* rows = (const double*)a.scratch;
    int c = ((const int32_t*)(rows + a.num_frames * W))[f];
    c = c < 0 ? 0 : (c >= a.num_clips ? a.num_clips - 1 : c);
    const ClipSpan s = clip_span(a, c, f);
    a.frames[f * a.frame_stride + 7 * J + r] = (float)clip_filtered_velocity(rows, w, J, r, f, s.t0, s.t1, s.dt);
}

extern "C" int64_t phc_clip_scratch_bytes(int64_t num_frames, int32_t num_bodies) {
    if (num_frames < 0 || num_bodies < 1) return PHC_EINVAL;
    return clip_scratch_bytes(num_frames, num_bodies);
}

extern "C" int32_t phc_clip_process(const phc_clip_args_t* a, void* stream) {
    const int32_t rc = clip_args_check(a);
    if (rc) return rc;
    const int fpb = clip_frames_per_block(a->num_bodies);
    const size_t lds = (size_t)fpb * ((size_t)a->frame_stride * 4 + 4);
    hipLaunchKernelGGL(k_clip_bodies, dim3((unsigned)((a->num_frames + fpb - 1) / fpb)), dim3(CLIP_BLOCK), lds, (hipStream_t)stream, *a, fpb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int32_t)e;
    const int64_t lanes = a->num_frames * 6 * a->num_bodies;
    hipLaunchKernelGGL(k_clip_filter, dim3((unsigned)((lanes + CLIP_BLOCK - 1) / CLIP_BLOCK)), dim3(CLIP_BLOCK), 0, (hipStream_t)stream, *a, clip_gauss_weights());
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
