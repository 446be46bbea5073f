// phc_clip_real.hip -- phc_clip_process_real: the robot branch of `_run_clip_job` (phc_amd/motion_lib.py: the height fix, `process_clip_real`, the fp32
// packing) for concatenated clips in three launches (contract: include/phc_amd.h; per-lane code: phc_clip_real.h, phc_clip.h).  fp64 throughout, one
// rounding at the fp32 store; built with -ffp-contract=off and without fast-math.
//
// k_clip_real_height (only with fix_height): one block per clip.  One lane per simulated body runs the FK of the clip's first frame and leaves its height
// and the third row of its rotation in LDS; the lanes then stride over the contact points and the block takes the fp64 minimum (exact in any order) into
// clip_dz[c] of the scratch.
// k_clip_real_bodies: a block owns a tile of `fpb` consecutive frames (16 for H1, 14 for G1).  One lane per frame finds the frame's clip; then one lane
// per (frame, body in NB+E) runs clip_real_body -- its ancestor chain from the root for frame f and, for the angular velocity, for frame f + 1 -- and
// writes its fp32 fields into the LDS image of the tile's records; the block copies the image out with lane i on float i of a record (the velocity
// columns, which the third launch owns, are skipped).  Latency-bound like k_clip_bodies: a chain of dependent fp64 sin / cos / division / square roots.
// k_clip_real_filter: k_clip_filter over the NB simulated bodies, at column 7 (NB + E) of the record.
#include <hip/hip_runtime.h>
#include "phc_clip_real.h"

using namespace phc;

__global__ __launch_bounds__(CLIP_BLOCK) void k_clip_real_height(phc_clip_real_args_t a) {
    __shared__ double s_body[CLIP_MAX_BODIES * 4];   // per simulated body: wpos z, wmat[2, :]
    __shared__ double s_min[CLIP_BLOCK];
    const int c = blockIdx.x;
    const int64_t f0 = clip_real_first_frame(a, c);
    if ((int)threadIdx.x < a.num_bodies) clip_real_height_body(a, f0, threadIdx.x, s_body + 4 * threadIdx.x);
    __syncthreads();
    double z = INFINITY;
    for (int k = threadIdx.x; k < a.num_contacts; k += CLIP_BLOCK) z = fmin(z, clip_real_contact_z(a, s_body, k));
    s_min[threadIdx.x] = z;
    __syncthreads();
    for (int w = CLIP_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_min[threadIdx.x] = fmin(s_min[threadIdx.x], s_min[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) clip_real_dz(a)[c] = s_min[0];
}

__global__ __launch_bounds__(CLIP_BLOCK) void k_clip_real_bodies(phc_clip_real_args_t a, int fpb) {
    extern __shared__ float s_rec[];                // [fpb, stride] the tile's records, then [fpb] i32 the frames' clips
    const int NB = a.num_bodies, E = a.num_ext, J = NB + E, stride = a.frame_stride;
    int* s_clip = (int*)(s_rec + fpb * stride);
    const int64_t f0 = (int64_t)blockIdx.x * fpb;
    const int nf = (int)(a.num_frames - f0 < fpb ? a.num_frames - f0 : fpb);
    double* rows = (double*)a.scratch;
    int32_t* frame_clip = clip_real_frame_clip(a);
    if (!a.fix_height && blockIdx.x == 0)           // (nobody reads clip_dz then; it is left defined)
        for (int i = threadIdx.x; i < a.num_clips; i += CLIP_BLOCK) clip_real_dz(a)[i] = 0.0;
    for (int i = threadIdx.x; i < nf; i += CLIP_BLOCK) {
        const int c = clip_of_frame(a.clip_start, a.num_clips, f0 + i);
        s_clip[i] = c;
        frame_clip[f0 + i] = c;
    }
    const int pad0 = clip_real_pad_begin(NB, E), npad = stride - pad0;
    for (int i = threadIdx.x; i < nf * npad; i += CLIP_BLOCK) s_rec[(i / npad) * stride + pad0 + i % npad] = 0.f;
    __syncthreads();
    for (int i = threadIdx.x; i < nf * J; i += CLIP_BLOCK) {
        const int fl = i / J, j = i - fl * J;
        const int64_t f = f0 + fl;
        ClipRealBody o;
        clip_real_body(a, f, j, clip_real_span(a, s_clip[fl], f), o);
        clip_real_body_store(o, NB, E, j, s_rec + fl * stride, rows + f * 6 * NB);
    }
    __syncthreads();
    const int W = stride - 6 * NB;                  // gts | grs, then dof_pos | dvs | pad
    for (int i = threadIdx.x; i < nf * W; i += CLIP_BLOCK) {
        const int fl = i / W, r = i - fl * W;
        const int col = r < 7 * J ? r : r + 6 * NB;
        a.frames[(f0 + fl) * stride + col] = s_rec[fl * stride + col];
    }
}

__global__ __launch_bounds__(CLIP_BLOCK) void k_clip_real_filter(phc_clip_real_args_t a, ClipWeights w) {
    const int NB = a.num_bodies, W = 6 * NB;
    const int64_t idx = (int64_t)blockIdx.x * CLIP_BLOCK + threadIdx.x;
    if (idx >= a.num_frames * W) return;
    const int64_t f = idx / W;
    const int r = (int)(idx - f * W);
    int c = clip_real_frame_clip(a)[f];
    c = c < 0 ? 0 : (c >= a.num_clips ? a.num_clips - 1 : c);
    const ClipRealSpan s = clip_real_span(a, c, f);
    a.frames[f * a.frame_stride + 7 * (NB + a.num_ext) + r] = (float)clip_filtered_velocity((const double*)a.scratch, w, NB, r, f, s.t0, s.t1, s.dt);
}

extern "C" int64_t phc_clip_real_scratch_bytes(int64_t num_frames, int32_t num_bodies, int32_t num_ext, int32_t num_clips) {
    if (num_frames < 0 || num_bodies < 1 || num_ext < 0 || num_clips < 1) return PHC_EINVAL;
    return clip_real_scratch_bytes(num_frames, num_bodies, num_clips);
}

extern "C" int32_t phc_clip_process_real(const phc_clip_real_args_t* a, void* stream) {
    const int32_t rc = clip_real_args_check(a);
    if (rc) return rc;
    hipError_t e;
    if (a->fix_height) {
        hipLaunchKernelGGL(k_clip_real_height, dim3((unsigned)a->num_clips), dim3(CLIP_BLOCK), 0, (hipStream_t)stream, *a);
        if ((e = hipGetLastError()) != hipSuccess) return (int32_t)e;
    }
    const int fpb = clip_real_frames_per_block(a->num_bodies, a->num_ext);
    const size_t lds = (size_t)fpb * ((size_t)a->frame_stride * 4 + 4);
    hipLaunchKernelGGL(k_clip_real_bodies, dim3((unsigned)((a->num_frames + fpb - 1) / fpb)), dim3(CLIP_BLOCK), lds, (hipStream_t)stream, *a, fpb);
    if ((e = hipGetLastError()) != hipSuccess) return (int32_t)e;
    const int64_t lanes = a->num_frames * 6 * a->num_bodies;
    hipLaunchKernelGGL(k_clip_real_filter, dim3((unsigned)((lanes + CLIP_BLOCK - 1) / CLIP_BLOCK)), dim3(CLIP_BLOCK), 0, (hipStream_t)stream, *a, clip_gauss_weights());
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
