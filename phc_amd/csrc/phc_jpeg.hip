// phc_jpeg.hip -- phc_jpeg_encode: the baseline JPEG scans of F device frames in one call (contract and coding rules: include/phc_amd.h; per-block and
// per-segment code, the worst-case derivation and the scratch layout: phc_jpeg.h).  Four launches on the caller's stream:
//   k_jpeg_blocks   256-thread blocks, one lane per 8 x 8 block of a component plane (Y blocks first, then Cb, then Cr: a wavefront is of one kind except at
//                   the two seams).  The 64 samples stay in registers (unrolled indices only); a lane stores its 128 bytes as eight 16-byte stores.
//   k_jpeg_entropy  64-thread blocks, one lane per restart segment; the code table (2.1 KB) is copied to LDS once per block.  Bit-serial and divergent by
//                   nature: the parallelism is the number of segments, which is why the host picks a short restart interval.
//   k_jpeg_scan     one 256-thread block per frame: exclusive sum of the segment lengths in tiles of 256 (Hillis-Steele in LDS, a running carry).
//   k_jpeg_copy     one wavefront per segment: byte i of the slot by lane i mod 64 (coalesced within the segment).
// No atomics: the stream depends on the input alone.  Built with -ffp-contract=off and without fast-math, as the host build of phc_jpeg.h is.
#include <hip/hip_runtime.h>
#include "phc_jpeg.h"

using namespace phc;

__device__ const JpegHuff d_jpeg_huff = jpeg_huff_make();

__global__ __launch_bounds__(256) void k_jpeg_blocks(JpegK k) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (int64_t)k.F * k.g.blocks) return;
    jpeg_block(k, gid / k.g.blocks, gid % k.g.blocks);
}

__global__ __launch_bounds__(64) void k_jpeg_entropy(JpegK k) {
    __shared__ JpegHuff h;
    for (int i = threadIdx.x; i < JPEG_HUFF_WORDS; i += 64) reinterpret_cast<uint32_t*>(&h)[i] = reinterpret_cast<const uint32_t*>(&d_jpeg_huff)[i];
    __syncthreads();
    const int64_t gid = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (gid >= (int64_t)k.F * k.g.nseg) return;
    jpeg_segment(k, h, gid / k.g.nseg, (int)(gid % k.g.nseg));
}

__global__ __launch_bounds__(256) void k_jpeg_scan(JpegK k) {
    __shared__ int32_t sh[256];
    const int64_t f = blockIdx.x;
    const int t = threadIdx.x, nseg = k.g.nseg;
    int32_t carry = 0;
    for (int base = 0; base < nseg; base += 256) {   // (uniform trip count: every barrier is met by the whole block)
        const int32_t v = base + t < nseg ? k.seg_len[f * nseg + base + t] : 0;
        sh[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int32_t add = t >= d ? sh[t - d] : 0;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        if (base + t < nseg) k.seg_off[f * nseg + base + t] = carry + sh[t] - v;
        carry += sh[255];
        __syncthreads();
    }
    if (t == 0) k.length[f] = carry;
}

__global__ __launch_bounds__(256) void k_jpeg_copy(JpegK k) {
    const int64_t fs = ((int64_t)blockIdx.x * 256 + threadIdx.x) / 64;
    if (fs >= (int64_t)k.F * k.g.nseg) return;
    jpeg_copy_segment(k, fs, (int)(threadIdx.x & 63), 64);
}

extern "C" int64_t phc_jpeg_frame_bound(int32_t width, int32_t height, int32_t restart_interval) {
    if (width < 1 || width > 65535 || height < 1 || height > 65535 || restart_interval < 1) return PHC_EINVAL;
    return jpeg_frame_bound(jpeg_geom(width, height, restart_interval));
}

extern "C" int64_t phc_jpeg_scratch_bytes(int64_t num_frames, int32_t width, int32_t height, int32_t restart_interval) {
    if (num_frames < 0 || width < 1 || width > 65535 || height < 1 || height > 65535 || restart_interval < 1) return PHC_EINVAL;
    return jpeg_layout(jpeg_geom(width, height, restart_interval), num_frames).total;
}

extern "C" int32_t phc_jpeg_encode(const phc_jpeg_args_t* a, void* stream) {
    const int32_t rc = jpeg_args_check(a);
    if (rc) return rc;
    if (a->num_frames == 0) return 0;
    const JpegK k = jpeg_kargs(a);
    const int64_t nb = (int64_t)k.F * k.g.blocks, ns = (int64_t)k.F * k.g.nseg;
    if ((nb + 255) / 256 > 0x7fffffffLL || (ns + 3) / 4 > 0x7fffffffLL) return PHC_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_jpeg_blocks, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, k);
    hipLaunchKernelGGL(k_jpeg_entropy, dim3((unsigned)((ns + 63) / 64)), dim3(64), 0, s, k);
    hipLaunchKernelGGL(k_jpeg_scan, dim3((unsigned)k.F), dim3(256), 0, s, k);
    hipLaunchKernelGGL(k_jpeg_copy, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, s, k);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
