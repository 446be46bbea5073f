// phc_distill.hip -- distilling a composed controller into one MLP ("Distillation"): the dataset recorder of the evaluation sweep and the
// pieces of a SiLU MLP trained by regression that are not GEMMs.  All four are memory-bound passes: 8-16 bytes per lane where rows and pointers allow it,
// an element path where they do not (the conventions of phc_learn.hip).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <math.h>
#include <stdint.h>
#include "../../include/phc_amd.h"
#include "phc_distill.h"

__device__ __forceinline__ float bf16_bits_to_f(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ uint32_t f_to_bf16_bits(float v) {
    const __hip_bfloat16 b = __float2bfloat16(v);
    return (uint32_t)*reinterpret_cast<const uint16_t*>(&b);
}
__device__ __forceinline__ void unpack8(const uint4 q, float (&v)[8]) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[2 * k] = __uint_as_float(w[k] << 16); v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u); }
}
__device__ __forceinline__ uint4 pack8(const float (&v)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = f_to_bf16_bits(v[2 * k]) | (f_to_bf16_bits(v[2 * k + 1]) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ------------------------------------------------------------------------------------------
// Recorder: one block per env.  Env i with step < rows[i] stores the observation it ACTED on (obs_prev), both actions and the reset flag at row
// row_start[i] + step of the batch block; then obs_prev[i] = obs_buf[i] for every env.  A lane loads its obs_prev and obs_buf elements before it stores
// either, and no other lane touches them.  V floats per lane for the observation rows (934 fp32 = 3736 bytes per row: 8-byte vectors); the action rows
// (69 fp32) are only 4-byte aligned: elements.
// ------------------------------------------------------------------------------------------
template <int V> struct vec_of;
template <> struct vec_of<1> { typedef float type; };
template <> struct vec_of<2> { typedef float2 type; };
template <> struct vec_of<4> { typedef float4 type; };

template <int V>
__global__ __launch_bounds__(256) void k_dataset_record(phc_record_args_t a) {
    typedef typename vec_of<V>::type vec_t;
    const int i = blockIdx.x;
    int64_t row = phc_record_row(a.rows[i], a.row_start[i], a.step);
    if (row >= a.capacity) row = -1;        // (a block that the host sized too small: never past the allocation)
    const int nv = a.obs_dim / V;
    const vec_t* cur = reinterpret_cast<const vec_t*>(a.obs_buf + (int64_t)i * a.obs_dim);
    vec_t* prev = reinterpret_cast<vec_t*>(a.obs_prev + (int64_t)i * a.obs_dim);
    vec_t* dst = row >= 0 ? reinterpret_cast<vec_t*>(a.obs + row * a.obs_dim) : nullptr;
    for (int c = threadIdx.x; c < nv; c += 256) {
        const vec_t p = prev[c], n = cur[c];
        if (dst) dst[c] = p;
        prev[c] = n;
    }
    if (row < 0) return;
    const int A = a.num_actions;
    for (int c = threadIdx.x; c < A; c += 256) {
        a.clean[row * A + c] = a.clean_actions[(int64_t)i * A + c];
        a.env[row * A + c] = a.actions[(int64_t)i * A + c];
    }
    if (threadIdx.x == 0) a.reset[row] = a.reset_buf[i];
}

// ------------------------------------------------------------------------------------------
// y = silu(z), bf16 in, fp32 arithmetic, bf16 out: 8 elements (16 bytes) per lane when both pointers are 16-byte aligned, elements otherwise and
// over the ragged tail.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_silu_bf16(const __hip_bfloat16* __restrict__ z, int64_t n, __hip_bfloat16* __restrict__ y, int vec_ok) {
    const int64_t i8 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i8 >= n) return;
    if (vec_ok && i8 + 8 <= n) {
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(z + i8), v);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = phc_silu_f(v[k]);
        *reinterpret_cast<uint4*>(y + i8) = pack8(v);
        return;
    }
    const int64_t i1 = i8 + 8 < n ? i8 + 8 : n;
    for (int64_t i = i8; i < i1; ++i) y[i] = __float2bfloat16(phc_silu_f(__bfloat162float(z[i])));
}

// ------------------------------------------------------------------------------------------
// gz = gy silu'(z) written back as bf16, and the fp32 column sums of the UNROUNDED products per 256-row chunk (the first stage of phc_colsum_bf16's two:
// same chunking, same partial layout [chunk, cols], finished by k_colsum_finish / phc_colsum_finish_batch).  Block = 64 columns x a 256-row chunk.
//   NC = 8: lane <-> 8 adjacent columns (16-byte loads / stores), 32 row lanes; needs cols % 8 == 0 and 16-byte aligned pointers.
//   NC = 1: lane <-> one column, 4 row lanes (k_colsum_relu_bf16's layout): any cols, any alignment.
// Fixed order everywhere: a lane adds its rows in order, then one lane per column adds the row lanes in order.
// ------------------------------------------------------------------------------------------
#define DS_ROWS 256   // == CS_ROWS of phc_learn.hip (phc_colsum_workspace / phc_colsum_chunks)
template <int NC>
__global__ __launch_bounds__(256) void k_colsum_silu_bf16(const __hip_bfloat16* __restrict__ gy, const __hip_bfloat16* __restrict__ z, int64_t rows, int cols,
                                                          __hip_bfloat16* __restrict__ gz, float* __restrict__ partial) {
    constexpr int CL = 64 / NC;      // column lanes
    constexpr int RL = 256 / CL;     // row lanes
    __shared__ float l[RL][64];
    const int cl = threadIdx.x % CL, ry = threadIdx.x / CL;
    const int c0 = blockIdx.x * 64 + cl * NC;
    const int64_t r0 = (int64_t)blockIdx.y * DS_ROWS;
    const int64_t r1 = r0 + DS_ROWS < rows ? r0 + DS_ROWS : rows;
    float acc[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) acc[k] = 0.f;
    if (c0 < cols) {            // (NC = 8: cols % 8 == 0, so the lane's 8 columns are all inside)
        if constexpr (NC == 8) {
            int64_t r = r0 + ry;
            for (; r + RL < r1; r += 2 * RL) {    // two rows' loads in flight
                float g0[8], z0[8], g1[8], z1[8];
                unpack8(*reinterpret_cast<const uint4*>(gy + r * cols + c0), g0); unpack8(*reinterpret_cast<const uint4*>(z + r * cols + c0), z0);
                unpack8(*reinterpret_cast<const uint4*>(gy + (r + RL) * cols + c0), g1); unpack8(*reinterpret_cast<const uint4*>(z + (r + RL) * cols + c0), z1);
#pragma unroll
                for (int k = 0; k < 8; ++k) { g0[k] = phc_silu_grad_f(g0[k], z0[k]); acc[k] += g0[k]; }
                *reinterpret_cast<uint4*>(gz + r * cols + c0) = pack8(g0);
#pragma unroll
                for (int k = 0; k < 8; ++k) { g1[k] = phc_silu_grad_f(g1[k], z1[k]); acc[k] += g1[k]; }
                *reinterpret_cast<uint4*>(gz + (r + RL) * cols + c0) = pack8(g1);
            }
            for (; r < r1; r += RL) {
                float g0[8], z0[8];
                unpack8(*reinterpret_cast<const uint4*>(gy + r * cols + c0), g0); unpack8(*reinterpret_cast<const uint4*>(z + r * cols + c0), z0);
#pragma unroll
                for (int k = 0; k < 8; ++k) { g0[k] = phc_silu_grad_f(g0[k], z0[k]); acc[k] += g0[k]; }
                *reinterpret_cast<uint4*>(gz + r * cols + c0) = pack8(g0);
            }
        } else {
            for (int64_t r = r0 + ry; r < r1; r += RL) {
                const float m = phc_silu_grad_f(__bfloat162float(gy[r * cols + c0]), __bfloat162float(z[r * cols + c0]));
                gz[r * cols + c0] = __float2bfloat16(m);
                acc[0] += m;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) l[ry][cl * NC + k] = acc[k];
    __syncthreads();
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (threadIdx.x < 64 && c < cols) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < RL; ++i) t += l[i][threadIdx.x];
        partial[(int64_t)blockIdx.y * cols + c] = t;
    }
}
// The second stage (k_colsum_finish of phc_learn.hip restated: that one is local to its file): 64 columns x 16 slices of the chunk list.
__global__ __launch_bounds__(1024) void k_distill_colsum_finish(const float* __restrict__ partial, int nchunks, int cols, float* __restrict__ out) {
    __shared__ float l[16][64];
    const int cx = threadIdx.x & 63, sy = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cx;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;      // (the same four accumulators in the same order: the one-call result has phc_colsum_finish_batch's bits)
    if (c < cols) {
        int k = sy;
        for (; k + 48 < nchunks; k += 64) {
            a0 += partial[(int64_t)k * cols + c]; a1 += partial[(int64_t)(k + 16) * cols + c];
            a2 += partial[(int64_t)(k + 32) * cols + c]; a3 += partial[(int64_t)(k + 48) * cols + c];
        }
        for (; k < nchunks; k += 16) a0 += partial[(int64_t)k * cols + c];
    }
    l[sy][cx] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sy == 0 && c < cols) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += l[i][cx];
        out[c] = t;
    }
}

// ------------------------------------------------------------------------------------------
// nn.MSELoss() and its gradient: loss = mean over batch x dim of (pred - target[row_index[r]])^2, grad = 2 (pred - target) / (batch dim) in pred's type.
// Flat over the batch x dim elements, four per lane (one 16-byte fp32 / 8-byte bf16 access to pred and grad when they are aligned and the four are inside;
// the gathered target rows -- 69 fp32 -- are elements).  The sum: fp32 per lane over at most a few elements, fp64 from there: wave, block, then a
// one-block second launch that adds the per-block partials in a fixed order (phc_ppo_loss's pattern).
// ------------------------------------------------------------------------------------------
#define MSE_BLOCKS 512
template <bool BF16>
__global__ __launch_bounds__(256) void k_mse_loss(const void* __restrict__ pred_, const float* __restrict__ target, const int64_t* __restrict__ idx, int64_t batch, int dim,
                                                  void* __restrict__ grad_, double* __restrict__ partial, int vec_ok) {
    __shared__ double l[4];
    const int64_t n = batch * dim;
    const float scale = 2.0f / (float)n;
    double acc = 0.0;
    for (int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i4 < n; i4 += (int64_t)gridDim.x * 1024) {
        const int cnt = (int)(n - i4 < 4 ? n - i4 : 4);
        const bool vec = vec_ok && cnt == 4;
        float p[4] = {0.f, 0.f, 0.f, 0.f}, g[4];
        if (BF16) {
            const __hip_bfloat16* pred = reinterpret_cast<const __hip_bfloat16*>(pred_);
            if (vec) {
                const uint2 q = *reinterpret_cast<const uint2*>(pred + i4);
                p[0] = __uint_as_float(q.x << 16); p[1] = __uint_as_float(q.x & 0xffff0000u); p[2] = __uint_as_float(q.y << 16); p[3] = __uint_as_float(q.y & 0xffff0000u);
            } else {
                for (int k = 0; k < cnt; ++k) p[k] = __bfloat162float(pred[i4 + k]);
            }
        } else {
            const float* pred = reinterpret_cast<const float*>(pred_);
            if (vec) { const float4 q = *reinterpret_cast<const float4*>(pred + i4); p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w; }
            else for (int k = 0; k < cnt; ++k) p[k] = pred[i4 + k];
        }
        int64_t r = i4 / dim;
        int d = (int)(i4 - r * dim);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g[k] = 0.f;
            if (k < cnt) {
                const int64_t q = idx ? idx[r] : r;
                const float e = p[k] - target[q * dim + d];
                s += e * e;
                g[k] = scale * e;
                if (++d == dim) { d = 0; ++r; }
            }
        }
        acc += (double)s;
        if (BF16) {
            __hip_bfloat16* grad = reinterpret_cast<__hip_bfloat16*>(grad_);
            if (vec) *reinterpret_cast<uint2*>(grad + i4) = make_uint2(f_to_bf16_bits(g[0]) | (f_to_bf16_bits(g[1]) << 16), f_to_bf16_bits(g[2]) | (f_to_bf16_bits(g[3]) << 16));
            else for (int k = 0; k < cnt; ++k) grad[i4 + k] = __float2bfloat16(g[k]);
        } else {
            float* grad = reinterpret_cast<float*>(grad_);
            if (vec) *reinterpret_cast<float4*>(grad + i4) = make_float4(g[0], g[1], g[2], g[3]);
            else for (int k = 0; k < cnt; ++k) grad[i4 + k] = g[k];
        }
    }
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) l[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (l[0] + l[1]) + (l[2] + l[3]);
}
__global__ __launch_bounds__(64) void k_mse_loss_finish(const double* __restrict__ partial, int nblocks, int64_t n, float* __restrict__ loss) {
    double t = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += 64) t += partial[b];
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
    if (threadIdx.x == 0) *loss = (float)(t / (double)n);
}

static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" {

int32_t phc_dataset_record(const phc_record_args_t* a, void* stream) {
    if (!a || !a->obs_buf || !a->obs_prev || !a->clean_actions || !a->actions || !a->reset_buf || !a->rows || !a->row_start || !a->obs || !a->clean || !a->env ||
        !a->reset)
        return PHC_EINVAL;
    if (a->num_envs < 1 || a->obs_dim < 1 || a->num_actions < 1 || a->step < 0 || a->capacity < 1) return PHC_EINVAL;
    const void* obs_ptrs[3] = {a->obs_buf, a->obs_prev, a->obs};
    int v = 4;
    for (int k = 0; k < 3; ++k) {
        if (v == 4 && !(aligned_to(obs_ptrs[k], 16) && a->obs_dim % 4 == 0)) v = 2;
        if (v == 2 && !(aligned_to(obs_ptrs[k], 8) && a->obs_dim % 2 == 0)) v = 1;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)a->num_envs);
    if (v == 4) hipLaunchKernelGGL(k_dataset_record<4>, grid, dim3(256), 0, st, *a);
    else if (v == 2) hipLaunchKernelGGL(k_dataset_record<2>, grid, dim3(256), 0, st, *a);
    else hipLaunchKernelGGL(k_dataset_record<1>, grid, dim3(256), 0, st, *a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

int32_t phc_silu_bf16(const void* z, int64_t rows, int32_t cols, void* y, void* stream) {
    if (!z || !y || rows < 1 || cols < 1) return PHC_EINVAL;
    const int64_t n = rows * (int64_t)cols;
    const int64_t blocks = (n + 2047) / 2048;
    if (blocks > 0x7fffffff) return PHC_EUNSUPPORTED;
    hipLaunchKernelGGL(k_silu_bf16, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const __hip_bfloat16*>(z), n,
                       reinterpret_cast<__hip_bfloat16*>(y), (int)(aligned_to(z, 16) && aligned_to(y, 16)));
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

int32_t phc_colsum_silu_bf16(const void* gy, const void* z, int64_t rows, int32_t cols, void* gz, float* out, float* workspace, void* stream) {
    if (!gy || !z || !gz || !workspace || rows < 1 || cols < 1) return PHC_EINVAL;
    const int64_t nchunks = (rows + DS_ROWS - 1) / DS_ROWS;
    if (nchunks > 65535) return PHC_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((cols + 63) / 64, (unsigned)nchunks);
    const __hip_bfloat16 *g = reinterpret_cast<const __hip_bfloat16*>(gy), *zz = reinterpret_cast<const __hip_bfloat16*>(z);
    if (cols % 8 == 0 && aligned_to(gy, 16) && aligned_to(z, 16) && aligned_to(gz, 16))
        hipLaunchKernelGGL(k_colsum_silu_bf16<8>, grid, dim3(256), 0, st, g, zz, rows, cols, reinterpret_cast<__hip_bfloat16*>(gz), workspace);
    else
        hipLaunchKernelGGL(k_colsum_silu_bf16<1>, grid, dim3(256), 0, st, g, zz, rows, cols, reinterpret_cast<__hip_bfloat16*>(gz), workspace);
    if (out) hipLaunchKernelGGL(k_distill_colsum_finish, dim3((cols + 63) / 64), dim3(1024), 0, st, workspace, (int)nchunks, cols, out);   // (NULL: phc_colsum_finish_batch later)
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

int64_t phc_mse_loss_workspace(void) { return MSE_BLOCKS * (int64_t)sizeof(double); }

int32_t phc_mse_loss(const void* pred, int32_t is_bf16, const float* target, const int64_t* row_index, int64_t batch, int32_t dim, void* grad, float* loss_out,
                     double* workspace, void* stream) {
    if (!pred || !target || !grad || !loss_out || !workspace || batch < 1 || dim < 1) return PHC_EINVAL;
    const int64_t n = batch * (int64_t)dim;
    const int64_t nb = (n + 1023) / 1024;
    const int nblocks = (int)(nb < MSE_BLOCKS ? nb : MSE_BLOCKS);
    const uintptr_t al = is_bf16 ? 8 : 16;
    const int vec_ok = aligned_to(pred, al) && aligned_to(grad, al);
    hipStream_t st = (hipStream_t)stream;
    if (is_bf16) hipLaunchKernelGGL(k_mse_loss<true>, dim3(nblocks), dim3(256), 0, st, pred, target, row_index, batch, dim, grad, workspace, vec_ok);
    else hipLaunchKernelGGL(k_mse_loss<false>, dim3(nblocks), dim3(256), 0, st, pred, target, row_index, batch, dim, grad, workspace, vec_ok);
    hipLaunchKernelGGL(k_mse_loss_finish, dim3(1), dim3(64), 0, st, workspace, nblocks, n, loss_out);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

}  // extern "C"
