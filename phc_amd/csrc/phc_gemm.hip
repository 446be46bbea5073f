// phc_gemm.hip -- native bf16 matrix-core kernels of the learner (DESIGN.md 4.3 "Native weight gradient").
//
// phc_wgrad_bf16: the weight gradient of a linear layer, gW = gZ^T X, with the ReLU mask of the layer's saved output applied to the
// output gradient on the way in, the bias gradient (column sums of gZ) taken from the same tiles, and a deterministic in-launch
// reduction of the row slices that ends in the fp32 gradient bucket (store or accumulate).  It replaces three launches of the library
// path (phc_colsum_relu_bf16, a batched GEMM whose slabs are rounded to bf16, phc_sum_slabs_bf16) and keeps fp32 from the MFMA
// accumulator to the bucket.
//
// Tiling.  One block (256 threads, 2 x 2 waves) owns a 128 (output feature j) x 128 (input feature c) tile of gW for one slice of the
// rows; a wave owns 64 x 64 of it as 2 x 2 v_mfma_f32_32x32x16_bf16 accumulators.  The reduction index (the batch row) is the SLOW
// index of both row-major operands, so both MFMA operands are transposed reads: a stage of 64 rows x 128 columns of gZ and of X sits
// row-major in LDS (256-byte rows) and ds_read_b64_tr_b16 delivers, to lane l, the four rows 8 (l >> 5) + 4 s .. + 3 of column (l & 31).
// LDS image: byte offset of 16-byte chunk ch (0..15) of row r = 256 r + 16 (ch ^ ((r & 3) << 2)): the four rows one transposed read
// gathers land in the four 64-byte quarters of the 64 banks, so the read is conflict-free; every lane address is 8-byte aligned.
// Stages are double-buffered through registers: the loads of stage i + 1 are in flight while stage i feeds the matrix cores.
//
// Split and reduction.  slices = phc_wgrad_bf16_slices(rows, n, k), a function of the shape alone.  With more than one slice every
// block writes its fp32 tile to the caller's workspace, publishes it (agent-scope release, then a ticket fetch_add), and the block that
// draws the last ticket of a tile acquires and adds the slabs IN SLICE ORDER, whichever block it happens to be: results do not depend
// on arrival order.  Tickets live in the workspace and are zeroed on the launch stream ahead of every launch -- by a one-block kernel, not by
// hipMemsetAsync: captured in a hipGraph, the memset node of this stack (HIP 7.0.51831 as bundled with torch 2.10) zeroes on the first replay and
// writes a stale 16-byte pattern {byte count, 1, 0x7000, 0} on every later one (measured with a graph holding nothing but the memset, 16 B to 4 KB).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/phc_amd.h"

#define WG_TM 128        // tile: output features (rows of gW)
#define WG_TN 128        // tile: input features (columns of gW)
#define WG_KT 64         // batch rows per LDS stage (four MFMA steps)
#define WG_THREADS 256
#define WG_MAX_SLICES 16
#define WG_MIN_SLICE_ROWS 512
#define WG_TARGET_BLOCKS 512   // two resident blocks per CU

typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
typedef short wg_s16x4 __attribute__((ext_vector_type(4)));
typedef float wg_f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) wg_s16x4* wg_lds_s16x4;

struct WgradArgs {
    const uint16_t* gy; const uint16_t* y; const uint16_t* x;
    int64_t ld_x, rows, rows_per_slice, ld_gw;
    int n, k, slices, tiles_n, tiles_m;
    float* gw; float* gb; uint16_t* gz;
    int accumulate, gb_accumulate;
    unsigned* tickets; float* slabs; float* gb_slabs;
};

static inline int wg_tiles(int v, int t) { return (v + t - 1) / t; }

static int wg_slices(int64_t rows, int n, int k) {
    const int64_t tiles = (int64_t)wg_tiles(n, WG_TM) * wg_tiles(k, WG_TN);
    int64_t s = (WG_TARGET_BLOCKS + tiles - 1) / tiles;
    const int64_t by_rows = rows / WG_MIN_SLICE_ROWS;
    if (s > by_rows) s = by_rows;
    if (s > WG_MAX_SLICES) s = WG_MAX_SLICES;
    return s < 1 ? 1 : (int)s;
}
// rows of one slice: a multiple of the MFMA step (16); with >= 512 rows per slice and <= 16 slices no slice is empty
static int64_t wg_rows_per_slice(int64_t rows, int slices) { return ((rows + slices - 1) / slices + 15) / 16 * 16; }

__device__ __forceinline__ int wg_lds_off(int row, int ch) { return row * 256 + ((ch ^ ((row & 3) << 2)) << 4); }

// y > 0 on bf16 bits: positive sign, not zero, not NaN (+inf passes)
__device__ __forceinline__ bool wg_pos(uint32_t h) { return h - 1u < 0x7f80u; }

__device__ __forceinline__ uint32_t wg_mask2(uint32_t g, uint32_t yy, bool all) {
    return (((int)all | (int)wg_pos(yy & 0xffffu)) ? (g & 0xffffu) : 0u) | (((int)all | (int)wg_pos(yy >> 16)) ? (g & 0xffff0000u) : 0u);
}

// 8 consecutive elements of row-major `p` at (row r, column c) as four packed words.
// VEC (p 16-byte aligned, ld and cols multiples of 8, c a multiple of 8: a chunk is inside or outside as a whole): ONE unconditional 16-byte load,
// from the matrix's first chunk when the lane's own is outside [0, r1) x [0, cols) -- no branch and no use of the data, so the loads of a stage are
// all in flight together behind the MFMA work; the CALLER zeroes an outside chunk when it stores it to LDS (wg_keep).
// Otherwise element loads, zero outside.
template <bool VEC>
__device__ __forceinline__ uint4 wg_load8(const uint16_t* __restrict__ p, int64_t ld, int64_t r, int64_t r1, int c, int cols) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (VEC) {
        const bool in = r < r1 && c < cols;
        return *reinterpret_cast<const uint4*>(in ? p + r * ld + c : p);
    }
    if (r >= r1 || c >= cols) return v;
    const uint16_t* q = p + r * ld + c;
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = c + i < cols ? (uint32_t)q[i] : 0u;
    v.x = e[0] | (e[1] << 16); v.y = e[2] | (e[3] << 16); v.z = e[4] | (e[5] << 16); v.w = e[6] | (e[7] << 16);
    return v;
}

__device__ __forceinline__ uint4 wg_keep(uint4 v, bool in) {
    v.x = in ? v.x : 0u; v.y = in ? v.y : 0u; v.z = in ? v.z : 0u; v.w = in ? v.w : 0u;
    return v;
}

template <bool VEC>
__device__ __forceinline__ void wg_store8(uint16_t* __restrict__ p, int64_t ld, int64_t r, int64_t r1, int c, int cols, uint4 v) {
    if (r >= r1 || c >= cols) return;
    uint16_t* q = p + r * ld + c;
    if (VEC) { *reinterpret_cast<uint4*>(q) = v; return; }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (c + i < cols) q[i] = (uint16_t)(w[i >> 1] >> ((i & 1) * 16));
}

// VG: gy / y / gz take 16-byte accesses (bases 16-byte aligned, n a multiple of 8); VX: the same for x (ld_x and k multiples of 8)
template <bool VG, bool VX>
__global__ __launch_bounds__(WG_THREADS, 2) void k_wgrad_bf16(const WgradArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * WG_KT * 256];   // [buffer][gz | x][stage rows][256 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    // block id -> (slice, tile), slice fastest: workgroups are dealt round-robin to the 8 XCDs, so the blocks of one slice -- which read the same
    // rows of gy / y / x, each tile of them 8 times over -- share an XCD and its L2 (with tiles fastest every XCD fetched its own copy of every
    // operand tile and the kernel ran at HBM rate: 135 us for 16384 x 1024 x 1024).  A pure speed choice: results do not depend on it.
    const int slice = blockIdx.x % a.slices, tile_id = blockIdx.x / a.slices;
    const int tn = tile_id % a.tiles_n, tm = tile_id / a.tiles_n;
    const int j0 = tm * WG_TM, c0 = tn * WG_TN;
    const int64_t rbeg = (int64_t)slice * a.rows_per_slice;
    int64_t rend = rbeg + a.rows_per_slice;
    if (rend > a.rows) rend = a.rows;
    const int nstages = rend > rbeg ? (int)((rend - rbeg + WG_KT - 1) / WG_KT) : 0;
    const bool side = tn == 0;                       // the blocks of the first column tile also produce gz and gb
    const bool want_gz = side && a.gz != nullptr, want_gb = side && a.gb != nullptr;

    // staging: thread -> 16-byte chunk (tid & 15) of rows (tid >> 4) + 16 p of the stage; the loads of a stage stay raw in registers (masking
    // them at once would wait for them ahead of the MFMA work they are meant to hide behind) and are masked when they go to LDS
    const int srow = tid >> 4, sch = tid & 15;
    constexpr int NP = WG_KT / 16;
    uint4 rg[NP], ry[NP], rx[NP];
    // without a mask the second operand is gy itself and every element passes: the same instruction stream either way (a branch around the y loads
    // would make each of them wait for its data before the next is issued)
    const uint16_t* __restrict__ yp = a.y ? a.y : a.gy;
    const bool nomask = a.y == nullptr;
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int stage) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int64_t r = rbeg + (int64_t)stage * WG_KT + srow + 16 * p;
            rg[p] = wg_load8<VG>(a.gy, a.n, r, rend, j0 + 8 * sch, a.n);
            ry[p] = wg_load8<VG>(yp, a.n, r, rend, j0 + 8 * sch, a.n);
            rx[p] = wg_load8<VX>(a.x, a.ld_x, r, rend, c0 + 8 * sch, a.k);
        }
    };
    auto commit = [&](int stage, int buf) {
        unsigned char* bg = lds + buf * (2 * WG_KT * 256);
        unsigned char* bx = bg + WG_KT * 256;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int row = srow + 16 * p;
            const bool rin = rbeg + (int64_t)stage * WG_KT + row < rend;
            rg[p] = wg_keep(rg[p], rin && j0 + 8 * sch < a.n);
            rx[p] = wg_keep(rx[p], rin && c0 + 8 * sch < a.k);
            rg[p].x = wg_mask2(rg[p].x, ry[p].x, nomask); rg[p].y = wg_mask2(rg[p].y, ry[p].y, nomask);
            rg[p].z = wg_mask2(rg[p].z, ry[p].z, nomask); rg[p].w = wg_mask2(rg[p].w, ry[p].w, nomask);
            *reinterpret_cast<uint4*>(bg + wg_lds_off(row, sch)) = rg[p];
            *reinterpret_cast<uint4*>(bx + wg_lds_off(row, sch)) = rx[p];
            if (want_gz) wg_store8<VG>(a.gz, a.n, rbeg + (int64_t)stage * WG_KT + row, rend, j0 + 8 * sch, a.n, rg[p]);
            if (want_gb) {
                const uint32_t w[4] = {rg[p].x, rg[p].y, rg[p].z, rg[p].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    bsum[2 * i] += __uint_as_float(w[i] << 16);
                    bsum[2 * i + 1] += __uint_as_float(w[i] & 0xffff0000u);
                }
            }
        }
    };

    // transposed-read addresses (see the header): lane 4 q + p of a 16-lane group supplies row q, columns 4 p .. 4 p + 3 of the group's block
    const int grp = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3, h = grp >> 1;
    int offA[2], offB[2];   // byte offsets inside a stage image for row 8 h + q (k-step 0, first half); + 4 rows / + 16 rows are + 1024 / + 4096 B
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int colA = wm * 64 + i * 32 + 16 * (grp & 1) + 4 * p4, colB = wn * 64 + i * 32 + 16 * (grp & 1) + 4 * p4;
        offA[i] = wg_lds_off(8 * h + q, colA >> 3) + (colA & 7) * 2;
        offB[i] = WG_KT * 256 + wg_lds_off(8 * h + q, colB >> 3) + (colB & 7) * 2;
    }

    wg_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    if (nstages > 0) { fetch(0); commit(0, 0); }
    __syncthreads();
    for (int st = 0; st < nstages; ++st) {
        const bool more = st + 1 < nstages;
        if (more) fetch(st + 1);
        const unsigned char* img = lds + (st & 1) * (2 * WG_KT * 256);
#pragma unroll
        for (int ks = 0; ks < WG_KT / 16; ++ks) {
            wg_bf16x8 fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                union { wg_s16x4 hh[2]; wg_bf16x8 v; } ua, ub;
                ua.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4)(img + offA[i] + ks * 4096));
                ua.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4)(img + offA[i] + ks * 4096 + 1024));
                ub.hh[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4)(img + offB[i] + ks * 4096));
                ub.hh[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4)(img + offB[i] + ks * 4096 + 1024));
                fa[i] = ua.v; fb[i] = ub.v;
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (more) commit(st + 1, (st + 1) & 1);
        __syncthreads();
    }

    // ---- bias gradient of this slice: 16 row lanes per column, added in lane order through LDS (the stage buffers are free now)
    float* lf = reinterpret_cast<float*>(lds);
    float gbv = 0.f;
    if (want_gb) {   // (block-uniform)
#pragma unroll
        for (int i = 0; i < 8; ++i) lf[srow * WG_TM + 8 * sch + i] = bsum[i];
        __syncthreads();
        if (tid < WG_TM) {
            gbv = lf[tid];
            for (int r = 1; r < 16; ++r) gbv += lf[r * WG_TM + tid];
        }
        __syncthreads();
    }

    const int tile = tile_id;
    if (a.slices > 1) {
        const int64_t ntiles = (int64_t)a.tiles_m * a.tiles_n;
        float4* slab = reinterpret_cast<float4*>(a.slabs) + ((int64_t)slice * ntiles + tile) * (16 * WG_THREADS);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    slab[((i * 2 + j) * 4 + g) * WG_THREADS + tid] = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        if (want_gb && tid < WG_TM) a.gb_slabs[((int64_t)slice * a.tiles_m + tm) * WG_TM + tid] = gbv;
        // publish, draw a ticket; the last arriver of the tile reduces
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        unsigned* flag = reinterpret_cast<unsigned*>(lds);
        if (tid == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned t = __hip_atomic_fetch_add(&a.tickets[tile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned last = t == (unsigned)(a.slices - 1);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            *flag = last;
        }
        __syncthreads();
        if (*flag == 0u) return;
        // slices in order; the 16 loads of one slice are independent and in flight together
        const float4* s0 = reinterpret_cast<const float4*>(a.slabs) + (int64_t)tile * (16 * WG_THREADS) + tid;
        const int64_t sstride = ntiles * (16 * WG_THREADS);
        for (int s = 0; s < a.slices; ++s) {
            float4 w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) w[u] = s0[s * sstride + u * WG_THREADS];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                wg_f32x16& c = acc[u >> 3][(u >> 2) & 1];
                const int g = u & 3;
                if (s == 0) { c[4 * g] = w[u].x; c[4 * g + 1] = w[u].y; c[4 * g + 2] = w[u].z; c[4 * g + 3] = w[u].w; }
                else { c[4 * g] += w[u].x; c[4 * g + 1] += w[u].y; c[4 * g + 2] += w[u].z; c[4 * g + 3] += w[u].w; }
            }
        }
        if (want_gb && tid < WG_TM) {
            const float* pb = a.gb_slabs + (int64_t)tm * WG_TM + tid;
            gbv = pb[0];
            for (int s = 1; s < a.slices; ++s) gbv += pb[(int64_t)s * a.tiles_m * WG_TM];
        }
    }

    // ---- C/D map of the 32x32 accumulator: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c0 + wn * 64 + j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int jj = j0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (jj < a.n && c < a.k) {
                    float* d = a.gw + (int64_t)jj * a.ld_gw + c;
                    *d = a.accumulate ? *d + acc[i][j][r] : acc[i][j][r];
                }
            }
        }
    if (want_gb && tid < WG_TM && j0 + tid < a.n) a.gb[j0 + tid] = a.gb_accumulate ? a.gb[j0 + tid] + gbv : gbv;
}

__global__ __launch_bounds__(256) void k_wgrad_zero_tickets(unsigned* __restrict__ tickets, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) tickets[i] = 0u;
}

// workspace: [tickets, one per tile, padded to 256 B][fp32 tile slabs: slices x tiles x 128 x 128][fp32 bias slabs: slices x tiles_m x 128]
static int64_t wg_ticket_bytes(int n, int k) { return ((int64_t)wg_tiles(n, WG_TM) * wg_tiles(k, WG_TN) * 4 + 255) / 256 * 256; }

extern "C" {

int32_t phc_wgrad_bf16_slices(int64_t rows, int32_t n, int32_t k) {
    if (rows < 1 || n < 1 || k < 1) return PHC_EINVAL;
    return wg_slices(rows, n, k);
}

int64_t phc_wgrad_bf16_workspace(int64_t rows, int32_t n, int32_t k) {
    if (rows < 1 || n < 1 || k < 1) return PHC_EINVAL;
    const int64_t s = wg_slices(rows, n, k), tm = wg_tiles(n, WG_TM), tn = wg_tiles(k, WG_TN);
    return wg_ticket_bytes(n, k) + s * tm * tn * (WG_TM * WG_TN * 4) + s * tm * (WG_TM * 4);
}

int32_t phc_wgrad_bf16(const void* gy, const void* y, const void* x, int64_t ld_x, int64_t rows, int32_t n, int32_t k, float* gw, int64_t ld_gw,
                       int32_t accumulate, void* gz, float* gb, int32_t gb_accumulate, void* workspace, void* stream) {
    if (!gy || !x || !gw || !workspace || rows < 1 || n < 1 || k < 1 || ld_x < k || ld_gw < k) return PHC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(gw) & 3) || (reinterpret_cast<uintptr_t>(gb) & 3)) return PHC_EINVAL;
    if ((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gz)) & 1) return PHC_EINVAL;
    WgradArgs a;
    a.gy = static_cast<const uint16_t*>(gy); a.y = static_cast<const uint16_t*>(y); a.x = static_cast<const uint16_t*>(x);
    a.ld_x = ld_x; a.rows = rows; a.ld_gw = ld_gw; a.n = n; a.k = k;
    a.slices = wg_slices(rows, n, k);
    a.rows_per_slice = wg_rows_per_slice(rows, a.slices);
    a.tiles_m = wg_tiles(n, WG_TM); a.tiles_n = wg_tiles(k, WG_TN);
    a.gw = gw; a.gb = gb; a.gz = static_cast<uint16_t*>(gz);
    a.accumulate = accumulate; a.gb_accumulate = gb_accumulate;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    const int64_t tb = wg_ticket_bytes(n, k);
    a.tickets = reinterpret_cast<unsigned*>(ws);
    a.slabs = reinterpret_cast<float*>(ws + tb);
    a.gb_slabs = a.slabs + (int64_t)a.slices * a.tiles_m * a.tiles_n * (WG_TM * WG_TN);
    if ((int64_t)a.tiles_m * a.tiles_n * a.slices > 0x7fffffff) return PHC_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (a.slices > 1) {
        const int ntiles = a.tiles_m * a.tiles_n;
        hipLaunchKernelGGL(k_wgrad_zero_tickets, dim3((ntiles + 255) / 256), dim3(256), 0, st, a.tickets, ntiles);
    }
    const uintptr_t gbits = reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gz);
    const bool vg = !(gbits & 15) && !(n & 7), vx = !(reinterpret_cast<uintptr_t>(x) & 15) && !(ld_x & 7) && !(k & 7);
    const dim3 grid((unsigned)((int64_t)a.tiles_n * a.tiles_m * a.slices)), block(WG_THREADS);
    if (vg && vx) hipLaunchKernelGGL((k_wgrad_bf16<true, true>), grid, block, 0, st, a);
    else if (vg) hipLaunchKernelGGL((k_wgrad_bf16<true, false>), grid, block, 0, st, a);
    else if (vx) hipLaunchKernelGGL((k_wgrad_bf16<false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_wgrad_bf16<false, false>), grid, block, 0, st, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

}  // extern "C"
