// phc_getup.hip -- phc_getup_assign and phc_task_draws (contract: include/phc_amd.h; per-env code and the rules: phc_getup.h).
//
// phc_getup_assign is ONE workgroup of 1024 threads (16 wavefronts) whatever N is: the ranks of the FALL envs and the list of free slots are prefix sums over
// all N envs and N slots, and a single workgroup orders its phases with workgroup barriers -- no second launch, no spinning on another block's flag, no atomics,
// and a result that cannot depend on a grid.  The work is a few words per env (N = 4096: four tiles), the launch is latency-bound either way.
//   phase 1  a lane per env, tiles of 1024: release, draw, decide, publish kind / normal_flag (getup_env_decide)
//   phase 2  per tile one block scan of (slot free, env FALL) packed in one word (16 bits each: a tile holds 1024) -- wavefront scans by __shfl_up, the 16
//            wavefront sums through LDS -- with the running totals carried from tile to tile: free_list[] in slot order, fall_list[] in env order
//   phase 3  a lane per FALL env: its slot free_list[pi(r)] (getup_env_pick)
//   phase 4  a lane per element of the teleported rows (13 + num_dof floats per FALL env), coalesced along the row (getup_env_teleport)
// The launch count behind the permutation key is read by every lane before the first barrier and written by lane 0 after the last: all lanes of a launch see
// one value, and a replayed capture finds the next one.
// Built with -ffp-contract=off and without fast-math: the draws compare floats that the host build of phc_getup.h must reproduce bit for bit.
#include <hip/hip_runtime.h>
#include "phc_getup.h"

using namespace phc;

// inclusive scan of `v` over the workgroup; `total` = the sum.  `wsum`: GETUP_BLOCK / 64 words of LDS.
__device__ __forceinline__ uint32_t block_scan_inclusive(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    __syncthreads();   // (the previous tile's readers of wsum are done)
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < GETUP_BLOCK / 64; ++w) {
        const uint32_t s = wsum[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(GETUP_BLOCK) void k_getup_assign(phc_getup_args_t a) {
    __shared__ uint32_t wsum[GETUP_BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t N = a.num_envs;
    const uint64_t count = (uint64_t)*a.launch_count;
    const float p_recovery = a.prob[0], p_fall = a.prob[1];
    for (int64_t i = tid; i < N; i += GETUP_BLOCK) getup_env_decide(a, i, p_recovery, p_fall, nullptr);
    __syncthreads();
    int64_t F = 0, n_f = 0;
    for (int64_t base = 0; base < N; base += GETUP_BLOCK) {
        const int64_t i = base + tid;
        const uint32_t is_free = i < N && a.avail[i] == 0, is_fall = i < N && a.kind[i] == GETUP_FALL;
        const uint32_t v = is_free | (is_fall << 16);
        uint32_t total;
        const uint32_t before = block_scan_inclusive(v, wsum, &total) - v;
        if (is_free) a.free_list[F + (before & 0xffffu)] = (int32_t)i;
        if (is_fall) a.fall_list[n_f + (before >> 16)] = i;
        F += total & 0xffffu;
        n_f += total >> 16;
    }
    __syncthreads();
    const uint64_t pkey = getup_perm_key(a.key, count, (uint32_t)F);
    for (int64_t r = tid; r < n_f; r += GETUP_BLOCK) getup_env_pick(a, r, F, r < F ? (int64_t)getup_perm(pkey, (uint32_t)F, (uint32_t)r) : -1);
    __syncthreads();
    const int W = 13 + a.num_dof;
    const int64_t moved = (n_f < F ? n_f : F) * W;
    for (int64_t e = tid; e < moved; e += GETUP_BLOCK) getup_env_teleport(a, e / W, (int)(e % W));
    if (tid == 0) *a.launch_count = (int64_t)(count + 1u);
}

__global__ __launch_bounds__(256) void k_task_draws(int num_envs, uint64_t key, int64_t env_offset, int32_t* __restrict__ k, float* __restrict__ cycle_phase,
                                                    float* __restrict__ offset_rand) {
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= num_envs) return;
    task_draws_env(key, env_offset, k, cycle_phase, offset_rand, env);
}

static inline int32_t launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

extern "C" int32_t phc_getup_assign(const phc_getup_args_t* a, void* stream) {
    const int32_t rc = getup_args_check(a);
    if (rc) return rc;
    if (a->num_envs == 0) return 0;
    hipLaunchKernelGGL(k_getup_assign, dim3(1), dim3(GETUP_BLOCK), 0, (hipStream_t)stream, *a);
    return launch_status();
}

extern "C" int32_t phc_task_draws(int32_t num_envs, uint64_t key, int64_t env_offset, int32_t* k, float* cycle_phase, float* offset_rand, void* stream) {
    const int32_t rc = task_draws_check(num_envs, env_offset, k);
    if (rc) return rc;
    if (num_envs == 0) return 0;
    hipLaunchKernelGGL(k_task_draws, dim3((unsigned)(((int64_t)num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, num_envs, key, env_offset, k,
                       cycle_phase, offset_rand);
    return launch_status();
}
