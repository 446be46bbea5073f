// phc_obs_aug.hip -- phc_obs_augment and phc_occl_advance (contract: include/phc_amd.h; per-lane code and the rules: phc_obs_aug.h).
//
// phc_obs_augment streams obs [N, num_obs] once: ONE workgroup of 256 threads per selection slot (a row, or an entry of env_ids), lanes along the column pairs,
// passes of 256 pairs while the row has more.  The row's flag / id and its counter are read once by every lane (one address: a broadcast), the workgroup of an
// unselected row leaves before any other access, and lane 0 writes k + 1 behind a workgroup barrier -- after every wavefront of the row has read k.  No row is
// shared between workgroups, so nothing races on k.
//   accesses  lane l of a pass touches columns 2 (p + l), 2 (p + l) + 1: a wavefront covers 512 contiguous bytes.  Where the row starts on an 8-byte boundary
//             (every row of an even width, every other row of an odd one) the pair is one 8-byte load and one 8-byte store; elsewhere two 4-byte accesses each,
//             which cover the same lines.  The last pair of an odd width is a single column either way.
//   dropout   the row's T <= 1024 decisions are drawn once into LDS (a byte each) by the first T lanes' passes, in front of the columns.
//   maths     a pair shares one logf / sqrtf and one sinf + cosf; two hashes per pair.  The library transcendentals make the kernel VALU-bound, not
//             HBM-bound (profiles/obs_device/README.md has the achieved fraction).
// phc_occl_advance: one lane per env over J <= 64 bodies.
// Built with -ffp-contract=off and without fast-math: the draws compare floats that the host build of phc_obs_aug.h must reproduce bit for bit, and a noised
// element may differ from it by the transcendentals alone.
#include <hip/hip_runtime.h>
#include "phc_obs_aug.h"

using namespace phc;

__global__ __launch_bounds__(OBS_AUG_BLOCK) void k_obs_augment(phc_obs_aug_args_t a) {
    __shared__ uint8_t drop_s[OBS_AUG_MAX_SAMPLES];
    const int tid = threadIdx.x;
    const int64_t env = obs_aug_env_of(a, (int64_t)blockIdx.x);
    if (env < 0) return;   // (uniform over the workgroup)
    const uint32_t k = (uint32_t)a.k[env], ge = (uint32_t)(a.env_offset + env);
    const int P = (a.num_obs + 1) / 2, W = obs_aug_width(a);
    const uint8_t* drop = nullptr;
    if (W > 0) {
        for (int t = tid; t < a.num_samples; t += OBS_AUG_BLOCK) drop_s[t] = obs_aug_dropped(a, ge, k, t);
        drop = drop_s;
    }
    __syncthreads();   // the decisions are in LDS; every wavefront has read k
    if (tid == 0) a.k[env] = (int32_t)(k + 1u);
    float* row = a.obs + env * (int64_t)a.num_obs;
    if (!(a.noise_std > 0.f) && !drop) return;
    if (((uintptr_t)row & 7u) == 0) {
        const int full = a.num_obs / 2;   // pairs with both columns
        for (int j = tid; j < full; j += OBS_AUG_BLOCK) {
            float z0 = 0.f, z1 = 0.f;
            if (a.noise_std > 0.f) aug_normal_pair(a.key, ge, k, (uint32_t)j, &z0, &z1);
            float2* p = reinterpret_cast<float2*>(row) + j;
            float2 v = *p;
            v.x = obs_aug_value(a, drop, W, 2 * j, v.x, z0);
            v.y = obs_aug_value(a, drop, W, 2 * j + 1, v.y, z1);
            *p = v;
        }
        if (full < P && tid == (full & (OBS_AUG_BLOCK - 1))) obs_aug_pair(a, row, drop, W, ge, k, full);   // the odd width's last column
    } else {
        for (int j = tid; j < P; j += OBS_AUG_BLOCK) obs_aug_pair(a, row, drop, W, ge, k, j);
    }
}

__global__ __launch_bounds__(256) void k_occl_advance(int num_envs, int J, uint64_t key, int64_t env_offset, int32_t* __restrict__ k, float prob, int32_t span_lo,
                                                      int32_t span_hi, int64_t* __restrict__ count, uint8_t* __restrict__ mask) {
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= num_envs) return;
    occl_advance_env(J, key, env_offset, k, prob, span_lo, span_hi, count, mask, env);
}

static inline int32_t launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

extern "C" int32_t phc_obs_augment(const phc_obs_aug_args_t* a, void* stream) {
    const int32_t rc = obs_augment_check(a);
    if (rc) return rc;
    const int64_t slots = obs_aug_slots(*a);
    if (slots == 0) return 0;
    hipLaunchKernelGGL(k_obs_augment, dim3((unsigned)slots), dim3(OBS_AUG_BLOCK), 0, (hipStream_t)stream, *a);
    return launch_status();
}

extern "C" int32_t phc_occl_advance(int32_t num_envs, int32_t J, uint64_t key, int64_t env_offset, int32_t* k, float prob, int32_t span_lo, int32_t span_hi,
                                    int64_t* count, uint8_t* mask, void* stream) {
    const int32_t rc = occl_advance_check(num_envs, J, env_offset, k, prob, span_lo, span_hi, count, mask);
    if (rc) return rc;
    if (num_envs == 0) return 0;
    hipLaunchKernelGGL(k_occl_advance, dim3((unsigned)(((int64_t)num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, num_envs, J, key, env_offset, k, prob,
                       span_lo, span_hi, count, mask);
    return launch_status();
}
