// phc_dr.hip -- phc_dr_advance: the per-env-step part of domain randomisation -- control delay and velocity push -- as one launch (contract: include/phc_amd.h;
// per-lane code: phc_dr.h).
//
// One lane per env, 256-thread blocks, tail lanes masked.  A lane reads its counter k, its delay and (Q + 2) D floats of its own rows; its draws come from
// (key, env_offset + env, k) -- the counter is the env's own, so no lane reads a word another lane of the launch writes and a replayed capture draws anew.
// Latency-bound.  Built with -ffp-contract=off and without fast-math: integer state and draws are bit-equal to the host build of phc_dr.h.
#include <hip/hip_runtime.h>
#include "phc_dr.h"

using namespace phc;

__global__ __launch_bounds__(256) void k_dr_advance(phc_dr_args_t a) {
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.num_envs) return;
    dr_env(a, env);
}

extern "C" int32_t phc_dr_advance(const phc_dr_args_t* a, void* stream) {
    const int32_t rc = dr_args_check(a);
    if (rc) return rc;
    if (a->num_envs == 0) return 0;
    hipLaunchKernelGGL(k_dr_advance, dim3((unsigned)(((int64_t)a->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
