// phc_push.hip -- phc_push_advance: one step of the push schedule as one launch (contract: include/phc_amd.h; per-lane code: phc_push.h).
//
// One lane per env, 256-thread blocks, tail lanes masked.  A lane loads its five state words (coalesced [N] arrays), draws its five uniforms from
// (key, env_offset + env, k) -- the counter k is the env's own, so no lane reads a word another lane of the launch writes and a replayed capture
// draws anew -- runs the transition and stores the state; of force[env] it touches at most the row it clears and the row it fills.
// Latency-bound (a few hundred bytes per lane, one dependent load where a push starts).  Built with -ffp-contract=off and without fast-math: the
// integer state is bit-equal to the host build of phc_push.h.
#include <hip/hip_runtime.h>
#include "phc_push.h"

using namespace phc;

__global__ __launch_bounds__(256) void k_push_advance(phc_push_args_t a) {
    const int64_t env = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (env >= a.num_envs) return;
    push_env(a, env);
}

extern "C" int32_t phc_push_advance(const phc_push_args_t* a, void* stream) {
    const int32_t rc = push_args_check(a);
    if (rc) return rc;
    if (a->num_envs == 0) return 0;
    hipLaunchKernelGGL(k_push_advance, dim3((unsigned)(((int64_t)a->num_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
