// phc_proj.hip -- phc_proj_advance: one env step of the thrown projectiles as one launch (contract: include/phc_amd.h; per-lane code: phc_proj.h).
//
// One lane group per env, G = 32 lanes (two envs per wavefront) when the model has at most 32 collision shapes, else 64; 256-thread blocks.  Lane s poses
// shape s once per launch and tests it in every sub-interval; the deepest candidate is found by two group minima (the gap, then the lowest shape index
// that holds it: phc_group.h), the winner's normal, contact point, normal velocity and owner come from its lane by ds_bpermute; every lane computes the
// impulse from them, and lane b adds it to its own body's row in registers and stores the row once at the end.  Slot state is loaded by every lane of
// the group from one address (one transaction) and stored by lane 0.  No lane returns early and no group operation stands under a divergent branch: the
// groups behind the last env run along on the last env and store nothing, and the sub-intervals of a slot are skipped only where no group of the wavefront
// has that slot in flight.
// Latency-bound: count x substeps dependent rounds of ~100 flops and two reductions.  Built with -ffp-contract=off and without fast-math.
// Also here: phc_proj_rows, the snapshot / select row copies around the task's two stepper launches (an env nothing struck keeps the plain launch's rows).
#include <hip/hip_runtime.h>
#include "phc_proj.h"
#include "phc_group.h"

using namespace phc;

template <int G>
struct ProjDevGroup {
    static constexpr int PER = 1;
    int lane;
    __device__ __forceinline__ void argmin(float& gap, int& idx) const {
        const float least = group_min<G>(gap);
        idx = group_min<G>(gap == least ? idx : 0x7fffffff);
        gap = least;
    }
    __device__ __forceinline__ bool any(bool v) const { return __any(v ? 1 : 0) != 0; }   // over the wavefront (both envs at G = 32): a uniform branch
    __device__ __forceinline__ float bcast(float v, int src) const { return group_bcast<G>(v, src); }
    __device__ __forceinline__ int bcast_i(int v, int src) const { return __shfl(v, src, G); }
};

template <int G>
__global__ __launch_bounds__(256) void k_proj_advance(phc_proj_args_t a) {
    const int64_t genv = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const bool live = genv < a.num_envs;
    ProjDevGroup<G> g;
    g.lane = (int)(threadIdx.x % G);
    proj_env(a, live ? genv : (int64_t)a.num_envs - 1, live, g, nullptr);
}

// phc_proj_rows: one block per env, the block's threads stride over the env's columns of every tensor pair (coalesced; a block whose env takes nothing leaves)
__global__ __launch_bounds__(256) void k_proj_rows(phc_proj_rows_t a) {
    proj_rows_env(a, (int64_t)blockIdx.x, (int)threadIdx.x, 256);
}

extern "C" int32_t phc_proj_rows(const phc_proj_rows_t* a, void* stream) {
    const int32_t rc = proj_rows_check(a);
    if (rc) return rc;
    if (a->num_envs == 0) return 0;
    hipLaunchKernelGGL(k_proj_rows, dim3((unsigned)a->num_envs), dim3(256), 0, (hipStream_t)stream, *a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

extern "C" int32_t phc_proj_advance(const phc_proj_args_t* a, void* stream) {
    const int32_t rc = proj_args_check(a);
    if (rc) return rc;
    if (a->num_envs == 0) return 0;
    const bool wide = a->num_shapes > 32 || a->num_bodies > 32;
    const int per_block = 256 / (wide ? 64 : 32);
    const dim3 grid((unsigned)(((int64_t)a->num_envs + per_block - 1) / per_block));
    if (wide) hipLaunchKernelGGL(k_proj_advance<64>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL(k_proj_advance<32>, grid, dim3(256), 0, (hipStream_t)stream, *a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
