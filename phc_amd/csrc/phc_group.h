// phc_group.h -- reductions and a broadcast over the G lanes of an env's lane group (device only; the env kernels of phc_kernels.hip and phc_eval.hip).
#pragma once
#include <hip/hip_runtime.h>

// Sum / or over the G lanes of an env's group, result in every lane.  Inside a row of 16 lanes the butterfly runs on DPP operands (quad_perm xor 1,
// xor 2, row_half_mirror, row_mirror: folded into the add, ~4 cycles each); only the steps across rows are ds_bpermute round trips (~64 cycles
// each, round 3: seven sums x five dependent permutes were 1.8 k cycles of the post-physics wavefront's 38 k).
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int G>
__device__ __forceinline__ float group_sum(float v) {
    v += __int_as_float(dpp_i<0xB1>(__float_as_int(v)));    // quad_perm:[1,0,3,2]
    v += __int_as_float(dpp_i<0x4E>(__float_as_int(v)));    // quad_perm:[2,3,0,1]
    v += __int_as_float(dpp_i<0x141>(__float_as_int(v)));   // row_half_mirror
    v += __int_as_float(dpp_i<0x140>(__float_as_int(v)));   // row_mirror
#pragma unroll
    for (int m = 16; m < G; m <<= 1) v += __shfl_xor(v, m, G);
    return v;
}
template <int G>
__device__ __forceinline__ int group_or(int v) {
    v |= dpp_i<0xB1>(v); v |= dpp_i<0x4E>(v); v |= dpp_i<0x141>(v); v |= dpp_i<0x140>(v);
#pragma unroll
    for (int m = 16; m < G; m <<= 1) v |= __shfl_xor(v, m, G);
    return v;
}
// Minimum over the G lanes of an env's group, result in every lane: the same butterfly.  Every lane of the group must be active -- a DPP operand read
// from a lane that EXEC has switched off is 0, which the sum ignores and the minimum does not.  (fminf: no NaN operands expected.)
template <int G>
__device__ __forceinline__ float group_min(float v) {
    v = fminf(v, __int_as_float(dpp_i<0xB1>(__float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_i<0x4E>(__float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_i<0x141>(__float_as_int(v))));
    v = fminf(v, __int_as_float(dpp_i<0x140>(__float_as_int(v))));
#pragma unroll
    for (int m = 16; m < G; m <<= 1) v = fminf(v, __shfl_xor(v, m, G));
    return v;
}
template <int G>
__device__ __forceinline__ int group_min(int v) {
    v = min(v, dpp_i<0xB1>(v)); v = min(v, dpp_i<0x4E>(v)); v = min(v, dpp_i<0x141>(v)); v = min(v, dpp_i<0x140>(v));
#pragma unroll
    for (int m = 16; m < G; m <<= 1) v = min(v, __shfl_xor(v, m, G));
    return v;
}
// The value that lane `src` (0 .. G-1) of the env's group holds, in every lane of the group.
template <int G>
__device__ __forceinline__ float group_bcast(float v, int src) { return __shfl(v, src, G); }

// Hand-over through LDS between the lanes of ONE wavefront: what the lanes wrote (or added with ds_add) in front of this point is what any lane reads behind it.
// PRECONDITION: the workgroup is a single wavefront (blockDim == 64).  The LDS operations of one wavefront are issued and performed in program order, so the
// hardware needs nothing here -- a read issued right behind the write returns the written data -- and the AMDGPU memory model emits no instruction for a
// wavefront-scope fence.  What is left is for the compiler: the two fences keep it from moving a memory access across the point, the wave barrier from moving
// anything else of the schedule.  __syncthreads() in the same place is a workgroup-scope fence: an `s_waitcnt lgkmcnt(0)` that drains the LDS queue before the
// next read may even be issued.  Kernels with larger workgroups keep __syncthreads().  (Not for hand-overs through global memory.)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
