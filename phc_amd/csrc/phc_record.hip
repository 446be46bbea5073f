// phc_record.hip -- phc_motion_record (contract: include/phc_amd.h; per-lane code, the rules and the hazards: phc_record.h).
//
// A streaming kernel: about 1 KB stored per env and call, nothing computed but the root's exp map and, for the robots, one axis x angle product per body.
// A group of G lanes per env, 256-thread workgroups (8 groups of 32 lanes, 4 of 64); an env's row is written by the lanes of ONE wavefront.
//   stores    the NB quaternions are 16 contiguous bytes per lane (64 NB contiguous bytes per group), the pose_aa rows 12 per lane, the dof_pos / ref_body_pos
//             columns consecutive floats over the lanes: whole 128-byte lines but for the ends of the runs.
//   loads     the reads of rigid_body_state (the quaternion out of every 52-byte body record) are the kernel's only gather; dof_state is read at stride 2
//             (the positions of the position / velocity pairs).  The model tables (joint type, DoF start, axis) are shared by every env and stay in cache.
//   counters  read by every lane in front of the wavefront-scope ordering point, updated by lane 0 behind it (phc_record.h, "counter race").
// Built with -ffp-contract=off and without fast-math: everything but the root's exp map is a copy or one product, compared bit for bit with the host build.
#include <hip/hip_runtime.h>
#include "phc_record.h"

using namespace phc;

template <int G>
__global__ __launch_bounds__(RECORD_BLOCK) void k_motion_record(phc_model_t m, phc_motion_record_args_t a) {
    const int lane = threadIdx.x & (G - 1);
    const int64_t env = ((int64_t)blockIdx.x * RECORD_BLOCK + threadIdx.x) / G;
    if (env >= a.num_envs) return;   // (a whole lane group takes or skips this together)
    const RecDecision d = record_decide(a, env);
    if (d.f >= 0) record_lane(m, a, env, d.f, lane, G);
    // every lane of the env's group has read the counters; nothing of the group's accesses may move across this point
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0) record_commit(a, env, d);
}

extern "C" int32_t phc_motion_record_width(int32_t num_bodies, int32_t num_ext, int32_t num_dof, int32_t flags) {
    if (num_bodies < 1 || num_ext < 0 || num_dof < 1 || num_dof > 3 * PHC_MAX_BODIES) return PHC_EINVAL;
    if ((int64_t)num_bodies + num_ext > PHC_MAX_BODIES) return PHC_EUNSUPPORTED;
    return record_width(num_bodies, num_ext, num_dof, flags);
}

extern "C" int32_t phc_motion_record(const phc_model_t* m, const phc_motion_record_args_t* a, void* stream) {
    const int32_t rc = motion_record_check(m, a);
    if (rc) return rc;
    const int G = record_group(a->num_bodies, a->num_ext);
    const unsigned blocks = (unsigned)(((int64_t)a->num_envs * G + RECORD_BLOCK - 1) / RECORD_BLOCK);
    if (G == 64) hipLaunchKernelGGL(k_motion_record<64>, dim3(blocks), dim3(RECORD_BLOCK), 0, (hipStream_t)stream, *m, *a);
    else hipLaunchKernelGGL(k_motion_record<32>, dim3(blocks), dim3(RECORD_BLOCK), 0, (hipStream_t)stream, *m, *a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
