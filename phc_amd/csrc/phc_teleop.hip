// phc_teleop.hip -- phc_teleop_rewards: HumanoidTeleop's regularisation rewards, their per-env state and the recovery window after a velocity push as one
// launch per env step, behind phc_im_post_physics (contract: include/phc_amd.h; per-lane code: phc_teleop.h).
//
// A group of 32 lanes per env, two envs per wavefront, 256-thread blocks (8 envs), whole groups of the tail masked.  Lanes run along a DoF row: lane l reads
// elements l, l + 32, ... of the env's rows of dof_state / dof_force / actions / last_* (consecutive addresses over the group), lane f < num_feet its foot.
// Every active term is summed over the group by phc_group.h's butterfly (four DPP steps and one cross-row permute, no LDS allocation, no atomics): a fixed
// order, so the same inputs give the same bits at any num_envs, and the host build of phc_teleop.h adds in that very order.  The term mask is uniform over the
// launch: a term that is off costs neither loads nor a reduction.  Latency-bound: the loads are requested in two rounds (the env's clock, its clip's table
// entries, rew_buf and the rows; then the frame records of the reference speed and the feet), each round's independent of one another.
// Built with -ffp-contract=off and without fast-math, like phc_dr.hip.
#include <hip/hip_runtime.h>
#include "phc_teleop.h"
#include "phc_group.h"

using namespace phc;

__global__ __launch_bounds__(256) void k_teleop_rewards(phc_motion_lib_t lib, phc_teleop_args_t a) {
    const int64_t env = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / PHC_TELEOP_G;
    const int lane = (int)(threadIdx.x % PHC_TELEOP_G);
    if (env >= a.num_envs) return;
    // two rounds of loads: the env's clock, its clip's table entries, rew_buf and the DoF rows; then the frame records and the feet
    const bool air = teleop_on(a, PHC_TELEOP_FEET_AIR_TIME);
    TeleopClock clock = {};
    if (air) clock = teleop_clock(lib, a, env);
    const float rew_in = teleop_rew_in(a, env, lane);
    TeleopSums s = teleop_rows_lane(a, env, lane);
    const float moving = air ? teleop_ref_moving(lib, a, clock) : 1.0f;
    teleop_feet_lane(a, env, lane, s);
#pragma unroll
    for (int t = 0; t < PHC_TELEOP_NUM_TERMS; ++t)
        if (teleop_on(a, t)) s.v[t] = group_sum<PHC_TELEOP_G>(s.v[t]);
    teleop_finish(a, env, lane, s, moving, rew_in);
}

extern "C" int32_t phc_teleop_rewards(const phc_motion_lib_t* lib, const phc_teleop_args_t* a, void* stream) {
    const int32_t rc = teleop_args_check(lib, a);
    if (rc) return rc;
    if (a->num_envs == 0) return 0;
    phc_motion_lib_t l = {};
    if (lib) l = *lib;
    const int64_t threads = (int64_t)a->num_envs * PHC_TELEOP_G;
    hipLaunchKernelGGL(k_teleop_rewards, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, l, *a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
