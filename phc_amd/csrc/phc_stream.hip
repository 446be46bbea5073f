// phc_stream.hip -- phc_stream_track: tracking of streamed keypoints (HumanoidImDemo / HumanoidImMCPDemo) as one launch per env step, behind
// phc_im_post_physics, and one behind every reset launch (contract: include/phc_amd.h; per-lane code: phc_stream.h).
//
// A group of 32 lanes per env, two envs per wavefront, 256-thread blocks (8 envs), whole groups of the tail masked.  Lanes run along the bodies: lane l
// carries bodies l and l + 32 (G1 has 38), so a ring sample [NB, 3] is read at consecutive addresses over the group; the root's ring, the env's counters and
// the fold rows are the same address in every lane of the group (one transaction).  The limb scale and track_err are summed over the group by phc_group.h's
// butterfly (four DPP steps and one cross-row permute, no LDS allocation, no atomics): a fixed order, so the same inputs give the same bits at any num_envs,
// and the host build of phc_stream.h adds in that very order.  The reference of the body in track slot 0 reaches the other lanes by one group broadcast.
// Latency-bound: per body, the L - 1 older ring samples and the fold rows are independent loads, all requested before the first store of the lane.
// Built with -ffp-contract=off and without fast-math, like phc_teleop.hip: the filter sums and the velocity difference are fp64, rounded once.
#include <hip/hip_runtime.h>
#include "phc_stream.h"
#include "phc_group.h"

using namespace phc;

__global__ __launch_bounds__(256) void k_stream_track(int nb, phc_im_params_t prm, phc_stream_args_t a) {
    const int64_t env = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / PHC_STREAM_G;
    const int lane = (int)(threadIdx.x % PHC_STREAM_G);
    if (env >= a.num_envs) return;
    StreamRef ref[PHC_STREAM_ROUNDS];
#pragma unroll
    for (int r = 0; r < PHC_STREAM_ROUNDS; ++r) ref[r].pos = ref[r].vel = v3(0.f, 0.f, 0.f);
    if (a.mode == PHC_STREAM_ADVANCE) {
        const StreamHead h = stream_head(a, env);
        const float scale = stream_scale(a, a.limb_scale ? group_sum<PHC_STREAM_G>(stream_limb_lane(a, nb, env, lane)) : 0.f);
#pragma unroll
        for (int r = 0; r < PHC_STREAM_ROUNDS; ++r) {
            const int j = lane + PHC_STREAM_G * r;
            if (j < nb) ref[r] = stream_advance_lane(a, nb, env, j, h, scale, j == 0);
        }
        if (lane == 0) stream_head_advance(a, env, h);
    } else {
#pragma unroll
        for (int r = 0; r < PHC_STREAM_ROUNDS; ++r) {
            const int j = lane + PHC_STREAM_G * r;
            if (j < nb) ref[r] = stream_load_lane(a, nb, env, j);
        }
    }
    // the reference of the body in track slot 0, from the lane and round that hold it
    const int src = a.track_root_body % PHC_STREAM_G;
    const V3 mine = a.track_root_body < PHC_STREAM_G ? ref[0].pos : ref[1].pos;
    const V3 ref_root = v3(group_bcast<PHC_STREAM_G>(mine.x, src), group_bcast<PHC_STREAM_G>(mine.y, src), group_bcast<PHC_STREAM_G>(mine.z, src));
    float err = 0.f;
#pragma unroll
    for (int r = 0; r < PHC_STREAM_ROUNDS; ++r) {
        const int j = lane + PHC_STREAM_G * r;
        if (j < nb) err += stream_obs_lane(prm, a, nb, env, j, ref[r], ref_root);
    }
    err = group_sum<PHC_STREAM_G>(err);
    if (lane == 0) stream_finish(prm, a, env, err);
}

extern "C" int32_t phc_stream_track(const phc_model_t* model, const phc_im_params_t* prm, const phc_stream_args_t* a, void* stream) {
    const int32_t rc = stream_args_check(model, prm, a);
    if (rc) return rc;
    if (a->num_envs == 0) return 0;
    const int64_t threads = (int64_t)a->num_envs * PHC_STREAM_G;
    hipLaunchKernelGGL(k_stream_track, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int)model->num_bodies, stream_params(*prm, *a), *a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}
