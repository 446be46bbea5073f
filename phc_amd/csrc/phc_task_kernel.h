// phc_task_kernel.h -- the two task kernels of the env step, k_im_post_physics and k_im_reset, as templates: phc_kernels.hip instantiates the generic ones
// (per joint family and group width), phc_kernels_plain.hip the PLAIN ones of the default SMPL task (phc_im_plain.h).  Two translation units because the
// compiler's output for a kernel depends on its module (the precedent is phc_sim_kernel.h / phc_sim_wrench.hip): the generic kernels stay instruction for
// instruction what they were before the plain ones existed.
#pragma once
#include <hip/hip_runtime.h>
#include "phc_im.h"
#include "phc_im_plain.h"
#include "phc_group.h"  // group_sum / group_or

using namespace phc;

// The task kernels are instantiated per joint family (DPJ = DoFs per joint: 3 spherical / 1 revolute) with the struct fields
// that select the family pinned to compile-time constants, so the SMPL instantiation carries none of the robot branches.
template <int DPJ>
__device__ __forceinline__ void pin_family(phc_motion_lib_t& lib, phc_im_params_t& prm) {
    lib.dofs_per_joint = DPJ; prm.dofs_per_joint = DPJ;
    if (DPJ == 3) { lib.num_ext_bodies = 0; prm.num_ext_bodies = 0; }
}
// The PLAIN instantiation (<DPJ = 3, G = 32> only) also pins every feature selector of phc_im_plain.h to the value the default SMPL task has: the paths behind them
// -- the other observation versions, zero_out_far, cycle_motion, fut_tracks, occlusion, the getup counters, the extra columns -- are then not compiled in, and
// the uniform branches on them no longer fence the loads (im_is_plain is the host's side of the same list; a launch takes this instantiation only when it holds).
template <bool PLAIN>
__device__ __forceinline__ void pin_plain(phc_im_params_t& prm, phc_im_buffers_t& buf) {
    if (PLAIN) {
#define PHC_PIN_VAL(s, f, v) s.f = (v);
#define PHC_PIN_NUL(s, f) s.f = nullptr;
        PHC_IM_PLAIN_FIELDS(PHC_PIN_VAL, PHC_PIN_NUL)
#undef PHC_PIN_VAL
#undef PHC_PIN_NUL
    }
}

template <int DPJ, int G, bool PLAIN = false>
__global__ __launch_bounds__(256) void k_im_post_physics(phc_model_t model, phc_motion_lib_t lib, phc_im_params_t prm,
                                                        phc_sim_state_t sim, phc_im_buffers_t buf, int n_reset_bodies) {
    pin_family<DPJ>(lib, prm);
    pin_plain<PLAIN>(prm, buf);
    const int lane = threadIdx.x & (G - 1);
    const int64_t env = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    if (env >= sim.num_envs) return;  // whole lane group exits together
    PHC_PTL(0, env, lane)
    if (blockIdx.x == 0 && threadIdx.x == 0 && buf.reset_rng_counter) *buf.reset_rng_counter += 1;   // (one writer; no reset launch runs concurrently)
    // Everything the launch reads that does not depend on something else it reads is REQUESTED here, before the first wait: the clip's table
    // entries, the body's and the root's state, the per-env scalars of the prologue (a wavefront waits for a load at its first use; this
    // kernel's wavefronts spend three quarters of their life waiting, profiles/r03_task/post_physics_timeline.txt)
    const int64_t progress = buf.progress_buf[env] + 1;  // humanoid.py:1637
    const FrameTab tab = frame_tab(lib, motion_id_of(buf, env));
    const int jb = lane < model.num_bodies ? lane : 0;
    const BodyState body = load_body(sim.rigid_body_state, env, model.num_bodies, jb);
    const BodyState root = load_body(sim.rigid_body_state, env, model.num_bodies, 0);
    const ImStepCtx c = im_post_prologue(lib, prm, sim, buf, env, progress);
    const float prev_goal = (prm.zero_out_far && buf.point_goal) ? buf.point_goal[env] : 0.f;  // read before lane 0 overwrites it
    PHC_PTL(1, env, lane)
    RewardPartial rp = im_post_lane(model, lib, prm, sim, buf, env, lane, c, tab, body, root);
    PHC_PTL(9, env, lane)
    amp_shift_lane(prm, buf, env, lane, G);   // (every S-th step; reads the old window, writes rows 1.. of the new one: after the frame in row 0)
    float s_pos = group_sum<G>(rp.pos), s_rot = group_sum<G>(rp.rot), s_vel = group_sum<G>(rp.vel), s_ang = group_sum<G>(rp.angvel);
    float s_pow = group_sum<G>(rp.power), s_dist = group_sum<G>(rp.dist);
    int fallen = group_or<G>(rp.fallen);
    PHC_PTL(10, env, lane)
    if (lane == 0)
        im_post_finalize(lib, prm, buf, model.num_bodies, env, c, progress, s_pos, s_rot, s_vel, s_ang, s_pow, s_dist, rp.root_dist,
                         prev_goal, fallen, n_reset_bodies);
    PHC_PTL(11, env, lane)
}

// Reset of a list of envs.  One lane group per (env, AMP history frame k): group k == 0 also imposes the state
// and recomputes the observations.  blockDim = 256.
// (which env and which start time: im_reset_pick, phc_im.h)

#ifdef PHC_SIM_PROFILE   // one lane group's timeline through the reset kernel (scripts/probes/reset_timeline.py; the product library has none of this)
static __device__ unsigned long long g_phc_rtl[64];   // (per translation unit; phc_debug_reset_timeline reads phc_kernels.hip's, and the instrumented library
static __device__ int g_phc_rtl_group = -1;            // launches the generic kernels only)  r * 16 + k of the group that stamps
#define PHC_RTL(i) if (rtl_on) { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0); const unsigned long long t_ = __builtin_readcyclecounter(); \
        if (lane == 0) g_phc_rtl[i] = t_; __builtin_amdgcn_sched_barrier(0); }
#else
#define PHC_RTL(i)
#endif

// Measured alternative (round 2, profiles/r02_notes.md): ONE workgroup per listed env with its S history-frame groups side by side
// (blockDim = G * S), so that the S lookups of an env -- S + 1 consecutive clip frames -- share a CU's L1: 46.6 us vs 34 us for this
// geometry (the ten groups of an env then hit one clip region, i.e. the same HBM channels, at the same instant).  Not kept.
template <int DPJ, bool RNG, int G, bool PLAIN = false>
__global__ __launch_bounds__(256) void k_im_reset(phc_model_t model, phc_motion_lib_t lib, phc_im_params_t prm, phc_sim_state_t sim,
                                                 phc_im_buffers_t buf, int num_reset, const int64_t* __restrict__ env_ids,
                                                 const float* __restrict__ phase, int start_at_zero, uint64_t rng_key) {
    pin_family<DPJ>(lib, prm);
    pin_plain<PLAIN>(prm, buf);
    const int lane = threadIdx.x & (G - 1);
    // listed env (grid.x); grid.y: 0 = state + self observation, 1 = task observation, 2 + k = AMP history frame k -- the heaviest groups
    // are dispatched first and no group carries more than one lookup chain
    const int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int k = (int)blockIdx.y;
#ifdef PHC_SIM_PROFILE
    const bool rtl_on = (int)(r * 16 + k) == g_phc_rtl_group;
#endif
    PHC_RTL(0)
    if (!im_reset_pick_live<RNG>(buf, r, k, lane, num_reset, env_ids)) return;
    const int64_t env = im_reset_pick_env<RNG>(buf, r, env_ids);
    const float t = im_reset_pick_time<RNG>(buf, lib, env, r, phase, start_at_zero, rng_key);   // (PHC_RTL(1) stood inside the pick)
    PHC_RTL(2)
    if (k < 2) im_reset_lane(model, lib, prm, sim, buf, env, lane, t, env_ids != nullptr, 1 << k);
    PHC_RTL(3)
    if (k >= 2) {
        if (prm.amp_ref_table != nullptr) im_reset_amp_table_lane(lib, prm, buf, model.num_bodies, env, lane, G, t, k - 2);
        else im_reset_amp_lane(lib, prm, buf, model.num_bodies, env, lane, t, k - 2);
    }
    PHC_RTL(4)
}
