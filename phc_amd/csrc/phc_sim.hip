// phc_sim.hip -- the articulated-body stepper (S10): the launches of k_sim_step (phc_sim_kernel.h) and their C-ABI entry points.
//
// Own translation unit because it is compiled with different code-generation flags than the task kernels
// (phc_amd/build.py): `-ffast-math -fno-slp-vectorize`.
//   * -fno-slp-vectorize: the SLP vectoriser packs the 3-vector algebra into v_pk_fma_f32 and then needs ~840 v_mov to
//     marshal register pairs (3975 static instructions, 16 scratch ops); without it 3466 instructions and no scratch;
//   * -ffast-math: v_rcp / v_sqrt / hardware sin-cos instead of the IEEE division and libm expansions: 1949 static
//     instructions.  The stepper has no reference arithmetic to match bit-for-bit (Isaac Gym is closed); its oracle
//     tolerances (tests/test_dynamics.py) hold with these approximations.  The task kernels, which ARE pinned to the
//     reference at 1e-5 and rely on IEEE NaN/division semantics, are NOT compiled this way.
#include <hip/hip_runtime.h>
#include "phc_aba.h"

// Phase profile of the stepper (scripts/sim_phase_profile.py builds a SEPARATE library with -DPHC_SIM_PROFILE; the product
// library never contains this): per-wavefront s_memtime deltas accumulated per phase, summed over wavefronts into a device array.
#ifdef PHC_SIM_PROFILE
__device__ unsigned long long g_phc_prof[16];
__device__ unsigned long long g_phc_prof_wg[8192][10];   // the same per workgroup (= wavefront), of the LAST launch: the launch lasts as long as its slowest wavefront
__device__ unsigned long long g_phc_prof_where[8192][2];   // round 5: [start cycle of the wavefront, XCC_ID << 32 | HW_ID]: WHERE and WHEN the slow wavefronts ran
extern "C" int32_t phc_debug_profile_wg(unsigned long long* out, int32_t nwg) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phc_prof_wg), sizeof(unsigned long long) * 10 * (nwg < 8192 ? nwg : 8192)) == hipSuccess ? 0 : -1;
}
extern "C" int32_t phc_debug_profile_where(unsigned long long* out, int32_t nwg) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phc_prof_where), sizeof(unsigned long long) * 2 * (nwg < 8192 ? nwg : 8192)) == hipSuccess ? 0 : -1;
}
extern "C" int32_t phc_debug_profile(unsigned long long* out16, int32_t reset) {
    if (out16 && hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_phc_prof), sizeof(g_phc_prof)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_phc_prof), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
// phase ablation (scripts/probes/sim_ablation.py): bit b set = phase b of the list there is skipped (timing only; the results are then meaningless)
__device__ int g_phc_skip;
extern "C" int32_t phc_debug_set_skip(int32_t mask) { return hipMemcpyToSymbol(HIP_SYMBOL(g_phc_skip), &mask, sizeof(mask)) == hipSuccess ? 0 : -1; }
// single-wave timeline (scripts/probes/sim_timeline.py): workgroup g_phc_tl_block stamps s_memtime at PHC_TL(id) points of sub-step 1
__device__ unsigned long long g_phc_tl[512];
__device__ int g_phc_tl_block = -1;
extern "C" int32_t phc_debug_timeline(unsigned long long* out512, int32_t block) {
    if (out512 && hipMemcpyFromSymbol(out512, HIP_SYMBOL(g_phc_tl), sizeof(g_phc_tl)) != hipSuccess) return -1;
    unsigned long long z[512] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phc_tl), z, sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_phc_tl_block), &block, sizeof(block)) == hipSuccess ? 0 : -1;
}
#define PHC_TL_DECL int tl_n = 0; const bool tl_on = (int)blockIdx.x == g_phc_tl_block;
#define PHC_TL(id) if (tl_on && tl_sub == 1 && tl_n < 255) { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_readcyclecounter(); \
        if (threadIdx.x == 0) { g_phc_tl[2 * tl_n] = (unsigned long long)(id); g_phc_tl[2 * tl_n + 1] = t_; } ++tl_n; __builtin_amdgcn_sched_barrier(0); }
#define PHC_SKIP_DECL const int skip_mask = g_phc_skip;
#define PHC_SKIP(b) ((skip_mask >> (b)) & 1)
#define PHC_PROF_DECL unsigned long long prof_acc[10] = {0}; unsigned long long prof_t = __builtin_readcyclecounter(); const unsigned long long prof_t0 = prof_t; \
        const unsigned long long prof_hw = ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) | (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);
#define PHC_PROF(i) if (!PHC_SKIP(15)) { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_waitcnt(0); const unsigned long long t_ = __builtin_readcyclecounter(); prof_acc[i] += t_ - prof_t; prof_t = t_; __builtin_amdgcn_sched_barrier(0); }
#define PHC_PROF_FLUSH if (threadIdx.x == 0 && !PHC_SKIP(15)) { for (int i_ = 0; i_ < 10; ++i_) { atomicAdd(&g_phc_prof[i_], prof_acc[i_]); if (blockIdx.x < 8192) g_phc_prof_wg[blockIdx.x][i_] = prof_acc[i_]; } atomicAdd(&g_phc_prof[15], 1ull); \
        if (blockIdx.x < 8192) { g_phc_prof_where[blockIdx.x][0] = prof_t0; g_phc_prof_where[blockIdx.x][1] = prof_hw; } }
#endif

// the kernel; with PHC_SIM_PROFILE the hooks above are compiled into it
#include "phc_sim_kernel.h"

template <bool STEP, int JT, bool SHAPES, bool RIGID>
static void sim_launch_cm(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions,
                          const float* off, const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream,
                          const int64_t* env_ids, int num_listed) {
    const int64_t groups = env_ids ? num_listed : sim->num_envs;
    const bool wide = model->num_bodies > 32;   // more bodies than a 32-lane group holds: one env per wavefront
    const bool occ3 = STEP && !RIGID && !SHAPES && JT == PHC_JT_SPHERICAL && !wide && prm.lane_mapping == 3;   // (experiment knob, see k_sim_step)
    const bool lag = STEP && !RIGID && prm.inertia_lag != 0;
    if (occ3)
        hipLaunchKernelGGL((k_sim_step<STEP, JT, 32, SHAPES, RIGID, (STEP && !RIGID && !SHAPES && JT == PHC_JT_SPHERICAL) ? 3 : 2>), dim3((groups + 1) / 2), dim3(64), 0, stream,
                           *model, prm, *sim, actions, off, scale, freeze, num_sim_calls, env_ids, num_listed, WrenchArgs<false>());
    else if (lag && wide)
        hipLaunchKernelGGL((k_sim_step<STEP, JT, 64, SHAPES, RIGID, 2, STEP && !RIGID>), dim3(groups), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, env_ids, num_listed, WrenchArgs<false>());
    else if (lag)
        hipLaunchKernelGGL((k_sim_step<STEP, JT, 32, SHAPES, RIGID, 2, STEP && !RIGID>), dim3((groups + 1) / 2), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, env_ids, num_listed, WrenchArgs<false>());
    else if (wide)
        hipLaunchKernelGGL((k_sim_step<STEP, JT, 64, SHAPES, RIGID>), dim3(groups), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, env_ids, num_listed, WrenchArgs<false>());
    else
        hipLaunchKernelGGL((k_sim_step<STEP, JT, 32, SHAPES, RIGID>), dim3((groups + 1) / 2), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, env_ids, num_listed, WrenchArgs<false>());
}
template <bool STEP, int JT, bool SHAPES>
static void sim_launch_jt(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions,
                          const float* off, const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream,
                          const int64_t* env_ids, int num_listed) {
    if (STEP && prm.contact_model == 1)   // rigid ground contact: its own instantiation, the penalty kernel is untouched by it
        sim_launch_cm<STEP, JT, SHAPES, STEP>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed);
    else
        sim_launch_cm<STEP, JT, SHAPES, false>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed);
}

template <bool STEP>
static void sim_launch(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions,
                       const float* off, const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream,
                       const int64_t* env_ids = nullptr, int num_listed = 0) {
    if (model->num_dof == model->num_bodies - 1 && model->num_bodies > 2)  // one revolute joint per body (robots; one shape)
        sim_launch_jt<STEP, PHC_JT_REVOLUTE, false>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed);
    else if (model->num_shapes > 1 && sim->env_shape != nullptr)   // per-env body shapes (SMPL family)
        sim_launch_jt<STEP, PHC_JT_SPHERICAL, true>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed);
    else
        sim_launch_jt<STEP, PHC_JT_SPHERICAL, false>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, env_ids, num_listed);
}

static inline int32_t launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

extern "C" {

static int32_t check_model(const phc_model_t* m) {
    if (!m || m->num_bodies < 1 || m->num_bodies > PHC_MAX_BODIES || !m->ints || !m->floats) return PHC_EINVAL;
    // all-spherical (SMPL family) or all-revolute (H1 / G1) articulations
    if (m->num_dof != 3 * (m->num_bodies - 1) && m->num_dof != m->num_bodies - 1) return PHC_EUNSUPPORTED;
    if (m->num_shapes > 1 && m->num_dof != 3 * (m->num_bodies - 1)) return PHC_EUNSUPPORTED;   // per-env shapes: SMPL family only
    if (m->num_shapes > 1 && (m->int_stride <= 0 || m->float_stride <= 0)) return PHC_EINVAL;
    return 0;
}

// the argument and option checks of a stepping launch: phc_sim_step and, from its own translation unit, phc_sim_step_wrench (not part of the public header)
int32_t phc_sim_step_check(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                              const float* pd_action_offset, const float* pd_action_scale, int32_t num_sim_calls) {
    int32_t rc = check_model(model);
    if (rc) return rc;
    if (!params || !sim || sim->num_envs < 0 || params->substeps < 1 || num_sim_calls < 0) return PHC_EINVAL;
    if (actions && (!pd_action_offset || !pd_action_scale)) return PHC_EINVAL;
    if (sim->num_envs == 0) return 0;
    // pairs are dealt round-robin to the lanes of an env's group: PHC_SC_MAX_PER_LANE each
    if (params->self_collision && model->num_collision_pairs > PHC_SC_MAX_PER_LANE * (model->num_bodies > 32 ? 64 : 32)) return PHC_EUNSUPPORTED;
    if (params->lane_mapping != 0 && params->lane_mapping != 1 && params->lane_mapping != 3) return PHC_EUNSUPPORTED;   // (2 was the two-bodies-per-lane kernel of rounds 1-2: removed)
    if (params->contact_model != 0 && params->contact_model != 1) return PHC_EUNSUPPORTED;
    if (params->contact_model == 1 && (params->contact_iterations < 2 || !(params->contact_impedance > 0.f))) return PHC_EINVAL;
    if (params->contact_model == 1 && params->inertia_lag) return PHC_EUNSUPPORTED;   // (the rigid model re-solves every sub-step contact_iterations times with fresh impedances)
    if (params->inertia_lag && params->lane_mapping == 3) return PHC_EUNSUPPORTED;   // (the three-wavefront experiment build has no lagged instantiation: it would silently run fresh)
    if (params->contact_model == 1 && model->max_body_contact_pts > 32) return PHC_EUNSUPPORTED;   // c_active / c_removed are 32-bit masks: a point beyond them could never be released
    if (params->inertia_lag && model->max_body_contact_pts > PHC_CP_BITS) return PHC_EUNSUPPORTED;  // c_touch: tail points would alternate between full and no force
    return 0;
}

int32_t phc_sim_step(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                     const float* pd_action_offset, const float* pd_action_scale, const int32_t* freeze_mask,
                     int32_t num_sim_calls, void* stream) {
    int32_t rc = phc_sim_step_check(model, params, sim, actions, pd_action_offset, pd_action_scale, num_sim_calls);
    if (rc || sim->num_envs == 0) return rc;
    sim_launch<true>(model, *params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, (hipStream_t)stream);
    return launch_status();
}

int32_t phc_refresh_body_state(const phc_model_t* model, const phc_sim_state_t* sim, void* stream) {
    int32_t rc = check_model(model);
    if (rc) return rc;
    if (!sim || sim->num_envs < 0) return PHC_EINVAL;
    if (sim->num_envs == 0) return 0;
    phc_sim_params_t prm = {};
    prm.substeps = 1;
    sim_launch<false>(model, prm, sim, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream);
    return launch_status();
}

int32_t phc_refresh_body_state_indexed(const phc_model_t* model, const phc_sim_state_t* sim, int32_t num, const int64_t* env_ids,
                                       void* stream) {
    int32_t rc = check_model(model);
    if (rc) return rc;
    if (!sim || num < 0 || (num > 0 && !env_ids)) return PHC_EINVAL;
    if (num == 0) return 0;
    phc_sim_params_t prm = {};
    prm.substeps = 1;
    sim_launch<false>(model, prm, sim, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, env_ids, num);
    return launch_status();
}

}  // extern "C"
