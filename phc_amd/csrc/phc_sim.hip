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
#include "phc_sim_check.h"

// the instrumented library stamps the generic kernel only
#ifdef PHC_SIM_PROFILE
int32_t g_phc_sim_force_generic = 1;
#else
int32_t g_phc_sim_force_generic = 0;
#endif

extern "C" {

int32_t phc_sim_force_generic(int32_t on) {
    const int32_t old = g_phc_sim_force_generic;
    g_phc_sim_force_generic = on ? 1 : 0;
    return old;
}

int32_t phc_sim_model_facts(const phc_model_t* model_on_host) { return sim_model_facts(model_on_host); }

int32_t phc_sim_is_plain(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions, const int32_t* freeze_mask,
                         int32_t num_sim_calls) {
    return sim_is_plain(model, params, sim, actions, freeze_mask, num_sim_calls) ? 1 : 0;
}

int32_t phc_sim_step(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                     const float* pd_action_offset, const float* pd_action_scale, const int32_t* freeze_mask,
                     int32_t num_sim_calls, void* stream) {
    int32_t rc = check_sim_step(model, params, sim, actions, pd_action_offset, pd_action_scale, num_sim_calls);
    if (rc || sim->num_envs == 0) return rc;
    sim_launch<true, false>(model, *params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, (hipStream_t)stream, nullptr, 0, WrenchArgs<false>());
    return launch_status();
}

int32_t phc_refresh_body_state(const phc_model_t* model, const phc_sim_state_t* sim, void* stream) {
    int32_t rc = check_model(model);
    if (rc) return rc;
    if (!sim || sim->num_envs < 0) return PHC_EINVAL;
    if (sim->num_envs == 0) return 0;
    phc_sim_params_t prm = {};
    prm.substeps = 1;
    sim_launch<false, false>(model, prm, sim, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, nullptr, 0, WrenchArgs<false>());
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
    sim_launch<false, false>(model, prm, sim, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, env_ids, num, WrenchArgs<false>());
    return launch_status();
}

// the same launch over num_envs slots of a device list whose entries are env ids or num_envs: the kernel idles a slot whose env is not below num_envs
int32_t phc_refresh_body_state_masked(const phc_model_t* model, const phc_sim_state_t* sim, const int64_t* fall_list, void* stream) {
    int32_t rc = check_model(model);
    if (rc) return rc;
    if (!sim || sim->num_envs < 0 || !fall_list) return PHC_EINVAL;
    if (sim->num_envs == 0) return 0;
    phc_sim_params_t prm = {};
    prm.substeps = 1;
    sim_launch<false, false>(model, prm, sim, nullptr, nullptr, nullptr, nullptr, 0, (hipStream_t)stream, fall_list, sim->num_envs, WrenchArgs<false>());
    return launch_status();
}

}  // extern "C"
