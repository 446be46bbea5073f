// phc_sim_wrench.hip -- phc_sim_step_wrench: the stepper with an external force / torque per rigid body (include/phc_amd.h), and the WRENCH instantiations of
// k_sim_step it launches.  Its own translation unit, compiled with phc_sim.hip's flags (phc_amd/build.py): see phc_sim_kernel.h.
#include "phc_sim_kernel.h"

extern "C" int32_t phc_sim_step_check(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                                      const float* pd_action_offset, const float* pd_action_scale, int32_t num_sim_calls);   // (phc_sim.hip)

// the WRENCH twins of phc_sim.hip's launches -- one env-shape block, two wavefronts per SIMD (phc_sim_step_wrench refuses the rest)
template <int JT, bool RIGID>
static void sim_launch_wrench_cm(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions, const float* off,
                                 const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream, const WrenchArgs<true>& wr) {
    const int64_t groups = sim->num_envs;
    const bool wide = model->num_bodies > 32;
    const bool lag = !RIGID && prm.inertia_lag != 0;
    if (lag && wide)
        hipLaunchKernelGGL((k_sim_step<true, JT, 64, false, RIGID, 2, !RIGID, true>), dim3(groups), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, nullptr, 0, wr);
    else if (lag)
        hipLaunchKernelGGL((k_sim_step<true, JT, 32, false, RIGID, 2, !RIGID, true>), dim3((groups + 1) / 2), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, nullptr, 0, wr);
    else if (wide)
        hipLaunchKernelGGL((k_sim_step<true, JT, 64, false, RIGID, 2, false, true>), dim3(groups), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, nullptr, 0, wr);
    else
        hipLaunchKernelGGL((k_sim_step<true, JT, 32, false, RIGID, 2, false, true>), dim3((groups + 1) / 2), dim3(64), 0, stream, *model, prm, *sim, actions, off, scale, freeze,
                           num_sim_calls, nullptr, 0, wr);
}
template <int JT>
static void sim_launch_wrench_jt(const phc_model_t* model, const phc_sim_params_t& prm, const phc_sim_state_t* sim, const float* actions, const float* off,
                                 const float* scale, const int32_t* freeze, int num_sim_calls, hipStream_t stream, const WrenchArgs<true>& wr) {
    if (prm.contact_model == 1) sim_launch_wrench_cm<JT, true>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, wr);
    else sim_launch_wrench_cm<JT, false>(model, prm, sim, actions, off, scale, freeze, num_sim_calls, stream, wr);
}

extern "C" int32_t phc_sim_step_wrench(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                            const float* pd_action_offset, const float* pd_action_scale, const int32_t* freeze_mask, int32_t num_sim_calls,
                            const float* ext_force, const float* ext_torque, int32_t wrench_sim_calls, void* stream) {
    const int32_t calls = wrench_sim_calls < 0 ? 0 : (wrench_sim_calls > num_sim_calls ? num_sim_calls : wrench_sim_calls);
    // no wrench: exactly phc_sim_step -- its checks, its launch
    if ((!ext_force && !ext_torque) || calls == 0)
        return phc_sim_step(model, params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, stream);
    if (model && model->num_shapes > 1) return PHC_EUNSUPPORTED;      // per-env body shapes: the instantiation closest to spilling has no wrench twin
    if (params && params->lane_mapping == 3) return PHC_EUNSUPPORTED;  // the three-wavefront experiment build has none either
    int32_t rc = phc_sim_step_check(model, params, sim, actions, pd_action_offset, pd_action_scale, num_sim_calls);
    if (rc || sim->num_envs == 0) return rc;
    WrenchArgs<true> wr;
    wr.force = ext_force; wr.torque = ext_torque; wr.nsub = calls * params->substeps;
    if (model->num_dof == model->num_bodies - 1 && model->num_bodies > 2)
        sim_launch_wrench_jt<PHC_JT_REVOLUTE>(model, *params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, (hipStream_t)stream, wr);
    else
        sim_launch_wrench_jt<PHC_JT_SPHERICAL>(model, *params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, (hipStream_t)stream, wr);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int32_t)e;
}

