// phc_sim_wrench.hip -- phc_sim_step_wrench: the stepper with an external force / torque per rigid body (include/phc_amd.h), and the WRENCH instantiations of
// k_sim_step it launches.  Its own translation unit, compiled with phc_sim.hip's flags (phc_amd/build.py): see phc_sim_kernel.h.
#include "phc_sim_kernel.h"
#include "phc_sim_check.h"

extern "C" int32_t phc_sim_step_wrench(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                            const float* pd_action_offset, const float* pd_action_scale, const int32_t* freeze_mask, int32_t num_sim_calls,
                            const float* ext_force, const float* ext_torque, int32_t wrench_sim_calls, void* stream) {
    const int32_t calls = wrench_sim_calls < 0 ? 0 : (wrench_sim_calls > num_sim_calls ? num_sim_calls : wrench_sim_calls);
    // no wrench: exactly phc_sim_step -- its checks, its launch
    if ((!ext_force && !ext_torque) || calls == 0)
        return phc_sim_step(model, params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, stream);
    int32_t rc = check_sim_step_wrench(model, params, sim, actions, pd_action_offset, pd_action_scale, num_sim_calls);
    if (rc || sim->num_envs == 0) return rc;
    WrenchArgs<true> wr;
    wr.force = ext_force; wr.torque = ext_torque; wr.nsub = calls * params->substeps;
    sim_launch<true, true>(model, *params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, (hipStream_t)stream, nullptr, 0, wr);
    return launch_status();
}
