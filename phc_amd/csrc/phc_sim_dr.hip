// phc_sim_dr.hip -- phc_sim_step_dr: the stepper with per-env physics (per-env friction, per-env model blocks for both joint families, torque noise;
// include/phc_amd.h), and the DR instantiations of k_sim_step it launches.  Its own translation unit, compiled with phc_sim.hip's flags (phc_amd/build.py):
// see phc_sim_kernel.h.
#include "phc_sim_kernel.h"
#include "phc_sim_check.h"

extern "C" int32_t phc_sim_step_dr(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                        const float* pd_action_offset, const float* pd_action_scale, const int32_t* freeze_mask, int32_t num_sim_calls,
                        const phc_sim_dr_t* dr, void* stream) {
    // nothing randomised and nothing phc_sim_step has no kernel for (env-shape blocks of a revolute model): exactly phc_sim_step -- its checks, its launch
    const bool tensors = dr && (dr->env_friction || dr->torque_noise);
    const bool revolute_blocks = model && model->num_shapes > 1 && model->num_dof == model->num_bodies - 1 && model->num_bodies > 2;
    if (!tensors && !revolute_blocks)
        return phc_sim_step(model, params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, stream);
    int32_t rc = check_sim_step_dr(model, params, sim, actions, pd_action_offset, pd_action_scale, num_sim_calls, dr);
    if (rc || sim->num_envs == 0) return rc;
    DrArgs<true> d = {};
    if (dr) { d.env_friction = dr->env_friction; d.torque_noise = dr->torque_noise; d.k = dr->k; d.key = dr->key; d.env_offset = dr->env_offset; }
    sim_launch<true, false, true>(model, *params, sim, actions, pd_action_offset, pd_action_scale, freeze_mask, num_sim_calls, (hipStream_t)stream, nullptr, 0,
                                  WrenchArgs<false>(), d);
    return launch_status();
}
