// phc_sim_check.h -- what the stepper's entry points refuse, stated once: phc_sim.hip, phc_sim_wrench.hip and the host emulation (oracle/hostemu/hostemu.cpp)
// return these codes from these conditions in this order.  Plain host C++ (no HIP; also compiled with every `float` a `double`, oracle/hostemu/hostemu64.cpp).
#pragma once
#include "phc_aba.h"   // PHC_SC_MAX_PER_LANE, PHC_CP_BITS, include/phc_amd.h

namespace phc {

inline int32_t check_model(const phc_model_t* m) {
    if (!m || m->num_bodies < 1 || m->num_bodies > PHC_MAX_BODIES || !m->ints || !m->floats) return PHC_EINVAL;
    // all-spherical (SMPL family) or all-revolute (H1 / G1) articulations
    if (m->num_dof != 3 * (m->num_bodies - 1) && m->num_dof != m->num_bodies - 1) return PHC_EUNSUPPORTED;
    if (m->num_shapes > 1 && m->num_dof != 3 * (m->num_bodies - 1)) return PHC_EUNSUPPORTED;   // per-env shapes: SMPL family only
    if (m->num_shapes > 1 && (m->int_stride <= 0 || m->float_stride <= 0)) return PHC_EINVAL;
    return 0;
}

// the argument and option checks of a stepping launch
inline int32_t check_sim_step(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
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

// a stepping launch with an external wrench: what it refuses on top of, and ahead of, check_sim_step
inline int32_t check_sim_step_wrench(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                                     const float* pd_action_offset, const float* pd_action_scale, int32_t num_sim_calls) {
    if (model && model->num_shapes > 1) return PHC_EUNSUPPORTED;      // per-env body shapes: the instantiation closest to spilling has no wrench twin
    if (params && params->lane_mapping == 3) return PHC_EUNSUPPORTED;  // the three-wavefront experiment build has none either
    return check_sim_step(model, params, sim, actions, pd_action_offset, pd_action_scale, num_sim_calls);
}

// a stepping launch with domain randomisation (phc_sim_step_dr): what it refuses ahead of check_sim_step, and the one thing it accepts that check_sim_step does
// not -- env-shape blocks of a revolute model (the blocks' strides are checked here, the rest of the model as one block)
inline int32_t check_sim_step_dr(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions,
                                 const float* pd_action_offset, const float* pd_action_scale, int32_t num_sim_calls, const phc_sim_dr_t* dr) {
    if (params && params->lane_mapping == 3) return PHC_EUNSUPPORTED;   // the three-wavefront experiment build has no DR twin
    if (!model) return PHC_EINVAL;
    const bool revolute = model->num_dof == model->num_bodies - 1 && model->num_bodies > 2;
    if (dr && dr->torque_noise && (!revolute || (params && params->control_mode == 0))) return PHC_EUNSUPPORTED;   // the target shift is the explicit drives' identity
    if (dr && dr->torque_noise && !dr->k) return PHC_EINVAL;
    if (dr && sim && (dr->env_offset < 0 || dr->env_offset > ((int64_t)1 << 32) || sim->num_envs < 0 ||
                      (dr->env_offset + (int64_t)sim->num_envs) * (int64_t)(model->num_dof > 0 ? model->num_dof : 1) > (int64_t)1 << 32)) return PHC_EINVAL;
    if (model->num_shapes > 1 && (model->int_stride <= 0 || model->float_stride <= 0 || !sim || !sim->env_shape)) return PHC_EINVAL;
    phc_model_t one = *model;
    one.num_shapes = 1;
    return check_sim_step(&one, params, sim, actions, pd_action_offset, pd_action_scale, num_sim_calls);
}

}  // namespace phc
