// phc_im_check.h -- what the task entry points refuse, stated once: phc_kernels.hip and the host emulation (oracle/hostemu/hostemu.cpp) return these codes from
// these conditions in this order.  Plain host C++ (no HIP), like phc_sim_check.h, which keeps the only check_model.
// A count of zero ("nothing to do") is accepted where the entry point returns 0 for it: conditions behind that return are not looked at.
#pragma once
#include "phc_sim_check.h"

namespace phc {

// model, motion library and task parameters of one articulation family: what every task launch but phc_motion_state needs
inline int32_t check_im(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm) {
    if (int32_t rc = check_model(model)) return rc;
    if (!lib || !prm || lib->num_bodies != model->num_bodies) return PHC_EINVAL;
    const int dpj = model->num_dof == model->num_bodies - 1 && model->num_bodies > 2 ? 1 : 3;
    if ((lib->dofs_per_joint == 1 ? 1 : 3) != dpj || (prm->dofs_per_joint == 1 ? 1 : 3) != dpj) return PHC_EINVAL;
    if (prm->num_ext_bodies < 0 || prm->num_ext_bodies != lib->num_ext_bodies || model->num_bodies + prm->num_ext_bodies > PHC_MAX_BODIES) return PHC_EINVAL;
    if (prm->num_ext_bodies > 0 && (!prm->ext_parent || !prm->ext_offset)) return PHC_EINVAL;
    if (!prm->track_slot || !prm->reset_mask || !prm->termination_distances || !prm->key_body_ids || !prm->amp_joint_slot) return PHC_EINVAL;
    return prm->num_key_bodies > 32 ? PHC_EUNSUPPORTED : 0;
}
inline int32_t check_im_post_physics(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                                     const phc_im_buffers_t* buf) {
    if (int32_t rc = check_im(model, lib, prm)) return rc;
    if (!sim || !buf || buf->amp_obs_in == buf->amp_obs_out) return PHC_EINVAL;
    if (prm->cycle_motion && (!buf->cycle_counter || !buf->cycle_phase)) return PHC_EINVAL;
    return prm->zero_out_far && !buf->point_goal ? PHC_EINVAL : 0;
}
inline int32_t check_im_reset(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                              const phc_im_buffers_t* buf, int32_t num_reset, const float* phase, int32_t start_at_zero) {
    if (int32_t rc = check_im(model, lib, prm)) return rc;
    return !sim || !buf || num_reset < 0 || (!start_at_zero && !phase) ? PHC_EINVAL : 0;
}
inline int32_t check_im_reset_done(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                                   const phc_im_buffers_t* buf) {
    if (int32_t rc = check_im(model, lib, prm)) return rc;
    if (!sim || !buf) return PHC_EINVAL;
    if (sim->num_envs == 0) return 0;
    return buf->reset_list && (!buf->reset_count || buf->reset_sublist_cap * PHC_RESET_SUBLISTS < sim->num_envs) ? PHC_EINVAL : 0;
}
inline int32_t check_im_reset_from_state(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_sim_state_t* sim,
                                         const phc_im_buffers_t* buf, int32_t num_reset, const int64_t* env_ids) {
    if (int32_t rc = check_im(model, lib, prm)) return rc;
    return !sim || !buf || num_reset < 0 || (num_reset > 0 && !env_ids) ? PHC_EINVAL : 0;
}
inline int32_t check_amp_obs_demo(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, int32_t n) {
    if (int32_t rc = check_im(model, lib, prm)) return rc;
    return n < 0 ? PHC_EINVAL : 0;
}
inline int32_t check_amp_ref_table(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, int64_t num_frames,
                                   const int64_t* next_frame, const float* table) {
    if (int32_t rc = check_im(model, lib, prm)) return rc;
    return !table || !next_frame || num_frames < 0 || num_frames > lib->num_frames_total ? PHC_EINVAL : 0;
}
inline int32_t check_motion_state(const phc_motion_lib_t* lib, int32_t n) {
    return !lib || n < 0 || lib->num_bodies + lib->num_ext_bodies > PHC_MAX_BODIES ? PHC_EINVAL : 0;
}

}  // namespace phc
