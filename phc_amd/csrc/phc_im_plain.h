// phc_im_plain.h -- the PLAIN feature set of the imitation task, stated once: the values the feature selectors of phc_im_params_t / phc_im_buffers_t have
// in the default SMPL task (`compose([...])` without overrides -> HumanoidIm), as the structs that task builds hold them (tests/test_task_plain_cpu.py builds
// them on the CPU and reads this list back).  Plain host C++ (no HIP), like phc_im_check.h.
//
// From the one list come both
//   im_is_plain(model, lib, prm, buf)   host: may this launch take the plain instantiation of k_im_post_physics / k_im_reset?
//   pin_plain(prm, buf)                 device (phc_task_kernel.h): the listed fields as compile-time constants inside that instantiation,
// so that what the kernel assumes and what the host checks cannot drift apart.
//
// One entry per line, VAL(struct, field, value) or NUL(struct, pointer field): a field is listed only if the default task's structs hold that value, a
// pointer only if the default task passes NULL for it.  Not listed on purpose: numeric parameters and sizes, termination_distances, the flags that follow
// flags.im_eval / flags.no_collision_check (use_mean_termination, disable_collision_check), enable_early_termination, and every pointer the default task
// does pass (cycle_counter and point_goal are always allocated; reset_list is cleared per launch for the masked sweep; amp_ref_table comes and goes with the
// motion library).
#pragma once
#include "../../include/phc_amd.h"

#define PHC_IM_PLAIN_FIELDS(VAL, NUL) \
    VAL(prm, obs_v, 6) \
    VAL(prm, self_obs_v, 1) \
    VAL(prm, amp_obs_v, 1) \
    VAL(prm, num_force_sensors, 0) \
    VAL(prm, num_self_obs_hist, 0) \
    VAL(prm, num_self_obs_extra, 0) \
    VAL(prm, num_amp_obs_extra, 0) \
    VAL(prm, num_traj_samples, 1) \
    VAL(prm, track_body_reward, 0) \
    VAL(prm, remove_base_rot, 0) \
    VAL(prm, zero_out_far, 0) \
    VAL(prm, zero_out_far_train, 0) \
    VAL(prm, cycle_motion, 0) \
    VAL(prm, cycle_motion_xp, 0) \
    VAL(prm, power_reward, 1) \
    VAL(prm, local_root_obs, 1) \
    VAL(prm, root_height_obs, 1) \
    NUL(prm, self_obs_extra) \
    NUL(prm, amp_obs_extra) \
    NUL(buf, sampled_motion_ids) \
    NUL(buf, recovery_counter) \
    NUL(buf, cycle_phase) \
    NUL(buf, body_state_hist) \
    NUL(buf, offset_rand) \
    NUL(buf, occl_mask)

namespace phc {

// lanes per env: 32 while the articulation (with its extended reference bodies) fits, else 64
inline int group_lanes(int num_bodies, int num_ext) { return num_bodies + num_ext > 32 ? 64 : 32; }

// every listed field at its listed value, the spherical joint family, 32 lanes per env
inline bool im_is_plain(const phc_model_t* model, const phc_motion_lib_t* lib, const phc_im_params_t* prm, const phc_im_buffers_t* buf) {
    if (!model || !lib || !prm || !buf) return false;
    if (lib->dofs_per_joint == 1 || prm->dofs_per_joint == 1 || group_lanes(model->num_bodies, prm->num_ext_bodies) != 32) return false;
#define PHC_PLAIN_VAL(s, f, v) if (s->f != (v)) return false;
#define PHC_PLAIN_NUL(s, f) if (s->f != nullptr) return false;
    PHC_IM_PLAIN_FIELDS(PHC_PLAIN_VAL, PHC_PLAIN_NUL)
#undef PHC_PLAIN_VAL
#undef PHC_PLAIN_NUL
    return true;
}

}  // namespace phc
