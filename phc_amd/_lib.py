"""ctypes binding of libphc_amd.so (the C ABI in include/phc_amd.h).

This is the only way the Python host side reaches the device code.  There is NO CPU
fallback: if the shared library is missing or a symbol is absent the import fails loudly.
"""
import ctypes as C
import os

# torch bundles its own libamdhip64.so: it must be in the process BEFORE libphc_amd.so is dlopen'ed, otherwise the
# system copy from /opt/rocm gets loaded next to it and kernels are registered with a runtime that owns no device
# (launches then fail with hipErrorNoDevice).  PyTorch is plumbing here: device memory, streams, torch.distributed.
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
# PHC_AMD_LIB: load another build of the SAME library (scripts/sim_phase_profile.py: the instrumented stepper); never a fallback
LIB_PATH = os.environ.get("PHC_AMD_LIB") or os.path.join(HERE, "libphc_amd.so")

c_f = C.c_float
c_i32 = C.c_int32
c_i64 = C.c_int64
c_p = C.c_void_p


class Model(C.Structure):
    _fields_ = [("num_bodies", c_i32), ("num_dof", c_i32), ("max_level", c_i32), ("num_contact_pts", c_i32),
                ("ints", c_p), ("floats", c_p), ("num_collision_pairs", c_i32),
                ("num_shapes", c_i32), ("int_stride", c_i32), ("float_stride", c_i32), ("max_body_contact_pts", c_i32), ("sim_plain_facts", c_i32)]


class MotionLib(C.Structure):
    _fields_ = [("frames", c_p), ("num_frames_total", c_i64), ("frame_stride", c_i32), ("num_bodies", c_i32),
                ("num_motions", c_i32), ("motion_lengths", c_p), ("motion_dt", c_p), ("motion_num_frames", c_p),
                ("length_starts", c_p), ("num_ext_bodies", c_i32), ("dofs_per_joint", c_i32)]


class SimState(C.Structure):
    _fields_ = [("num_envs", c_i32), ("root_states", c_p), ("dof_state", c_p), ("rigid_body_state", c_p),
                ("contact_force", c_p), ("dof_force", c_p), ("pd_target", c_p), ("force_sensor", c_p), ("env_shape", c_p), ("pd_ref", c_p)]


class SimParams(C.Structure):
    _fields_ = [("sim_dt", c_f), ("substeps", c_i32), ("control_freq_inv", c_i32), ("gravity_z", c_f),
                ("contact_stiffness", c_f), ("contact_damping", c_f), ("friction", c_f), ("friction_viscous", c_f),
                ("angular_damping", c_f), ("max_angular_velocity", c_f), ("contact_offset", c_f),
                ("control_mode", c_i32), ("limit_stiffness", c_f), ("limit_damping", c_f),
                ("self_collision", c_i32), ("self_stiffness_scale", c_f), ("self_damping_ratio", c_f), ("lane_mapping", c_i32),
                ("num_force_sensors", c_i32), ("force_sensor_body", c_i32 * 4),
                ("contact_model", c_i32), ("contact_iterations", c_i32), ("contact_impedance", c_f), ("max_depenetration_velocity", c_f),
                ("bounce_threshold_velocity", c_f), ("restitution", c_f), ("inertia_lag", c_i32), ("force_average", c_i32)]


class ColsumJob(C.Structure):
    _fields_ = [("partial", c_p), ("out", c_p), ("nchunks", c_i32), ("cols", c_i32), ("accumulate", c_i32)]


class ImParams(C.Structure):
    _fields_ = [("dt", c_f), ("max_episode_length", c_i32),
                ("k_pos", c_f), ("k_rot", c_f), ("k_vel", c_f), ("k_ang_vel", c_f),
                ("w_pos", c_f), ("w_rot", c_f), ("w_vel", c_f), ("w_ang_vel", c_f),
                ("power_reward", c_i32), ("power_coefficient", c_f),
                ("enable_early_termination", c_i32), ("use_mean_termination", c_i32), ("disable_collision_check", c_i32),
                ("local_root_obs", c_i32), ("root_height_obs", c_i32),
                ("num_track_bodies", c_i32), ("track_slot", c_p), ("reset_mask", c_p), ("num_reset_bodies", c_i32), ("first_reset_body", c_i32),
                ("termination_distances", c_p),
                ("num_key_bodies", c_i32), ("key_body_ids", c_p),
                ("num_amp_joints", c_i32), ("amp_joint_slot", c_p),
                ("num_amp_obs_steps", c_i32), ("num_amp_obs_per_step", c_i32),
                ("num_self_obs", c_i32), ("num_task_obs", c_i32),
                ("cycle_motion", c_i32), ("zero_out_far", c_i32), ("close_distance", c_f), ("far_distance", c_f),
                ("dofs_per_joint", c_i32), ("num_ext_bodies", c_i32), ("ext_parent", c_p), ("ext_offset", c_p), ("obs_v", c_i32),
                ("self_obs_v", c_i32), ("num_force_sensors", c_i32), ("amp_obs_v", c_i32),
                ("remove_base_rot", c_i32), ("num_self_obs_extra", c_i32), ("num_amp_obs_extra", c_i32),
                ("num_traj_samples", c_i32), ("traj_sample_timestep", c_f), ("track_body_reward", c_i32), ("num_self_obs_hist", c_i32), ("zero_out_far_train", c_i32), ("zero_out_far_steps", c_i32), ("cycle_motion_xp", c_i32),
                ("self_obs_extra", c_p), ("amp_obs_extra", c_p), ("amp_ref_table", c_p)]


class ImBuffers(C.Structure):
    _fields_ = [("progress_buf", c_p), ("reset_buf", c_p), ("terminate_buf", c_p), ("rew_buf", c_p), ("reward_raw", c_p),
                ("obs_buf", c_p), ("amp_obs_in", c_p), ("amp_obs_out", c_p), ("sampled_motion_ids", c_p),
                ("motion_start_times", c_p), ("motion_start_times_offset", c_p), ("global_offset", c_p),
                ("ref_body_pos", c_p), ("ref_body_rot", c_p), ("ref_body_vel", c_p), ("ref_dof_pos", c_p),
                ("cycle_counter", c_p), ("recovery_counter", c_p), ("point_goal", c_p), ("cycle_phase", c_p),
                ("reset_list", c_p), ("reset_count", c_p), ("reset_slot", c_i32), ("reset_sublist_cap", c_i32), ("body_state_hist", c_p), ("offset_rand", c_p), ("occl_mask", c_p), ("amp_env_stride", C.c_int64), ("reset_rng_counter", c_p)]


class PpoParams(C.Structure):
    _fields_ = [("e_clip", c_f), ("critic_coef", c_f), ("entropy_coef", c_f), ("bounds_loss_coef", c_f), ("clip_value", c_i32)]


RENDER_PALETTE = 16          # PHC_RENDER_PALETTE
RENDER_MARKER_ID = 1000      # PHC_RENDER_MARKER_ID
RENDER_MAX_PIXELS = 1 << 24  # PHC_RENDER_MAX_PIXELS
RENDER_MAX_SHAPES = 128      # PHC_RENDER_MAX_SHAPES
RENDER_MAX_MARKERS = 128     # PHC_RENDER_MAX_MARKERS


class Camera(C.Structure):
    _fields_ = [("env", c_i32), ("eye", c_f * 3), ("target", c_f * 3), ("up", c_f * 3), ("fov_y", c_f)]


class RenderScene(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_bodies", c_i32), ("body_state", c_p), ("capsules", c_p), ("num_capsules", c_i32),
                ("num_shape_blocks", c_i32), ("capsule_stride", c_i64), ("env_shape", c_p), ("markers", c_p), ("num_markers", c_i32),
                ("marker_radius", c_f), ("palette", (c_f * 3) * RENDER_PALETTE), ("marker_color", c_f * 3), ("ground_color", (c_f * 3) * 2),
                ("sky_color", c_f * 3), ("light_dir", c_f * 3), ("ambient", c_f), ("diffuse", c_f), ("marker_radii", c_p), ("marker_colors", c_p)]


RENDER_MESH_ID = 2000            # PHC_RENDER_MESH_ID
RENDER_MAX_INSTANCES = 128       # PHC_RENDER_MAX_INSTANCES
RENDER_MAX_TRIANGLES = 1 << 22   # PHC_RENDER_MAX_TRIANGLES
RENDER_MESH_MIN_CROSS = 1.0e-12  # PHC_RENDER_MESH_MIN_CROSS


class BvhNode(C.Structure):
    _fields_ = [("lo", c_f * 3), ("skip", c_i32), ("hi", c_f * 3), ("leaf", c_i32)]


class MeshInstance(C.Structure):
    _fields_ = [("owner", c_i32), ("root", c_i32), ("pos", c_f * 3), ("quat", c_f * 4), ("center", c_f * 3), ("radius", c_f), ("rgb", c_f * 3)]


class RenderMeshes(C.Structure):
    _fields_ = [("num_vertices", c_i32), ("num_triangles", c_i32), ("num_nodes", c_i32), ("num_instances", c_i32), ("vertices", c_p),
                ("triangles", c_p), ("tri_perm", c_p), ("nodes", c_p), ("instances", C.POINTER(MeshInstance)), ("instances_dev", c_p)]


class EvalArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_bodies", c_i32), ("root_idx", c_i32), ("step", c_i32), ("bound", c_i32), ("dt", c_f),
                ("rigid_body_state", c_p), ("progress_buf", c_p), ("terminate_buf", c_p), ("motion_ids", c_p), ("motion_start_times", c_p),
                ("motion_start_times_offset", c_p), ("global_offset", c_p), ("clip_steps", c_p), ("history", c_p), ("sums", c_p), ("count", c_p),
                ("failed", c_p), ("status", c_p), ("mpjpe_step", c_p), ("gt_out", c_p)]


class PushArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_bodies", c_i32), ("num_listed", c_i32), ("pause_lo", c_i32), ("pause_hi", c_i32), ("duration", c_i32),
                ("direction", c_i32), ("force_lo", c_f), ("force_hi", c_f), ("key", C.c_uint64), ("env_offset", c_i64), ("bodies", c_p),
                ("progress_buf", c_p), ("remaining", c_p), ("countdown", c_p), ("body", c_p), ("k", c_p), ("started", c_p), ("force", c_p)]


PROJ_MAX_SLOTS, PROJ_MAX_SHAPES = 4, 64   # PHC_PROJ_MAX_SLOTS, PHC_PROJ_MAX_SHAPES


class ProjArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_bodies", c_i32), ("num_shapes", c_i32), ("num_listed", c_i32), ("count", c_i32), ("pause_lo", c_i32),
                ("pause_hi", c_i32), ("life_steps", c_i32), ("substeps", c_i32), ("dt", c_f), ("gravity_z", c_f), ("radius", c_f), ("restitution", c_f),
                ("friction", c_f), ("mass_lo", c_f), ("mass_hi", c_f), ("speed_lo", c_f), ("speed_hi", c_f), ("dist_lo", c_f), ("dist_hi", c_f),
                ("elev_lo", c_f), ("elev_hi", c_f), ("key", C.c_uint64), ("env_offset", c_i64), ("bodies", c_p), ("capsules", c_p), ("owner", c_p),
                ("body_com", c_p), ("body_inv_mass", c_p), ("body_inv_inertia", c_p), ("rigid_body_state", c_p), ("progress_buf", c_p), ("life", c_p),
                ("countdown", c_p), ("thrown", c_p), ("hits", c_p), ("last_hit", c_p), ("k", c_p), ("pos", c_p), ("vel", c_p), ("mass", c_p),
                ("force", c_p), ("torque", c_p)]


PROJ_MAX_ROWSETS, PROJ_SNAPSHOT, PROJ_SELECT = 8, 0, 1   # PHC_PROJ_MAX_ROWSETS, PHC_PROJ_SNAPSHOT, PHC_PROJ_SELECT


class ProjRows(C.Structure):
    _fields_ = [("num_envs", c_i32), ("count", c_i32), ("num_sets", c_i32), ("mode", c_i32), ("last_hit", c_p), ("base", c_p * PROJ_MAX_ROWSETS),
                ("shadow", c_p * PROJ_MAX_ROWSETS), ("width", c_i32 * PROJ_MAX_ROWSETS)]


class GetupArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_dof", c_i32), ("recovery_steps", c_i32), ("reserved", c_i32), ("key", C.c_uint64), ("env_offset", c_i64),
                ("prob", c_p), ("reset_buf", c_p), ("terminate_buf", c_p), ("fall_root", c_p), ("fall_dof_pos", c_p), ("root_states", c_p), ("dof_state", c_p),
                ("avail", c_p), ("assign", c_p), ("recovery_counter", c_p), ("k", c_p), ("launch_count", c_p), ("kind", c_p), ("normal_flag", c_p),
                ("fall_list", c_p), ("free_list", c_p)]


class ObsAugArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_obs", c_i32), ("self_obs_size", c_i32), ("num_samples", c_i32), ("dropout_p", C.c_float), ("noise_std", C.c_float),
                ("key", C.c_uint64), ("env_offset", c_i64), ("obs", c_p), ("k", c_p), ("row_flag", c_p), ("env_ids", c_p), ("n_ids", c_i64)]


P = C.POINTER
class SimDr(C.Structure):
    _fields_ = [("env_friction", c_p), ("torque_noise", c_p), ("k", c_p), ("key", C.c_uint64), ("env_offset", c_i64)]


class DrArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_dof", c_i32), ("delay_lo", c_i32), ("delay_hi", c_i32), ("push_interval", c_i32), ("max_push_vel_xy", c_f),
                ("key", C.c_uint64), ("env_offset", c_i64), ("progress_buf", c_p), ("actions", c_p), ("action_queue", c_p), ("delay", c_p), ("k", c_p),
                ("delayed_actions", c_p), ("root_states", c_p)]


class ClipArgs(C.Structure):
    _fields_ = [("num_clips", c_i32), ("num_bodies", c_i32), ("num_trees", c_i32), ("frame_stride", c_i32), ("num_frames", c_i64), ("parents", c_p),
                ("local_translation", c_p), ("clip_tree", c_p), ("clip_start", c_p), ("clip_dt", c_p), ("quat", c_p), ("trans", c_p), ("scratch", c_p),
                ("scratch_bytes", c_i64), ("frames", c_p)]


class ClipRealArgs(C.Structure):
    _fields_ = [("num_clips", c_i32), ("num_bodies", c_i32), ("num_ext", c_i32), ("num_contacts", c_i32), ("frame_stride", c_i32), ("fix_height", c_i32),
                ("num_frames", c_i64), ("parents", c_p), ("offsets", c_p), ("rest_mat", c_p), ("pose_aa", c_p), ("trans", c_p), ("clip_start", c_p),
                ("clip_dt", c_p), ("contact_body", c_p), ("contact_pos", c_p), ("contact_radius", c_p), ("scratch", c_p), ("scratch_bytes", c_i64),
                ("frames", c_p)]


TELEOP_TERMS = ("dof_pos_limits", "torque_limits", "torques", "dof_vel", "dof_acc", "action_rate", "slippage", "feet_contact_forces", "stumble",
                "feet_air_time_teleop", "feet_ori")   # PHC_TELEOP_*: the bit of each term
TELEOP_MAX_FEET = 8   # PHC_TELEOP_MAX_FEET


class TeleopArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_dof", c_i32), ("num_bodies", c_i32), ("num_feet", c_i32), ("num_im_cols", c_i32), ("term_mask", C.c_uint32),
                ("order", c_i32 * len(TELEOP_TERMS)), ("scale", c_f * len(TELEOP_TERMS)), ("feet", c_i32 * TELEOP_MAX_FEET), ("dt", c_f),
                ("max_contact_force", c_f), ("push_interval", c_i32), ("recovery_steps", c_i32), ("dof_state", c_p), ("dof_limits_lower", c_p),
                ("dof_limits_upper", c_p), ("torque_limits", c_p), ("dof_force", c_p), ("actions", c_p), ("contact_force", c_p), ("rigid_body_state", c_p),
                ("progress_buf", c_p), ("motion_start_times", c_p), ("motion_start_times_offset", c_p), ("sampled_motion_ids", c_p), ("dr_k", c_p),
                ("recovery_counter", c_p), ("last_actions", c_p), ("last_dof_vel", c_p), ("feet_air_time", c_p), ("last_contacts", c_p), ("rew_buf", c_p),
                ("reward_im", c_p), ("reward_raw", c_p)]


STREAM_MAX_WINDOW = 64   # PHC_STREAM_MAX_WINDOW
STREAM_MAX_PAIRS = 8     # PHC_STREAM_MAX_PAIRS
STREAM_ADVANCE, STREAM_OBSERVE = 0, 1   # PHC_STREAM_*: phc_stream_args_t.mode


class StreamArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("mode", c_i32), ("window", c_i32), ("fold_window", c_i32), ("frame_rows", c_i32), ("limb_scale", c_i32),
                ("num_pairs", c_i32), ("pair_parent", c_i32 * STREAM_MAX_PAIRS), ("pair_child", c_i32 * STREAM_MAX_PAIRS),
                ("pair_length", c_f * STREAM_MAX_PAIRS), ("frame_mat", c_f * 9), ("dt", c_f), ("close_distance", c_f), ("far_distance", c_f),
                ("track_root_body", c_i32), ("frames", c_p), ("perm", c_p), ("fold", c_p), ("ring_body", c_p), ("ring_root", c_p), ("head", c_p),
                ("count", c_p), ("has_prev", c_p), ("cur_ref", c_p), ("cur_vel", c_p), ("rigid_body_state", c_p), ("obs_buf", c_p), ("reset_buf", c_p),
                ("terminate_buf", c_p), ("track_err", c_p)]


FIT_MAX_MATCHED = 32   # PHC_FIT_MAX_MATCHED


class FitArgs(C.Structure):
    _fields_ = [("num_bodies", c_i32), ("num_ext", c_i32), ("num_matched", c_i32), ("num_clips", c_i32), ("num_frames", c_i64), ("lr", C.c_double),
                ("parents", c_p), ("offsets", c_p), ("rest", c_p), ("axis", c_p), ("range", c_p), ("match_body", c_p), ("match_slot", c_p), ("subtree", c_p),
                ("clip_start", c_p), ("clip_start_host", c_p), ("target", c_p), ("root_trans_offset", c_p), ("dof", c_p), ("dof_m", c_p), ("dof_v", c_p),
                ("root_rot", c_p), ("root_rot_m", c_p), ("root_rot_v", c_p), ("root_off", c_p), ("root_off_m", c_p), ("root_off_v", c_p), ("step", c_p),
                ("loss", c_p), ("scratch", c_p), ("scratch_bytes", c_i64)]


class RecordArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("obs_dim", c_i32), ("num_actions", c_i32), ("step", c_i32), ("capacity", c_i64), ("obs_buf", c_p), ("obs_prev", c_p),
                ("clean_actions", c_p), ("actions", c_p), ("reset_buf", c_p), ("rows", c_p), ("row_start", c_p), ("obs", c_p), ("clean", c_p), ("env", c_p),
                ("reset", c_p)]


RECORD_REF, RECORD_SEED, RECORD_ONE_SEGMENT = 1, 2, 4   # PHC_RECORD_*: phc_motion_record_args_t.flags


class MotionRecordArgs(C.Structure):
    _fields_ = [("num_envs", c_i32), ("num_bodies", c_i32), ("num_ext", c_i32), ("num_dof", c_i32), ("cap", c_i32), ("width", c_i32), ("flags", c_i32),
                ("dt", c_f), ("root_states", c_p), ("dof_state", c_p), ("rigid_body_state", c_p), ("progress_buf", c_p), ("flag", c_p), ("motion_ids", c_p),
                ("motion_start_times", c_p), ("motion_start_times_offset", c_p), ("ref_body_pos", c_p), ("limit", c_p), ("frames", c_p), ("header", c_p),
                ("len", c_p), ("seg", c_p), ("closed", c_p), ("dropped", c_p)]


class JpegArgs(C.Structure):
    _fields_ = [("num_frames", c_i32), ("width", c_i32), ("height", c_i32), ("restart_interval", c_i32), ("row_stride", c_i64), ("frame_stride", c_i64),
                ("rgba", c_p), ("qtab", c_p), ("out", c_p), ("out_stride", c_i64), ("length", c_p), ("coef", c_p), ("scratch", c_p), ("scratch_bytes", c_i64)]


_SIGNATURES = {
    "phc_abi_version": ([], c_i32),
    "phc_motion_state": ([P(MotionLib), c_i32] + [c_p] * 15, c_i32),
    "phc_sample_time_interval": ([P(MotionLib), c_i32, c_p, c_p, c_p, c_p], c_i32),
    "phc_sim_step": ([P(Model), P(SimParams), P(SimState), c_p, c_p, c_p, c_p, c_i32, c_p], c_i32),
    "phc_sim_step_wrench": ([P(Model), P(SimParams), P(SimState), c_p, c_p, c_p, c_p, c_i32, c_p, c_p, c_i32, c_p], c_i32),
    "phc_refresh_body_state": ([P(Model), P(SimState), c_p], c_i32),
    "phc_im_post_physics": ([P(Model), P(MotionLib), P(ImParams), P(SimState), P(ImBuffers), c_p], c_i32),
    "phc_amp_ref_table": ([P(Model), P(MotionLib), P(ImParams), c_i64, c_p, c_p, c_p], c_i32),
    "phc_im_reset": ([P(Model), P(MotionLib), P(ImParams), P(SimState), P(ImBuffers), c_i32, c_p, c_p, c_i32, c_p], c_i32),
    "phc_im_reset_done": ([P(Model), P(MotionLib), P(ImParams), P(SimState), P(ImBuffers), C.c_uint64, C.c_uint64, c_i32, c_p], c_i32),
    "phc_im_reset_from_state": ([P(Model), P(MotionLib), P(ImParams), P(SimState), P(ImBuffers), c_i32, c_p, c_i32, c_p], c_i32),
    "phc_refresh_body_state_indexed": ([P(Model), P(SimState), c_i32, c_p, c_p], c_i32),
    "phc_amp_obs_demo": ([P(Model), P(MotionLib), P(ImParams), c_i32, c_p, c_p, c_p, c_p], c_i32),
    "phc_gae": ([c_i32, c_i32, c_p, c_p, c_p, c_p, c_f, c_f, c_p, c_p], c_i32),
    "phc_fk": ([P(Model), c_i64, c_p, c_p, c_p, c_p, c_p], c_i32),
    "phc_running_norm_workspace": ([c_i64, c_i32], c_i64),
    "phc_running_norm": ([c_p, c_p, c_i64, c_i32, c_p, c_p, c_f, c_f, c_p, c_i32, c_i32, c_p, c_p, c_p, c_p, c_p], c_i32),
    "phc_colsum_workspace": ([c_i64, c_i32], c_i64),
    "phc_colsum_bf16": ([c_p, c_i64, c_i32, c_p, c_p, c_p], c_i32),
    "phc_colsum_relu_bf16": ([c_p, c_p, c_i64, c_i32, c_p, c_p, c_p, c_p], c_i32),
    "phc_sum_slabs_bf16": ([c_p, c_i32, c_i64, c_p, c_i32, c_p], c_i32),
    "phc_wgrad_bf16_slices": ([c_i64, c_i32, c_i32], c_i32),
    "phc_wgrad_bf16_workspace": ([c_i64, c_i32, c_i32], c_i64),
    "phc_wgrad_bf16": ([c_p, c_p, c_p, c_i64, c_i64, c_i32, c_i32, c_p, c_i64, c_i32, c_p, c_p, c_i32, c_p, c_p], c_i32),
    "phc_split3_bf16": ([c_p, c_i64, c_p, c_i64, c_i64, c_i32, c_i64, c_i32, c_p, c_i32, c_p, c_i64, c_i64, c_i32, c_p], c_i32),
    "phc_colsum_chunks": ([c_i64], c_i32),
    "phc_linear1_chunks": ([c_i64], c_i32),
    "phc_colsum_finish_batch": ([c_i32, P(ColsumJob), c_p], c_i32),
    "phc_rollout_bookkeeping": ([c_p, c_f, c_p, c_p, c_p, c_i32, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p], c_i32),
    "phc_disc_bce": ([c_p, c_i32, c_i32, c_i32, c_f, c_p, c_p, c_p], c_i32),
    "phc_sumsq_workspace": ([], c_i64),
    "phc_weighted_sumsq": ([c_i32, c_p, c_p, c_p, c_i32, c_p, c_p, c_p], c_i32),
    "phc_policy_sample": ([c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_f, c_p, c_i64, c_i32, c_p, c_p, c_p, c_p, c_p, c_p], c_i32),
    "phc_linear1_workspace": ([c_i64, c_i32], c_i64),
    "phc_linear1_forward": ([c_p, c_p, c_p, c_i64, c_i32, c_p, c_p], c_i32),
    "phc_linear1_backward": ([c_p, c_p, c_p, c_i64, c_i32, c_p, c_p, c_p, c_p], c_i32),
    "phc_adam_workspace": ([], c_i64),
    "phc_adam_clip_step": ([c_p, c_p, c_p, c_p, c_i64, c_f, c_f, c_f, c_f, c_f, c_i64, c_f, c_p, c_p, c_p, c_p, c_p], c_i32),
    "phc_ppo_loss_workspace": ([], c_i64),
    "phc_ppo_loss": ([c_p, c_p, c_i32] + [c_p] * 9 + [c_i64, c_i32, P(PpoParams), c_p, c_p, c_p, c_p, c_p], c_i32),
    "phc_render": ([P(RenderScene), P(Camera), c_i32, c_i32, c_i32, c_p, c_p, c_p, c_p], c_i32),
    "phc_render_mesh": ([P(RenderScene), P(RenderMeshes), P(Camera), c_i32, c_i32, c_i32, c_p, c_p, c_p, c_p, c_p], c_i32),
    "phc_eval_accumulate": ([P(MotionLib), P(EvalArgs), c_p], c_i32),
    "phc_push_advance": ([P(PushArgs), c_p], c_i32),
    "phc_proj_advance": ([P(ProjArgs), c_p], c_i32),
    "phc_proj_rows": ([P(ProjRows), c_p], c_i32),
    "phc_jpeg_frame_bound": ([c_i32, c_i32, c_i32], c_i64),
    "phc_jpeg_scratch_bytes": ([c_i64, c_i32, c_i32, c_i32], c_i64),
    "phc_jpeg_encode": ([P(JpegArgs), c_p], c_i32),
}
# Optional symbols: typed when the library has them.  An older build of the same ABI selected with PHC_AMD_LIB (an A/B baseline) lacks them and still loads; a
# caller that needs one fails on the missing attribute.
_OPTIONAL_SIGNATURES = {
    "phc_im_is_plain": ([P(Model), P(MotionLib), P(ImParams), P(ImBuffers)], c_i32),
    "phc_task_force_generic": ([c_i32], c_i32),
    "phc_sim_model_facts": ([P(Model)], c_i32),
    "phc_sim_is_plain": ([P(Model), P(SimParams), P(SimState), c_p, c_p, c_i32], c_i32),
    "phc_sim_force_generic": ([c_i32], c_i32),
    "phc_sim_step_dr": ([P(Model), P(SimParams), P(SimState), c_p, c_p, c_p, c_p, c_i32, P(SimDr), c_p], c_i32),
    "phc_dr_advance": ([P(DrArgs), c_p], c_i32),
    "phc_clip_scratch_bytes": ([c_i64, c_i32], c_i64),
    "phc_clip_process": ([P(ClipArgs), c_p], c_i32),
    "phc_clip_real_scratch_bytes": ([c_i64, c_i32, c_i32, c_i32], c_i64),
    "phc_clip_process_real": ([P(ClipRealArgs), c_p], c_i32),
    "phc_teleop_rewards": ([P(MotionLib), P(TeleopArgs), c_p], c_i32),
    "phc_stream_track": ([P(Model), P(ImParams), P(StreamArgs), c_p], c_i32),
    "phc_dataset_record": ([P(RecordArgs), c_p], c_i32),
    "phc_silu_bf16": ([c_p, c_i64, c_i32, c_p, c_p], c_i32),
    "phc_colsum_silu_bf16": ([c_p, c_p, c_i64, c_i32, c_p, c_p, c_p, c_p], c_i32),
    "phc_mse_loss_workspace": ([], c_i64),
    "phc_mse_loss": ([c_p, c_i32, c_p, c_p, c_i64, c_i32, c_p, c_p, c_p, c_p], c_i32),
    "phc_fit_scratch_bytes": ([c_i64, c_i32, c_i32], c_i64),
    "phc_fit_iterate": ([P(FitArgs), c_i32, c_p], c_i32),
    "phc_fit_sph_scratch_bytes": ([c_i64, c_i32, c_i32], c_i64),
    "phc_fit_sph_iterate": ([P(FitArgs), c_i32, c_p], c_i32),
    "phc_getup_assign": ([P(GetupArgs), c_p], c_i32),
    "phc_refresh_body_state_masked": ([P(Model), P(SimState), c_p, c_p], c_i32),
    "phc_im_reset_from_state_masked": ([P(Model), P(MotionLib), P(ImParams), P(SimState), P(ImBuffers), c_p, c_p], c_i32),
    "phc_task_draws": ([c_i32, C.c_uint64, c_i64, c_p, c_p, c_p, c_p], c_i32),
    "phc_obs_augment": ([P(ObsAugArgs), c_p], c_i32),
    "phc_occl_advance": ([c_i32, c_i32, C.c_uint64, c_i64, c_p, C.c_float, c_i32, c_i32, c_p, c_p, c_p], c_i32),
    "phc_motion_record_width": ([c_i32, c_i32, c_i32, c_i32], c_i32),
    "phc_motion_record": ([P(Model), P(MotionRecordArgs), c_p], c_i32),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES) + tuple(_OPTIONAL_SIGNATURES)

_lib = None


def load():
    """dlopen libphc_amd.so and type every entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build the HIP extension first "
                          "(python -m phc_amd.build or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export the symbol
        fn.argtypes = argtypes
        fn.restype = restype
    for name, (argtypes, restype) in _OPTIONAL_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes = argtypes
            fn.restype = restype
    if lib.phc_abi_version() != 37:
        raise ImportError("libphc_amd.so ABI version mismatch")
    _lib = lib
    return lib


class PhcError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        kind = {-1: "invalid argument", -2: "unsupported configuration"}.get(rc, f"hipError {rc}")
        raise PhcError(f"{what} failed: {kind}")
