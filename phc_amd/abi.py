"""Helpers that fill the C-ABI structs of include/phc_amd.h from array objects.

Works for torch tensors (product: device pointers) and for numpy arrays (oracle/hostemu: host
pointers) -- the structs only carry raw addresses and sizes.
"""
import ctypes as C

import numpy as np

from . import _lib as L

MAX_BODIES = 64  # PHC_MAX_BODIES
NUM_INT_TABLES = 21  # PHC_NTAB


def ptr(x):
    """Raw address of a torch tensor / numpy array (must be contiguous), or None."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"], "numpy array must be C-contiguous"
        return x.ctypes.data
    assert x.is_contiguous(), "tensor must be contiguous"
    return x.data_ptr()


def model_struct(ints, floats, num_bodies, num_dof, max_level, num_contact_pts, num_shapes=1):
    """`num_shapes` > 1: ints / floats are [K, ...] stacks of K packed models of one topology (model.py pack_shapes())."""
    m = L.Model()
    m.num_shapes = int(num_shapes)
    if num_shapes > 1:
        assert ints.ndim == 2 and floats.ndim == 2 and ints.shape[0] == floats.shape[0] == num_shapes
        m.int_stride, m.float_stride = int(ints.shape[1]), int(floats.shape[1])
        m.num_collision_pairs = int(ints[:, 4 + NUM_INT_TABLES * MAX_BODIES].max())
    else:
        m.num_collision_pairs = int(ints.reshape(-1)[4 + NUM_INT_TABLES * MAX_BODIES])   # count stored right after the int tables (model.py pack())
    m.num_bodies, m.num_dof, m.max_level, m.num_contact_pts = num_bodies, num_dof, max_level, num_contact_pts
    per_body = ints.reshape(max(1, int(num_shapes)), -1)[:, 4 + 9 * MAX_BODIES:4 + 10 * MAX_BODIES]   # int table 9: contact points per body
    m.max_body_contact_pts = int(per_body.max())
    m.ints, m.floats = ptr(ints), ptr(floats)
    m.sim_plain_facts = _sim_plain_facts(m, ints, floats)
    return m


def _sim_plain_facts(m, ints, floats):
    """phc_model_t.sim_plain_facts: what phc_sim_model_facts says about a HOST copy of the tables (the stepper's launch chooser cannot read device memory;
    csrc/phc_sim_plain.h).  0 -- the generic kernels -- for stacked shape blocks and for a library that predates the function (an A/B baseline)."""
    fn = getattr(L.load(), "phc_sim_model_facts", None)
    if fn is None or m.num_shapes > 1:
        return 0
    hi, hf = (np.ascontiguousarray(t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()) for t in (ints, floats))
    if hi.dtype != np.int32 or hf.dtype != np.float32:   # (the double-precision host emulation packs float64 tables)
        return 0
    h = L.Model()
    C.memmove(C.byref(h), C.byref(m), C.sizeof(m))
    h.ints, h.floats = hi.ctypes.data, hf.ctypes.data
    return int(fn(C.byref(h)))


def motion_lib_struct(frames, frame_stride, num_bodies, motion_lengths, motion_dt, motion_num_frames, length_starts,
                      num_ext_bodies=0, dofs_per_joint=3):
    s = L.MotionLib()
    s.num_ext_bodies, s.dofs_per_joint = int(num_ext_bodies), int(dofs_per_joint)
    s.frames = ptr(frames)
    s.num_frames_total = int(frames.shape[0])
    s.frame_stride = int(frame_stride)
    s.num_bodies = int(num_bodies)
    s.num_motions = int(motion_lengths.shape[0])
    s.motion_lengths, s.motion_dt = ptr(motion_lengths), ptr(motion_dt)
    s.motion_num_frames, s.length_starts = ptr(motion_num_frames), ptr(length_starts)
    return s


def sim_state_struct(num_envs, root_states, dof_state, rigid_body_state, contact_force, dof_force, pd_target, force_sensor=None, env_shape=None, pd_ref=None):
    s = L.SimState()
    s.pd_ref = ptr(pd_ref)
    s.force_sensor = ptr(force_sensor)
    s.env_shape = ptr(env_shape)
    s.num_envs = int(num_envs)
    s.root_states, s.dof_state, s.rigid_body_state = ptr(root_states), ptr(dof_state), ptr(rigid_body_state)
    s.contact_force, s.dof_force, s.pd_target = ptr(contact_force), ptr(dof_force), ptr(pd_target)
    return s


def sim_params_struct(sim_dt=1 / 60, substeps=2, control_freq_inv=2, gravity_z=-9.81, contact_stiffness=1.0e5,
                      contact_damping=1.0e3, friction=1.0, friction_viscous=2.0e3, angular_damping=0.01,
                      max_angular_velocity=100.0, contact_offset=0.02, control_mode=0, limit_stiffness=0.0, limit_damping=0.0, lane_mapping=0,
                      self_collision=0, self_stiffness_scale=0.25, self_damping_ratio=0.5, force_sensor_bodies=(), contact_model=0,
                      contact_iterations=4, contact_impedance=1.0e5, max_depenetration_velocity=10.0, bounce_threshold_velocity=0.2, restitution=0.0,
                      inertia_lag=0, force_average=0):
    p = L.SimParams()
    if isinstance(contact_model, str) and contact_model not in ("penalty", "tgs", "rigid"):
        raise ValueError(f"solver.contact must be 'penalty' or 'tgs' (alias 'rigid'), not {contact_model!r}")
    p.contact_model = {"penalty": 0, "tgs": 1, "rigid": 1}.get(contact_model, contact_model)
    p.inertia_lag, p.force_average = int(bool(inertia_lag)), int(bool(force_average))
    if p.contact_model == 1 and p.inertia_lag:
        raise ValueError("solver.inertia_lag needs the penalty contact model (the rigid model re-solves every sub-step with fresh impedances)")
    if p.contact_model == 1 and int(contact_iterations) < 2:
        raise ValueError("solver.contact_iterations must be >= 2 for the rigid contact model")
    p.contact_iterations, p.contact_impedance = int(contact_iterations), float(contact_impedance)
    p.max_depenetration_velocity, p.bounce_threshold_velocity, p.restitution = float(max_depenetration_velocity), float(bounce_threshold_velocity), float(restitution)
    assert len(force_sensor_bodies) <= 4, "at most 4 force sensors"
    p.num_force_sensors = len(force_sensor_bodies)
    for i, b in enumerate(force_sensor_bodies):
        p.force_sensor_body[i] = int(b)
    p.sim_dt, p.substeps, p.control_freq_inv, p.gravity_z = sim_dt, substeps, control_freq_inv, gravity_z
    p.contact_stiffness, p.contact_damping, p.friction, p.friction_viscous = contact_stiffness, contact_damping, friction, friction_viscous
    p.angular_damping, p.max_angular_velocity, p.contact_offset = angular_damping, max_angular_velocity, contact_offset
    p.control_mode, p.limit_stiffness, p.limit_damping = int(control_mode), float(limit_stiffness), float(limit_damping)
    p.lane_mapping = int(lane_mapping)
    p.self_collision, p.self_stiffness_scale, p.self_damping_ratio = int(self_collision), float(self_stiffness_scale), float(self_damping_ratio)
    return p


def frame_stride_for(num_bodies, num_ext_bodies=0, dofs_per_joint=3):
    """Floats per frame record (layout in include/phc_amd.h): pos 3 | rot 4 per body incl. the extended ones, vel 3 | angvel 3
    per simulated body, then local_rot 4 per body + dof_vel 3 per joint (spherical models) or dof_pos + dof_vel per DoF
    (revolute models); padded to a multiple of 4 floats (16 B) so every record starts float4-aligned."""
    nbe = num_bodies + num_ext_bodies
    n = nbe * 7 + num_bodies * 6 + ((num_bodies - 1) * 2 if dofs_per_joint == 1 else num_bodies * 4 + (num_bodies - 1) * 3)
    return (n + 3) // 4 * 4


def pack_frames(gts, grs, gvs, gavs, lrs, dvs, xp=np, gts_ext=None, grs_ext=None, dof_pos=None):
    """[F,NB,3/4] field tensors -> [F, stride] records (layout of phc_motion_lib_t).  Spherical models pass `lrs` (local
    rotations); revolute models pass `dof_pos` [F,ND] instead (and `dvs` [F,ND]); `gts_ext / grs_ext` [F,E,3/4] are the
    extended reference bodies."""
    F_, nb = gts.shape[0], gts.shape[1]
    ne = 0 if gts_ext is None else gts_ext.shape[1]
    dpj = 1 if dof_pos is not None else 3
    stride = frame_stride_for(nb, ne, dpj)
    if xp is np:
        out = np.zeros((F_, stride), dtype=np.float32)
        cat = lambda a, b: np.concatenate([a, b], axis=1)
    else:
        out = xp.zeros((F_, stride), dtype=xp.float32, device=gts.device)
        cat = lambda a, b: xp.cat([a, b], dim=1)
    pos = gts if ne == 0 else cat(gts, gts_ext)
    rot = grs if ne == 0 else cat(grs, grs_ext)
    o = 0
    fields = [(pos, (nb + ne) * 3), (rot, (nb + ne) * 4), (gvs, nb * 3), (gavs, nb * 3)]
    fields += [(dof_pos, nb - 1), (dvs, nb - 1)] if dpj == 1 else [(lrs, nb * 4), (dvs, (nb - 1) * 3)]
    for arr, w in fields:
        out[:, o:o + w] = arr.reshape(F_, w)
        o += w
    return out


def clip_args_struct(num_clips, num_frames, num_bodies, num_trees, parents, local_translation, clip_tree, clip_start, clip_dt, quat, trans, scratch,
                     scratch_bytes, frames, frame_stride=None):
    """phc_clip_args_t (phc_clip_process): the arrays are torch tensors / numpy arrays or raw addresses (views into one staging buffer)."""
    a = L.ClipArgs()
    a.num_clips, a.num_bodies, a.num_trees, a.num_frames = int(num_clips), int(num_bodies), int(num_trees), int(num_frames)
    a.frame_stride = frame_stride_for(int(num_bodies), 0, 3) if frame_stride is None else int(frame_stride)
    addr = lambda x: x if x is None or isinstance(x, int) else ptr(x)
    a.parents, a.local_translation, a.clip_tree, a.clip_start, a.clip_dt = (addr(x) for x in (parents, local_translation, clip_tree, clip_start, clip_dt))
    a.quat, a.trans, a.scratch, a.frames = addr(quat), addr(trans), addr(scratch), addr(frames)
    a.scratch_bytes = int(scratch_bytes)
    return a


CLIP_REAL_ARRAYS = ("parents", "offsets", "rest_mat", "pose_aa", "trans", "clip_start", "clip_dt", "contact_body", "contact_pos", "contact_radius")


def clip_real_args_struct(num_clips, num_frames, num_bodies, num_ext, num_contacts, fix_height, scratch, scratch_bytes, frames, frame_stride=None, **arrays):
    """phc_clip_real_args_t (phc_clip_process_real): `arrays` holds every name of CLIP_REAL_ARRAYS as a torch tensor / numpy array, a raw address (a view into one
    staging buffer) or None."""
    assert set(arrays) == set(CLIP_REAL_ARRAYS), sorted(set(arrays) ^ set(CLIP_REAL_ARRAYS))
    a = L.ClipRealArgs()
    a.num_clips, a.num_bodies, a.num_ext, a.num_contacts, a.num_frames = int(num_clips), int(num_bodies), int(num_ext), int(num_contacts), int(num_frames)
    a.fix_height = 1 if fix_height else 0
    a.frame_stride = frame_stride_for(int(num_bodies), int(num_ext), 1) if frame_stride is None else int(frame_stride)
    addr = lambda x: x if x is None or isinstance(x, int) else ptr(x)
    for k in CLIP_REAL_ARRAYS:
        setattr(a, k, addr(arrays[k]))
    a.scratch, a.frames, a.scratch_bytes = addr(scratch), addr(frames), int(scratch_bytes)
    return a


FIT_ARRAYS = ("parents", "offsets", "rest", "axis", "range", "match_body", "match_slot", "subtree", "clip_start", "clip_start_host", "target",
              "root_trans_offset", "dof", "dof_m", "dof_v", "root_rot", "root_rot_m", "root_rot_v", "root_off", "root_off_m", "root_off_v", "step", "loss")


def fit_args_struct(num_bodies, num_ext, num_matched, num_clips, num_frames, lr, scratch, scratch_bytes, **arrays):
    """phc_fit_args_t (phc_fit_iterate): `arrays` holds every name of FIT_ARRAYS as a torch tensor / numpy array or a raw address; clip_start_host is host memory."""
    assert set(arrays) == set(FIT_ARRAYS), sorted(set(arrays) ^ set(FIT_ARRAYS))
    a = L.FitArgs()
    a.num_bodies, a.num_ext, a.num_matched, a.num_clips, a.num_frames = int(num_bodies), int(num_ext), int(num_matched), int(num_clips), int(num_frames)
    a.lr = float(lr)
    addr = lambda x: x if x is None or isinstance(x, int) else ptr(x)
    for k in FIT_ARRAYS:
        setattr(a, k, addr(arrays[k]))
    a.scratch, a.scratch_bytes = addr(scratch), int(scratch_bytes)
    return a


GETUP_ARRAYS = ("prob", "reset_buf", "terminate_buf", "fall_root", "fall_dof_pos", "root_states", "dof_state", "avail", "assign", "recovery_counter", "k",
                "launch_count", "kind", "normal_flag", "fall_list", "free_list")
GETUP_MAX_ENVS = 1 << 20   # GETUP_MAX_ENVS (csrc/phc_getup.h): PHC_EUNSUPPORTED above
GETUP_BLOCK = 1024         # GETUP_BLOCK: envs per scan tile


def getup_args_struct(num_envs, num_dof, key, env_offset=0, recovery_steps=0, **arrays):
    """phc_getup_args_t (phc_getup_assign): `arrays` holds every name of GETUP_ARRAYS as a torch tensor / numpy array, a raw address or None."""
    assert set(arrays) == set(GETUP_ARRAYS), sorted(set(arrays) ^ set(GETUP_ARRAYS))
    a = L.GetupArgs()
    a.num_envs, a.num_dof, a.recovery_steps, a.reserved = int(num_envs), int(num_dof), int(recovery_steps), 0
    a.key, a.env_offset = int(key), int(env_offset)
    for k in GETUP_ARRAYS:
        x = arrays[k]
        setattr(a, k, x if x is None or isinstance(x, int) else ptr(x))
    return a


OBS_AUG_MAX_OBS, OBS_AUG_MAX_SAMPLES, OCCL_MAX_BODIES = 65536, 1024, 64   # csrc/phc_obs_aug.h: PHC_EUNSUPPORTED above


def obs_aug_args_struct(obs, k, self_obs_size, num_samples, dropout_p, noise_std, key, env_offset=0, row_flag=None, env_ids=None, num_envs=None, num_obs=None, n_ids=None):
    """phc_obs_aug_args_t (phc_obs_augment): `obs` [N, num_obs] fp32 contiguous and `k` [N] int32 as tensors / arrays (sizes taken from `obs`) or raw
    addresses (then with `num_envs`, `num_obs`); one of `row_flag` [N] int64 / `env_ids` [n] int64 (n its length, or `n_ids` with an address), or neither = all rows."""
    a = L.ObsAugArgs()
    if num_envs is None:
        num_envs, num_obs = obs.shape
    a.num_envs, a.num_obs, a.self_obs_size, a.num_samples = int(num_envs), int(num_obs), int(self_obs_size), int(num_samples)
    a.dropout_p, a.noise_std, a.key, a.env_offset = float(dropout_p), float(noise_std), int(key), int(env_offset)
    for name, x in (("obs", obs), ("k", k), ("row_flag", row_flag), ("env_ids", env_ids)):
        setattr(a, name, x if x is None or isinstance(x, int) else ptr(x))
    a.n_ids = int(n_ids) if n_ids is not None else (0 if env_ids is None else int(env_ids.shape[0]))
    return a


def im_params_struct(dt, max_episode_length, reward_specs, power_reward, power_coefficient, enable_early_termination,
                     use_mean_termination, disable_collision_check, local_root_obs, root_height_obs, num_track_bodies,
                     track_slot, reset_mask, num_reset_bodies, first_reset_body, termination_distances, num_key_bodies, key_body_ids,
                     num_amp_joints, amp_joint_slot, num_amp_obs_steps, num_amp_obs_per_step, num_self_obs, num_task_obs,
                     cycle_motion=False, zero_out_far=False, close_distance=0.25, far_distance=3.0,
                     dofs_per_joint=3, ext_parent=None, ext_offset=None, obs_v=6, self_obs_v=1, num_force_sensors=0, amp_obs_v=1,
                     remove_base_rot=False, self_obs_extra=None, amp_obs_extra=None, zero_out_far_train=False, zero_out_far_steps=90,
                     cycle_motion_xp=False, num_self_obs_hist=0, track_body_reward=False, num_traj_samples=1, traj_sample_timestep=1 / 30, amp_ref_table=None):
    """`self_obs_extra` / `amp_obs_extra`: fp32 [N, E] per-env constant observation columns (shape parameters, limb weights) or None."""
    p = L.ImParams()
    p.remove_base_rot = int(bool(remove_base_rot))
    p.num_self_obs_hist = int(num_self_obs_hist)
    p.track_body_reward = int(bool(track_body_reward))
    p.num_traj_samples, p.traj_sample_timestep = int(num_traj_samples), float(np.float32(traj_sample_timestep))
    p.zero_out_far_train, p.zero_out_far_steps, p.cycle_motion_xp = int(bool(zero_out_far_train)), int(zero_out_far_steps), int(bool(cycle_motion_xp))
    p.num_self_obs_extra = 0 if self_obs_extra is None else int(self_obs_extra.shape[1])
    p.num_amp_obs_extra = 0 if amp_obs_extra is None else int(amp_obs_extra.shape[1])
    p.self_obs_extra, p.amp_obs_extra = ptr(self_obs_extra), ptr(amp_obs_extra)
    p.amp_ref_table = ptr(amp_ref_table)
    p.amp_obs_v = int(amp_obs_v)
    p.obs_v = int(obs_v)
    p.self_obs_v, p.num_force_sensors = int(self_obs_v), int(num_force_sensors)
    p.dofs_per_joint = int(dofs_per_joint)
    p.num_ext_bodies = 0 if ext_parent is None else int(ext_parent.shape[0])
    p.ext_parent, p.ext_offset = ptr(ext_parent), ptr(ext_offset)
    p.dt = float(np.float32(dt))
    p.max_episode_length = int(max_episode_length)
    for k in ("k_pos", "k_rot", "k_vel", "k_ang_vel", "w_pos", "w_rot", "w_vel", "w_ang_vel"):
        setattr(p, k, float(reward_specs[k]))
    p.power_reward, p.power_coefficient = int(bool(power_reward)), float(power_coefficient)
    p.enable_early_termination = int(bool(enable_early_termination))
    p.use_mean_termination = int(bool(use_mean_termination))
    p.disable_collision_check = int(bool(disable_collision_check))
    p.local_root_obs, p.root_height_obs = int(bool(local_root_obs)), int(bool(root_height_obs))
    p.num_track_bodies, p.track_slot = int(num_track_bodies), ptr(track_slot)
    p.reset_mask, p.num_reset_bodies = ptr(reset_mask), int(num_reset_bodies)
    p.first_reset_body = int(first_reset_body)
    p.termination_distances = ptr(termination_distances)
    p.num_key_bodies, p.key_body_ids = int(num_key_bodies), ptr(key_body_ids)
    p.num_amp_joints, p.amp_joint_slot = int(num_amp_joints), ptr(amp_joint_slot)
    p.num_amp_obs_steps, p.num_amp_obs_per_step = int(num_amp_obs_steps), int(num_amp_obs_per_step)
    p.num_self_obs, p.num_task_obs = int(num_self_obs), int(num_task_obs)
    p.cycle_motion, p.zero_out_far = int(bool(cycle_motion)), int(bool(zero_out_far))
    p.close_distance, p.far_distance = float(close_distance), float(far_distance)
    return p


RESET_SUBLISTS = 16  # PHC_RESET_SUBLISTS
RESET_COUNT_STRIDE = 32  # PHC_RESET_COUNT_STRIDE


def reset_sublist_cap(num_envs):
    """Capacity of one device reset sub-list (include/phc_amd.h: phc_im_buffers_t.reset_sublist_cap)."""
    blocks = (num_envs + 7) // 8
    return 8 * ((blocks + RESET_SUBLISTS - 1) // RESET_SUBLISTS)


def im_buffers_struct(progress_buf, reset_buf, terminate_buf, rew_buf, reward_raw, obs_buf, amp_obs_in, amp_obs_out,
                      sampled_motion_ids, motion_start_times, motion_start_times_offset, global_offset,
                      ref_body_pos=None, ref_body_rot=None, ref_body_vel=None, ref_dof_pos=None,
                      cycle_counter=None, recovery_counter=None, point_goal=None, cycle_phase=None, reset_list=None, reset_count=None,
                      reset_slot=0, offset_rand=None, body_state_hist=None, occl_mask=None, amp_env_stride=0, reset_rng_counter=None):
    b = L.ImBuffers()
    b.amp_env_stride = int(amp_env_stride)
    b.reset_rng_counter = ptr(reset_rng_counter)
    b.occl_mask = ptr(occl_mask)
    b.offset_rand = ptr(offset_rand)
    b.body_state_hist = ptr(body_state_hist)
    b.reset_list, b.reset_count, b.reset_slot = ptr(reset_list), ptr(reset_count), int(reset_slot)
    b.reset_sublist_cap = 0 if reset_list is None else int(reset_list.shape[0]) // RESET_SUBLISTS
    b.progress_buf, b.reset_buf, b.terminate_buf = ptr(progress_buf), ptr(reset_buf), ptr(terminate_buf)
    b.rew_buf, b.reward_raw, b.obs_buf = ptr(rew_buf), ptr(reward_raw), ptr(obs_buf)
    # (windows inside longer per-env strips come as non-contiguous views: their first element is what the kernels need)
    first = lambda t: t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()
    b.amp_obs_in, b.amp_obs_out = (ptr(t) if amp_env_stride == 0 else first(t) for t in (amp_obs_in, amp_obs_out))
    b.sampled_motion_ids = ptr(sampled_motion_ids)
    b.motion_start_times, b.motion_start_times_offset = ptr(motion_start_times), ptr(motion_start_times_offset)
    b.global_offset = ptr(global_offset)
    b.ref_body_pos, b.ref_body_rot, b.ref_body_vel, b.ref_dof_pos = ptr(ref_body_pos), ptr(ref_body_rot), ptr(ref_body_vel), ptr(ref_dof_pos)
    b.cycle_counter, b.recovery_counter = ptr(cycle_counter), ptr(recovery_counter)
    b.point_goal, b.cycle_phase = ptr(point_goal), ptr(cycle_phase)
    return b


def task_index_tables(model, track_bodies, reset_bodies, key_bodies, amp_remove_names=("L_Hand", "R_Hand", "L_Toe", "R_Toe"),
                      has_dof_subset=True):
    """Per-body index tables the task kernels use (all int32 numpy, length PHC_MAX_BODIES).

    track_slot / reset_mask follow `_build_key_body_ids_tensor` (humanoid.py:1674-1691) on cfg.env.trackBodies /
    reset_bodies; amp_joint_slot follows the dof_subset construction (humanoid.py:388-413)."""
    MB = MAX_BODIES
    names = model.body_names
    track_slot = np.full(MB, -1, dtype=np.int32)
    for s, n in enumerate(track_bodies):
        track_slot[names.index(n)] = s
    reset_mask = np.zeros(MB, dtype=np.int32)
    for n in reset_bodies:
        reset_mask[names.index(n)] = 1
    key_ids = np.array([names.index(n) for n in key_bodies], dtype=np.int32)
    amp_slot = np.full(MB, -1, dtype=np.int32)
    s = 0
    for j in range(1, len(names)):
        if (not has_dof_subset) or names[j] not in amp_remove_names:
            amp_slot[j] = s
            s += 1
    return track_slot, reset_mask, key_ids, amp_slot, s


def teleop_args_struct(num_envs, num_dof, rew_buf, reward_raw, reward_im=None, terms=(), scales=None, dt=1 / 30, num_bodies=0, feet=(), max_contact_force=0.0,
                       push_interval=0, recovery_steps=60, **arrays):
    """phc_teleop_args_t (phc_teleop_rewards).  `terms`: names of _lib.TELEOP_TERMS in column order; `scales`: {name: reward_specs value x dt}; `arrays`: the
    nullable inputs and state arrays by field name (torch tensors / numpy arrays; what a term that is off would read may stay out)."""
    a = L.TeleopArgs()
    a.num_envs, a.num_dof, a.num_bodies, a.num_feet = int(num_envs), int(num_dof), int(num_bodies), len(feet)
    assert len(feet) <= L.TELEOP_MAX_FEET, "at most PHC_TELEOP_MAX_FEET feet"
    for i, b in enumerate(feet):
        a.feet[i] = int(b)
    a.num_im_cols = 0 if reward_im is None else int(reward_im.shape[1])
    mask = 0
    for r, name in enumerate(terms):
        t = L.TELEOP_TERMS.index(name)
        mask |= 1 << t
        a.order[r] = t
        a.scale[t] = float(np.float32((scales or {}).get(name, 1.0)))
    a.term_mask = mask
    a.dt, a.max_contact_force = float(np.float32(dt)), float(np.float32(max_contact_force))
    a.push_interval, a.recovery_steps = int(push_interval), int(recovery_steps)
    a.rew_buf, a.reward_raw, a.reward_im = ptr(rew_buf), ptr(reward_raw), ptr(reward_im)
    known = {n for n, _ in L.TeleopArgs._fields_}
    for name, x in arrays.items():
        if name not in known:
            raise TypeError(f"phc_teleop_args_t has no field {name!r}")
        setattr(a, name, ptr(x))
    return a


def stream_args_struct(num_envs, window, fold, frames, *, mode=L.STREAM_ADVANCE, limb_pairs=(), limb_lengths=(), limb_scale=False, frame_mat=None, dt=1 / 30,
                       close_distance=0.25, far_distance=3.0, track_root_body=0, **arrays):
    """phc_stream_args_t (phc_stream_track).  `fold`: the fp64 table [4, FW, FW] of phc_amd.stream.fold_table; `frames`: the staging buffer [1 or N, NB, 3];
    `limb_pairs`: (parent, child) body indices; `frame_mat`: 3 x 3, row-major; `arrays`: the other pointer fields by name (torch tensors / numpy arrays)."""
    a = L.StreamArgs()
    a.num_envs, a.mode, a.window = int(num_envs), int(mode), int(window)
    a.fold_window = 0 if fold is None else int(fold.shape[-1])
    a.frame_rows = 0 if frames is None else int(frames.shape[0])
    assert len(limb_pairs) <= L.STREAM_MAX_PAIRS and len(limb_pairs) == len(limb_lengths), "at most PHC_STREAM_MAX_PAIRS limb pairs, a length each"
    a.limb_scale, a.num_pairs = int(bool(limb_scale)), len(limb_pairs)
    for k, ((p, c), ln) in enumerate(zip(limb_pairs, limb_lengths)):
        a.pair_parent[k], a.pair_child[k], a.pair_length[k] = int(p), int(c), float(np.float32(ln))
    M = np.eye(3) if frame_mat is None else np.asarray(frame_mat, dtype=np.float64).reshape(3, 3)
    for k, v in enumerate(M.reshape(-1)):
        a.frame_mat[k] = float(np.float32(v))
    a.dt, a.close_distance, a.far_distance = float(np.float32(dt)), float(np.float32(close_distance)), float(np.float32(far_distance))
    a.track_root_body = int(track_root_body)
    a.fold, a.frames = ptr(fold), ptr(frames)
    known = {n for n, _ in L.StreamArgs._fields_}
    for name, x in arrays.items():
        if name not in known:
            raise TypeError(f"phc_stream_args_t has no field {name!r}")
        setattr(a, name, ptr(x))
    return a


def record_args_struct(num_envs, obs_dim, num_actions, step, capacity, **arrays):
    """phc_record_args_t (phc_dataset_record): `arrays` are the pointer fields by name (torch tensors / numpy arrays, contiguous)."""
    a = L.RecordArgs()
    a.num_envs, a.obs_dim, a.num_actions, a.step, a.capacity = int(num_envs), int(obs_dim), int(num_actions), int(step), int(capacity)
    known = {n for n, _ in L.RecordArgs._fields_}
    for name, x in arrays.items():
        if name not in known:
            raise TypeError(f"phc_record_args_t has no field {name!r}")
        setattr(a, name, ptr(x))
    return a


def motion_record_args_struct(num_envs, num_bodies, num_ext, num_dof, cap, dt, *, ref=False, seed=False, one_segment=False, **arrays):
    """phc_motion_record_args_t (phc_motion_record): W follows from the sizes and `ref`; `arrays` are the pointer fields by name (torch tensors / numpy arrays,
    contiguous)."""
    a = L.MotionRecordArgs()
    a.num_envs, a.num_bodies, a.num_ext, a.num_dof, a.cap = int(num_envs), int(num_bodies), int(num_ext), int(num_dof), int(cap)
    a.flags = (L.RECORD_REF if ref else 0) | (L.RECORD_SEED if seed else 0) | (L.RECORD_ONE_SEGMENT if one_segment else 0)
    a.width = motion_record_width(num_bodies, num_ext, num_dof, ref)
    a.dt = float(np.float32(dt))
    known = {n for n, _ in L.MotionRecordArgs._fields_}
    for name, x in arrays.items():
        if name not in known:
            raise TypeError(f"phc_motion_record_args_t has no field {name!r}")
        setattr(a, name, ptr(x))
    return a


def jpeg_args_struct(num_frames, width, height, restart_interval, row_stride, frame_stride, out_stride, scratch_bytes, **arrays):
    """phc_jpeg_args_t (phc_jpeg_encode): strides in bytes; `arrays` are rgba, qtab (HOST memory: uint8 [2, 64], zigzag order), out, length, scratch and
    optionally coef, as torch tensors / numpy arrays (contiguous) or raw addresses (a strided view's first element)."""
    a = L.JpegArgs()
    a.num_frames, a.width, a.height, a.restart_interval = int(num_frames), int(width), int(height), int(restart_interval)
    a.row_stride, a.frame_stride, a.out_stride, a.scratch_bytes = int(row_stride), int(frame_stride), int(out_stride), int(scratch_bytes)
    assert set(arrays) <= {"rgba", "qtab", "out", "length", "scratch", "coef"}, sorted(arrays)
    for name, x in arrays.items():
        setattr(a, name, x if x is None or isinstance(x, int) else ptr(x))
    return a


def motion_record_width(num_bodies, num_ext, num_dof, ref=False):
    """W of a frame row (phc_motion_record_width): root_pos 3 | body quaternions 4 NB | pose_aa 3 (NB + E) | dof_pos D | root velocities 6 | time 1 | ref_body_pos 3 NB."""
    return 3 + 4 * int(num_bodies) + 3 * (int(num_bodies) + int(num_ext)) + int(num_dof) + 7 + (3 * int(num_bodies) if ref else 0)
