"""TEST INFRASTRUCTURE ONLY -- array-in / array-out restatement of ONE post-physics step and ONE reset of the imitation task, composed from the
primitives of phc_oracle.py, with an optional branch trace (the sibling of dyn_oracle.sim_step for the task kernels).

    post_step(lib, cfg, st, dtype, trace)    HumanoidIm.post_physics_step: pre-physics counters, _compute_reward, _compute_reset, observations
    reset_step(lib, cfg, t, dtype, ...)      HumanoidIm._reset_envs at given start times: imposed state, observations, AMP history
    reset_from_state(lib, cfg, st, dtype)    the getup reset that keeps the simulator state

It needs no task object and nothing the code under test produced.  `dtype`: np.float32 follows the reference's operation order; np.float64 runs the
same formulas on the same fp32 inputs.  The clock and index arithmetic (motion_time, calc_frame_blend, sample_time_interval) stays fp32 in both: the
contract there is bit-exact.  `trace` (a dict) receives, per env, each branch taken and its deciding quantity.

    lib   the dict phc_oracle.get_motion_state / get_motion_state_robot take
    cfg   task_cfg(...): the options phc_im_params_t carries
    st    the per-env state before the step (see post_step)

Only tests/ may import this module."""
import numpy as np

import phc_oracle as po

F = np.float32
FRAME_KEYS = ("gts", "grs", "gvs", "gavs", "lrs", "dvs", "dof_pos", "gts_t", "grs_t")
TRANSITION_DISTANCE = 0.25   # humanoid_im.py:891


def task_cfg(num_bodies, **kw):
    """The options of one launch, with the default SMPL task's values.  `track_ids` / `reset_ids`: body indices (track_ids in slot order);
    `amp_joint_bodies`: the bodies whose joint enters the AMP observation, in slot order; `termination_distances`: per body [num_bodies]."""
    c = dict(num_bodies=num_bodies, dt=1 / 30, max_episode_length=300, specs=po.DEFAULT_REWARD_SPECS, power_reward=True, power_coefficient=0.0005,
             enable_early_termination=True, use_mean_termination=False, disable_collision_check=False, local_root_obs=True, root_height_obs=True,
             track_ids=np.arange(num_bodies), reset_ids=np.arange(num_bodies), termination_distances=np.full(num_bodies, 0.25, F),
             key_ids=np.zeros(0, np.int64), amp_joint_bodies=np.arange(1, num_bodies), num_amp_obs_steps=10, cycle_motion=False, zero_out_far=False,
             close_distance=0.25, far_distance=3.0, zero_out_far_train=False, zero_out_far_steps=90, cycle_motion_xp=False, obs_v=6, amp_obs_v=1,
             remove_base_rot=False, track_body_reward=False, dofs_per_joint=3, ext_parent=None, ext_pos=None, num_traj_samples=1, traj_sample_timestep=1 / 30)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    return c


def cast_lib(lib, dtype):
    return {k: (v.astype(dtype) if k in FRAME_KEYS else v) for k, v in lib.items()}


def lookup(lib, ids, times, offset, dtype):
    """get_motion_state / get_motion_state_robot (motion_lib_base.py:437-520, motion_lib_real.py:236-361) on `lib` cast to `dtype`, times fp32."""
    D = np.dtype(dtype).type
    return _lookup_generic(cast_lib(lib, D), np.asarray(ids, np.int64), np.asarray(times, F), None if offset is None else np.asarray(offset).astype(D), D)


def _lookup_generic(lib, ids, times, off, D):
    """(phc_oracle's lookups hard-wire fp32 constants; this is the same sequence of operations with the blend factor cast to D)"""
    idx0, idx1, blend = po.calc_frame_blend(times, lib["motion_lengths"][ids], lib["motion_num_frames"][ids], lib["motion_dt"][ids])
    f0, f1 = idx0 + lib["length_starts"][ids], idx1 + lib["length_starts"][ids]
    b1 = blend.astype(D)[:, None]
    b2 = b1[:, :, None]
    one = D(1)
    o = D(0) if off is None else off[:, None, :]
    lerp = lambda a, b: (one - b2) * a[f0] + b2 * a[f1]
    r = dict(rg_pos=lerp(lib["gts"], lib["gts"]) + o, body_vel=lerp(lib["gvs"], lib["gvs"]), body_ang_vel=lerp(lib["gavs"], lib["gavs"]),
             rb_rot=po.slerp(lib["grs"][f0], lib["grs"][f1], b2), f0l=f0, f1l=f1, blend=blend)
    if "dof_pos" in lib:
        r["dof_vel"] = (one - b1) * lib["dvs"][f0] + b1 * lib["dvs"][f1]
        r["dof_pos"] = (one - b1) * lib["dof_pos"][f0] + b1 * lib["dof_pos"][f1]
        r["rg_pos_t"] = lerp(lib["gts_t"], lib["gts_t"]) + o
        r["rg_rot_t"] = po.slerp(lib["grs_t"][f0], lib["grs_t"][f1], b2)
    else:
        r["dof_vel"] = lerp(lib["dvs"], lib["dvs"]).reshape(len(ids), -1)
        r["dof_pos"] = po.quat_to_exp_map(po.slerp(lib["lrs"][f0], lib["lrs"][f1], b2)[:, 1:]).reshape(len(ids), -1)
    r["root_pos"], r["root_rot"] = r["rg_pos"][:, 0].copy(), r["rb_rot"][:, 0].copy()
    return r


def motion_time(progress, dt, start, start_off):
    """humanoid_im.py:879,752,1118 -- fp32, left to right."""
    return (progress.astype(F) * F(dt) + start.astype(F)) + start_off.astype(F)


def disk_offset(uv, D):
    """humanoid_im.py:971-977,1135-1140: a point of the 5 m disk from two uniform draws."""
    rd = np.sqrt(uv[:, 0].astype(D)) * D(5)
    ang = uv[:, 1].astype(D) * D(F(np.pi)) * D(2)
    return np.stack([np.cos(ang) * rd, np.sin(ang) * rd], -1)


def _rot(q, v):
    """my_quat_rotate of [N, J, 3] vectors by per-env [N, 4] quaternions."""
    N, J = v.shape[:2]
    return po.my_quat_rotate(np.repeat(q[:, None], J, axis=1).reshape(-1, 4), v.reshape(-1, 3)).reshape(N, J, 3)


def _qmul_env(q, r):
    N, J = r.shape[:2]
    return po.quat_mul(np.repeat(q[:, None], J, axis=1).reshape(-1, 4), r.reshape(-1, 4)).reshape(N, J, 4)


def heading_root(cfg, root_rot):
    return po.remove_base_rot(root_rot) if cfg["remove_base_rot"] else root_rot


def self_obs(cfg, body_pos, body_rot, body_vel, body_ang_vel):
    """compute_humanoid_observations_smpl_max (humanoid.py:1995-2050), no shape columns."""
    N, J = body_pos.shape[:2]
    root_rot = heading_root(cfg, body_rot[:, 0])
    hinv = po.calc_heading_quat_inv(root_rot)
    lp = _rot(hinv, body_pos - body_pos[:, :1]).reshape(N, J * 3)[:, 3:]
    lr = po.quat_to_tan_norm(_qmul_env(hinv, body_rot).reshape(-1, 4)).reshape(N, J * 6)
    if not cfg["local_root_obs"]:
        lr[:, 0:6] = po.quat_to_tan_norm(root_rot)
    parts = ([body_pos[:, 0, 2:3]] if cfg["root_height_obs"] else []) + [lp, lr, _rot(hinv, body_vel).reshape(N, -1), _rot(hinv, body_ang_vel).reshape(N, -1)]
    return np.concatenate(parts, axis=-1)


def self_obs_hist(cfg, body_pos, body_rot, body_vel, body_ang_vel):
    """compute_humanoid_observations_smpl_max_v2 (humanoid.py:2054-2108): [N, T, J, .] states, oldest first, the last one current; every step's block is
    taken about the CURRENT root and heading, its height column is that step's root height, its raw root rotation that step's."""
    N, T, J = body_pos.shape[:3]
    root_rot = heading_root(cfg, body_rot[:, -1, 0])
    hinv = np.repeat(po.calc_heading_quat_inv(root_rot), T, axis=0)
    flat = lambda a: a.reshape(N * T, J, a.shape[-1])
    lp = _rot(hinv, flat(body_pos - body_pos[:, -1:, :1])).reshape(N, T, J * 3)[..., 3:]
    lr = po.quat_to_tan_norm(_qmul_env(hinv, flat(body_rot)).reshape(-1, 4)).reshape(N, T, J * 6)
    if not cfg["local_root_obs"]:
        lr[..., 0:6] = po.quat_to_tan_norm(body_rot[:, :, 0].reshape(-1, 4)).reshape(N, T, 6)
    parts = ([body_pos[:, :, 0, 2:3]] if cfg["root_height_obs"] else []) + [lp, lr, _rot(hinv, flat(body_vel)).reshape(N, T, -1),
                                                                            _rot(hinv, flat(body_ang_vel)).reshape(N, T, -1)]
    return np.concatenate(parts, axis=-1).reshape(N, -1)


def task_obs(cfg, root_pos, root_rot, b, r, dof=None, ref_dof=None):
    """compute_imitation_observations{,_v2,_v3,_v6,_v7,_v8,_v9} (humanoid_im.py:1203-1520) at time_steps = 1.  `b` / `r`: (pos, rot, vel, angvel) of
    the tracked bodies, simulated and reference; `dof` / `ref_dof` [N, J - 1, 3]: obs_v 2."""
    v = cfg["obs_v"]
    N, J = b[0].shape[:2]
    rr = heading_root(cfg, root_rot)
    hinv, h = po.calc_heading_quat_inv(rr), po.calc_heading_quat(rr)
    dpos = _rot(hinv, r[0] - b[0]).reshape(N, -1)
    dvel = _rot(hinv, r[2] - b[2]).reshape(N, -1)
    lref = _rot(hinv, r[0] - root_pos[:, None]).reshape(N, -1)
    if v == 7:
        return np.concatenate([dpos, dvel, lref], -1)
    drot = po.quat_mul(r[1], po.quat_conjugate(b[1]))
    h_e = np.repeat(h[:, None], J, axis=1).reshape(-1, 4)
    drot = po.quat_to_tan_norm(po.quat_mul(_qmul_env(hinv, drot).reshape(-1, 4), h_e)).reshape(N, -1)
    dav = _rot(hinv, r[3] - b[3]).reshape(N, -1)
    lrot = po.quat_to_tan_norm(_qmul_env(hinv, r[1]).reshape(-1, 4)).reshape(N, -1)
    if v == 3:
        return np.concatenate([dpos, drot], -1)
    if v in (1, 2):
        return np.concatenate([dpos, drot, dvel, dav] + ([(ref_dof - dof).reshape(N, -1)] if v == 2 else []), -1)
    if v == 8:
        return np.concatenate([dpos, drot, dvel, dav, lref, lrot, _rot(hinv, r[2]).reshape(N, -1), _rot(hinv, r[3]).reshape(N, -1)], -1)
    if v == 9:
        return np.concatenate([dpos, drot, dvel[:, :3], dav[:, :3], lref, lrot], -1)
    assert v in (4, 6), v
    return np.concatenate([dpos, drot, dvel, dav, lref, lrot], -1)


def amp_obs(cfg, root_pos, root_rot, root_vel, root_ang_vel, dof_pos, dof_vel, key_pos, key_vel=None):
    """build_amp_observations_smpl / _smpl_v2 / _robot (humanoid_amp.py:967-1104).  dof_pos / dof_vel: [N, NJ, 3] (spherical) or [N, NJ] (revolute)."""
    N = root_pos.shape[0]
    rr = heading_root(cfg, root_rot)
    hinv = po.calc_heading_quat_inv(rr)
    rot_obs = po.quat_to_tan_norm(po.quat_mul(hinv, rr) if cfg["local_root_obs"] else rr)
    sub = np.asarray(cfg["amp_joint_bodies"]) - 1
    if cfg["dofs_per_joint"] == 1:
        dof_obs, dv = dof_pos[:, sub], dof_vel[:, sub]
    else:
        dof_obs = po.quat_to_tan_norm(po.exp_map_to_quat(dof_pos[:, sub].reshape(-1, 3))).reshape(N, -1)   # dof_to_obs_smpl humanoid.py:1756-1765
        dv = dof_vel[:, sub].reshape(N, -1)
    parts = ([root_pos[:, 2:3]] if cfg["root_height_obs"] else []) + [rot_obs, po.my_quat_rotate(hinv, root_vel), po.my_quat_rotate(hinv, root_ang_vel),
                                                                     dof_obs, dv, _rot(hinv, key_pos - root_pos[:, None]).reshape(N, -1)]
    if cfg["amp_obs_v"] == 2:
        parts.append(_rot(hinv, key_vel).reshape(N, -1))
    return np.concatenate(parts, -1)


def imitation_reward(cfg, bp, br, bv, bw, rp, rr, rv, rw, D, trace=None):
    """compute_imitation_reward (humanoid_im.py:1524-1554)."""
    s = {k: D(F(v)) for k, v in cfg["specs"].items()}
    d = rp - bp
    m_pos = (d * d).mean(-1).mean(-1)
    ang, _ = po.quat_to_angle_axis(po.quat_mul(rr, po.quat_conjugate(br)))
    m_rot = (ang * ang).mean(-1)
    d = rv - bv
    m_vel = (d * d).mean(-1).mean(-1)
    d = rw - bw
    m_ang = (d * d).mean(-1).mean(-1)
    raw = np.stack([np.exp(-s["k_pos"] * m_pos), np.exp(-s["k_rot"] * m_rot), np.exp(-s["k_vel"] * m_vel), np.exp(-s["k_ang_vel"] * m_ang)], -1)
    rew = s["w_pos"] * raw[:, 0] + s["w_rot"] * raw[:, 1] + s["w_vel"] * raw[:, 2] + s["w_ang_vel"] * raw[:, 3]
    if trace is not None:
        dq = po.quat_mul(rr, po.quat_conjugate(br))
        with np.errstate(invalid="ignore"):
            trace.update(rot_angle=ang, rot_w=dq[..., 3], rot_sin=np.sqrt(1 - dq[..., 3] ** 2),
                         exp_arg=np.stack([s["k_pos"] * m_pos, s["k_rot"] * m_rot, s["k_vel"] * m_vel, s["k_ang_vel"] * m_ang], -1))
    return rew, raw


def extend(body_pos, body_rot, ext_parent, ext_pos):
    """humanoid_im.py:917-919."""
    ext_parent = np.asarray(ext_parent, np.int64)
    N, E = body_pos.shape[0], len(ext_parent)
    ep = np.broadcast_to(np.asarray(ext_pos).astype(body_pos.dtype)[None], (N, E, 3)).reshape(-1, 3)
    cur = po.my_quat_rotate(body_rot[:, ext_parent].reshape(-1, 4), ep).reshape(N, E, 3) + body_pos[:, ext_parent]
    return np.concatenate([body_pos, cur], 1), np.concatenate([body_rot, body_rot[:, ext_parent]], 1)


def heading_horizontal(cfg, root_rot):
    """Length of the horizontal part of the root's rotated x axis: the conditioning of calc_heading's atan2."""
    x = np.zeros(root_rot.shape[:-1] + (3,), root_rot.dtype)
    x[..., 0] = 1
    d = po.my_quat_rotate(heading_root(cfg, root_rot), x)
    return np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)


def _zero_out_far(cfg, D, root_pos, b, r, trace, key):
    """humanoid_im.py:783-797 / 834-845 on the tracked subsets (lists of [N, J, .], modified in place).  -> the distance (_point_goal)."""
    dist = np.sqrt(((root_pos - r[0][:, 0]) ** 2).sum(-1))
    close, far = dist > D(F(cfg["close_distance"])), dist > D(F(cfg["far_distance"]))
    r[0][close, 1:], r[1][close, 1:] = b[0][close, 1:], b[1][close, 1:]
    r[2][close], r[3][close] = b[2][close], b[3][close]
    fd = D(F(cfg["far_distance"]))
    r[0][far, 0] = (r[0][far, 0] - b[0][far, 0]) / dist[far, None] * fd + b[0][far, 0]
    if trace is not None:
        trace[key + "_dist"], trace[key + "_close"], trace[key + "_far"] = dist, close, far
    return dist


def _task_block(cfg, D, body, ref1, dof_pos, ref1_dof_pos, occl, trace, key="zof"):
    """_compute_task_obs (humanoid_im.py:728-871) after the lookup: subsets, zero_out_far, occlusion, the version's function."""
    ids = np.asarray(cfg["track_ids"])
    b = [a[:, ids].copy() for a in body]
    r = [a[:, ids].copy() for a in ref1]
    root_pos, root_rot = body[0][:, 0], body[1][:, 0]
    pg = None
    if cfg["zero_out_far"] and cfg["obs_v"] not in (1, 2, 3):
        pg = _zero_out_far(cfg, D, root_pos, b, r, trace, key)
    if occl is not None and cfg["obs_v"] not in (1, 2, 3):
        m = occl.astype(bool)
        for k in ((0, 1) if cfg["obs_v"] == 7 else (0, 1, 2, 3)):
            r[k][m] = b[k][m]
    dof = ref_dof = None
    if cfg["obs_v"] == 2:
        nj = cfg["num_bodies"] - 1
        dof, ref_dof = dof_pos.reshape(-1, nj, 3)[:, ids[1:] - 1], ref1_dof_pos.reshape(-1, nj, 3)[:, ids[1:] - 1]
    return task_obs(cfg, root_pos, root_rot, b, r, dof, ref_dof), pg


def _amp_from_state(cfg, body, dof_pos, dof_vel):
    """HumanoidAMP._compute_amp_observations (humanoid_amp.py:672-707)."""
    N, nj = body[0].shape[0], cfg["num_bodies"] - 1
    k = np.asarray(cfg["key_ids"])
    sph = cfg["dofs_per_joint"] != 1
    return amp_obs(cfg, body[0][:, 0], body[1][:, 0], body[2][:, 0], body[3][:, 0], dof_pos.reshape(N, nj, 3) if sph else dof_pos,
                   dof_vel.reshape(N, nj, 3) if sph else dof_vel, body[0][:, k], body[2][:, k])


def post_step(lib, cfg, st, dtype=F, trace=None):
    """One post_physics_step.  `st` (per env, before the step): progress (the incoming progress_buf), motion_ids, start, start_off, goff [N, 3],
    body_pos / body_rot / body_vel / body_ang_vel [N, NB, .], dof_pos, dof_vel, dof_force [N, ND]; optional cycle_counter, recovery_counter,
    point_goal, cycle_phase, occl_mask [N, tracked], offset_rand [N, 2].
    -> dict: progress, reset, terminate, reward, reward_raw, self_obs, task_obs, amp_obs, ref1_pos / _rot / _vel / _dof_pos, start, start_off, goff,
    cycle_counter, recovery_counter, point_goal."""
    D = np.dtype(dtype).type
    nb, N = cfg["num_bodies"], len(st["progress"])
    mids = np.asarray(st["motion_ids"], np.int64)
    body = [np.asarray(st[k]).astype(D) for k in ("body_pos", "body_rot", "body_vel", "body_ang_vel")]
    dof_pos, dof_vel, dof_force = (np.asarray(st[k]).astype(D) for k in ("dof_pos", "dof_vel", "dof_force"))
    progress = np.asarray(st["progress"], np.int64) + 1                                              # humanoid.py:1637
    start, start_off = np.asarray(st["start"], F).copy(), np.asarray(st["start_off"], F).copy()
    goff_rew = np.asarray(st["goff"]).astype(D)
    goff = goff_rew.copy()
    dec = lambda c: np.zeros(N, np.int64) if c is None else np.where(np.asarray(c) > 1, np.asarray(c, np.int64) - 1, 0)
    cycle_cnt, recovery_cnt = dec(st.get("cycle_counter")), dec(st.get("recovery_counter"))          # humanoid_im.py:1076-1079, getup :198-201
    t_rew = motion_time(progress, cfg["dt"], start, start_off)                                       # :879
    mlen = lib["motion_lengths"][mids].astype(F)
    pass_len = t_rew >= mlen                                                                         # :1121
    pass_time, cycled, t0 = pass_len, np.zeros(N, bool), t_rew
    if cfg["cycle_motion"]:
        pass_time = progress >= cfg["max_episode_length"] - 1                                        # :1120
        cycled = pass_len
        start_off = np.where(cycled, (-progress).astype(F) * F(cfg["dt"]), start_off).astype(F)      # :1126
        start = np.where(cycled, po.sample_time_interval(np.asarray(st["cycle_phase"], F), mlen), start).astype(F)   # :1127
        cycle_cnt = np.where(cycled, 60, cycle_cnt)                                                  # :1128
        rp = lookup(lib, mids, start, None, D)["rg_pos"][:, 0]
        new_xy = body[0][:, 0, :2] - rp[:, :2]                                                       # :1142
        uv = st.get("offset_rand")
        if uv is not None and cfg["cycle_motion_xp"]:
            new_xy = new_xy + np.asarray(uv).astype(D)
        elif uv is not None and cfg["zero_out_far"] and cfg["zero_out_far_train"]:
            new_xy = new_xy + disk_offset(np.asarray(uv), D)
        goff[cycled, :2] = new_xy[cycled]
        t0 = motion_time(progress, cfg["dt"], start, start_off)                                      # :1144
    out_progress = np.where(recovery_cnt > 0, progress - 1, progress)                                # humanoid_im_getup.py:215
    t1 = motion_time(out_progress + 1, cfg["dt"], start, start_off)                                  # :752
    # ---- _compute_reward (:876-948): the clock and the offset from BEFORE a clip restart
    rr = lookup(lib, mids, t_rew, goff_rew, D)
    ext = cfg["ext_parent"] is not None and len(cfg["ext_parent"]) > 0
    tr_rew = {} if trace is not None else None
    if cfg["track_body_reward"]:
        i = np.asarray(cfg["track_ids"])
        rew, raw = imitation_reward(cfg, body[0][:, i], body[1][:, i], body[2][:, i], body[3][:, i], rr["rg_pos"][:, i], rr["rb_rot"][:, i],
                                    rr["body_vel"][:, i], rr["body_ang_vel"][:, i], D, tr_rew)
    elif ext:
        bp, br = extend(body[0], body[1], cfg["ext_parent"], cfg["ext_pos"])
        rew, raw = imitation_reward(cfg, bp, br, body[2], body[3], np.concatenate([rr["rg_pos"], rr["rg_pos_t"][:, nb:]], 1),
                                    np.concatenate([rr["rb_rot"], rr["rg_rot_t"][:, nb:]], 1), rr["body_vel"], rr["body_ang_vel"], D, tr_rew)
    else:
        rew, raw = imitation_reward(cfg, *body, rr["rg_pos"], rr["rb_rot"], rr["body_vel"], rr["body_ang_vel"], D, tr_rew)
    root_dist = np.sqrt(((body[0][:, 0] - rr["rg_pos"][:, 0]) ** 2).sum(-1))                          # :892
    if cfg["zero_out_far"]:
        delta = np.asarray(st["point_goal"]).astype(D) - root_dist
        pg = np.minimum(delta, D(F(1.0) / F(3.0))) * D(9)                                            # compute_point_goal_reward :1558-1562
        far = root_dist > D(TRANSITION_DISTANCE)
        raw = np.where(far[:, None], D(0), raw * D(0.5))
        raw[:, 0] += pg
        rew = pg + np.where(far, D(0), rew * D(0.5))
        if trace is not None:
            trace.update(pg_delta=delta, reward_far=far)
    power = np.abs(dof_force * dof_vel).sum(-1)
    if cfg["power_reward"]:
        pr = -D(F(cfg["power_coefficient"])) * power
        pr[progress <= 3] = 0                                                                        # :943
        rew = rew + pr
        raw = np.concatenate([raw, pr[:, None]], -1)
    # ---- _compute_reset (:1117-1190)
    r0 = lookup(lib, mids, t0, goff, D)
    rid = np.asarray(cfg["reset_ids"])
    td = np.asarray(cfg["termination_distances"], F).astype(D)
    dist = np.sqrt(((body[0][:, rid] - r0["rg_pos"][:, rid]) ** 2).sum(-1))
    occl = st.get("occl_mask")
    if occl is not None:
        slot = np.full(nb, -1)
        slot[np.asarray(cfg["track_ids"])] = np.arange(len(cfg["track_ids"]))
        oc = np.asarray(occl).astype(bool)[:, np.maximum(slot[rid], 0)] & (slot[rid] >= 0)[None]
        dist = np.where(oc, D(0), dist)                                                              # :1180-1181 ref = body
    mean = dist.mean(-1)
    fallen = (mean > td[rid][0]) if cfg["use_mean_termination"] else (dist > td[rid][None]).any(-1)  # :1586-1588
    terminated = np.zeros(N, np.int64)
    if cfg["enable_early_termination"]:
        f = fallen & (progress > 1)
        if cfg["disable_collision_check"]:
            f = np.zeros(N, bool)
        terminated = f.astype(np.int64)
    reset = np.where(pass_time, 1, terminated)
    rec = ~pass_time & (cycle_cnt > 0)                                                               # :1186-1188
    reset, terminated = np.where(rec, 0, reset), np.where(rec, 0, terminated)
    reset, terminated = np.where(recovery_cnt > 0, 0, reset), np.where(recovery_cnt > 0, 0, terminated)   # humanoid_im_getup.py:212-214
    # ---- observations for the next policy step (:694-726)
    r1 = lookup(lib, mids, t1, goff, D)
    ref1 = [r1["rg_pos"], r1["rb_rot"], r1["body_vel"], r1["body_ang_vel"]]
    tobs, point_goal = _task_block(cfg, D, body, ref1, dof_pos, r1["dof_pos"], occl, trace)
    T = cfg["num_traj_samples"]
    if T > 1:                                                                                        # env.fut_tracks (:743-749): time-major blocks
        assert cfg["obs_v"] in (6, 7, 9)
        blocks = [tobs]
        for k in range(1, T):
            tk = (((out_progress + 1).astype(F) * F(cfg["dt"]) + F(k) * F(cfg["traj_sample_timestep"])) + start) + start_off
            rk = lookup(lib, mids, tk, goff, D)
            blocks.append(_task_block(dict(cfg, zero_out_far=False), D, body, [rk["rg_pos"], rk["rb_rot"], rk["body_vel"], rk["body_ang_vel"]],
                                      dof_pos, rk["dof_pos"], None, None)[0])
        tobs = np.concatenate(blocks, -1)
    sobs, hist_out = self_obs(cfg, *body), None
    if st.get("body_state_hist") is not None:                                                        # self_obs_v 2 (humanoid.py:2054-2108, 1621-1631)
        hist = np.asarray(st["body_state_hist"])
        cur = np.concatenate([np.asarray(st[k], F) for k in ("body_pos", "body_rot", "body_vel", "body_ang_vel")], -1)
        allst = np.concatenate([hist, cur[:, None]], 1).astype(D)
        sobs = self_obs_hist(cfg, allst[..., 0:3], allst[..., 3:7], allst[..., 7:10], allst[..., 10:13])
        hist_out = np.concatenate([hist[:, 1:], cur[:, None]], 1)
    if st.get("force_sensor") is not None:                                                           # self_obs_v 3 (humanoid.py:2113-2169)
        sobs = np.concatenate([sobs, np.asarray(st["force_sensor"]).astype(D)], -1)
    out = dict(progress=out_progress, reset=reset.astype(np.int64), terminate=terminated.astype(np.int64), reward=rew, reward_raw=raw,
               self_obs=sobs, body_state_hist=hist_out, task_obs=tobs, amp_obs=_amp_from_state(cfg, body, dof_pos, dof_vel),
               ref1_pos=r1["rg_pos"], ref1_rot=r1["rb_rot"], ref1_vel=r1["body_vel"], ref1_dof_pos=r1["dof_pos"],
               start=start, start_off=start_off, goff=goff, cycle_counter=cycle_cnt, recovery_counter=recovery_cnt,
               point_goal=point_goal if point_goal is not None else st.get("point_goal"))
    if trace is not None:
        trace.update(tr_rew)
        trace.update(progress=progress, t_rew=t_rew, t0=t0, t1=t1, motion_length=mlen, pass_len=pass_len, pass_time=pass_time, cycled=cycled,
                     cycle_cnt=cycle_cnt, recovery_cnt=recovery_cnt, dist=dist, term_dist=td[rid], mean_dist=mean, mean_threshold=td[rid][0],
                     fallen=fallen, root_dist=root_dist, power=power, power_counted=progress > 3, termination_armed=progress > 1,
                     is_recovery=rec, heading_horizontal=heading_horizontal(cfg, body[1][:, 0]))
    return out


def _amp_from_ref(cfg, r):
    N, nj = r["rg_pos"].shape[0], cfg["num_bodies"] - 1
    k = np.asarray(cfg["key_ids"])
    sph = cfg["dofs_per_joint"] != 1
    return amp_obs(cfg, r["rg_pos"][:, 0], r["rb_rot"][:, 0], r["body_vel"][:, 0], r["body_ang_vel"][:, 0],
                   r["dof_pos"].reshape(N, nj, 3) if sph else r["dof_pos"], r["dof_vel"].reshape(N, nj, 3) if sph else r["dof_vel"],
                   r["rg_pos"][:, k], r["body_vel"][:, k])


def reset_step(lib, cfg, motion_ids, t, dtype=F, offset_rand=None, occl_mask=None, trace=None):
    """HumanoidIm._reset_envs (humanoid.py:585-621; humanoid_amp.py:378-398,508-528,559-637; humanoid_im.py:955-1023) with the start times `t` given:
    the imposed state IS the reference at t, the observations are those of progress 0, the AMP history frame k comes from the reference at t - k dt."""
    D = np.dtype(dtype).type
    mids, t = np.asarray(motion_ids, np.int64), np.asarray(t, F)
    N = len(mids)
    r = lookup(lib, mids, t, None, D)
    body = [r["rg_pos"], r["rb_rot"], r["body_vel"], r["body_ang_vel"]]
    goff = np.zeros((N, 3), D)
    far_start = offset_rand is not None and cfg["zero_out_far"] and cfg["zero_out_far_train"]
    if far_start:
        goff[:, :2] = disk_offset(np.asarray(offset_rand), D)                                        # humanoid_im.py:966-980
    zero = np.zeros(N, F)
    r1 = lookup(lib, mids, motion_time(np.ones(N, np.int64), cfg["dt"], t, zero), goff, D)
    tobs, pg = _task_block(cfg, D, body, [r1["rg_pos"], r1["rb_rot"], r1["body_vel"], r1["body_ang_vel"]], r["dof_pos"], r1["dof_pos"], occl_mask, trace)
    S = cfg["num_amp_obs_steps"]
    hist = [_amp_from_ref(cfg, lookup(lib, mids, t + (-F(cfg["dt"])) * F(k), None, D)) for k in range(S)]      # humanoid_amp.py:575-603
    return dict(body_pos=body[0], body_rot=body[1], body_vel=body[2], body_ang_vel=body[3], dof_pos=r["dof_pos"], dof_vel=r["dof_vel"],
                self_obs=self_obs(cfg, *body), task_obs=tobs, amp_obs=np.stack(hist, 1), ref1_pos=r1["rg_pos"], start=t, start_off=zero, goff=goff,
                progress=np.zeros(N, np.int64), cycle_counter=np.full(N, cfg["zero_out_far_steps"] if far_start else 0, np.int64), point_goal=pg)


def reset_from_state(lib, cfg, st, dtype=F, fill_history=True, trace=None):
    """HumanoidImGetup's reset that keeps the simulator state (humanoid_im_getup.py:136-196): observations at progress 0 against the env's unchanged
    clock, AMP frame 0 (or every frame) from the state."""
    D = np.dtype(dtype).type
    mids = np.asarray(st["motion_ids"], np.int64)
    N = len(mids)
    body = [np.asarray(st[k]).astype(D) for k in ("body_pos", "body_rot", "body_vel", "body_ang_vel")]
    dof_pos, dof_vel = np.asarray(st["dof_pos"]).astype(D), np.asarray(st["dof_vel"]).astype(D)
    r1 = lookup(lib, mids, motion_time(np.ones(N, np.int64), cfg["dt"], np.asarray(st["start"], F), np.asarray(st["start_off"], F)),
                np.asarray(st["goff"]).astype(D), D)
    tobs, pg = _task_block(cfg, D, body, [r1["rg_pos"], r1["rb_rot"], r1["body_vel"], r1["body_ang_vel"]], dof_pos, r1["dof_pos"], st.get("occl_mask"), trace)
    a = _amp_from_state(cfg, body, dof_pos, dof_vel)
    if trace is not None:
        trace["heading_horizontal"] = heading_horizontal(cfg, body[1][:, 0])
    return dict(self_obs=self_obs(cfg, *body), task_obs=tobs, amp_obs=a, amp_frames=cfg["num_amp_obs_steps"] if fill_history else 1,
                pd_target=dof_pos, ref1_pos=r1["rg_pos"], progress=np.zeros(N, np.int64), point_goal=pg)
