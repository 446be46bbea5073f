"""`+record.motion=<out.pkl>`: record the motion the policy actually produced and export it as a clip library `MotionLibSMPL` / `MotionLibReal` load back.

What the reference does by hand -- `_record_states` / `_write_states_to_file` behind a viewer key (phc/env/tasks/base_task.py:242-246,405-440,
humanoid.py:445-453, humanoid_im.py:401-466), `_hack_output_motion` (humanoid_amp.py:827-873), the robots' dump layout
(scripts/data_process/fit_smpl_motion.py:165-187) -- with three to five `.cpu().clone()` copies per env step, a hard-coded `fps = 60` and a format its own
motion library cannot load.  Here every env step is ONE launch (`phc_motion_record`, issued behind the post-physics launch on the same stream: include/phc_amd.h
has the row layout and the row rule, csrc/phc_record.h the per-lane code) that appends a frame row per env to a block on the task's device, and the block is
copied to the host once per batch (sweep) or every `cap` steps (play).  `record_rows` is the torch statement of the same rule, used when `BACKEND = "torch"`.

Sweep (`im_eval.evaluate`): `begin_batch` after the batch's reset (frame 0 = the reset state, `seed`), `record` after every env step with `terminate_buf` as the
flag and one segment per env: a clip that fails ends at its terminating frame; `end_batch` cuts every clip to its length and drops the wrapped-around
duplicates of the last batch.  Play (`run.play`): `begin_play`, `record` with `reset_buf` as the flag -- segments `<env>_<segment>` --, a flush every `cap` steps
(default 1024 frames per env) and at `close`."""
import ctypes as C
import os

import numpy as np
import torch

BACKEND = None   # None: the launch (a HIP device is required); "torch": the torch statement everywhere (tests compare the two)
DEFAULT_CAP = 1024


# ---- the row in torch ------------------------------------------------------------------------------------------------------------------------------------
def quat_to_exp_map(q):
    """isaacgym_torch_utils.py:250-290 on xyzw quaternions [..., 4] (csrc/phc_math.h quat_to_exp_map)."""
    w = q[..., 3]
    sin_theta = torch.sqrt(1 - w * w)
    angle = 2 * torch.acos(w)
    angle = torch.atan2(torch.sin(angle), torch.cos(angle))
    mask = sin_theta.abs() > 1e-5
    axis = torch.where(mask[..., None], q[..., 0:3] / sin_theta[..., None], torch.tensor([0.0, 0.0, 1.0], dtype=q.dtype, device=q.device).expand(q.shape[:-1] + (3,)))
    return axis * torch.where(mask, angle, torch.zeros_like(angle))[..., None]


def frame_rows(src, tables, num_ext, dt, ref):
    """-> [N, W] fp32: the frame row of every env (include/phc_amd.h).  `src`: the task's tensors by the field names of phc_motion_record_args_t; `tables`:
    (joint_type [NB], dof_start [NB], axis [NB, 3]) of the model (torch, on the tensors' device)."""
    root, N = src["root_states"], src["root_states"].shape[0]
    rbs = src["rigid_body_state"].view(N, -1, 13)
    NB = rbs.shape[1]
    dof_pos = src["dof_state"].view(N, -1, 2)[..., 0]
    jt, ds, axis = tables
    aa = torch.zeros((N, NB + num_ext, 3), dtype=torch.float32, device=root.device)
    aa[:, 0] = quat_to_exp_map(root[:, 3:7])
    sph = torch.nonzero(jt == 1).flatten()
    sph = sph[sph > 0]
    if len(sph):
        aa[:, sph] = dof_pos[:, (ds[sph][:, None] + torch.arange(3, device=root.device)[None]).flatten()].view(N, len(sph), 3)
    rev = torch.nonzero(jt == 2).flatten()
    rev = rev[rev > 0]
    if len(rev):
        aa[:, rev] = axis[rev][None] * dof_pos[:, ds[rev]][..., None]
    t = src["progress_buf"].to(torch.float32) * np.float32(dt) + src["motion_start_times"] + src["motion_start_times_offset"]
    parts = [root[:, 0:3], rbs[:, :, 3:7].reshape(N, -1), aa.reshape(N, -1), dof_pos, root[:, 7:13], t[:, None]]
    if ref:
        parts.append(src["ref_body_pos"].reshape(N, -1))
    return torch.cat([p.to(torch.float32) for p in parts], dim=1)


def record_rows(rows, src, state, cap, seed=False, one_segment=False):
    """The row rule in torch (include/phc_amd.h, phc_motion_record): `rows` [N, W] of `frame_rows`; `state` = dict(frames [N, cap, W], header [N, cap, 4],
    len, seg, closed, dropped [N] int32, limit [N] int32 or None)."""
    ln, seg, closed, dropped, limit = state["len"], state["seg"], state["closed"], state["dropped"], state.get("limit")
    room = torch.full_like(ln, cap) if limit is None else torch.clamp(limit, max=cap)
    alive = closed == 0
    write = alive & (ln < room)
    drop = alive & ~(ln < room)
    flag = torch.zeros_like(ln) if seed else (src["flag"] != 0).to(torch.int32)
    e = torch.nonzero(write).flatten()
    f = ln[e].long()
    state["frames"][e, f] = rows[e]
    state["header"][e, f] = torch.stack([seg[e], src["progress_buf"][e].to(torch.int32), src["motion_ids"][e].to(torch.int32), flag[e]], dim=1)
    ln += write.to(torch.int32)
    dropped += drop.to(torch.int32)
    ends = alive & (flag != 0)
    if one_segment:
        closed |= ends.to(torch.int32)
    else:
        seg += ends.to(torch.int32)


def exp_map_to_quat(e):
    """isaacgym_torch_utils.py:342-365 in numpy: exp maps [..., 3] -> xyzw quaternions (the `body_quat` of the reference's state dump)."""
    e = np.asarray(e, dtype=np.float64)
    angle = np.linalg.norm(e, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        axis = e / angle[..., None]
    angle = np.arctan2(np.sin(angle), np.cos(angle))
    mask = np.abs(angle) > 1e-5
    angle = np.where(mask, angle, 0.0)
    axis = np.where(mask[..., None], axis, np.array([0.0, 0.0, 1.0]))
    axis = axis / np.maximum(np.linalg.norm(axis, axis=-1, keepdims=True), 1e-9)
    q = np.concatenate([axis * np.sin(0.5 * angle)[..., None], np.cos(0.5 * angle)[..., None]], axis=-1)
    return (q / np.maximum(np.linalg.norm(q, axis=-1, keepdims=True), 1e-9)).astype(np.float32)


def check_max_frames(max_frames):
    if max_frames is None:
        return None
    if isinstance(max_frames, bool) or int(max_frames) != max_frames or int(max_frames) < 1:
        raise ValueError(f"record.max_frames must be a positive integer, not {max_frames!r}")
    return int(max_frames)


def options(cfg):
    """`+record.motion=<out.pkl>` [`+record.ref=True`] [`+record.max_frames=N`] -> dict(path, ref, max_frames), or None without the switch."""
    rec = (cfg.get("record", None) or {}) if cfg is not None else {}
    path = rec.get("motion", None)
    if not path:
        return None
    return dict(path=str(path), ref=bool(rec.get("ref", False)), max_frames=check_max_frames(rec.get("max_frames", None)))


def refuse_training(cfg):
    """`train()` with the switch: the recorder belongs to the player (run.play, test=True) and to the evaluation sweep."""
    if options(cfg) is not None:
        raise NotImplementedError("+record.motion records in play (test=True) and in the evaluation sweep (im_eval=True), not while training")


def refuse_ranks(world):
    if int(world) > 1:
        raise ValueError(f"+record.motion records in one process, not on {int(world)} ranks")


class MotionRecorder:
    def __init__(self, task, max_frames=None, ref=False):
        self.task, self.ref, self.max_frames = task, bool(ref), check_max_frames(max_frames)
        self.clips = []          # dicts: key, frames [T, W], header [T, 4], failed, env, source (the library's clip, or None)
        self.dropped = 0         # frames refused for want of room, all envs
        self._state = None
        self._seen = set()
        dev = torch.device(task.device) if not isinstance(task.device, torch.device) else task.device
        if dev.type != "cuda" and BACKEND != "torch":
            raise RuntimeError(f"+record.motion launches phc_motion_record on a HIP device; the task's tensors are on {dev} (there is no CPU fallback)")
        self._launch = BACKEND != "torch"
        self.NB, self.D, self.E = int(task.num_bodies), int(task.num_dof), int(getattr(task, "num_extend_bodies", 0))
        from .abi import motion_record_width
        self.W = motion_record_width(self.NB, self.E, self.D, self.ref)
        self.is_robot = bool(getattr(task, "_is_robot", False))

    # ---- the block --------------------------------------------------------------------------------------------------------------------------------------
    def _open(self, cap, limit, one_segment, flag_name):
        t, N = self.task, int(self.task.num_envs)
        dev = t._root_states.device
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        self._state = dict(frames=torch.zeros((N, cap, self.W), dtype=torch.float32, device=dev), header=z(N, cap, 4), len=z(N), seg=z(N), closed=z(N), dropped=z(N),
                           limit=None if limit is None else torch.as_tensor(np.asarray(limit), dtype=torch.int32, device=dev).contiguous())
        self._cap, self._one_segment, self._flag_name, self._held = int(cap), bool(one_segment), flag_name, 0
        if not self._launch:
            m = t.model
            axis = np.zeros((self.NB, 3), dtype=np.float32)
            for j in range(self.NB):
                if int(m.joint_type[j]) == 2:
                    axis[j] = np.asarray(m.dof_axis[int(m.dof_start[j])], dtype=np.float32)
            self._tables = (torch.as_tensor(np.asarray(m.joint_type[:self.NB]), device=dev).long(), torch.as_tensor(np.asarray(m.dof_start[:self.NB]), device=dev).long(),
                            torch.from_numpy(axis).to(dev))

    def _sources(self):
        t = self.task
        src = dict(root_states=t._root_states, dof_state=t._dof_state, rigid_body_state=t._rigid_body_state, progress_buf=t.progress_buf,
                   flag=getattr(t, self._flag_name), motion_ids=t._sampled_motion_ids, motion_start_times=t._motion_start_times,
                   motion_start_times_offset=t._motion_start_times_offset)
        if self.ref:
            src["ref_body_pos"] = t.ref_body_pos
        return {k: v.detach().contiguous() for k, v in src.items()}

    def _append(self, seed=False):
        t, s = self.task, self._state
        src = self._sources()
        if self._launch:
            from . import _lib as L
            from .abi import motion_record_args_struct
            a = motion_record_args_struct(t.num_envs, self.NB, self.E, self.D, self._cap, t.dt, ref=self.ref, seed=seed, one_segment=self._one_segment,
                                          **src, **{k: v for k, v in s.items() if v is not None})
            L.check(L.load().phc_motion_record(t._model_struct, C.byref(a), torch.cuda.current_stream(s["frames"].device).cuda_stream), "phc_motion_record")
        else:
            record_rows(frame_rows(src, self._tables, self.E, t.dt, self.ref), src, s, self._cap, seed=seed, one_segment=self._one_segment)
        self._held += 1

    def _to_host(self):
        """ONE copy of the block (and its counters) to the host."""
        s = self._state
        return {k: s[k].cpu().numpy() for k in ("frames", "header", "len", "seg", "closed", "dropped")}

    # ---- sweep ------------------------------------------------------------------------------------------------------------------------------------------
    def begin_batch(self, num_steps, keys):
        """After the batch's `env.reset()`: `num_steps` [N] of the loaded clips (wrapped-around duplicates of the last batch included), their keys."""
        num_steps = np.maximum(np.asarray(num_steps, dtype=np.int64), 1)
        cap = int(num_steps.max())
        if self.max_frames is not None:
            cap = min(cap, self.max_frames)
        self._keys = [str(k) for k in keys]
        self._open(cap, num_steps.astype(np.int32), True, "_terminate_buf")
        self._append(seed=True)

    def record(self):
        """After an env step (sweep and play)."""
        self._append()
        if not self._one_segment and self._held >= self._cap:
            self.flush()

    def end_batch(self):
        if self._state is None:
            return
        h = self._to_host()
        data = getattr(self.task._motion_lib, "_motion_data_load", None) or {}
        for i, key in enumerate(self._keys):
            n = int(h["len"][i])
            if key in self._seen or n == 0:     # a wrapped-around duplicate of the last batch
                continue
            self._seen.add(key)
            self.clips.append(dict(key=key, env=i, frames=h["frames"][i, :n].copy(), header=h["header"][i, :n].copy(), failed=bool(h["header"][i, n - 1, 3]),
                                   source=data.get(key) if hasattr(data, "get") else None))
        self.dropped += int(h["dropped"].sum())
        self._state = None

    # ---- play -------------------------------------------------------------------------------------------------------------------------------------------
    def begin_play(self):
        """After the rollout's `env.reset()`: frame 0 of every env's first segment is the reset state."""
        self._open(self.max_frames or DEFAULT_CAP, None, False, "reset_buf")
        self._open_segments = {}   # (env, segment) -> index into self.clips
        self._append(seed=True)

    def flush(self):
        """Play: the block to the host, split by segment id, appended to the (env, segment) clips; the block starts over."""
        h, s = self._to_host(), self._state
        for i in range(len(h["len"])):
            n = int(h["len"][i])
            segs = h["header"][i, :n, 0]
            for sg in np.unique(segs):
                rows = np.flatnonzero(segs == sg)
                part = dict(frames=h["frames"][i, rows].copy(), header=h["header"][i, rows].copy())
                at = self._open_segments.get((i, int(sg)))
                if at is None:
                    self._open_segments[(i, int(sg))] = len(self.clips)
                    self.clips.append(dict(key=f"{i}_{int(sg)}", env=i, failed=False, source=None, **part))
                else:
                    c = self.clips[at]
                    c["frames"], c["header"] = np.concatenate([c["frames"], part["frames"]]), np.concatenate([c["header"], part["header"]])
        self.dropped += int(h["dropped"].sum())
        s["len"].zero_()
        s["dropped"].zero_()
        self._held = 0

    def close(self):
        """Play: the last flush -> {"record_dropped": frames refused, "record_clips": segments held}."""
        if self._state is not None and not self._one_segment:
            self.flush()
            self._state = None
        for c in self.clips:
            c["failed"] = bool(c["header"][-1, 3]) if len(c["header"]) else False
        return {"record_dropped": int(self.dropped), "record_clips": len(self.clips)}

    # ---- export -----------------------------------------------------------------------------------------------------------------------------------------
    def _split(self, frames):
        NB, E, D = self.NB, self.E, self.D
        o, out = 0, {}
        for name, w in (("root_pos", 3), ("body_quat", 4 * NB), ("pose_aa", 3 * (NB + E)), ("dof_pos", D), ("root_vel", 6), ("time", 1)) + ((("ref", 3 * NB),) if self.ref else ()):
            out[name] = frames[:, o:o + w]
            o += w
        assert o == self.W
        return out

    def library(self):
        """clip key -> clip, in the layout `MotionLibSMPL._clip_payload` (SMPL family) / `MotionLibReal._clip_payload` (robots) reads."""
        dt = float(self.task.dt)
        fps = 1.0 / dt
        fps = int(round(fps)) if abs(fps - round(fps)) < 1e-6 else fps
        lib = {}
        for c in self.clips:
            p = self._split(c["frames"])
            T = len(c["frames"])
            quat = p["body_quat"].reshape(T, self.NB, 4)
            if self.is_robot:
                clip = {"root_trans_offset": p["root_pos"].copy(), "pose_aa": p["pose_aa"].reshape(T, self.NB + self.E, 3).copy(), "dof": p["dof_pos"].copy(),
                        "root_rot": quat[:, 0].copy(), "fps": fps}
            else:
                clip = {"pose_quat_global": quat.copy(), "root_trans_offset": p["root_pos"].copy(), "pose_aa": p["pose_aa"].reshape(T, 3 * self.NB).copy(), "fps": fps}
            src = c.get("source")
            for k in ("beta", "gender"):
                if src is not None and k in src:
                    clip[k] = src[k]
            lib[c["key"]] = clip
        return lib

    def states(self):
        """clip key -> the fields of the reference's state dump (humanoid_im.py:407-465), with `fps = 1 / dt` and per-clip `failed`, `frames`, `motion_time`.
        A `skeleton_tree` dict needs poselib: the model's parent indices and local translations stand in its place (`skeleton_parents`,
        `skeleton_local_translation`)."""
        t = self.task
        m = t.model
        shapes = getattr(t, "humanoid_shapes", None)
        shapes = None if shapes is None else shapes.detach().cpu().numpy()
        fps = 1.0 / float(t.dt)
        out = {}
        for c in self.clips:
            p = self._split(c["frames"])
            T = len(c["frames"])
            root_quat = p["body_quat"].reshape(T, self.NB, 4)[:, 0]
            d = {"skeleton_parents": np.asarray(m.parent[:self.NB]).copy(), "skeleton_local_translation": np.asarray(m.local_translation[:self.NB]).copy(),
                 "trans": p["root_pos"].copy(), "root_states_seg": np.concatenate([p["root_pos"], root_quat, p["root_vel"]], axis=1), "dof_pos": p["dof_pos"].copy(),
                 "fps": fps, "betas": None if shapes is None else shapes[c["env"]].copy(), "failed": bool(c["failed"]), "frames": T, "motion_time": p["time"][:, 0].copy()}
            if not self.is_robot:
                d["body_quat"] = np.concatenate([root_quat[:, None], exp_map_to_quat(p["dof_pos"].reshape(T, -1, 3))], axis=1)
            if self.ref:
                d["ref_body_pos_full"] = p["ref"].reshape(T, self.NB, 3).copy()
            out[c["key"]] = d
        return out

    def export(self, path, log=print):
        """joblib dict clip key -> clip at `path`, the state dump next to it as `<stem>_states.pkl`; -> (path, states path)."""
        import joblib
        path = str(path)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        stem, ext = os.path.splitext(path)
        states_path = stem + "_states" + (ext or ".pkl")
        joblib.dump(self.library(), path)
        joblib.dump(self.states(), states_path)
        if log is not None:
            log(f"recorded {len(self.clips)} clips ({sum(len(c['frames']) for c in self.clips)} frames, {self.dropped} dropped) -> {path}, {states_path}")
        return path, states_path
