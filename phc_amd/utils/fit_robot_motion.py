"""Retargeting fit: SMPL joint trajectories -> robot (H1 / G1) motion clips (f-4; reference scripts/data_process/fit_smpl_motion.py:56-186).

The reference's `process_motion` has two halves:
  1. AMASS pose + the robot-fitted SMPL shape -> SMPL joint positions (`SMPL_Parser.get_joints_verts`, :78-99).  That half needs the SMPL
     model files and smpl_sim; neither ships with the reference nor exists on this machine, so it stays OUTSIDE: this module takes the
     joint trajectories `smpl_joints [T, 24, 3]` (SMPL_BONE_ORDER_NAMES order, already scaled / grounded as :86-89 does) as its input;
  2. the fit itself (:101-150): per frame the robot's joint angles, root rotation (initialised with the SMPL root's heading, :97-98) and one
     global root offset are optimised with Adam (lr 0.02, 500 iterations) so that the robot's matched bodies (`robot.joint_matches`, incl.
     the extended hand / head bodies) follow the matched SMPL joints: loss = mean |p_robot - p_smpl| + 0.01 mean(dof^2); after every step
     the angles are clamped to the joint ranges and smoothed along time by a 5-tap gaussian (sigma 0.75); finally the clip is moved to the
     ground by the lowest point of the FIRST frame (:164-170: mesh vertices there; here the links' convex-hull support points stand in
     for the meshes, as in MotionLibReal.fix_trans_height).  That half is what this module runs -- differentiable forward kinematics of
     `Humanoid_Batch.fk_batch` (torch_humanoid_batch.py:163-257) in torch, on the CPU or on the device -- and its output has the schema the
     reference dumps (:172-179) and MotionLibReal reads.

`gaussian_filter_1d_batch` comes from smpl_sim (not vendored: restated as a replicate-padded 1-d convolution with the normalised kernel).

    python -m phc_amd.utils.fit_robot_motion --robot unitree_h1 --joints joints.npz --out h1_clips.pkl
where joints.npz holds, per clip key, `<key>/smpl_joints [T,24,3]`, `<key>/root_trans [T,3]` and `<key>/root_aa [T,3]` (SMPL root axis-angle).
"""
import math

import numpy as np
import torch

from .. import _lib as L

SMPL_BONE_ORDER_NAMES = ["Pelvis", "L_Hip", "R_Hip", "Torso", "L_Knee", "R_Knee", "Spine", "L_Ankle", "R_Ankle", "Chest", "L_Toe", "R_Toe",
                         "Neck", "L_Thorax", "R_Thorax", "Head", "L_Shoulder", "R_Shoulder", "L_Elbow", "R_Elbow", "L_Wrist", "R_Wrist", "L_Hand",
                         "R_Hand"]


def _aa_to_mat(aa):
    """Rodrigues, batched [..., 3] -> [..., 3, 3]: R = I + A [aa]x + B [aa]x^2 with A = sin(t) / t, B = (1 - cos t) / t^2 and their series near
    t = 0 -- the fit starts from all-zero joint angles, where a formula through the normalised axis has a vanishing gradient
    (pytorch3d.axis_angle_to_matrix, which the reference uses, is smooth there too)."""
    t2 = (aa * aa).sum(-1, keepdim=True)
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)
    t = torch.sqrt(t2s)
    A = torch.where(small, 1.0 - t2 / 6.0, torch.sin(t) / t)
    B = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(t)) / t2s)
    x, y, z = aa[..., 0], aa[..., 1], aa[..., 2]
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], dim=-1).reshape(aa.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=aa.dtype, device=aa.device).expand(K.shape)
    return eye + A[..., None] * K + B[..., None] * (K @ K)


def _quat_wxyz_to_mat(q):
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(q.shape[:-1] + (3, 3))


class RobotFK:
    """Differentiable `Humanoid_Batch.forward_kinematics_batch` (torch_humanoid_batch.py:224-257) for the NB simulated + E extended bodies:
    world position = parent rotation * offset + parent position; world rotation = parent * rest rotation * joint rotation."""

    def __init__(self, model, extend_config, device="cpu", dtype=torch.float32):
        names = list(model.body_names)
        self.names = names + [e["joint_name"] for e in extend_config]
        self.parents = list(np.asarray(model.parent)) + [names.index(e["parent_name"]) for e in extend_config]
        t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype, device=device)
        self.offsets = torch.cat([t(model.local_translation), t([e["pos"] for e in extend_config]).reshape(-1, 3)], dim=0)
        self.rest = _quat_wxyz_to_mat(torch.cat([t(model.local_rotation), t([e["rot"] for e in extend_config]).reshape(-1, 4)], dim=0))
        self.num_bodies, self.num_ext = len(names), len(extend_config)
        axis = np.zeros((model.num_bodies - 1, 3))
        for i in range(1, model.num_bodies):
            axis[i - 1] = model.dof_axis[model.dof_start[i]]
        self.dof_axis = t(axis)                                      # [ND, 3] (one revolute joint per body)
        lo, hi = model.dof_limits()
        self.joints_range = torch.stack([t(lo), t(hi)], dim=-1)      # [ND, 2]

    def __call__(self, pose_aa, root_trans):
        """pose_aa [T, NB+E, 3] (root axis-angle, axis * angle per joint, zeros for the extended bodies), root_trans [T, 3]
        -> world positions [T, NB+E, 3], world rotation matrices [T, NB+E, 3, 3]."""
        pose_aa, root_trans = pose_aa.to(self.offsets), root_trans.to(self.offsets)
        R = _aa_to_mat(pose_aa)
        pos, rot = [None] * len(self.parents), [None] * len(self.parents)
        for i, p in enumerate(self.parents):
            if p < 0:
                pos[i], rot[i] = root_trans, R[:, 0]
            else:
                pos[i] = (rot[p] @ self.offsets[i]) + pos[p]
                rot[i] = rot[p] @ (self.rest[i] @ R[:, i])
        return torch.stack(pos, dim=1), torch.stack(rot, dim=1)


def gaussian_filter_time(x, kernel_size=5, sigma=0.75):
    """[T, D] smoothed along T (fit_smpl_motion.py:103-105,134: smpl_sim's gaussian_filter_1d_batch; restated, see module docstring)."""
    half = kernel_size // 2
    k = torch.exp(-0.5 * (torch.arange(-half, half + 1, dtype=x.dtype, device=x.device) / sigma) ** 2)
    k = (k / k.sum()).view(1, 1, -1)
    xt = x.t().unsqueeze(1)                                          # [D, 1, T]
    xt = torch.nn.functional.pad(xt, (half, half), mode="replicate")
    return torch.nn.functional.conv1d(xt, k).squeeze(1).t()


def heading_rotvec(root_aa):
    """:97-98: the SMPL root rotation with the y-up base rotation removed, reduced to its heading (rotation about z), as a rotation vector."""
    from scipy.spatial.transform import Rotation as sRot
    q = (sRot.from_rotvec(np.asarray(root_aa, dtype=np.float64)) * sRot.from_quat([0.5, 0.5, 0.5, 0.5]).inv())
    d = q.apply(np.array([1.0, 0.0, 0.0]))
    yaw = np.arctan2(d[:, 1], d[:, 0])                               # torch_utils.calc_heading
    out = np.zeros((len(yaw), 3))
    out[:, 2] = yaw
    return out


class _FitProblem:
    """What one clip's fit works on (fit_smpl_motion.py:91-98): the FK, the matched bodies and their targets, the root trajectory and the start values."""

    def __init__(self, model, robot_cfg, smpl_joints, root_trans, root_aa=None, device="cpu", dtype=torch.float32):
        npdt = np.float32 if dtype == torch.float32 else np.float64
        self.model, self.device, self.dtype = model, device, dtype
        self.ext = list(robot_cfg.get("extend_config", []))
        self.fk = RobotFK(model, self.ext, device=device, dtype=dtype)
        self.pick_r = [self.fk.names.index(m[0]) for m in robot_cfg["joint_matches"]]
        self.pick_s = [SMPL_BONE_ORDER_NAMES.index(m[1]) for m in robot_cfg["joint_matches"]]
        self.t = lambda a: torch.as_tensor(np.asarray(a, dtype=npdt), device=device)
        self.joints = self.t(smpl_joints)
        self.T = self.joints.shape[0]
        trans = self.t(root_trans)
        self.root_trans_offset = trans + (self.joints[:, 0] - trans)       # :91-92
        self.gt_root = self.t(heading_rotvec(root_aa) if root_aa is not None else np.zeros((self.T, 3)))
        self.nd, self.ne = model.num_bodies - 1, len(self.ext)
        self.zeros_ext = torch.zeros((self.T, self.ne, 3), device=device, dtype=dtype)
        self.target = self.joints[:, self.pick_s]

    def pose(self, dof, root_rot):
        return torch.cat([root_rot[:, None], self.fk.dof_axis * dof, self.zeros_ext], dim=1)


def _fit_loop(pb, iterations, lr, log=None):
    """The optimisation (:101-150) -> dof [T, ND, 1], root_rot [T, 3], root_off [1, 3] (leaf tensors) and the last evaluated loss."""
    fk, device, dtype = pb.fk, pb.device, pb.dtype
    dof = torch.zeros((pb.T, pb.nd, 1), device=device, dtype=dtype, requires_grad=True)
    root_rot = pb.gt_root.clone().requires_grad_(True)
    root_off = torch.zeros((1, 3), device=device, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([dof, root_rot, root_off], lr=lr)
    lo, hi = fk.joints_range[:, 0, None], fk.joints_range[:, 1, None]
    loss_val = float("nan")
    for it in range(iterations):
        pos, _ = fk(pb.pose(dof, root_rot), pb.root_trans_offset + root_off)
        loss = (pos[:, pb.pick_r] - pb.target).norm(dim=-1).mean() + 0.01 * torch.mean(torch.square(dof))   # :116-121
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            dof.clamp_(lo, hi)                                                                           # :131
            dof.copy_(gaussian_filter_time(dof[..., 0])[..., None])                                       # :134
        loss_val = float(loss.detach())
        if log is not None and (it % 50 == 0 or it == iterations - 1):
            log(f"iter {it}: {loss_val * 1000:.3f}")
    return dof, root_rot, root_off, loss_val


def _fit_dump(pb, dof, root_rot, root_off, loss_val, fps):
    """The tail both backends share: final clamp, grounding by the first frame's support points, the keypoint error, the reference's dump dict (:164-179)."""
    fk, model, device, t = pb.fk, pb.model, pb.device, pb.t
    lo, hi = fk.joints_range[:, 0, None], fk.joints_range[:, 1, None]
    with torch.no_grad():
        dof.clamp_(lo, hi)
        pose_aa = pb.pose(dof, root_rot)
        root_dump = (pb.root_trans_offset + root_off).clone()
        # move to the ground by the lowest point of the first frame (:164-170; support points instead of mesh vertices)
        pos0, rot0 = fk(pose_aa[:1], root_dump[:1])
        cb = torch.as_tensor(np.asarray(model.contact_body), device=device, dtype=torch.long)
        cp = t(model.contact_pos)
        z = pos0[0, cb, 2] + (rot0[0, cb][:, 2, :] * cp).sum(-1) - t(model.contact_radius)
        h = float(z.min())
        root_dump[:, 2] -= h
        joints_dump = pb.joints.clone()
        joints_dump[..., 2] -= h
        pos, _ = fk(pose_aa, root_dump)
        err = (pos[:, pb.pick_r] - joints_dump[:, pb.pick_s]).norm(dim=-1).mean()
    from scipy.spatial.transform import Rotation as sRot
    return {"root_trans_offset": root_dump.cpu().numpy(), "pose_aa": pose_aa.cpu().numpy(), "dof": dof[..., 0].detach().cpu().numpy(),
            "root_rot": sRot.from_rotvec(root_rot.detach().cpu().numpy()).as_quat(), "smpl_joints": joints_dump.cpu().numpy(), "fps": fps,
            "fit_loss": loss_val, "fit_keypoint_error": float(err)}


def fit_clip_state(model, robot_cfg, smpl_joints, root_trans, root_aa=None, iterations=500, lr=0.02, device="cpu", dtype=torch.float32):
    """The optimised parameters of `fit_clip` before its tail: dof [T, ND], root rotation vectors [T, 3], root_off [3] as numpy arrays, and the loss."""
    pb = _FitProblem(model, robot_cfg, smpl_joints, root_trans, root_aa, device, dtype)
    dof, root_rot, root_off, loss_val = _fit_loop(pb, iterations, lr)
    return dof[..., 0].detach().cpu().numpy(), root_rot.detach().cpu().numpy(), root_off[0].detach().cpu().numpy(), loss_val


def fit_clip(model, robot_cfg, smpl_joints, root_trans, root_aa=None, iterations=500, lr=0.02, device="cpu", fps=30, log=None, dtype=torch.float32):
    """One clip.  smpl_joints [T, 24, 3], root_trans [T, 3] (the SMPL root position the joints were computed with), root_aa [T, 3] SMPL root
    axis-angle (None: heading 0).  Returns the reference's dump dict (fit_smpl_motion.py:172-179).  `dtype`: the precision of the whole fit
    (torch.float64: the oracle of the device fit's tests)."""
    pb = _FitProblem(model, robot_cfg, smpl_joints, root_trans, root_aa, device, dtype)
    dof, root_rot, root_off, loss_val = _fit_loop(pb, iterations, lr, log)
    return _fit_dump(pb, dof, root_rot, root_off, loss_val, fps)


FIT_LOG_SEGMENT = 50   # iterations between two reads of the loss when `fit_clips(backend="device")` is given a `log`
FIT_TIMING = None      # a list: `fit_clips(backend="device")` appends (frames, clips, iterations, milliseconds between two events around phc_fit_iterate) per chunk


def fit_model_arrays(model, robot_cfg):
    """The model half of phc_fit_args_t as numpy arrays (fp32 values are the ones `RobotFK` computes with in fp32): parents, offsets, rest [NB + E, 9], axis,
    range, match_body, match_slot (entry m reads column m of the targets) and subtree (bit m of word j: matched entry m hangs below, or is, body j)."""
    ext = list(robot_cfg.get("extend_config", []))
    fk = RobotFK(model, ext)
    nb = fk.num_bodies
    parents = np.asarray(fk.parents, dtype=np.int32)
    match_body = np.asarray([fk.names.index(m[0]) for m in robot_cfg["joint_matches"]], dtype=np.int32)
    subtree = np.zeros(nb, dtype=np.uint32)
    for m, b in enumerate(match_body[:32]):
        k = int(b)
        while k >= 0:
            if k < nb:
                subtree[k] |= np.uint32(1 << m)
            k = int(parents[k])
    return dict(parents=parents, offsets=fk.offsets.numpy().astype(np.float32), rest=fk.rest.reshape(-1, 9).numpy().astype(np.float32),
                axis=fk.dof_axis.numpy().astype(np.float32), range=fk.joints_range.numpy().astype(np.float32), match_body=match_body,
                match_slot=np.arange(len(match_body), dtype=np.int32), subtree=subtree)


def _fit_chunk_device(lib, marr, pbs, iterations, lr, device, log):
    """One chunk of clips on the device -> per clip (dof [T, ND], root_rot [T, 3], root_off [3], loss)."""
    from .. import abi
    nb, ne, M = pbs[0].fk.num_bodies, pbs[0].ne, len(pbs[0].pick_r)
    nd, C = nb - 1, len(pbs)
    start = np.concatenate([[0], np.cumsum([pb.T for pb in pbs])]).astype(np.int64)
    F_ = int(start[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    dev = {k: up(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in marr.items()}
    dev["clip_start"] = up(start)
    dev["target"] = torch.cat([pb.target for pb in pbs]).contiguous().to(device)
    dev["root_trans_offset"] = torch.cat([pb.root_trans_offset for pb in pbs]).contiguous().to(device)
    dev["root_rot"] = torch.cat([pb.gt_root for pb in pbs]).contiguous().to(device)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)
    dev.update(dof=z(F_, nd), dof_m=z(F_, nd), dof_v=z(F_, nd), root_rot_m=z(F_, 3), root_rot_v=z(F_, 3), root_off=z(C, 3), root_off_m=z(C, 3),
               root_off_v=z(C, 3), step=z(C, dtype=torch.int32), loss=z(C))
    sb = int(lib.phc_fit_scratch_bytes(F_, C, nb + ne))
    if sb < 0:
        raise RuntimeError(f"phc_fit_scratch_bytes refused {F_} frames, {C} clips, {nb + ne} bodies")
    scratch = torch.empty(sb, dtype=torch.uint8, device=device)
    args = abi.fit_args_struct(nb, ne, M, C, F_, lr, scratch, sb, clip_start_host=start, **dev)
    stream = torch.cuda.current_stream(device).cuda_stream
    segments = [iterations] if log is None else [min(FIT_LOG_SEGMENT, iterations - i) for i in range(0, iterations, FIT_LOG_SEGMENT)] or [0]
    done = 0
    timing = None if FIT_TIMING is None else [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    if timing:
        timing[0].record(torch.cuda.current_stream(device))
    for n in segments:   # (segmenting does not change a bit of the result)
        L.check(lib.phc_fit_iterate(args, int(n), stream), "phc_fit_iterate")
        done += n
        if log is not None and n > 0:
            log(f"iter {done - 1}: " + " ".join(f"{v * 1000:.3f}" for v in dev["loss"].cpu().tolist()))
    if timing:
        timing[1].record(torch.cuda.current_stream(device))
        timing[1].synchronize()
        FIT_TIMING.append((F_, C, int(iterations), timing[0].elapsed_time(timing[1])))
    dof, root_rot, root_off, loss = (dev[k].cpu() for k in ("dof", "root_rot", "root_off", "loss"))
    return [(dof[start[c]:start[c + 1]].clone(), root_rot[start[c]:start[c + 1]].clone(), root_off[c].clone(),
             float(loss[c]) if iterations > 0 else float("nan")) for c in range(C)]


def fit_clips(model, robot_cfg, clips, iterations=500, lr=0.02, backend="host", device="cpu", chunk_frames=262144, fps=30, log=None):
    """A library.  `clips`: key -> (smpl_joints [T, 24, 3], root_trans [T, 3], root_aa [T, 3] | None); returns key -> the dump dict of `fit_clip`.
    backend "host": `fit_clip` per clip on `device` (torch autograd).  backend "device": all clips of a chunk (whole clips, at most `chunk_frames` frames)
    at once in phc_fit_iterate on the HIP device `device` -- the same iteration in fp32 with an analytic gradient -- and the shared tail on the host;
    `log(str)` then receives the clips' losses every FIT_LOG_SEGMENT iterations.  There is no fallback from one backend to the other."""
    if backend not in ("host", "device"):
        raise ValueError(f"fit_clips: unknown backend {backend!r} (host | device)")
    keys = list(clips)
    for k in keys:
        if np.asarray(clips[k][0]).shape[0] < 1:
            raise ValueError(f"fit_clips: clip {k!r} has no frames")
    if backend == "host":
        return {k: fit_clip(model, robot_cfg, *clips[k], iterations=iterations, lr=lr, device=device, fps=fps,
                            log=None if log is None else (lambda s, k=k: log(f"{k} {s}"))) for k in keys}
    from ..motion_lib import _clip_chunks
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available() or torch.version.hip is None:
        raise RuntimeError(f"fit_clips: backend=device runs on a HIP device only (no fallback), not on {dev}; use backend=host")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    lib = L.load()
    if not hasattr(lib, "phc_fit_iterate"):
        raise RuntimeError("this build of libphc_amd.so has no phc_fit_iterate; use backend=host")
    if len(robot_cfg["joint_matches"]) > L.FIT_MAX_MATCHED:
        raise RuntimeError(f"fit_clips: backend=device takes at most {L.FIT_MAX_MATCHED} matched bodies; use backend=host")
    marr = fit_model_arrays(model, robot_cfg)
    pbs = [_FitProblem(model, robot_cfg, *clips[k]) for k in keys]
    out = {}
    for u0, u1 in _clip_chunks([pb.T for pb in pbs], int(chunk_frames)):
        states = _fit_chunk_device(lib, marr, pbs[u0:u1], int(iterations), lr, dev, None if log is None else (lambda s, u0=u0, u1=u1: log(f"clips {u0}..{u1 - 1} {s}")))
        for k, pb, (dof, root_rot, root_off, loss) in zip(keys[u0:u1], pbs[u0:u1], states):
            out[k] = _fit_dump(pb, dof[..., None], root_rot, root_off[None], loss, fps)
    return out


def main(argv=None):
    import argparse
    import joblib
    from ..cfg_defaults import GROUPS
    from ..model import load_model
    from .. import robots
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--robot", default="unitree_h1", choices=["unitree_h1", "unitree_h1_nohead", "unitree_g1"])
    ap.add_argument("--joints", required=True, help="npz: <key>/smpl_joints, <key>/root_trans, <key>/root_aa")
    ap.add_argument("--out", required=True)
    ap.add_argument("--iterations", type=int, default=500)
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--backend", default="host", choices=["host", "device"], help="host: torch autograd per clip; device: phc_fit_iterate over chunks of clips")
    ap.add_argument("--chunk-frames", type=int, default=262144, help="backend=device: frames fitted at once")
    a = ap.parse_args(argv)
    rc = GROUPS["robot"][a.robot]
    model = load_model(f"{rc['humanoid_type']}_humanoid")
    robots.apply_robot_gains(model, robots.ROBOTS[rc["humanoid_type"]])
    data = np.load(a.joints)
    keys = sorted({k.split("/")[0] for k in data.files})
    clips = {k: (data[f"{k}/smpl_joints"], data[f"{k}/root_trans"], data[f"{k}/root_aa"] if f"{k}/root_aa" in data.files else None) for k in keys}
    out = fit_clips(model, rc, clips, a.iterations, backend=a.backend, device=a.device, chunk_frames=a.chunk_frames, log=lambda s: print(s, flush=True))
    joblib.dump(out, a.out)
    print(f"wrote {len(out)} clips to {a.out}")


if __name__ == "__main__":
    main()
