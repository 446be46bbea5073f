"""Keypoints to clips: the spherical-joint fit of the SMPL humanoid family.  Joint POSITIONS `[T, K, 3]` (a pose estimator, a text-to-motion model, a marker
solver, or the body positions of any clip) -> a clip library `MotionLibSMPL` loads (joint ROTATIONS).  The machinery is the retargeting fit's
(`fit_robot_motion`) with one spherical joint per body instead of one revolute joint.

The iteration, stated once (csrc/phc_fit_sph.h restates it in fp32 with an analytic gradient).  Per frame the parameters are `rot [NB, 3]` rotation vectors:
row 0 is the root's world rotation, row b >= 1 body b's rotation in its parent's frame; per clip `root_off [3]`:

    R_b = R_parent rest_b exp(rot_b)        p_b = p_parent + R_parent offset_b        p_0 = keypoint_root + root_off
    loss = mean_{t, m} |p_{match_body[m]} - g_{t, match_slot[m]}| + 0.01 mean(rot[:, 1:]^2)

Adam (lr 0.02) on rot and root_off; then every component of rot[:, 1:] is clamped to `model.dof_limits()` (the SMPL humanoid's DoF positions are exactly
these exp-map components) and smoothed along time by the 5-tap gaussian (sigma 0.75, replicate padding).  The root rotation is neither clamped nor filtered.
The root rotation starts at the per-frame Kabsch alignment of the root's matched children (started at zero the fit stays centimetres off); the joint
vectors and root_off start at 0.

What the keypoints do not determine: the twist about a bone whose far end is the only keypoint below it (the regulariser holds it near 0), and the rotation
of a body with no keypoint strictly below it (leaves: toes, hands, head; they stay at rest).

    python -m phc_amd.utils.fit_keypoints --joints kp.npz --out clips.pkl [--model smpl_humanoid] [--fps 30] [--order smpl] [--up y] [--bone-lengths model]
                                          [--iterations 500] [--backend device --device cuda:0] [--chunk-frames N]
where kp.npz holds, per clip key, `<key>/joints [T, K, 3]` and optionally `<key>/fps`.
"""
import numpy as np
import torch

from .. import _lib as L
from .fit_robot_motion import FIT_LOG_SEGMENT, _aa_to_mat, _quat_wxyz_to_mat, gaussian_filter_time

FIT_SPH_MAX_BODIES = 32   # FIT_SPH_MAX_BODIES (csrc/phc_fit_sph.h)
FIT_TIMING = None         # a list: backend="device" appends (frames, clips, iterations, milliseconds between two events around phc_fit_sph_iterate) per chunk
UNMATCHED_22 = ("L_Hand", "R_Hand")


def check_model(model):
    """The fit's model: all joints spherical, at most FIT_SPH_MAX_BODIES bodies."""
    if not getattr(model, "all_spherical", False):
        raise ValueError("fit_keypoint_clips fits all-spherical models (the SMPL family); a model with revolute joints is fitted by "
                         "phc_amd.utils.fit_robot_motion.fit_clips")
    if model.num_bodies > FIT_SPH_MAX_BODIES:
        raise ValueError(f"fit_keypoint_clips takes at most {FIT_SPH_MAX_BODIES} bodies, the model has {model.num_bodies}")


def resolve_bodies(model, K, bodies=None):
    """The model body index of each keypoint column.  Default: the model's own order (K = NB), or the same without the hands (K = NB - 2)."""
    names = list(model.body_names)
    if bodies is None:
        if K == len(names):
            bodies = names
        elif K == len(names) - len(UNMATCHED_22) and all(n in names for n in UNMATCHED_22):
            bodies = [n for n in names if n not in UNMATCHED_22]
        else:
            raise ValueError(f"{K} keypoint columns match neither the model's {len(names)} bodies nor those without {UNMATCHED_22}: name them with `bodies`")
    bodies = list(bodies)
    if len(bodies) != K:
        raise ValueError(f"the keypoints have {K} columns, `bodies` names {len(bodies)}")
    for n in bodies:
        if n not in names:
            raise ValueError(f"unknown body {n!r} (the model has {names})")
    if len(set(bodies)) != len(bodies):
        raise ValueError("`bodies` names a body twice")
    idx = [names.index(n) for n in bodies]
    if 0 not in idx:
        raise ValueError(f"the root body {names[0]!r} must be among the keypoints (the root position is read from it)")
    return idx


def sph_model_arrays(model, match_body, match_slot=None):
    """The model half of phc_fit_args_t for phc_fit_sph_iterate as numpy arrays: parents, offsets, rest [NB, 9], range [3 (NB - 1), 2], match_body,
    match_slot (entry m reads column match_slot[m] of the targets) and subtree (bit m of word j: matched entry m hangs below, or is, body j).  No `axis`."""
    nb = model.num_bodies
    parents = np.asarray(model.parent, dtype=np.int32)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=torch.float32)
    rest = _quat_wxyz_to_mat(t(model.local_rotation)).reshape(-1, 9).numpy()
    lo, hi = model.dof_limits()
    match_body = np.asarray(match_body, dtype=np.int32)
    return dict(parents=parents, offsets=np.asarray(model.local_translation, dtype=np.float32), rest=rest.astype(np.float32),
                range=np.stack([lo, hi], axis=-1).astype(np.float32).reshape(3 * (nb - 1), 2), match_body=match_body,
                match_slot=np.arange(len(match_body), dtype=np.int32) if match_slot is None else np.asarray(match_slot, dtype=np.int32),
                subtree=subtree_words(parents, match_body))


def subtree_words(parents, match_body):
    sub = np.zeros(len(parents), dtype=np.uint32)
    for m, b in enumerate(np.asarray(match_body)[:32]):
        k = int(b)
        while k >= 0:
            sub[k] |= np.uint32(1 << m)
            k = int(parents[k])
    return sub


def sph_fk(marr, root_rot, rot, root_pos):
    """The statement's forward kinematics in torch (any float dtype; differentiable): root_rot [T, 3], rot [T, NB - 1, 3], root_pos [T, 3]
    -> world positions [T, NB, 3], world rotation matrices [T, NB, 3, 3]."""
    t = lambda a: a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a), dtype=root_rot.dtype, device=root_rot.device)
    offsets, rest = t(marr["offsets"]), t(marr["rest"]).reshape(-1, 3, 3)
    Rj = _aa_to_mat(rot)
    nb = len(marr["parents"])
    pos, R = [None] * nb, [None] * nb
    for i, p in enumerate(marr["parents"]):
        if p < 0:
            pos[i], R[i] = root_pos, _aa_to_mat(root_rot)
        else:
            pos[i] = R[p] @ offsets[i] + pos[p]
            R[i] = R[p] @ (rest[i] @ Rj[:, i - 1])
    return torch.stack(pos, dim=1), torch.stack(R, dim=1)


def prepare_keypoints(model, joints, idx, order="mujoco", up="z", bone_lengths="keep"):
    """The processed input [T, K, 3] fp64: SMPL joint order -> the model's (order="smpl"), y-up -> z-up (up="y"), both as `phc_amd.stream` does them; matched
    bones rescaled to the model's lengths, parents first (bone_lengths="model")."""
    from .. import stream
    g = np.asarray(joints, dtype=np.float64)
    if g.ndim != 3 or g.shape[2] != 3:
        raise ValueError(f"keypoints are [T, K, 3], not {g.shape}")
    if order not in ("mujoco", "smpl"):
        raise ValueError(f"order must be mujoco or smpl, not {order!r}")
    if up not in ("z", "y"):
        raise ValueError(f"up must be z or y, not {up!r}")
    if bone_lengths not in ("keep", "model"):
        raise ValueError(f"bone_lengths must be keep or model, not {bone_lengths!r}")
    if order == "smpl":
        if g.shape[1] != len(stream.SMPL_2_MUJOCO) or model.num_bodies != len(stream.SMPL_2_MUJOCO):
            raise ValueError("order=smpl: the SMPL joint order exists for 24 keypoints of the 24-body SMPL family only")
        g = g[:, list(stream.SMPL_2_MUJOCO)]
    if up == "y":
        g = g @ np.asarray(stream.TO_ISAAC_MAT, dtype=np.float64).T
    if bone_lengths == "model":
        col = {b: k for k, b in enumerate(idx)}
        out = g.copy()
        for b in sorted(idx):
            if b == 0:
                continue
            p = int(model.parent[b])
            if p not in col:
                raise ValueError(f"bone_lengths=model: the parent of body {model.body_names[b]!r} ({model.body_names[p]!r}) is not among the keypoints")
            d = g[:, col[b]] - g[:, col[p]]
            n = np.linalg.norm(d, axis=-1, keepdims=True)
            out[:, col[b]] = out[:, col[p]] + d / np.where(n > 0, n, 1.0) * float(np.linalg.norm(model.local_translation[b]))
        g = out
    return np.ascontiguousarray(g)


def kabsch_root(model, g, idx):
    """Per frame the rotation vector of the rotation that best aligns the model's rest offsets of the root's matched children to g_child - g_root."""
    from scipy.spatial.transform import Rotation as sRot
    col = {b: k for k, b in enumerate(idx)}
    kids = [b for b in sorted(idx) if b != 0 and int(model.parent[b]) == 0]
    if len(kids) < 2:
        raise ValueError(f"the root's start rotation needs at least two keypoints on children of {model.body_names[0]!r}, there are {len(kids)}")
    A = np.asarray(model.local_translation, dtype=np.float64)[kids]                  # [n, 3]
    B = g[:, [col[b] for b in kids]] - g[:, col[0]][:, None]                         # [T, n, 3]
    H = np.einsum("ni,tnj->tij", A, B)
    U, _, Vt = np.linalg.svd(H)
    V, Ut = np.swapaxes(Vt, -1, -2), np.swapaxes(U, -1, -2)
    D = np.tile(np.eye(3), (len(g), 1, 1))
    D[:, 2, 2] = np.sign(np.linalg.det(V @ Ut))
    return sRot.from_matrix(V @ D @ Ut).as_rotvec()


class _SphProblem:
    """One clip: its processed keypoints, its targets in entry order, the root trajectory and the start values (numpy fp64)."""

    def __init__(self, model, joints, idx, order, up, bone_lengths):
        self.g = prepare_keypoints(model, joints, idx, order, up, bone_lengths)
        if self.g.shape[1] != len(idx):
            raise ValueError(f"the keypoints have {self.g.shape[1]} columns, `bodies` names {len(idx)}")
        self.T = self.g.shape[0]
        self.root_trans = np.ascontiguousarray(self.g[:, idx.index(0)])
        self.root_rot0 = kabsch_root(model, self.g, idx)


def _fit_host(marr, pb, iterations, lr, device, dtype, log):
    """torch autograd + torch.optim.Adam on the module's statement -> (rot [T, ND], root_rot [T, 3], root_off [3], last evaluated loss)."""
    nb, M = len(marr["parents"]), len(marr["match_body"])
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype, device=device)
    g, rto = t(pb.g), t(pb.root_trans)
    rot = torch.zeros((pb.T, nb - 1, 3), dtype=dtype, device=device, requires_grad=True)
    root_rot = t(pb.root_rot0).requires_grad_(True)
    root_off = torch.zeros((1, 3), dtype=dtype, device=device, requires_grad=True)
    opt = torch.optim.Adam([rot, root_rot, root_off], lr=lr)
    lo, hi = t(marr["range"][:, 0]), t(marr["range"][:, 1])
    mb, ms = list(marr["match_body"]), list(marr["match_slot"])
    marr = dict(marr, offsets=t(marr["offsets"]), rest=t(marr["rest"]))      # (on the fit's device once, not per iteration)
    loss_val = float("nan")
    for it in range(iterations):
        pos, _ = sph_fk(marr, root_rot, rot, rto + root_off)
        loss = (pos[:, mb] - g[:, ms]).norm(dim=-1).mean() + (0.01 * torch.mean(torch.square(rot)) if nb > 1 else 0.0)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            if nb > 1:
                flat = rot.view(pb.T, -1)
                flat.clamp_(lo, hi)
                flat.copy_(gaussian_filter_time(flat))
        loss_val = float(loss.detach())
        if log is not None and (it % FIT_LOG_SEGMENT == 0 or it == iterations - 1):
            log(f"iter {it}: {loss_val * 1000:.3f}")
    return rot.detach().reshape(pb.T, -1).cpu().numpy(), root_rot.detach().cpu().numpy(), root_off[0].detach().cpu().numpy(), loss_val


def fit_keypoint_state(model, joints, *, bodies=None, iterations=500, lr=0.02, device="cpu", dtype=torch.float32, order="mujoco", up="z", bone_lengths="keep"):
    """The optimised parameters of one clip's host fit before its tail: rot [T, 3 (NB - 1)], root rotation vectors [T, 3], root_off [3], and the loss."""
    check_model(model)
    idx = resolve_bodies(model, np.asarray(joints).shape[1], bodies)
    return _fit_host(sph_model_arrays(model, idx), _SphProblem(model, joints, idx, order, up, bone_lengths), int(iterations), lr, device, dtype, None)


def _dump(marr, pb, rot, root_rot, root_off, loss_val, fps):
    """The tail both backends share: the `MotionLibSMPL` clip layout `MotionRecorder.library()` writes, plus the processed keypoints and the fit's figures."""
    from scipy.spatial.transform import Rotation as sRot
    nb = len(marr["parents"])
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    root_pos = pb.root_trans + np.asarray(root_off, dtype=np.float64)
    pos, R = sph_fk(marr, t(root_rot), t(rot).reshape(pb.T, nb - 1, 3), t(root_pos))
    err = (pos[:, list(marr["match_body"])] - t(pb.g)[:, list(marr["match_slot"])]).norm(dim=-1).mean()
    quat = sRot.from_matrix(R.numpy().reshape(-1, 3, 3)).as_quat().reshape(pb.T, nb, 4)       # xyzw
    pose_aa = np.concatenate([np.asarray(root_rot, dtype=np.float64), np.asarray(rot, dtype=np.float64)], axis=1)
    return {"pose_quat_global": quat.astype(np.float32), "root_trans_offset": root_pos.astype(np.float32), "pose_aa": pose_aa.astype(np.float32), "fps": fps,
            "keypoints": pb.g.astype(np.float32), "fit_loss": loss_val, "fit_keypoint_error": float(err)}


def _fit_chunk_device(lib, marr, pbs, iterations, lr, device, log):
    """One chunk of clips through phc_fit_sph_iterate -> per clip (rot [T, ND], root_rot [T, 3], root_off [3], loss)."""
    from .. import abi
    nb, M = len(marr["parents"]), len(marr["match_body"])
    nd, C = 3 * (nb - 1), len(pbs)
    start = np.concatenate([[0], np.cumsum([pb.T for pb in pbs])]).astype(np.int64)
    F_ = int(start[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    dev = {k: up(v.view(np.int32) if v.dtype == np.uint32 else v) for k, v in marr.items()}
    dev["axis"] = None
    dev["clip_start"] = up(start)
    dev["target"] = up(f32(np.concatenate([pb.g for pb in pbs])))
    dev["root_trans_offset"] = up(f32(np.concatenate([pb.root_trans for pb in pbs])))
    dev["root_rot"] = up(f32(np.concatenate([pb.root_rot0 for pb in pbs])))
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)
    dev.update(dof=z(F_, nd), dof_m=z(F_, nd), dof_v=z(F_, nd), root_rot_m=z(F_, 3), root_rot_v=z(F_, 3), root_off=z(C, 3), root_off_m=z(C, 3),
               root_off_v=z(C, 3), step=z(C, dtype=torch.int32), loss=z(C))
    sb = int(lib.phc_fit_sph_scratch_bytes(F_, C, nb))
    if sb < 0:
        raise RuntimeError(f"phc_fit_sph_scratch_bytes refused {F_} frames, {C} clips, {nb} bodies")
    scratch = torch.empty(sb, dtype=torch.uint8, device=device)
    args = abi.fit_args_struct(nb, 0, M, C, F_, lr, scratch, sb, clip_start_host=start, **dev)
    stream = torch.cuda.current_stream(device).cuda_stream
    segments = [iterations] if log is None else [min(FIT_LOG_SEGMENT, iterations - i) for i in range(0, iterations, FIT_LOG_SEGMENT)] or [0]
    done = 0
    timing = None if FIT_TIMING is None else [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    if timing:
        timing[0].record(torch.cuda.current_stream(device))
    for n in segments:   # (segmenting does not change a bit of the result)
        L.check(lib.phc_fit_sph_iterate(args, int(n), stream), "phc_fit_sph_iterate")
        done += n
        if log is not None and n > 0:
            log(f"iter {done - 1}: " + " ".join(f"{v * 1000:.3f}" for v in dev["loss"].cpu().tolist()))
    if timing:
        timing[1].record(torch.cuda.current_stream(device))
        timing[1].synchronize()
        FIT_TIMING.append((F_, C, int(iterations), timing[0].elapsed_time(timing[1])))
    rot, root_rot, root_off, loss = (dev[k].cpu().numpy() for k in ("dof", "root_rot", "root_off", "loss"))
    return [(rot[start[c]:start[c + 1]].copy(), root_rot[start[c]:start[c + 1]].copy(), root_off[c].copy(),
             float(loss[c]) if iterations > 0 else float("nan")) for c in range(C)]


def fit_keypoint_clips(model, clips, *, bodies=None, iterations=500, lr=0.02, backend="host", device="cpu", chunk_frames=262144, fps=30, order="mujoco", up="z",
                       bone_lengths="keep", log=None, dtype=torch.float32):
    """A library.  `clips`: key -> keypoints [T, K, 3]; `bodies`: the model body name of each keypoint column (default: `resolve_bodies`).  Returns key -> a clip
    in the `MotionLibSMPL` layout (`pose_quat_global [T, NB, 4]` xyzw in model order, `root_trans_offset`, `pose_aa [T, 3 NB]`, `fps`) plus `keypoints` (the
    processed input), `fit_loss` and `fit_keypoint_error`.  `fps`: a number for all clips or key -> number.
    backend "host": torch autograd + torch.optim.Adam per clip on `device` in `dtype`.  backend "device": all clips of a chunk (whole clips, at most
    `chunk_frames` frames) at once in phc_fit_sph_iterate on the HIP device `device` -- the same iteration in fp32 with an analytic gradient; `log(str)` then
    receives the clips' losses every FIT_LOG_SEGMENT iterations.  There is no fallback from one backend to the other."""
    if backend not in ("host", "device"):
        raise ValueError(f"fit_keypoint_clips: unknown backend {backend!r} (host | device)")
    check_model(model)
    keys = list(clips)
    if not keys:
        return {}
    for k in keys:
        if np.asarray(clips[k]).shape[0] < 1:
            raise ValueError(f"fit_keypoint_clips: clip {k!r} has no frames")
    idx = resolve_bodies(model, np.asarray(clips[keys[0]]).shape[1], bodies)
    if len(idx) > L.FIT_MAX_MATCHED:
        raise ValueError(f"fit_keypoint_clips takes at most {L.FIT_MAX_MATCHED} keypoints")
    marr = sph_model_arrays(model, idx)
    pbs = [_SphProblem(model, clips[k], idx, order, up, bone_lengths) for k in keys]
    fps_of = (lambda k: fps[k]) if isinstance(fps, dict) else (lambda k: fps)
    if backend == "host":
        return {k: _dump(marr, pb, *_fit_host(marr, pb, int(iterations), lr, device, dtype, None if log is None else (lambda s, k=k: log(f"{k} {s}"))), fps_of(k))
                for k, pb in zip(keys, pbs)}
    from ..motion_lib import _clip_chunks
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available() or torch.version.hip is None:
        raise RuntimeError(f"fit_keypoint_clips: backend=device runs on a HIP device only (no fallback), not on {dev}; use backend=host")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    lib = L.load()
    out = {}
    for u0, u1 in _clip_chunks([pb.T for pb in pbs], int(chunk_frames)):
        states = _fit_chunk_device(lib, marr, pbs[u0:u1], int(iterations), lr, dev, None if log is None else (lambda s, u0=u0, u1=u1: log(f"clips {u0}..{u1 - 1} {s}")))
        for k, pb, st in zip(keys[u0:u1], pbs[u0:u1], states):
            out[k] = _dump(marr, pb, *st, fps_of(k))
    return out


def clip_keypoints(model, clip):
    """The body positions [T, NB, 3] of a `MotionLibSMPL`-layout clip (`pose_quat_global`, `root_trans_offset`): what a keypoint source would have seen."""
    from scipy.spatial.transform import Rotation as sRot
    q = np.asarray(clip["pose_quat_global"], dtype=np.float64)
    T, nb = q.shape[:2]
    R = sRot.from_quat(q.reshape(-1, 4)).as_matrix().reshape(T, nb, 3, 3)
    pos = np.zeros((T, nb, 3))
    pos[:, 0] = np.asarray(clip["root_trans_offset"], dtype=np.float64)
    for b in range(1, nb):
        p = int(model.parent[b])
        pos[:, b] = pos[:, p] + R[:, p] @ np.asarray(model.local_translation[b], dtype=np.float64)
    return pos


def main(argv=None):
    import argparse
    import joblib
    from ..model import load_model
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--joints", required=True, help="npz: <key>/joints [T, K, 3], optionally <key>/fps")
    ap.add_argument("--out", required=True)
    ap.add_argument("--model", default="smpl_humanoid")
    ap.add_argument("--fps", type=float, default=30)
    ap.add_argument("--order", default="mujoco", choices=["mujoco", "smpl"])
    ap.add_argument("--up", default="z", choices=["z", "y"])
    ap.add_argument("--bone-lengths", default="keep", choices=["keep", "model"])
    ap.add_argument("--iterations", type=int, default=500)
    ap.add_argument("--backend", default="host", choices=["host", "device"], help="host: torch autograd per clip; device: phc_fit_sph_iterate over chunks of clips")
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--chunk-frames", type=int, default=262144, help="backend=device: frames fitted at once")
    a = ap.parse_args(argv)
    model = load_model(a.model)
    data = np.load(a.joints)
    keys = sorted({k.rsplit("/", 1)[0] for k in data.files})
    default_fps = int(a.fps) if float(a.fps).is_integer() else a.fps
    fps = {k: (float(data[f"{k}/fps"]) if f"{k}/fps" in data.files else default_fps) for k in keys}
    fps = {k: int(v) if float(v).is_integer() else v for k, v in fps.items()}
    out = fit_keypoint_clips(model, {k: data[f"{k}/joints"] for k in keys}, iterations=a.iterations, backend=a.backend, device=a.device,
                             chunk_frames=a.chunk_frames, fps=fps, order=a.order, up=a.up, bone_lengths=a.bone_lengths, log=lambda s: print(s, flush=True))
    joblib.dump(out, a.out)
    err = [c["fit_keypoint_error"] for c in out.values()]
    print(f"wrote {len(out)} clips to {a.out}; mean keypoint error {1000 * float(np.mean(err)):.2f} mm")


if __name__ == "__main__":
    main()
