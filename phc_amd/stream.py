"""Keypoint streams (config group `stream`): what HumanoidImDemo / HumanoidImMCPDemo track instead of a clip of the motion library -- the output of a pose
estimator, a text-to-motion model or a VR rig, one frame of keypoints [N, NB, 3] per env step (reference: phc/env/tasks/humanoid_im_mcp_demo.py:252-317,
which polls an HTTP server; the server is not built, the per-step path is phc_stream_track, include/phc_amd.h).

    +stream.file=kp.npy             # [T, NB, 3] (every env the same frame) or [T, N, NB, 3]
    +stream.motion=synthetic:3:1    # any env.motion_file spec: the clip's body positions at t = k dt, through the motion library
    +stream.loop=True               # wrap at the end of the source; False: hold the last frame
    +stream.order=mujoco            # joint order of the frames: mujoco (the model's) | smpl (SMPL family: the reference's smpl_2_mujoco)
    +stream.up=z                    # z: frames are in the simulator's frame | y: y-up frames, rotated by the reference's to_isaac_mat
    +stream.limb_scale=True         # normalise limb lengths (default: SMPL family True, robots False)
    +stream.limb_pairs=[[0,1],..]   # (parent, child) body indices; default: bodies 1..5 against their parents
    +stream.limb_lengths=[0.1061, 0.3624, 0.4015, 0.1384, 0.1132]
    +stream.root_sigma=[5,5,10]     # gaussian sigma (frames) of the root translation per axis; 0 = no filter
    +stream.body_sigma=2            # ... of the root-relative bodies
    +stream.window=30               # frames held (the reference's deque(maxlen=30))
    +stream.dt=<task dt>            # the finite difference's time step (the reference hard-codes 1/30)

Without `file` / `motion` the caller hands frames in with `task.set_keypoints(j3d)`."""
import math

import numpy as np
import torch

from . import _lib as L

KEYS = ("file", "motion", "loop", "order", "up", "limb_scale", "limb_pairs", "limb_lengths", "root_sigma", "body_sigma", "window", "dt")
SMPL_2_MUJOCO = (0, 1, 4, 7, 10, 2, 5, 8, 11, 3, 6, 9, 12, 15, 13, 16, 18, 20, 22, 14, 17, 19, 21, 23)   # humanoid_im_mcp_demo.py:32
MEAN_LIMB_LENGTHS = (0.1061, 0.3624, 0.4015, 0.1384, 0.1132)                                              # humanoid_im_mcp_demo.py:66
# sRot.from_euler('xyz', [-pi / 2, 0, 0]).as_matrix() (humanoid_im_mcp_demo.py:56), cos(pi / 2) as fp64 gives it
_C = math.cos(-math.pi / 2)
TO_ISAAC_MAT = ((1.0, 0.0, 0.0), (0.0, _C, 1.0), (0.0, -1.0, _C))
TRUNCATE = 4.0   # scipy.ndimage.gaussian_filter1d's default


def fold_row(sigma, length):
    """Weights w[0 .. length) (oldest first, fp64) with sum_k w[k] x[k] == scipy.ndimage.gaussian_filter1d(x, sigma, mode="mirror")[-1] for `length`
    samples: the kernel of radius int(4 sigma + 0.5) centred on the newest sample, its taps past either end folded back by the mirror rule
    (d c b | a b c d | c b a: period 2 (length - 1)).  sigma 0: the identity."""
    w = np.zeros(length, dtype=np.float64)
    if sigma <= 0:
        w[-1] = 1.0
        return w
    radius = int(TRUNCATE * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    phi = phi / phi.sum()
    period = 2 * (length - 1)
    for k, p in zip(x, phi):
        i = length - 1 + int(k)
        if period == 0:
            i = 0
        else:
            i %= period
            if i >= length:
                i = period - i
        w[i] += p
    return w


def fold_table(root_sigma, body_sigma, window):
    """fp64 [4, window, window]: table[s, L - 1, :L] = fold_row(sigma_s, L); s = 0, 1, 2 the root translation's axes, 3 the bodies (phc_stream_args_t.fold)."""
    sig = [float(s) for s in root_sigma] + [float(body_sigma)]
    t = np.zeros((4, window, window), dtype=np.float64)
    for s, sigma in enumerate(sig):
        for n in range(1, window + 1):
            t[s, n - 1, :n] = fold_row(sigma, n)
    return t


def parse_options(cfg, *, is_smpl, num_bodies, parents, task_dt):
    """The `stream` group -> a dict with every key of KEYS resolved (`perm`: int32 [NB] or None; `frame_mat`: 3 x 3).  An unknown key is a ValueError."""
    cfg = dict(cfg or {})
    unknown = set(cfg) - set(KEYS)
    if unknown:
        raise ValueError(f"unknown stream option(s): {sorted(unknown)}")
    o = {"file": cfg.get("file"), "motion": cfg.get("motion"), "loop": bool(cfg.get("loop", True))}
    if o["file"] is not None and o["motion"] is not None:
        raise ValueError("stream.file and stream.motion are two sources: give one")
    order = str(cfg.get("order", "mujoco"))
    if order not in ("mujoco", "smpl"):
        raise ValueError(f"stream.order must be mujoco or smpl, not {order!r}")
    if order == "smpl" and not (is_smpl and num_bodies == len(SMPL_2_MUJOCO)):
        raise ValueError("stream.order=smpl: the SMPL joint order exists for the 24-body SMPL family only")
    o["order"], o["perm"] = order, (np.array(SMPL_2_MUJOCO, dtype=np.int32) if order == "smpl" else None)
    up = str(cfg.get("up", "z"))
    if up not in ("z", "y"):
        raise ValueError(f"stream.up must be z or y, not {up!r}")
    o["up"], o["frame_mat"] = up, (np.array(TO_ISAAC_MAT, dtype=np.float64) if up == "y" else np.eye(3))
    o["limb_scale"] = bool(cfg.get("limb_scale", is_smpl))
    if "limb_pairs" in cfg:
        pairs = [tuple(int(v) for v in p) for p in cfg["limb_pairs"]]
    else:   # humanoid_im_mcp_demo.py:266-270: bodies 0..5 that have a parent
        pairs = [(int(parents[i]), i) for i in range(min(6, num_bodies)) if int(parents[i]) != -1]
    lengths = [float(v) for v in cfg.get("limb_lengths", MEAN_LIMB_LENGTHS)]
    if o["limb_scale"]:
        if not pairs or len(pairs) > L.STREAM_MAX_PAIRS or any(len(p) != 2 for p in pairs):
            raise ValueError(f"stream.limb_pairs: 1 to {L.STREAM_MAX_PAIRS} [parent, child] pairs")
        if len(lengths) != len(pairs):
            raise ValueError(f"stream.limb_lengths has {len(lengths)} entries for {len(pairs)} stream.limb_pairs")
        if any(not (0 <= b < num_bodies) for p in pairs for b in p):
            raise ValueError(f"stream.limb_pairs: body indices lie in [0, {num_bodies})")
        if any(not (v > 0 and math.isfinite(v)) for v in lengths):
            raise ValueError("stream.limb_lengths must be positive")
    else:
        pairs, lengths = [], []
    o["limb_pairs"], o["limb_lengths"] = pairs, lengths
    rs = cfg.get("root_sigma", [5, 5, 10])
    rs = [rs] * 3 if isinstance(rs, (int, float)) else list(rs)
    if len(rs) != 3 or any(float(s) < 0 for s in rs) or float(cfg.get("body_sigma", 2)) < 0:
        raise ValueError("stream.root_sigma (a number or one per axis) and stream.body_sigma must be >= 0")
    o["root_sigma"], o["body_sigma"] = [float(s) for s in rs], float(cfg.get("body_sigma", 2))
    o["window"] = int(cfg.get("window", 30))
    if not (1 <= o["window"] <= L.STREAM_MAX_WINDOW):
        raise ValueError(f"stream.window must lie in [1, {L.STREAM_MAX_WINDOW}]")
    o["dt"] = float(cfg.get("dt", task_dt))
    if not (o["dt"] > 0 and math.isfinite(o["dt"])):
        raise ValueError("stream.dt must be positive")
    return o


class KeypointSource:
    """Frames of keypoints on the device, one per env step: `frame(k)` -> [N or 1, NB, 3] fp32 contiguous; `next()` = frame of the source's own counter.

    `frames`: a tensor [T, NB, 3] / [T, N, NB, 3] (stream.file); or `lookup`: k -> tensor with `length`s per env (stream.motion, see `from_motion_lib`)."""

    def __init__(self, frames=None, loop=True, lookup=None):
        self.loop, self.k = bool(loop), 0
        self._frames, self._lookup = frames, lookup

    @classmethod
    def from_file(cls, path, num_envs, num_bodies, device, loop=True):
        x = np.load(path)
        if x.ndim == 3:
            x = x[:, None]
        if x.ndim != 4 or x.shape[0] < 1 or x.shape[1] not in (1, num_envs) or tuple(x.shape[2:]) != (num_bodies, 3):
            raise ValueError(f"stream.file={path}: shape {tuple(x.shape)}; expected [T, {num_bodies}, 3] or [T, {num_envs}, {num_bodies}, 3]")
        return cls(frames=torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device), loop=loop)

    @classmethod
    def from_motion_lib(cls, lib, num_envs, dt, device, loop=True):
        """The clips of `lib` (clip e % num_motions for env e) sampled at t = k dt: the body positions of its motion state, looked up per step."""
        ids = torch.arange(num_envs, device=device, dtype=torch.long) % lib.num_motions()
        last = torch.floor(lib.get_motion_length(ids) / dt).to(torch.long)   # frames 0 .. floor(length / dt)
        steps = last + 1

        def lookup(k):
            kk = torch.remainder(torch.full_like(steps, k), steps) if loop else torch.clamp(last, max=k)
            return lib.get_motion_state(ids, kk.to(torch.float32) * dt)["rg_pos"].contiguous()
        return cls(loop=loop, lookup=lookup)

    def __len__(self):
        return 0 if self._frames is None else int(self._frames.shape[0])

    def frame(self, k):
        if self._lookup is not None:
            return self._lookup(int(k))
        T = self._frames.shape[0]
        return self._frames[int(k) % T if self.loop else min(int(k), T - 1)]

    def next(self):
        f = self.frame(self.k)
        self.k += 1
        return f

    def restart(self):
        self.k = 0
