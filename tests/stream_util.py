"""TEST INFRASTRUCTURE shared by tests/test_stream_cpu.py and tests/test_stream_gpu.py: the host build of phc_amd/csrc/phc_stream.h (tests/stream_shim.cpp,
g++), a numpy-backed caller with the layout of phc_stream_args_t, seeded keypoint streams and body states of any shape, and a fp64 numpy restatement of the
launch that filters with scipy's own gaussian_filter1d (the kernel's folded table never enters it)."""
import collections
import ctypes as C
import functools
import json
import os

import numpy as np
from scipy.ndimage import gaussian_filter1d

from phc_amd import _lib as L
from phc_amd import abi
from phc_amd import stream as S
from teleop_util import TOL   # |a - b| <= TOL max(1, |b|): the bound of the post-physics floats
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
VR_TRACK = ["Head", "L_Hand", "R_Hand"]   # env_vr's trackBodies
STATE = ("ring_body", "ring_root", "head", "count", "has_prev", "cur_ref", "cur_vel")


@functools.lru_cache(maxsize=None)
def shim():
    lib = host_build.shim("stream_shim.cpp", "phc_stream.hip")
    for fn in (lib.stream_args_check_of, lib.stream_track_host):
        fn.argtypes = [C.POINTER(L.Model), C.POINTER(L.ImParams), C.POINTER(L.StreamArgs)]
        fn.restype = C.c_int
    return lib


def host_launch(model, prm, a):
    return shim().stream_track_host(C.byref(model), C.byref(prm), C.byref(a))


def close(a, b, what="", tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, f"{what}: shapes {a.shape} / {b.shape}"
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    worst = float(err.max()) if err.size else 0.0
    assert worst <= tol, f"{what}: largest error {worst:.3e} (bound {tol})"
    return worst


@functools.lru_cache(maxsize=None)
def smpl_model():
    """(body names, parents) of the shipped SMPL model, MuJoCo order."""
    d = json.load(open(os.path.join(ROOT, "phc_amd", "assets", "smpl_humanoid.json")))
    return list(d["body_names"]), [int(p) for p in d["parent"]]


def options(nb, **cfg):
    """The resolved `stream` options (phc_amd.stream.parse_options) for a model of nb bodies: the SMPL family at 24, a robot otherwise."""
    is_smpl = nb == 24
    parents = smpl_model()[1] if is_smpl else [-1] + list(range(nb - 1))
    return S.parse_options(cfg, is_smpl=is_smpl, num_bodies=nb, parents=parents, task_dt=1 / 30)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------
def keypoint_stream(steps, rows, nb, seed=0, offset=None, jitter=0.01, drift=0.3):
    """[steps, rows, nb, 3] fp32: a skeleton-sized cloud per row (root first, limbs a few decimetres long) that drifts (up to `drift` m/s per axis) and
    wobbles smoothly, plus noise -- what a pose estimator sends.  `offset` [rows, 3]: where each row's root starts."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-0.6, 0.6, (rows, nb, 3))
    base[:, 0] = 0
    base[:, 1:6] = base[:, 0:5] + rng.uniform(0.1, 0.4, (rows, 5, 3)) * rng.choice([-1.0, 1.0], (rows, 5, 3))   # the default limb pairs: real lengths
    t = np.arange(steps)[:, None, None, None] / 30.0
    sway = 0.15 * np.sin(2 * np.pi * (0.7 * t + rng.uniform(0, 1, (rows, nb, 3))))
    root = (np.zeros((rows, 3)) if offset is None else np.asarray(offset, np.float64))[None, :, None, :] + t * rng.uniform(-drift, drift, (rows, 1, 3))
    return (base[None] + sway + root + rng.standard_normal((steps, rows, nb, 3)) * jitter).astype(F)


def body_states(steps, n, nb, seed=1):
    """[steps, n, nb, 13] fp32 rigid-body states: bodies around a root near the origin, unit quaternions, metre-per-second velocities."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((steps, n, nb, 13))
    x[..., :3] = rng.uniform(-0.7, 0.7, (steps, n, nb, 3)) + rng.uniform(-0.2, 0.2, (steps, n, 1, 3))
    x[..., 3:7] /= np.linalg.norm(x[..., 3:7], axis=-1, keepdims=True)
    return x.astype(F)


# ---- the caller -------------------------------------------------------------------------------------------------------------------------------------
class Runner:
    """State and arguments of phc_stream_track over the steps of a stream, in host memory (`to` = a copy) or on the device (`to` = numpy -> torch tensor,
    `back` = tensor -> numpy); `launch(model, prm, args)` is the host build or the entry point.  `track`: the tracked bodies' indices, slot order."""

    def __init__(self, n, nb, track, opts, launch, to=lambda a: np.array(a, copy=True), back=lambda a: a, zero_out_far=True, close_distance=0.25,
                 far_distance=3.0, remove_base_rot=False, num_self_obs=7, preset_prev=False):
        self.n, self.nb, self.track, self.o, self.launch, self.to, self.back = n, nb, list(track), opts, launch, to, back
        W, J = opts["window"], len(track)
        self.num_self_obs, self.num_task_obs = num_self_obs, 9 * J
        self.state = dict(ring_body=to(np.zeros((n, W, nb, 3), F)), ring_root=to(np.zeros((n, W, 3), F)), head=to(np.zeros(n, np.int32)),
                          count=to(np.zeros(n, np.int32)), has_prev=to(np.full(n, 1 if preset_prev else 0, np.uint8)), cur_ref=to(np.zeros((n, nb, 3), F)),
                          cur_vel=to(np.zeros((n, nb, 3), F)))
        self.out = dict(obs_buf=to(np.full((n, num_self_obs + 9 * J), 7.0, F)), reset_buf=to(np.ones(n, np.int64)), terminate_buf=to(np.ones(n, np.int64)),
                        track_err=to(np.full(n, -1.0, F)))
        slot = np.full(abi.MAX_BODIES, -1, np.int32)
        slot[self.track] = np.arange(J)
        self.fold = to(S.fold_table(opts["root_sigma"], opts["body_sigma"], W))
        self.perm = None if opts["perm"] is None else to(opts["perm"])
        self._slot = to(slot)
        self.model = L.Model()
        self.model.num_bodies = nb
        p = self.prm = L.ImParams()
        p.dt, p.obs_v, p.num_traj_samples, p.num_track_bodies, p.track_slot = 1 / 30, 7, 1, J, abi.ptr(self._slot)
        p.num_self_obs, p.num_task_obs, p.zero_out_far, p.remove_base_rot = num_self_obs, 9 * J, int(zero_out_far), int(remove_base_rot)
        p.close_distance, p.far_distance = 123.0, 456.0   # the launch takes the stream's own distances, not these
        self.close_distance, self.far_distance = close_distance, far_distance

    def args(self, frames, rbs, mode):
        o = self.o
        a = abi.stream_args_struct(self.n, o["window"], self.fold, frames, mode=mode, limb_pairs=o["limb_pairs"], limb_lengths=o["limb_lengths"],
                                   limb_scale=o["limb_scale"], frame_mat=o["frame_mat"], dt=o["dt"], close_distance=self.close_distance,
                                   far_distance=self.far_distance, track_root_body=self.track[0], perm=self.perm, rigid_body_state=rbs, **self.state, **self.out)
        return a

    def step(self, frames, rbs, mode=L.STREAM_ADVANCE):
        """One launch -> dict of numpy copies: the outputs and the state afterwards."""
        f = None if frames is None else self.to(np.ascontiguousarray(frames, F))
        r = self.to(np.ascontiguousarray(rbs, F))
        a = self.args(f, r, mode)
        self._keep = (f, r, a)
        rc = self.launch(self.model, self.prm, a)
        assert rc == 0, rc
        return self.snapshot()

    def snapshot(self):
        return {k: np.array(self.back(v), copy=True) for k, v in {**self.state, **self.out}.items()}

    def restart(self, ids):
        """What task.restart_stream(ids) does."""
        for k in ("head", "count", "has_prev"):
            v = np.array(self.back(self.state[k]), copy=True)
            v[ids] = 0
            self.state[k] = self.to(v)


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------------
def _qmul(a, b):
    ax, ay, az, aw = np.moveaxis(a, -1, 0)
    bx, by, bz, bw = np.moveaxis(b, -1, 0)
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def _qrot(q, v):
    qv, w = q[..., :3], q[..., 3:4]
    return v * (2 * w * w - 1) + 2 * w * np.cross(qv, v) + 2 * qv * (qv * v).sum(-1, keepdims=True)


def heading_inv(root_rot, remove_base_rot=False):
    """The inverse heading rotation of the observation functions: about z by minus the yaw of the root's x axis."""
    q = np.asarray(root_rot, np.float64)
    if remove_base_rot:
        q = _qmul(q, np.broadcast_to(np.array([-0.5, -0.5, -0.5, 0.5]), q.shape))
    x = _qrot(q, np.broadcast_to(np.array([1.0, 0.0, 0.0]), q.shape[:-1] + (3,)))
    half = -0.5 * np.arctan2(x[..., 1], x[..., 0])
    z = np.zeros_like(half)
    return np.stack([z, z, np.sin(half), np.cos(half)], axis=-1)


class Restate:
    """Steps 1-9 of the launch in fp64 numpy, env by env, the way the reference writes them (humanoid_im_mcp_demo.py:255-310): deques and scipy's
    gaussian_filter1d(mode="mirror").  `preset_prev`: the reference's start, prev_ref_body_pos = 0 (first velocity = position / dt)."""

    def __init__(self, n, nb, opts, preset_prev=False):
        self.n, self.nb, self.o = n, nb, opts
        W = opts["window"]
        self.root = [collections.deque(maxlen=W) for _ in range(n)]
        self.body = [collections.deque(maxlen=W) for _ in range(n)]
        self.prev = [np.zeros((nb, 3)) if preset_prev else None for _ in range(n)]
        self.M = np.asarray(opts["frame_mat"], np.float64).astype(F).astype(np.float64)   # the struct holds it as fp32

    def restart(self, ids):
        for e in ids:
            self.root[e].clear(); self.body[e].clear()
            self.prev[e] = None

    @staticmethod
    def _filt(x, sigma):
        x = np.asarray(x, np.float64)
        return x[-1] if sigma == 0 else gaussian_filter1d(x, sigma, axis=0, mode="mirror")[-1]

    def advance(self, frames):
        """frames [n or 1, nb, 3] -> (ref [n, nb, 3], vel [n, nb, 3]) fp64."""
        o = self.o
        ref, vel = np.zeros((self.n, self.nb, 3)), np.zeros((self.n, self.nb, 3))
        for e in range(self.n):
            p = np.asarray(frames[0 if frames.shape[0] == 1 else e], np.float64)
            if o["perm"] is not None:
                p = p[o["perm"]]
            trans = p[0].copy()
            q = p - trans
            if o["limb_scale"]:
                q = q / np.mean([np.linalg.norm(q[a] - q[b]) / ln for (a, b), ln in zip(o["limb_pairs"], o["limb_lengths"])])
            self.root[e].append(trans)
            self.body[e].append(q)
            roots = np.array(self.root[e])
            t = np.array([self._filt(roots[:, c], o["root_sigma"][c]) for c in range(3)])
            ref[e] = (self._filt(np.array(self.body[e]), o["body_sigma"]) + t) @ self.M.T
            if self.prev[e] is not None:
                vel[e] = (ref[e] - self.prev[e]) / o["dt"]
            self.prev[e] = ref[e].copy()
        return ref, vel


def observe(rbs, ref, vel, track, zero_out_far=True, close_distance=0.25, far_distance=3.0, remove_base_rot=False):
    """Gating (humanoid_im_mcp_demo.py:296-306), compute_imitation_observations_v7 and track_err in fp64 -> (task obs [n, 9 J], err [n], distance [n])."""
    rbs, ref, vel = (np.asarray(x, np.float64) for x in (rbs, ref, vel))
    pos, v = rbs[..., :3], rbs[..., 7:10]
    root_pos, hinv = pos[:, 0], heading_inv(rbs[:, 0, 3:7], remove_base_rot)
    bp, bv, rp, rv = pos[:, track], v[:, track], ref[:, track].copy(), vel[:, track].copy()
    err = np.linalg.norm(bp - rp, axis=-1).mean(-1)
    dist = np.linalg.norm(root_pos - rp[:, 0], axis=-1)
    if zero_out_far:
        z = dist > close_distance
        rp[z, 1:] = bp[z, 1:]
        rv[z] = bv[z]
        f = dist > far_distance
        rp[f, 0] = (rp[f, 0] - bp[f, 0]) / dist[f, None] * far_distance + bp[f, 0]
    h = np.broadcast_to(hinv[:, None], bp.shape[:2] + (4,))
    obs = np.concatenate([_qrot(h, rp - bp).reshape(len(rbs), -1), _qrot(h, rv - bv).reshape(len(rbs), -1),
                          _qrot(h, rp - root_pos[:, None]).reshape(len(rbs), -1)], axis=-1)
    return obs, err, dist
