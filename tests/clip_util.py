"""Shared by tests/test_clip_device_cpu.py and tests/test_clip_device_gpu.py: the host build of phc_amd/csrc/phc_clip.h (tests/clip_shim.cpp, g++), the
constructed clips, the oracle (`process_clip` + float32 + `abi.pack_frames`: the existing host path, never the code under test) and the field-by-field
comparison at the tolerances that follow from "both sides compute in fp64 and round once"."""
import ctypes as C
import functools

import numpy as np

import host_build

GUARD = 0x5A5A5A5A
LENGTHS = (2, 3, 8, 9, 16, 17, 18, 40)      # the filter radius (8) exceeds, meets and undershoots the clip
FPS = (30, 60, 30, 60, 60, 30, 60, 30)
TREE = (0, 1, 1, 0, 1, 0, 0, 1)
EPS32 = 2.0 ** -23                            # one fp32 rounding flip, relative to max(|host|, 1)
ANG_FLOOR = 1e-5                              # rad/s at 30 fps: acos near 1 turns a few fp64 ulps into ~5e-8 rad per frame; margin ~5

EINVAL, EUNSUPPORTED = -1, -2
# (field, value, code) phc_clip_process must refuse, for the 3-body case (113 frames, 8 clips, 2 trees)
BAD_ARGS = (("num_clips", 0, EINVAL), ("num_clips", -1, EINVAL), ("num_bodies", 0, EINVAL), ("num_bodies", 65, EUNSUPPORTED), ("num_trees", 0, EINVAL),
            ("frame_stride", 57, EINVAL), ("frame_stride", 64, EINVAL), ("frame_stride", 0, EINVAL), ("scratch_bytes", 0, EINVAL), ("num_frames", 15, EINVAL),
            ("num_frames", 1 << 40, EUNSUPPORTED))


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("clip_shim.cpp", "phc_clip.hip")
    lib.clip_args_check_of.argtypes = [C.POINTER(L.ClipArgs)]
    lib.clip_args_check_of.restype = C.c_int
    lib.clip_scratch_bytes_of.argtypes = [C.c_longlong, C.c_int]
    lib.clip_scratch_bytes_of.restype = C.c_longlong
    lib.clip_frames_per_block_of.argtypes = [C.c_int]
    lib.clip_frames_per_block_of.restype = C.c_int
    lib.clip_weights.argtypes = [C.c_void_p]
    lib.clip_weights.restype = None
    lib.clip_process_host.argtypes = [C.POINTER(L.ClipArgs)]
    lib.clip_process_host.restype = C.c_int
    return lib


def trees():
    """name -> (parents [J], local translations [2, J, 3]: two body shapes of one topology)."""
    from phc_amd.model import load_model
    m = load_model("smpl_humanoid")
    rng = np.random.RandomState(11)
    out = {"smpl": (np.asarray(m.parent, dtype=np.int32), np.asarray(m.local_translation, dtype=np.float64)),
           "chain3": (np.array([-1, 0, 1], dtype=np.int32), rng.uniform(-0.4, 0.4, (3, 3))),
           "star5": (np.array([-1, 0, 0, 0, 0], dtype=np.int32), rng.uniform(-0.4, 0.4, (5, 3)))}
    return {k: (p, np.stack([lt, lt * 1.15 + rng.uniform(-0.02, 0.02, lt.shape)])) for k, (p, lt) in out.items()}


def _q_axis_angle(axis, angle):
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    return np.concatenate([axis * np.sin(0.5 * angle)[..., None], np.cos(0.5 * angle)[..., None]], axis=-1)


@functools.lru_cache(maxsize=None)
def make_case(name, seed=0):
    """Eight clips (LENGTHS) on tree `name`: per frame every joint turns 0.01 .. 0.3 rad about a random axis (slow in the even clips, fast in the odd ones, and
    the roots move at very different speeds: a filter that leaks across a clip boundary shows far above tolerance); some joints keep a bit-identical local
    rotation over the whole clip (sin_t ~ 1e-8: masked on both sides); the last joint steps 2.5 rad per frame (the angle wrap, away from pi); a tenth of the
    global quaternions is negated as a whole (pos_unit).  -> dict of the arguments of `process_clips_device`."""
    from phc_amd.motion_lib import _q_mul
    parents, lts = trees()[name]
    J = len(parents)
    rng = np.random.RandomState(1000 + seed)
    quats, trans = [], []
    for u, (T, fps) in enumerate(zip(LENGTHS, FPS)):
        lo, hi = ((0.01, 0.05), (0.2, 0.3))[u % 2]
        step = _q_axis_angle(rng.normal(size=(T, J, 3)), rng.uniform(lo, hi, (T, J)))
        held = [j for j in range(1, J - 1) if rng.uniform() < 0.3] or ([1] if J > 2 and u % 2 else [])
        local = np.zeros((T, J, 4))
        local[0] = _q_axis_angle(rng.normal(size=(J, 3)), rng.uniform(0.1, 1.0, J))
        for t in range(1, T):
            local[t] = _q_mul(local[t - 1], step[t])
            local[t] /= np.linalg.norm(local[t], axis=-1, keepdims=True)
        local[:, held] = local[0, held]
        wrap_axis = rng.normal(size=3)
        local[:, J - 1] = _q_axis_angle(np.broadcast_to(wrap_axis, (T, 3)), 0.3 + 2.5 * np.arange(T))
        g = np.zeros_like(local)
        for j in range(J):
            g[:, j] = local[:, j] if parents[j] < 0 else _q_mul(g[:, parents[j]], local[:, j])
        g[rng.uniform(size=(T, J)) < 0.1] *= -1.0
        v = (-1.0) ** u * (3.0 + 2.0 * u) * np.array([np.cos(u), np.sin(u), 0.1])
        tr = np.array([0.3 * u, -0.2 * u, 0.9]) + v * (np.arange(T)[:, None] / fps) + rng.normal(scale=0.01, size=(T, 3))
        quats.append(g)
        trans.append(tr)
    return dict(parents=parents, local_translations=lts, clip_tree=np.array(TREE, dtype=np.int32), quats=quats, trans=trans, fps=list(FPS))


@functools.lru_cache(maxsize=None)
def oracle(name, seed=0):
    """-> (records [F, stride] float32 of the existing host path, fps per frame [F]); asserts the condition on the inputs: no joint / frame of the host path
    has sin_t in [1e-6, 1e-4] (the `sin_t > 1e-5` branch of dvs is a threshold, not a tolerance: nothing is excluded from the comparison)."""
    from phc_amd import abi
    from phc_amd.motion_lib import _q_conj, _q_mul, process_clip
    c = make_case(name, seed)
    recs, masked = [], 0
    for t, g, tr, fps in zip(c["clip_tree"], c["quats"], c["trans"], c["fps"]):
        p = process_clip(c["parents"], c["local_translations"][t], g, tr, fps)
        w = _q_mul(_q_conj(p["lrs"][:-1]), p["lrs"][1:])[..., 3][:, 1:]
        sin_t = np.sqrt(np.maximum(1 - w * w, 0.0))
        assert not ((sin_t >= 1e-6) & (sin_t <= 1e-4)).any(), "inputs too close to the sin_t threshold"
        masked += int((sin_t <= 1e-5).sum())
        f = {k: p[k].astype(np.float32) for k in ("gts", "grs", "gvs", "gavs", "lrs", "dvs")}
        recs.append(abi.pack_frames(f["gts"], f["grs"], f["gvs"], f["gavs"], f["lrs"], f["dvs"]))
    assert masked > 0, "the case must hold some joints still"
    assert any((g[..., 3] < 0).any() for g in c["quats"])
    return np.concatenate(recs), np.repeat(np.asarray(c["fps"], dtype=np.float64), LENGTHS)


def fields(J):
    o, out = 0, {}
    for k, w in (("gts", 3 * J), ("grs", 4 * J), ("gvs", 3 * J), ("gavs", 3 * J), ("lrs", 4 * J), ("dvs", 3 * (J - 1)), ("pad", 3)):
        out[k] = slice(o, o + w)
        o += w
    return out


def compare(got, want, fps_frame, scale=1.0, what=""):
    """Field by field: grs and the pad floats bit-equal; gts / lrs / gvs within `scale` fp32 rounding flips; gavs / dvs the same plus the floor."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    J = want.shape[1] // 20
    worst = {}
    for k, s in fields(J).items():
        a, b = got[:, s].astype(np.float64), want[:, s].astype(np.float64)
        if k in ("grs", "pad"):
            worst[k] = float(np.abs(a - b).max())
            ok = np.array_equal(got[:, s], want[:, s])
        else:
            tol = EPS32 * np.maximum(np.abs(b), 1.0)
            if k in ("gavs", "dvs"):
                tol = tol + ANG_FLOOR * (fps_frame / 30.0)[:, None]
            ratio = np.abs(a - b) / (scale * tol)
            worst[k] = float(ratio.max())
            ok = worst[k] <= 1.0
        print(f"{what} {k}: worst {'|diff|' if k in ('grs', 'pad') else '|diff| / tolerance'} = {worst[k]:.3e}")
        assert ok, (what, k, worst[k])
    return worst


def host_args(c, frames, scratch, keep):
    """phc_clip_args_t over numpy arrays (host memory: for the host build only).  `keep` collects the arrays the struct points into."""
    from phc_amd import abi
    nf = np.array([q.shape[0] for q in c["quats"]], dtype=np.int64)
    J = len(c["parents"])
    arrs = dict(parents=np.ascontiguousarray(c["parents"], dtype=np.int32), lt=np.ascontiguousarray(c["local_translations"], dtype=np.float64),
                tree=np.ascontiguousarray(c["clip_tree"], dtype=np.int32), start=np.concatenate([[0], np.cumsum(nf)]).astype(np.int64),
                dt=1.0 / np.asarray(c["fps"], dtype=np.float64), quat=np.ascontiguousarray(np.concatenate(c["quats"]), dtype=np.float64),
                trans=np.ascontiguousarray(np.concatenate(c["trans"]), dtype=np.float64))
    keep.append(arrs)
    return abi.clip_args_struct(len(nf), int(nf.sum()), J, arrs["lt"].shape[0], arrs["parents"], arrs["lt"], arrs["tree"], arrs["start"], arrs["dt"],
                                arrs["quat"], arrs["trans"], scratch, scratch.nbytes, frames)


def host_process(name, seed=0):
    """The two launches' per-lane functions looped over by the host build -> records [F, stride] float32 (guard words behind frames and scratch checked)."""
    c = make_case(name, seed)
    J, F_ = len(c["parents"]), int(sum(LENGTHS))
    sb = int(shim().clip_scratch_bytes_of(F_, J))
    frames = np.full(F_ * 20 * J + 4, np.float32(7.0), dtype=np.float32)
    frames[-4:].view(np.int32)[:] = GUARD
    scratch = np.zeros(sb // 8 + 2, dtype=np.float64)
    scratch[-2:].view(np.int64)[:] = GUARD
    keep = []
    a = host_args(c, frames[:-4].reshape(F_, 20 * J), scratch[:-2], keep)
    assert shim().clip_process_host(a) == 0
    assert (frames[-4:].view(np.int32) == GUARD).all() and (scratch[-2:].view(np.int64) == GUARD).all()
    return frames[:-4].reshape(F_, 20 * J).copy()
