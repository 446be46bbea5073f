"""Shared by tests/test_obs_aug_cpu.py and tests/test_obs_aug_gpu.py: the host build of phc_amd/csrc/phc_obs_aug.h (tests/obs_aug_shim.cpp, g++), the caller-side
state of one phc_obs_augment / phc_occl_advance launch in host memory with guard elements behind every array, and two oracles: a numpy restatement of
HumanoidIm._fut_dropout + _add_obs_noise and of _update_occl_training (phc_amd/env/tasks/humanoid_im.py) fed with explicit uniforms / normals -- the oracle of
the rules -- and an fp64 Box-Muller on the same 24-bit integers -- the oracle of the noise values."""
import copy
import ctypes as C
import functools

import numpy as np

import host_build

GUARD = 16            # guard elements of the array's own type behind every array
GUARD_BYTE = 0x5A
KEY = 0x0F1E2D3C4B5A6978
OCCL_KEY = 0x8796A5B4C3D2E1F0
BLOCK = 256           # OBS_AUG_BLOCK: column pairs per workgroup pass, checked against the shim in the CPU tests
R_MAX = 5.77          # sqrt(-2 ln 2^-24) = 5.768
DONE_SETS = ("none", "all", "first", "last", "alternate")
# (N, num_obs, so, T, dropout_p, noise_std): a sparse product of N in (1, 2, 63, 64, 65, 257), num_obs in (1, 2, 7, 255, 256, 257, 513, 1025) -- odd and even
# widths, fewer pairs than a wavefront, one pair more than a workgroup pass (513 -> 257 pairs), more than one pass -- so in (0, 1, num_obs), T in (1, 3) where the
# tail divides, dropout_p in (0, 0.1, 1), noise_std in (0, 0.1)
CASES = ((1, 1, 0, 1, 0.0, 0.1), (2, 2, 1, 1, 0.1, 0.1), (63, 7, 1, 3, 0.1, 0.1), (64, 255, 0, 3, 1.0, 0.1), (65, 256, 1, 3, 0.1, 0.1), (257, 257, 257, 1, 0.1, 0.1),
         (2, 513, 0, 3, 0.1, 0.0), (65, 1025, 1, 1, 0.0, 0.1), (63, 1025, 1025, 3, 1.0, 0.1), (257, 7, 1, 3, 1.0, 0.0), (64, 513, 0, 3, 0.1, 0.1), (1, 257, 1, 1, 0.1, 0.1),
         (2, 255, 0, 3, 0.1, 0.1), (65, 2, 0, 1, 0.0, 0.0), (64, 256, 1, 3, 0.0, 0.1), (257, 1, 1, 3, 0.1, 0.1))
OCCL_N, OCCL_J = (1, 63, 64, 65, 257), (1, 9, 24, 25, 64)


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("obs_aug_shim.cpp", "phc_obs_aug.hip")
    p, i32, i64, u64, f = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float
    for name, args, res in (("obs_aug_sizeof_args", [], C.c_int), ("obs_aug_block", [], C.c_int), ("obs_aug_max_obs", [], C.c_int),
                            ("obs_aug_max_samples", [], C.c_int), ("occl_max_bodies", [], C.c_int),
                            ("aug_uniforms_rows", [u64, p, p, C.c_int, C.c_uint32, C.c_int, p], None),
                            ("aug_normals_rows", [u64, p, p, C.c_int, C.c_int, p], None),
                            ("aug_box_muller_of", [f, f, p], None),
                            ("obs_augment_check_of", [C.POINTER(L.ObsAugArgs)], C.c_int),
                            ("occl_advance_check_of", [i32, i32, i64, p, f, i32, i32, p, p], C.c_int),
                            ("obs_augment_host_of", [C.POINTER(L.ObsAugArgs)], None),
                            ("occl_advance_host_of", [i32, i32, u64, i64, p, f, i32, i32, p, p], None)):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    return lib


# ---- draws of the host build ---------------------------------------------------------------------------------------------------------------------------
def uniforms(key, genv, ks, index0, n_index):
    """-> [n, n_index, 2] fp32: u(index0 + i, which) of the global envs `genv` at the counts `ks`."""
    genv, ks = np.ascontiguousarray(genv, dtype=np.int64), np.ascontiguousarray(ks, dtype=np.int32)
    out = np.zeros((len(genv), n_index, 2), dtype=np.float32)
    shim().aug_uniforms_rows(key, genv.ctypes.data, ks.ctypes.data, len(genv), index0, n_index, out.ctypes.data)
    return out


def normals(key, genv, ks, num_obs):
    """-> [n, num_obs] fp32: the host build's normals of one call on each of the global envs `genv` at the counts `ks`."""
    genv, ks = np.ascontiguousarray(genv, dtype=np.int64), np.ascontiguousarray(ks, dtype=np.int32)
    out = np.zeros((len(genv), num_obs), dtype=np.float32)
    shim().aug_normals_rows(key, genv.ctypes.data, ks.ctypes.data, len(genv), num_obs, out.ctypes.data)
    return out


def box_muller(a, b):
    out = np.zeros(2, dtype=np.float32)
    shim().aug_box_muller_of(float(a), float(b), out.ctypes.data)
    return out


def normals_f64(key, genv, ks, num_obs):
    """The fp64 Box-Muller on the same 24-bit integers -> (z [n, num_obs] fp64, r [n, num_obs] fp64: the pair's radius at each column)."""
    P = (num_obs + 1) // 2
    u = uniforms(key, genv, ks, 0, P).astype(np.float64)
    ia, ib = np.rint(u[..., 0] * 2 ** 24), np.rint(u[..., 1] * 2 ** 24)      # exact: the uniforms are multiples of 2^-24
    assert np.array_equal(ia / 2 ** 24, u[..., 0]) and np.array_equal(ib / 2 ** 24, u[..., 1])
    r = np.sqrt(-2.0 * np.log(1.0 - ia / 2 ** 24))
    theta = 2.0 * np.pi * (ib / 2 ** 24)
    z = np.stack([r * np.cos(theta), r * np.sin(theta)], axis=-1).reshape(len(u), 2 * P)[:, :num_obs]
    return z, np.repeat(r, 2, axis=1)[:, :num_obs]


def noise_bound(value, r, noise_std):
    """E = 2^-23 |o'| + noise_std r 2^-19 of a noised element against the fp64 oracle: one fp32 rounding of the sum; theta = 2 pi b rounded in fp32 (<= 7.5e-7
    absolute, <= 1e-6 on cos / sin with a 2-ulp library), r relative to about 2^-22 -- together below 1.2e-6 r, and 2^-19 r is about 1.6 times that."""
    return 2.0 ** -23 * np.abs(value) + noise_std * r * 2.0 ** -19


def done_mask(n, which):
    m = np.zeros(n, dtype=bool)
    if which == "all":
        m[:] = True
    elif which == "first":
        m[0] = True
    elif which == "last":
        m[-1] = True
    elif which == "alternate":
        m[::2] = True
    else:
        assert which == "none"
    return m


class _Guarded:
    """Arrays in host memory, each the head of a backing buffer that ends in GUARD guard elements."""
    ARRAYS = {}

    def _alloc(self):
        self.back = {}
        for name, (dtype, shape) in self.ARRAYS.items():
            size = int(np.prod(shape(self)))
            b = np.zeros(size + GUARD, dtype=dtype)
            b.view(np.uint8)[size * b.itemsize:] = GUARD_BYTE
            self.back[name] = b

    def __getitem__(self, name):
        shp = self.ARRAYS[name][1](self)
        return self.back[name][:int(np.prod(shp))].reshape(shp)

    def clone(self):
        return copy.deepcopy(self)

    def guards_intact(self):
        return all((b.view(np.uint8)[-GUARD * b.itemsize:] == GUARD_BYTE).all() for b in self.back.values())

    def pointers(self):
        return {name: b.ctypes.data for name, b in self.back.items()}


class AugState(_Guarded):
    """Everything phc_obs_aug_args_t points at.  `form`: "all", "flag" (`select` = a done-set name or a bool mask) or "ids" (`select` = the id list)."""
    ARRAYS = {"obs": (np.float32, lambda s: (s.n, s.num_obs)), "k": (np.int32, lambda s: (s.n,)), "row_flag": (np.int64, lambda s: (s.n,)),
              "env_ids": (np.int64, lambda s: (s.n_ids,))}

    def __init__(self, n, num_obs, so, T, dropout_p, noise_std, form="all", select=None, seed=0, key=KEY, env_offset=0):
        rng = np.random.default_rng(seed)
        self.n, self.num_obs, self.so, self.T, self.dropout_p, self.noise_std = n, num_obs, so, T, dropout_p, noise_std
        self.form, self.key, self.env_offset = form, key, env_offset
        ids = np.asarray(select if form == "ids" else [], dtype=np.int64)
        self.n_ids = len(ids)
        self._alloc()
        self["obs"][...] = rng.standard_normal((n, num_obs)).astype(np.float32)
        self["k"][:] = rng.integers(0, 100, n)
        if form == "flag":
            mask = done_mask(n, select) if isinstance(select, str) else np.asarray(select)
            self["row_flag"][:] = np.where(mask, rng.integers(1, 5, n), 0)    # any non-zero value selects
        self["env_ids"][:] = ids

    def rows(self):
        """The selected envs, in the order the launch's slots list them."""
        if self.form == "ids":
            return self["env_ids"].copy()
        return np.flatnonzero(self["row_flag"] != 0) if self.form == "flag" else np.arange(self.n)

    def args(self, pointers=None):
        from phc_amd import abi
        p = pointers or self.pointers()
        a = abi.obs_aug_args_struct(int(p["obs"]), int(p["k"]), self.so, self.T, self.dropout_p, self.noise_std, self.key, env_offset=self.env_offset,
                                    row_flag=int(p["row_flag"]) if self.form == "flag" else None, env_ids=int(p["env_ids"]) if self.form == "ids" else None,
                                    num_envs=self.n, num_obs=self.num_obs, n_ids=self.n_ids)
        return a

    def run_host(self):
        shim().obs_augment_host_of(self.args())


class OcclState(_Guarded):
    ARRAYS = {"k": (np.int32, lambda s: (s.n,)), "count": (np.int64, lambda s: (s.n, s.J)), "mask": (np.uint8, lambda s: (s.n, s.J))}

    def __init__(self, n, J, prob=0.1, span=(30, 60), seed=0, key=OCCL_KEY, env_offset=0):
        rng = np.random.default_rng(seed)
        self.n, self.J, self.prob, self.span, self.key, self.env_offset = n, J, prob, span, key, env_offset
        self._alloc()
        self["k"][:] = rng.integers(0, 100, n)
        self["count"][...] = rng.integers(0, 4, (n, J)) * rng.integers(0, 20, (n, J))   # zeros, ones and running spans
        self["mask"][...] = 7                                                           # stale

    def call(self, fn, pointers=None, *tail):
        p = pointers or self.pointers()
        return fn(self.n, self.J, self.key, self.env_offset, int(p["k"]), self.prob, self.span[0], self.span[1], int(p["count"]), int(p["mask"]), *tail)

    def run_host(self):
        self.call(shim().occl_advance_host_of)


# ---- the oracle of the rules ---------------------------------------------------------------------------------------------------------------------------
def oracle_augment(state, u_drop, z):
    """HumanoidIm._fut_dropout + _add_obs_noise of phc_amd/env/tasks/humanoid_im.py in numpy on a clone of `state`, for the rows `state.rows()`:
    `torch.rand((rows, T)) >= p` is `u_drop >= p` of the given uniforms [rows, T], `torch.randn((rows, num_obs))` is `z`.  -> the clone."""
    s = state.clone()
    rows, so, T = s.rows(), s.so, s.T
    obs = s["obs"]
    if T > 1 and s.dropout_p > 0 and len(rows) > 0:
        keep = (u_drop >= np.float32(s.dropout_p)).astype(np.float32)
        blocks = obs[rows, so:].reshape(len(rows), T, -1) * keep[:, :, None]
        obs[rows, so:] = blocks.reshape(len(rows), -1)
    if s.noise_std > 0 and len(rows) > 0:
        obs[rows] = obs[rows] + z.astype(np.float32) * np.float32(s.noise_std)
    s["k"][rows] += 1
    return s


def oracle_occl(state, u, v):
    """HumanoidIm._update_occl_training in numpy on a clone: torch.bernoulli(prob) is `u < prob`, torch.randint(lo, hi) is lo + floor(v (hi - lo)) clamped
    to hi - 1 (u, v [N, J]).  The overwrite of the mask is the reference's (humanoid_im.py:1091-1092)."""
    s = state.clone()
    lo, hi = s.span
    start = u < np.float32(s.prob)
    start[:, 0] = False
    spans = np.minimum(lo + np.floor(v * np.float32(hi - lo)).astype(np.int64), hi - 1)
    s["count"][...] = np.maximum(np.where(start, spans, s["count"]) - 1, 0)
    idx = s["count"] > 0
    idx[:] = True
    idx[:, 9:24] = False
    s["mask"][...] = idx
    s["k"][:] += 1
    return s, start, spans


def draws_of(state):
    """The host build's draws for one call on `state`: (u_drop [rows, T], z fp32 [rows, num_obs], z fp64, r fp64)."""
    rows = state.rows()
    genv, ks = state.env_offset + rows, state["k"][rows]
    P = (state.num_obs + 1) // 2
    u_drop = uniforms(state.key, genv, ks, P, max(state.T, 1))[:, :, 0]
    z64, r = normals_f64(state.key, genv, ks, state.num_obs)
    return u_drop, normals(state.key, genv, ks, state.num_obs), z64, r


def assert_bytes_equal(a, b, names, what=""):
    for name in names:
        x, y = a.back[name].view(np.uint8), b.back[name].view(np.uint8)
        assert np.array_equal(x, y), f"{what}{name}: {np.flatnonzero(x != y)[:8]} (byte offsets) differ"


def check_call(before, after, what="", same_library=False):
    """`after` is `before` one phc_obs_augment call later (host build or device).  Counters, dropout decisions, zeroed blocks, untouched rows, inputs and
    guard elements exact; every noised element within `noise_bound` of the fp64 oracle -- and, for the host build (`same_library`: the oracle's fp32 normals
    come from the same libm), equal to the numpy restatement.  -> the largest error of a noised element as a fraction of its bound (0 without noise)."""
    u_drop, z32, z64, r = draws_of(before)
    want = oracle_augment(before, u_drop, z32)
    rows = before.rows()
    assert after.guards_intact(), what
    assert_bytes_equal(after, before, ("row_flag", "env_ids"), what)
    assert np.array_equal(after["k"], want["k"]), what
    rest = np.setdiff1d(np.arange(before.n), rows)
    assert np.array_equal(after["obs"][rest].view(np.uint32), before["obs"][rest].view(np.uint32)), what + "an unselected row changed"
    if len(rows) == 0:
        return 0.0
    dropped = np.zeros((len(rows), before.num_obs), dtype=bool)
    if before.T > 1 and before.dropout_p > 0 and before.so < before.num_obs:
        W = (before.num_obs - before.so) // before.T
        dropped[:, before.so:] = np.repeat(u_drop < np.float32(before.dropout_p), W, axis=1)
    got = after["obs"][rows]
    if not before.noise_std > 0:
        assert (got.view(np.uint32)[dropped] == 0).all(), what + "a dropped column is not +0.0f"
        assert np.array_equal(got.view(np.uint32)[~dropped], before["obs"][rows].view(np.uint32)[~dropped]), what + "a kept column changed"
        assert np.array_equal(got, want["obs"][rows]), what
        return 0.0
    if same_library:
        assert np.array_equal(got, want["obs"][rows]), what + "the host build differs from the numpy restatement"
    base = np.where(dropped, 0.0, before["obs"][rows].astype(np.float64))
    ref = base + float(np.float32(before.noise_std)) * z64
    ratio = np.abs(got.astype(np.float64) - ref) / noise_bound(got.astype(np.float64), r, float(np.float32(before.noise_std)))
    assert np.isfinite(got).all() and float(ratio.max()) <= 1.0, f"{what}error / bound = {float(ratio.max()):.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return float(ratio.max())
