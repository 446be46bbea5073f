"""Shared by tests/test_getup_device_cpu.py and tests/test_getup_device_gpu.py: the host build of phc_amd/csrc/phc_getup.h (tests/getup_shim.cpp, g++), the
caller-side state of one phc_getup_assign launch in host memory with guard words behind every array, and a numpy restatement of
HumanoidImGetup._reset_envs (phc_amd/env/tasks/humanoid_im_getup.py) fed with explicit uniforms and an explicit permutation -- the oracle of the rules."""
import copy
import ctypes as C
import functools

import numpy as np

import host_build

GUARD_WORDS = 16      # bytes-wise: 16 elements of the array's own type behind every array
GUARD_BYTE = 0x5A
KEY = 0x1234ABCD5678EF01
WAVE, BLOCK = 64, 1024   # wavefront size; GETUP_BLOCK (the scan tile), checked against the shim in the CPU tests
SIZES = (1, 2, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)   # the last spans three tiles
DONE_SETS = ("none", "all", "first", "last", "alternate")
# name -> dtype, shape(n, d); the order of phc_amd.abi.GETUP_ARRAYS
ARRAYS = {"prob": (np.float32, lambda n, d: (2,)), "reset_buf": (np.int64, lambda n, d: (n,)), "terminate_buf": (np.int64, lambda n, d: (n,)),
          "fall_root": (np.float32, lambda n, d: (n, 13)), "fall_dof_pos": (np.float32, lambda n, d: (n, d)), "root_states": (np.float32, lambda n, d: (n, 13)),
          "dof_state": (np.float32, lambda n, d: (n, d, 2)), "avail": (np.int64, lambda n, d: (n,)), "assign": (np.int64, lambda n, d: (n,)),
          "recovery_counter": (np.int32, lambda n, d: (n,)), "k": (np.int32, lambda n, d: (n,)), "launch_count": (np.int64, lambda n, d: (1,)),
          "kind": (np.int32, lambda n, d: (n,)), "normal_flag": (np.int64, lambda n, d: (n,)), "fall_list": (np.int64, lambda n, d: (n,)),
          "free_list": (np.int32, lambda n, d: (n,))}
OUTPUTS = ("root_states", "dof_state", "avail", "assign", "recovery_counter", "k", "launch_count", "kind", "normal_flag", "fall_list")   # free_list is scratch


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("getup_shim.cpp", "phc_getup.hip")
    for name, args, res in (("getup_sizeof_args", [], C.c_int), ("getup_block", [], C.c_int), ("getup_max_envs", [], C.c_int),
                            ("getup_draws_batch", [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_void_p], None),
                            ("getup_perm_of", [C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p], None),
                            ("getup_args_check_of", [C.POINTER(L.GetupArgs)], C.c_int),
                            ("task_draws_check_of", [C.c_int32, C.c_int64, C.c_void_p], C.c_int),
                            ("getup_assign_host_of", [C.POINTER(L.GetupArgs), C.c_void_p, C.c_void_p], None),
                            ("task_draws_host", [C.c_int32, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p], None)):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    return lib


def draws(key, env0, n_env, k0, n_k):
    out = np.zeros((n_k, n_env, 2), dtype=np.float32)
    shim().getup_draws_batch(key, env0, n_env, k0, n_k, out.ctypes.data)
    return out


def perm(key, count, F):
    out = np.zeros(F, dtype=np.int32)
    shim().getup_perm_of(key, count, F, out.ctypes.data)
    return out


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


class GetupState:
    """Everything phc_getup_args_t points at, in host memory.  Every array is the head of a backing buffer that ends in GUARD_WORDS guard elements."""

    def __init__(self, n, d=3, seed=0, key=KEY, env_offset=0, recovery_steps=8, prob=(0.5, 0.5), holders=0.5, done="alternate", terminate="mixed"):
        rng = np.random.default_rng(seed)
        self.n, self.d, self.key, self.env_offset, self.recovery_steps = n, d, key, env_offset, recovery_steps
        self.back = {}
        for name, (dtype, shape) in ARRAYS.items():
            size = int(np.prod(shape(n, d)))
            b = np.zeros(size + GUARD_WORDS, dtype=dtype)
            b.view(np.uint8)[size * b.itemsize:] = GUARD_BYTE
            self.back[name] = b
        for name in ("fall_root", "fall_dof_pos", "root_states", "dof_state"):
            self[name][...] = rng.standard_normal(self[name].shape).astype(np.float32)
        self["prob"][:] = prob
        self["reset_buf"][:] = done_mask(n, done) if isinstance(done, str) else done
        self["terminate_buf"][:] = {"zeros": np.zeros(n), "ones": np.ones(n), "mixed": rng.integers(0, 2, n)}[terminate]
        # a consistent pool: a random subset of the envs holds distinct random slots, the others never held one (assign 0)
        hold = rng.random(n) < holders
        slots = rng.permutation(n)[:int(hold.sum())]
        self["assign"][hold] = slots
        self["avail"][slots] = 1
        self["recovery_counter"][:] = rng.integers(0, 5, n)
        self["k"][:] = rng.integers(0, 100, n)
        self["launch_count"][0] = 41
        for name, fill in (("kind", 9), ("normal_flag", 9), ("fall_list", -7), ("free_list", -7)):   # stale outputs
            self[name][:] = fill

    def __getitem__(self, name):
        dtype, shape = ARRAYS[name]
        shp = shape(self.n, self.d)
        return self.back[name][:int(np.prod(shp))].reshape(shp)

    def clone(self):
        return copy.deepcopy(self)

    def args(self, pointers=None):
        """phc_getup_args_t over this state's host memory, or over `pointers` (name -> raw address: the device copies of the GPU tests)."""
        from phc_amd import abi
        p = pointers or {name: self.back[name].ctypes.data for name in ARRAYS}
        return abi.getup_args_struct(self.n, self.d, self.key, env_offset=self.env_offset, recovery_steps=self.recovery_steps, **{k: int(p[k]) for k in ARRAYS})

    def run_host(self, u=None, perm_given=None):
        """The host build of the launch, in place."""
        u = None if u is None else np.ascontiguousarray(u, dtype=np.float32)
        pg = None if perm_given is None else np.ascontiguousarray(perm_given, dtype=np.int32)
        assert u is None or u.shape == (self.n, 2)
        shim().getup_assign_host_of(self.args(), None if u is None else u.ctypes.data, None if pg is None else pg.ctypes.data)

    def guards_intact(self):
        return all((b.view(np.uint8)[-GUARD_WORDS * b.itemsize:] == GUARD_BYTE).all() for b in self.back.values())

    def free_after_release(self):
        """The slots free once every done env released its own, in slot order (what the explicit permutation of a test indexes)."""
        avail = self["avail"].copy()
        held = self["assign"][self["reset_buf"] != 0]
        avail[held[(held >= 0) & (held < self.n)]] = 0
        return np.flatnonzero(avail == 0)


def oracle(state, u, perm_given):
    """HumanoidImGetup._reset_envs(reset_buf.nonzero()) of phc_amd/env/tasks/humanoid_im_getup.py in numpy, up to the reset launches, on a clone of `state`:
    torch.bernoulli(p) == 1 is `u < p` of the given uniform, `free[torch.randperm(F)][:n_f]` is `free[perm_given[:n_f]]`.  The zeroing of the NORMAL envs'
    recovery counters is the reset launch's (phc_im_reset_done), not this function's.  -> (the clone, kind [N])."""
    s = state.clone()
    n = s.n
    env_ids = np.flatnonzero(s["reset_buf"] != 0)
    kind = np.zeros(n, dtype=np.int32)
    if len(env_ids) == 0:
        return s, kind
    held = s["assign"][env_ids]
    s["avail"][held[(held >= 0) & (held < n)]] = 0    # (torch would raise on an index outside [0, N): the launch releases nothing there)
    p_recovery, p_fall = s["prob"]
    want_recovery = u[env_ids, 0] < p_recovery
    recovery_mask = want_recovery & (s["terminate_buf"][env_ids] == 1)
    recovery_ids, rest = env_ids[recovery_mask], env_ids[~recovery_mask]
    fall_mask = u[rest, 1] < p_fall
    fall_ids, normal_ids = rest[fall_mask], rest[~fall_mask]
    if len(fall_ids) > 0:
        free = np.flatnonzero(s["avail"] == 0)
        assert free.shape[0] >= fall_ids.shape[0]
        pick = free[np.asarray(perm_given)[:fall_ids.shape[0]]]
        s["root_states"][fall_ids] = s["fall_root"][pick]
        s["dof_state"][fall_ids, :, 0] = s["fall_dof_pos"][pick]
        s["dof_state"][fall_ids, :, 1] = 0
        s["avail"][pick] = 1
        s["assign"][fall_ids] = pick
    s["recovery_counter"][np.concatenate([fall_ids, recovery_ids])] = s.recovery_steps
    kind[normal_ids], kind[recovery_ids], kind[fall_ids] = 1, 2, 3
    return s, kind


def assert_equal_states(a, b, what=""):
    """Bit equality of every output array (and of the inputs, which a launch must leave alone), guard words included."""
    for name in ARRAYS:
        if name == "free_list":
            continue
        x, y = a.back[name].view(np.uint8), b.back[name].view(np.uint8)
        assert np.array_equal(x, y), f"{what}{name}: {np.flatnonzero(x != y)[:8]} (byte offsets) differ"
