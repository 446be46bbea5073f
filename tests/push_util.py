"""Shared by tests/test_push_device_cpu.py and tests/test_push_device_gpu.py: the host build of phc_amd/csrc/phc_push.h (tests/push_shim.cpp, g++) and a
numpy-backed caller of it with the state layout of phc_push_args_t."""
import ctypes as C
import functools

import numpy as np

import host_build

GUARD = 0x5A5A5A5A   # int32 guard word; as float bits 1.5e16


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("push_shim.cpp", "phc_push.hip")
    lib.push_draws_batch.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    lib.push_draws_batch.restype = None
    lib.push_args_check_of.argtypes = [C.POINTER(L.PushArgs)]
    lib.push_args_check_of.restype = C.c_int
    lib.push_pause_of.argtypes = [C.POINTER(L.PushArgs), C.c_float]
    lib.push_pause_of.restype = C.c_int
    lib.push_step_given.argtypes = [C.POINTER(L.PushArgs), C.c_void_p, C.c_void_p]
    lib.push_step_given.restype = None
    lib.push_advance_host.argtypes = [C.POINTER(L.PushArgs)]
    lib.push_advance_host.restype = None
    return lib


def draws(key, env0, n_env, k0, n_k):
    out = np.zeros((n_k, n_env, 5), dtype=np.float32)
    shim().push_draws_batch(key, env0, n_env, k0, n_k, out.ctypes.data)
    return out


class HostPush:
    """Caller-side state of one schedule in host memory, stepped by the host build."""

    def __init__(self, n, nb, listed, pause=(6, 12), duration=3, direction=0, force=(200.0, 400.0), key=0x1234ABCD5678EF01, env_offset=0):
        from phc_amd import _lib as L
        self.n, self.nb = n, nb
        self.bodies = np.asarray(listed, dtype=np.int32)
        self.state = np.zeros((5, n), dtype=np.int32)   # remaining, countdown, body, k, started
        self.state[2] = -1
        self.force = np.zeros((n, nb, 3), dtype=np.float32)
        a = L.PushArgs()
        a.num_envs, a.num_bodies, a.num_listed = n, nb, len(listed)
        a.pause_lo, a.pause_hi = pause
        a.duration, a.direction = duration, direction
        a.force_lo, a.force_hi = force
        a.key, a.env_offset = key, env_offset
        a.bodies, a.force = self.bodies.ctypes.data, self.force.ctypes.data
        for i, name in enumerate(("remaining", "countdown", "body", "k", "started")):
            setattr(a, name, self.state[i].ctypes.data)
        self.args = a

    remaining = property(lambda self: self.state[0])
    countdown = property(lambda self: self.state[1])
    body = property(lambda self: self.state[2])
    started = property(lambda self: self.state[4])

    def advance(self, progress=None):
        p = None if progress is None else np.ascontiguousarray(progress, dtype=np.int64)
        self.args.progress_buf = None if p is None else p.ctypes.data
        shim().push_advance_host(self.args)
        self.args.progress_buf = None

    def step_given(self, u, reset):
        u = np.ascontiguousarray(u, dtype=np.float32)
        r = np.ascontiguousarray(reset, dtype=np.uint8)
        assert u.shape == (5, self.n) and r.shape == (self.n,)
        shim().push_step_given(self.args, u.ctypes.data, r.ctypes.data)

    def pause_of(self, u0):
        return shim().push_pause_of(self.args, float(u0))
