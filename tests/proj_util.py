"""Shared by tests/test_projectile_cpu.py and tests/test_projectile_gpu.py: the host build of phc_amd/csrc/phc_proj.h (tests/proj_shim.cpp, g++), a
numpy-backed caller of it with the state layout of phc_proj_args_t and guard words behind every array, posed body states, and `Oracle`: the rules of
include/phc_amd.h (phc_proj_advance) stated in fp64 numpy, from the rules and not from the header's code.  The oracle takes the uniforms of the draws
from the host build (they are exact fp32 numbers; their law is tested on its own) and the same fp32 inputs, upcast."""
import ctypes as C
import functools
import math

import numpy as np

import host_build

GUARD = 0x5A5A5A5A   # int32 guard word; as float bits 1.5e16
PAD = 16
INT_NAMES = ("life", "countdown", "thrown", "hits", "last_hit")
U32 = 2.0 ** -24     # fp32 unit round-off


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("proj_shim.cpp", "phc_proj.hip")
    lib.proj_draws_batch.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    lib.proj_draws_batch.restype = None
    lib.proj_args_check_of.argtypes = [C.POINTER(L.ProjArgs)]
    lib.proj_args_check_of.restype = C.c_int
    lib.proj_pause_of.argtypes = [C.POINTER(L.ProjArgs), C.c_float]
    lib.proj_pause_of.restype = C.c_int
    lib.proj_rows_check_of.argtypes = [C.POINTER(L.ProjRows)]
    lib.proj_rows_check_of.restype = C.c_int
    lib.proj_rows_host.argtypes = [C.POINTER(L.ProjRows)]
    lib.proj_rows_host.restype = None
    lib.proj_advance_host.argtypes = [C.POINTER(L.ProjArgs), C.c_void_p]
    lib.proj_advance_host.restype = None
    return lib


def draws(key, env0, n_env, k0, n_k, slot):
    out = np.zeros((n_k, n_env, 8), dtype=np.float32)
    shim().proj_draws_batch(key, env0, n_env, k0, n_k, slot, out.ctypes.data)
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    from phc_amd.model import load_model
    return load_model(name)


def tables(m):
    from phc_amd.projectile import model_tables
    return model_tables(m)


def quat_rot(q, v):
    """Rotation of v by the unit quaternion q (xyzw), fp64."""
    qv, w = q[..., :3], q[..., 3:4]
    t = 2.0 * np.cross(qv, v)
    return v + w * t + np.cross(qv, t)


def posed_rbs(m, n, seed=0, tilt=0.3, vel=0.3, ang=0.5, height=0.95):
    """[n, NB, 13] float32: the bodies at their rest offsets below a root at `height`, each turned by a small random rotation and given small random
    velocities -- any rows are valid input of the launch (it reads body states, it does not ask that they fit a joint)."""
    rng = np.random.default_rng(seed)
    nb = m.num_bodies
    pos = np.zeros((nb, 3))
    for i in range(1, nb):
        pos[i] = pos[m.parent[i]] + m.local_translation[i]
    rbs = np.zeros((n, nb, 13))
    rbs[..., 0:3] = pos + np.array([0.0, 0.0, height]) + rng.normal(0, 0.02, (n, 1, 3))
    axis = rng.normal(size=(n, nb, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * tilt * rng.uniform(-1, 1, (n, nb, 1))
    rbs[..., 3:6], rbs[..., 6:7] = axis * np.sin(half), np.cos(half)
    rbs[..., 7:10] = rng.normal(0, vel, (n, nb, 3))
    rbs[..., 10:13] = rng.normal(0, ang, (n, nb, 3))
    return rbs.astype(np.float32)


def _guarded(shape, dtype, fill=0):
    n = int(np.prod(shape))
    buf = np.full(n + PAD, GUARD, dtype=np.int32)
    view = buf[:n].view(dtype).reshape(shape)
    view[...] = fill
    return buf, view


DEFAULTS = dict(count=1, pause=(3, 6), life_steps=60, substeps=8, dt=1 / 30, gravity_z=-9.81, radius=0.1, restitution=0.2, friction=1.0, mass=(1.0, 5.0),
                speed=(5.0, 10.0), dist=(2.0, 4.0), elev=(0.0, math.pi / 6), key=0x1234ABCD5678EF01, env_offset=0, listed=(0,))


def fill_args(a, n, m, tab, **kw):
    o = dict(DEFAULTS, **kw)
    a.num_envs, a.num_bodies, a.num_shapes, a.num_listed, a.count = n, m.num_bodies, len(tab["owner"]), len(o["listed"]), o["count"]
    a.pause_lo, a.pause_hi = o["pause"]
    a.life_steps, a.substeps, a.dt, a.gravity_z = o["life_steps"], o["substeps"], o["dt"], o["gravity_z"]
    a.radius, a.restitution, a.friction = o["radius"], o["restitution"], o["friction"]
    (a.mass_lo, a.mass_hi), (a.speed_lo, a.speed_hi), (a.dist_lo, a.dist_hi), (a.elev_lo, a.elev_hi) = o["mass"], o["speed"], o["dist"], o["elev"]
    a.key, a.env_offset = o["key"], o["env_offset"]
    return o


class HostProj:
    """Caller-side state of one schedule in host memory, every written array followed by guard words; stepped by the host build."""

    def __init__(self, m, n, rbs, capsules=None, **kw):
        from phc_amd import _lib as L
        self.m, self.n, self.nb = m, n, m.num_bodies
        self.tab = dict(tables(m))
        if capsules is not None:
            self.tab["capsules"] = np.ascontiguousarray(capsules, dtype=np.float32)
        self.rbs = np.ascontiguousarray(rbs, dtype=np.float32).reshape(n, self.nb, 13)
        a = self.args = L.ProjArgs()
        self.opt = fill_args(a, n, m, self.tab, **kw)
        P = self.P = self.opt["count"]
        self.bodies = np.asarray(self.opt["listed"], dtype=np.int32)
        self._bufs = {}
        for name in INT_NAMES:
            self._bufs[name], v = _guarded((P, n), np.int32, -1 if name == "last_hit" else 0)
            setattr(self, name, v)
        self._bufs["k"], self.k = _guarded((n,), np.int32)
        self._bufs["pos"], self.pos = _guarded((P, n, 3), np.float32)
        self._bufs["vel"], self.vel = _guarded((P, n, 3), np.float32)
        self._bufs["mass"], self.mass = _guarded((P, n), np.float32)
        self._bufs["force"], self.force = _guarded((n, self.nb, 3), np.float32)
        self._bufs["torque"], self.torque = _guarded((n, self.nb, 3), np.float32)
        self.pos[..., 2] = -1000.0
        t = self.tab
        a.bodies, a.capsules, a.owner = self.bodies.ctypes.data, t["capsules"].ctypes.data, t["owner"].ctypes.data
        a.body_com, a.body_inv_mass, a.body_inv_inertia = t["com"].ctypes.data, t["inv_mass"].ctypes.data, t["inv_inertia"].ctypes.data
        a.rigid_body_state = self.rbs.ctypes.data
        for name in INT_NAMES + ("k", "pos", "vel", "mass", "force", "torque"):
            setattr(a, name, getattr(self, name).ctypes.data)

    def advance(self, progress=None, margin=None):
        p = None if progress is None else np.ascontiguousarray(progress, dtype=np.int64)
        self.args.progress_buf = None if p is None else p.ctypes.data
        shim().proj_advance_host(self.args, None if margin is None else margin.ctypes.data)
        self.args.progress_buf = None

    def guards_intact(self):
        return all((b[-PAD:] == GUARD).all() for b in self._bufs.values())

    def place(self, slot, env, x, v, mass, life=5, countdown=9):
        """Put a flying projectile into a slot (the state a throw would have left)."""
        self.life[slot, env], self.countdown[slot, env] = life, countdown
        self.pos[slot, env], self.vel[slot, env], self.mass[slot, env] = x, v, mass

    def started(self):
        """Mark the schedule as past its first launch (k > 0: no reset unless progress says so)."""
        self.k[:] = 1
        self.countdown[:] = 1 << 20


def rows_case(n=5, count=2, widths=(13, 7, 1), seed=0):
    """Tensor pairs for phc_proj_rows with guard words behind every array: -> (base list, shadow list, last_hit [P, N], buffers), envs 1 and n - 1 struck."""
    rng = np.random.default_rng(seed)
    bufs, base, shadow = [], [], []
    for w in widths:
        for dst, lo in ((base, 0.0), (shadow, 100.0)):
            b, v = _guarded((n, w), np.float32)
            v[...] = lo + rng.random((n, w), dtype=np.float32)
            bufs.append(b)
            dst.append(v)
    b, last_hit = _guarded((count, n), np.int32, -1)
    bufs.append(b)
    last_hit[0, 1], last_hit[count - 1, n - 1] = 3, 0   # (shape 0 is a hit too)
    return base, shadow, last_hit, bufs


def rows_args(base_ptrs, shadow_ptrs, widths, last_hit_ptr, n, count, mode):
    from phc_amd import _lib as L
    a = L.ProjRows()
    a.num_envs, a.count, a.num_sets, a.mode, a.last_hit = n, count, len(widths), mode, last_hit_ptr
    for i, w in enumerate(widths):
        a.base[i], a.shadow[i], a.width[i] = base_ptrs[i], shadow_ptrs[i], w
    return a


class Oracle:
    """The rules in fp64.  Built from a HostProj: takes over its parameters (as the fp32 numbers the launch is handed), tables, body states and its
    current slot state.  `margin` [N] after a step: the least margin of the tests whose flip alone would change a decision -- |gap| (m) of a shape the
    sphere approaches (vn < 0), |vn| (m/s) of a shape it overlaps, |x.z - radius| while it falls, |v.z| while it is below the ground's contact height."""

    def __init__(self, h):
        a = h.args
        self.h, self.n, self.nb, self.P = h, h.n, h.nb, h.P
        for f in ("pause_lo", "pause_hi", "life_steps", "substeps", "dt", "gravity_z", "radius", "restitution", "friction", "mass_lo", "mass_hi", "speed_lo",
                  "speed_hi", "dist_lo", "dist_hi", "elev_lo", "elev_hi", "key", "env_offset", "num_listed"):
            setattr(self, f, getattr(a, f))
        self.tab = {k: v.astype(np.float64) if v.dtype == np.float32 else v.copy() for k, v in h.tab.items()}
        self.bodies = h.bodies.copy()
        for name in INT_NAMES + ("k",):
            setattr(self, name, getattr(h, name).astype(np.int64))
        for name in ("pos", "vel", "mass"):
            setattr(self, name, getattr(h, name).astype(np.float64))
        self.force, self.torque = np.zeros((self.n, self.nb, 3)), np.zeros((self.n, self.nb, 3))
        self.margin = np.full(self.n, np.inf)
        self.hit_log = []   # (env, slot, shape, j, n, r, dist) of every hit of the last step

    def _pause(self, u0):
        span = self.pause_hi - self.pause_lo   # (an integer decision on fp32 numbers: the product in fp32, as the contract's floor is)
        return self.pause_lo + min(int(np.floor(np.float32(u0) * np.float32(span + 1))), span)

    def step(self, progress=None):
        rbs = self.h.rbs.astype(np.float64)
        cap, owner = self.tab["capsules"], self.tab["owner"]
        g, R, e_, h = self.gravity_z, self.radius, self.restitution, self.dt / self.substeps
        self.force[:], self.torque[:], self.margin[:], self.hit_log = 0.0, 0.0, np.inf, []
        active = cap[:, 6] > 0
        for env in range(self.n):
            k = int(self.k[env])
            reset = k == 0 or (progress is not None and progress[env] == 0)
            B = rbs[env]
            x_b, q_b, v_b, w_b = B[owner, 0:3], B[owner, 3:7], B[owner, 7:10], B[owner, 10:13]
            ra, rb = quat_rot(q_b, cap[:, 0:3]), quat_rot(q_b, cap[:, 3:6])
            A0, B0, VA, VB = x_b + ra, x_b + rb, v_b + np.cross(w_b, ra), v_b + np.cross(w_b, rb)
            for p in range(self.P):
                u = draws(self.key, self.env_offset + env, 1, k, 1, p)[0, 0]
                pause = self._pause(u[0])
                life, x, v, m = int(self.life[p, env]), self.pos[p, env].copy(), self.vel[p, env].copy(), float(self.mass[p, env])
                self.last_hit[p, env] = -1
                if reset:
                    life, self.countdown[p, env], x[2], v = 0, pause, -1000.0, np.zeros(3)
                if life == 0:
                    if self.countdown[p, env] > 0:
                        self.countdown[p, env] -= 1
                    else:
                        x, v, m = self._throw(B, u.astype(np.float64), int(np.floor(np.float32(u[1]) * np.float32(self.num_listed))))
                        life = self.life_steps
                        self.thrown[p, env] += 1
                if life > 0:
                    struck = False
                    for i in range(self.substeps):
                        t = (i + 1) * h
                        v[2] += g * h
                        x = x + v * h
                        if v[2] < 0:
                            self.margin[env] = min(self.margin[env], abs(x[2] - R))
                        if x[2] < R:
                            self.margin[env] = min(self.margin[env], abs(v[2]))
                            if v[2] < 0:
                                vt = math.hypot(v[0], v[1])
                                dv = min(self.friction * (1 + e_) * abs(v[2]), vt)
                                if vt > 0:
                                    v[0:2] -= dv * v[0:2] / vt
                                v[2], x[2] = -e_ * v[2], R
                        if struck:
                            continue
                        At, Bt = A0 + VA * t, B0 + VB * t
                        ab = Bt - At
                        l2 = (ab * ab).sum(-1)
                        s = np.clip(np.where(l2 > 0, ((x - At) * ab).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0), 0.0, 1.0)
                        c = At + ab * s[:, None]
                        d = x - c
                        dist = np.linalg.norm(d, axis=-1)
                        nrm = np.where(dist[:, None] > 0, d / np.where(dist > 0, dist, 1.0)[:, None], np.array([0.0, 0.0, 1.0]))
                        gap = dist - R - cap[:, 6]
                        vn = ((v - (VA + (VB - VA) * s[:, None])) * nrm).sum(-1)
                        for sel, val in ((active & (vn < 0), gap), (active & (gap < 0), vn)):
                            if sel.any():
                                self.margin[env] = min(self.margin[env], np.abs(val[sel]).min())
                        cand = np.nonzero(active & (gap < 0) & (vn < 0))[0]
                        if len(cand):
                            w = int(cand[np.argmin(gap[cand])])   # (argmin returns the first of equal values: the lowest index)
                            b, n_ = int(owner[w]), nrm[w]
                            cp = c[w] + cap[w, 6] * n_
                            rc = quat_rot(B[b, 3:7], self.tab["com"][b])
                            com = B[b, 0:3] + rc + (B[b, 7:10] + np.cross(B[b, 10:13], rc)) * t
                            r = cp - com
                            Rm = np.stack([quat_rot(B[b, 3:7], np.eye(3)[i]) for i in range(3)], axis=1)
                            Iw = Rm @ self.tab["inv_inertia"][b].reshape(3, 3) @ Rm.T
                            denom = 1.0 / m + self.tab["inv_mass"][b] + n_ @ np.cross(Iw @ np.cross(r, n_), r)
                            j = -(1 + e_) * vn[w] / denom
                            v = v + j * n_ / m
                            f = -j * n_ / self.dt
                            self.force[env, b] += f
                            self.torque[env, b] += np.cross(r, f)
                            self.hits[p, env] += 1
                            self.last_hit[p, env] = w
                            self.hit_log.append(dict(env=env, slot=p, shape=w, j=j, n=n_, r=r, dist=dist[w], vn=vn[w], m=m))
                            struck = True
                    life -= 1
                    if life == 0:
                        self.countdown[p, env], x[2], v = pause, -1000.0, np.zeros(3)
                self.life[p, env], self.pos[p, env], self.vel[p, env], self.mass[p, env] = life, x, v, m
            self.k[env] = k + 1

    def _throw(self, B, u, j):
        b = int(self.bodies[min(j, self.num_listed - 1)])
        lerp = lambda lo, hi, t: lo + t * (hi - lo)
        m, s, d = lerp(self.mass_lo, self.mass_hi, u[2]), lerp(self.speed_lo, self.speed_hi, u[3]), lerp(self.dist_lo, self.dist_hi, u[4])
        az, el = 2 * math.pi * u[5], lerp(self.elev_lo, self.elev_hi, u[6])
        rc = quat_rot(B[b, 3:7], self.tab["com"][b])
        xt, vt = B[b, 0:3] + rc, B[b, 7:10] + np.cross(B[b, 10:13], rc)
        tf = d / s
        x0 = xt + d * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        x0[2] = max(x0[2], self.radius + 0.01)
        v0 = (xt + vt * tf - x0) / tf - 0.5 * np.array([0.0, 0.0, self.gravity_z]) * tf
        return x0, v0, m


def float_bounds(o, speed, reach=4.5, K=64):
    """The fp32 bounds of one step against the fp64 oracle, to first order in the unit round-off u = 2^-24, from the case's magnitudes:
      pos_tol   = K u reach        a coordinate (|.| <= reach metres) goes through at most K = 64 rounded operations (posing ~20, 8 sub-intervals x 3);
      vel_free  = K u speed        the same for a velocity component in free flight and for a capsule point's velocity (|.| <= speed);
      n_err     = 2 pos_tol / dist the unit normal d / |d|, d = x - c known to 2 pos_tol, dist the least centre distance of the step's hits;
      vn_err    = 2 vel_free + 2 speed n_err;
      j_err     = m (1 + e) vn_err + |j| (K u + 4 n_err)      j = M_eff (1 + e) |vn| with M_eff <= m; the denominator's n and r enter as products;
      force_tol = j_err / dt;   torque_tol = |r| force_tol + (|j| / dt) 2 pos_tol;   vel_tol = vel_free + j_err / m + (|j| / m) n_err.
    -> (pos_tol m, vel_tol m/s, force_tol N, torque_tol N m) for the hits in `o.hit_log` (no hit: the flight terms alone)."""
    pos_tol, vel_free = K * U32 * reach, K * U32 * speed
    if not o.hit_log:
        return pos_tol, vel_free, 0.0, 0.0
    dist = min(hl["dist"] for hl in o.hit_log)
    jmax, mmax, mmin = max(abs(hl["j"]) for hl in o.hit_log), max(hl["m"] for hl in o.hit_log), min(hl["m"] for hl in o.hit_log)
    rmax = max(float(np.linalg.norm(hl["r"])) for hl in o.hit_log)
    n_err = 2 * pos_tol / dist
    j_err = mmax * (1 + o.restitution) * (2 * vel_free + 2 * speed * n_err) + jmax * (K * U32 + 4 * n_err)
    force_tol = j_err / o.dt
    return pos_tol, vel_free + j_err / mmin + jmax / mmin * n_err, force_tol, rmax * force_tol + jmax / o.dt * 2 * pos_tol


def compare(h, o, bounds, what=""):
    """Decisions exact, floats inside `bounds`; -> the worst float differences (pos, vel, force, torque)."""
    for name in INT_NAMES + ("k",):
        np.testing.assert_array_equal(getattr(h, name), getattr(o, name), err_msg=f"{what}: {name}")
    fly = o.life > 0
    worst = [float(np.abs(h.pos.astype(np.float64) - o.pos)[fly].max(initial=0.0)), float(np.abs(h.vel.astype(np.float64) - o.vel)[fly].max(initial=0.0)),
             float(np.abs(h.force.astype(np.float64) - o.force).max()), float(np.abs(h.torque.astype(np.float64) - o.torque).max())]
    assert (h.pos[~fly][:, 2] == -1000.0).all() and (h.vel[~fly] == 0).all(), f"{what}: a parked projectile sits at z = -1000"
    for w, b, name in zip(worst, bounds, ("pos", "vel", "force", "torque")):
        assert w <= b, f"{what}: {name} differs by {w:.3e}, bound {b:.3e}"
    assert h.guards_intact(), what
    return worst
