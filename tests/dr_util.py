"""TEST INFRASTRUCTURE for the domain-randomisation tests (tests/test_domain_rand_cpu.py, tests/test_domain_rand_gpu.py): the host build of
phc_amd/csrc/phc_dr.h (tests/dr_shim.cpp, g++), a numpy-backed caller of it with the state layout of phc_dr_args_t, the cases (states, variants, amplitudes)
both files use, and the oracle: the double-precision host stepper run once per env on that env's own statically modified model and friction."""
import copy
import ctypes as C
import functools

import numpy as np

import dyn_oracle as do
import hostemu_util as hu
import wrench_util as wu
from phc_amd import abi
import host_build
F = np.float32
KEY = 0x1234ABCD5678EF01
VEL_TOL, VEL_TOL_RIGID = 3e-3, 1e-2   # wrench_util.assert_standing
H1_OVER = ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"]


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("dr_shim.cpp", "phc_dr.hip")
    lib.dr_noise_u_batch.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    lib.dr_noise_u_batch.restype = None
    lib.dr_shifted_target.argtypes = [C.c_float] * 4
    lib.dr_shifted_target.restype = C.c_float
    lib.dr_delay_law.argtypes = [C.c_int, C.c_int, C.c_float]
    lib.dr_delay_law.restype = C.c_int
    lib.dr_args_check_of.argtypes = [C.POINTER(L.DrArgs)]
    lib.dr_args_check_of.restype = C.c_int
    lib.check_sim_step_dr_of.argtypes = [C.POINTER(L.Model), C.POINTER(L.SimParams), C.POINTER(L.SimState), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.POINTER(L.SimDr)]
    lib.check_sim_step_dr_of.restype = C.c_int
    lib.dr_advance_host.argtypes = [C.POINTER(L.DrArgs)]
    lib.dr_advance_host.restype = None
    return lib


def noise_u(key, k, call, index0, n):
    out = np.zeros(n, dtype=F)
    shim().dr_noise_u_batch(key, k, call, index0, n, out.ctypes.data)
    return out


class HostDr:
    """Caller-side state of phc_dr_advance in host memory, stepped by the host build."""
    STATE = ("action_queue", "delay", "k", "delayed_actions", "root_states")

    def __init__(self, n, d, delay=(1, 3), push_interval=0, max_push_vel_xy=0.0, key=KEY, env_offset=0):
        from phc_amd import _lib as L
        self.n, self.d = n, d
        self.action_queue = np.zeros((delay[1] + 1, n, d), dtype=F)
        self.delay = np.zeros(n, dtype=np.int32)
        self.k = np.zeros(n, dtype=np.int32)
        self.delayed_actions = np.zeros((n, d), dtype=F)
        self.root_states = np.zeros((n, 13), dtype=F)
        a = L.DrArgs()
        a.num_envs, a.num_dof, a.delay_lo, a.delay_hi = n, d, delay[0], delay[1]
        a.push_interval, a.max_push_vel_xy, a.key, a.env_offset = push_interval, max_push_vel_xy, key, env_offset
        for name in self.STATE:
            setattr(a, name, getattr(self, name).ctypes.data)
        self.args = a

    def advance(self, actions, progress=None):
        act = np.ascontiguousarray(actions, dtype=F)
        p = None if progress is None else np.ascontiguousarray(progress, dtype=np.int64)
        self.args.actions, self.args.progress_buf = act.ctypes.data, None if p is None else p.ctypes.data
        shim().dr_advance_host(self.args)
        self.args.actions = self.args.progress_buf = None


# the 12-step script of the delay tests: N = 5, D = 19, delays [1, 3]; progress 0 = the env was reset since the last step
SCRIPT_N, SCRIPT_D, SCRIPT_STEPS = 5, 19, 12


def script():
    """(actions [12, 5, 19], progress [12, 5] int64): env 1 is reset at steps 4 and 9, env 3 at step 6, env 4 at step 11."""
    rng = np.random.default_rng(5)
    actions = rng.normal(0, 1, (SCRIPT_STEPS, SCRIPT_N, SCRIPT_D)).astype(F)
    progress = np.ones((SCRIPT_STEPS, SCRIPT_N), dtype=np.int64) * np.arange(1, SCRIPT_STEPS + 1)[:, None]
    for t, e in ((4, 1), (9, 1), (6, 3), (11, 4)):
        progress[t, e] = 0
    progress[0] = 0
    return actions, progress


# ---- states and variants of the stepper cases ------------------------------------------------------------------------------------------------------------
def sliding_state(model, n, robot, seed=0, height=1.05):
    """Standing, the lowest contact point 4 mm inside the plane, root velocity (1.0, -0.6) m/s, joint rates N(0, 0.3): the feet slide, so friction matters."""
    rng = np.random.default_rng(seed)
    if robot:
        root, dof, target = wu.robot_rest_state(model, n, height)
    else:
        root, dof, target = wu.smpl_state(model, n, "ground", seed=seed)
    dof[:, :, 1] = rng.normal(0, 0.3, dof[:, :, 1].shape)
    for e in range(n):
        Q, R, p = do.kinematics(model, do.State(root[e].astype(np.float64), dof[e].astype(np.float64), model))
        low = min(p[i][2] + (R[i] @ model.contact_pos[k])[2] - model.contact_radius[k] for k, i in enumerate(model.contact_body))
        root[e, 2] += -low - 0.004
    root[:, 7], root[:, 8] = 1.0, -0.6
    return root, dof, target


def robot_params(lag=1, mode=2, **kw):
    return wu.params(control_mode=mode, sim_dt=1 / 200, limit_stiffness=2000.0, limit_damping=20.0, inertia_lag=lag, **kw)


def variant(model, which):
    """The statically modified models of the issue's effect-size table."""
    from phc_amd.domain_rand import scale_mass, shift_com
    m = copy.copy(model)
    m.mass, m.com, m.inertia_origin, m.dof_kp, m.dof_kd = (np.array(a, copy=True) for a in (model.mass, model.com, model.inertia_origin, model.dof_kp, model.dof_kd))
    hip = "left_hip_pitch_link" if "left_hip_pitch_link" in model.body_names else model.body_names[1]
    if which == "mass":
        for b in ("pelvis", "torso_link", hip):
            scale_mass(m, model.body_names.index(b), 1.3)
    elif which == "com":
        shift_com(m, model.body_names.index("torso_link"), (0.1, -0.1, 0.2))
    elif which == "gain":
        m.dof_kp, m.dof_kd = m.dof_kp * 1.25, m.dof_kd * 0.75
    elif which == "all":
        for b in ("pelvis", "torso_link", hip):
            scale_mass(m, model.body_names.index(b), 0.8)
        shift_com(m, model.body_names.index("torso_link"), (-0.05, 0.1, -0.1))
        m.dof_kp, m.dof_kd = m.dof_kp * 0.8, m.dof_kd * 1.2
    else:
        assert which == "nominal"
    return m


def with_friction(prm, mu):
    from phc_amd import _lib as L
    p = L.SimParams()
    C.memmove(C.byref(p), C.byref(prm), C.sizeof(prm))
    p.friction = max(float(mu), 0.0)
    return p


def oracle(models, env_shape, prm, root, dof, target, num_sim_calls, friction=None, noise=None):
    """The fp64 host stepper, env by env: env e with models[env_shape[e]] and friction[e].  `noise` = (amp [n, D], k [n], key, env_offset): one 1-call launch per
    simulate call, chained, each with the target shifted by u amp / kp (u from the host build of phc_dr.h, kp of the env's model)."""
    n = root.shape[0]
    keys = ("root", "dof", "rbs")
    outs = []
    for e in range(n):
        m = models[int(env_shape[e])] if env_shape is not None else models[0]
        p = prm if friction is None else with_friction(prm, friction[e])
        r, d, t = root[e:e + 1].astype(np.float64), dof[e:e + 1].astype(np.float64), np.asarray(target[e:e + 1], np.float64)
        if noise is None:
            o = hu.host_sim_step(m, p, r, d, t, num_sim_calls, f64=True)
        else:
            amp, k, key, off = noise
            D = m.num_dof
            for c in range(num_sim_calls):
                u = noise_u(key, int(k[e]), c, (off + e) * D, D).astype(np.float64)
                kp = np.asarray(m.dof_kp, np.float64)
                shift = np.where(kp != 0, u * amp[e].astype(np.float64) / np.where(kp != 0, kp, 1.0), 0.0)
                o = hu.host_sim_step(m, p, r, d, t + shift[None], 1, f64=True)
                r, d = o["root"], o["dof"]
        outs.append(o)
    return {k: np.concatenate([o[k] for o in outs], 0) for k in keys}


def effect(ref, nominal):
    """Largest body-velocity change of a randomised run against the nominal one."""
    return float(np.abs(ref["rbs"][..., 7:13] - nominal["rbs"][..., 7:13]).max())


# ---- the device launch -------------------------------------------------------------------------------------------------------------------------------------
def hip_step_dr(models, env_shape, prm, root, dof, target, num_sim_calls, friction=None, noise=None, pad_envs=1, null_dr=False, plain=False, expect=0):
    """One phc_sim_step_dr launch through the C ABI (`plain`: phc_sim_step on models[0]).  The per-env tensors hold `pad_envs` envs more than the launch, NaN /
    out-of-range: a lane of a missing env that read them would poison its workgroup.  -> dict of numpy arrays (and the return code under "rc")."""
    import torch

    from backends import get_backend
    from phc_amd import _lib as L
    from phc_amd.model import pack_shapes
    be = get_backend("hip")
    m0 = models[0]
    n, nb, nd = root.shape[0], m0.num_bodies, m0.num_dof
    K = len(models)
    ints, floats = pack_shapes(models) if K > 1 else m0.pack()
    ints_d, floats_d = be.arr(ints), be.arr(floats)
    ms = abi.model_struct(ints_d, floats_d, nb, nd, m0.max_level, max(len(m.contact_body) for m in models), num_shapes=K)
    a = dict(root=be.arr(np.asarray(root, F)), dof=be.arr(np.asarray(dof, F)), rbs=be.zeros((n, nb, 13)), cf=be.zeros((n, nb, 3)), df=be.zeros((n, nd)),
             pd=be.arr(np.asarray(target, F)))
    shape_d = None
    if env_shape is not None:
        full = np.zeros(n + pad_envs, np.int32)   # (a block index is an address: the padding stays in range)
        full[:n] = env_shape
        shape_d = be.arr(full)
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"], env_shape=shape_d)
    dr = L.SimDr()
    keep = []
    if friction is not None:
        full = np.full(n + pad_envs, np.nan, F)
        full[:n] = friction
        keep.append(be.arr(full))
        dr.env_friction = abi.ptr(keep[-1])
    if noise is not None:
        amp, k, key, off = noise
        full = np.full((n + pad_envs, nd), np.nan, F)
        full[:n] = amp
        keep.append(be.arr(full))
        dr.torque_noise = abi.ptr(keep[-1])
        keep.append(be.arr(np.asarray(k, np.int32)))
        dr.k = abi.ptr(keep[-1])
        dr.key, dr.env_offset = key, off
    s = torch.cuda.current_stream().cuda_stream
    if plain:
        rc = be.lib.phc_sim_step(ms, prm, sim, None, None, None, None, num_sim_calls, s)
    else:
        rc = be.lib.phc_sim_step_dr(ms, prm, sim, None, None, None, None, num_sim_calls, None if null_dr else C.byref(dr), s)
    assert rc == expect, rc
    be.sync()
    out = {k: be.np(a[k]) for k in ("root", "dof", "rbs", "cf", "df", "pd")}
    out["rc"] = rc
    return out
