"""TEST INFRASTRUCTURE shared by tests/test_teleop_cpu.py and tests/test_teleop_gpu.py: the host build of phc_amd/csrc/phc_teleop.h (tests/teleop_shim.cpp,
g++), a numpy-backed caller with the layout of phc_teleop_args_t, a small motion library whose root velocity is prescribed frame by frame, seeded inputs of
any shape, and the comparison at the project's bound for the post-physics floats."""
import ctypes as C
import functools

import numpy as np

from phc_amd import _lib as L
from phc_amd import abi
import host_build
F = np.float32
TERMS = L.TELEOP_TERMS
TOL = 2e-5   # |a - b| <= TOL max(1, |b|): the bound of the post-physics floats
H1_OVER = ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"]
STATE = ("last_actions", "last_dof_vel", "feet_air_time", "last_contacts", "recovery_counter")
INPUTS = ("dof_state", "dof_limits_lower", "dof_limits_upper", "torque_limits", "dof_force", "actions", "contact_force", "rigid_body_state", "progress_buf",
          "motion_start_times", "motion_start_times_offset", "dr_k")
# the nullable fields each term reads (include/phc_amd.h)
NEEDS = {"dof_pos_limits": ("dof_state", "dof_limits_lower", "dof_limits_upper"), "torque_limits": ("dof_force", "torque_limits"), "torques": ("dof_force",),
         "dof_vel": ("dof_state",), "dof_acc": ("dof_state", "last_dof_vel"), "action_rate": ("actions", "last_actions"),
         "slippage": ("contact_force", "rigid_body_state"), "feet_contact_forces": ("contact_force",), "stumble": ("contact_force",),
         "feet_air_time_teleop": ("contact_force", "feet_air_time", "last_contacts", "progress_buf", "motion_start_times", "motion_start_times_offset"),
         "feet_ori": ("rigid_body_state",)}


@functools.lru_cache(maxsize=None)
def shim():
    lib = host_build.shim("teleop_shim.cpp", "phc_teleop.hip")
    for fn in (lib.teleop_args_check_of, lib.teleop_rewards_host):
        fn.argtypes = [C.POINTER(L.MotionLib), C.POINTER(L.TeleopArgs)]
        fn.restype = C.c_int
    return lib


def close(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert a.shape == b.shape and (err.size == 0 or float(err.max()) <= TOL), f"{what}: largest error {float(err.max()) if err.size else 0:.3e} (bound {TOL})"
    return float(err.max()) if err.size else 0.0


def velocity_lib(ref_root_vel, dt):
    """(struct, keep-alive arrays): one clip per env with S + 2 frames 1 / dt apart; frame p = 1 .. S holds root velocity ref_root_vel[p - 1], frames 0 and
    S + 1 hold 7 m/s: a lookup at progress p dt reads ref_root_vel[p - 1], one frame off reads something else.  Two revolute bodies."""
    S, n = ref_root_vel.shape[:2]
    nf, nb = S + 2, 2
    gvs = np.zeros((n, nf, nb, 3), dtype=F)
    gvs[:, :, 0] = 7.0
    gvs[:, 1:S + 1, 0] = np.swapaxes(ref_root_vel, 0, 1)
    z = lambda *s: np.zeros(s, dtype=F)
    grs = z(n * nf, nb, 4)
    grs[..., 3] = 1
    frames = abi.pack_frames(z(n * nf, nb, 3), grs, gvs.reshape(n * nf, nb, 3), z(n * nf, nb, 3), None, z(n * nf, nb - 1), dof_pos=z(n * nf, nb - 1))
    keep = dict(frames=frames, lengths=np.full(n, (nf - 1) * F(dt), dtype=F), dts=np.full(n, dt, dtype=F), nfs=np.full(n, nf, dtype=np.int64),
                starts=np.arange(n, dtype=np.int64) * nf)
    return keep


def lib_struct(keep, to=lambda a: a):
    k = {n: to(a) for n, a in keep.items()}
    return abi.motion_lib_struct(k["frames"], k["frames"].shape[1], 2, k["lengths"], k["dts"], k["nfs"], k["starts"], dofs_per_joint=1), k


def random_case(n, d, feet, nb=None, steps=1, seed=0, dt=0.02):
    """Seeded inputs of `steps` steps for arbitrary sizes: dict of arrays named after the fields of phc_teleop_args_t ([steps, ...] for the per-step ones)."""
    rng = np.random.default_rng(seed)
    nb = nb or max(feet) + 2
    nf = len(feet)
    x = dict(dof_limits_lower=rng.uniform(-2, -0.5, d).astype(F), dof_limits_upper=rng.uniform(0.5, 2, d).astype(F), torque_limits=rng.uniform(20, 200, d).astype(F))
    x["dof_state"] = np.stack([rng.uniform(-2.5, 2.5, (steps, n, d)), rng.standard_normal((steps, n, d)) * 3], axis=-1).astype(F)
    x["dof_force"] = (rng.uniform(-1.3, 1.3, (steps, n, d)) * x["torque_limits"]).astype(F)
    x["actions"] = rng.standard_normal((steps, n, d)).astype(F)
    cf = (rng.standard_normal((steps, n, nb, 3)) * np.array([3, 3, 1])).astype(F)
    cf *= rng.choice(np.array([0, 0.3, 1, 30, 300], dtype=F), (steps, n, nb, 1))
    x["contact_force"] = cf
    rbs = rng.standard_normal((steps, n, nb, 13)).astype(F)
    rbs[..., 3:7] /= np.linalg.norm(rbs[..., 3:7], axis=-1, keepdims=True)
    x["rigid_body_state"] = rbs
    x["ref_root_vel"] = (rng.standard_normal((steps, n, 3)) * 0.15).astype(F)
    x["rew_in"] = rng.uniform(0.2, 1.0, (steps, n)).astype(F)
    x["reward_im"] = rng.uniform(0, 1, (steps, n, 5)).astype(F)
    x["feet_air_time0"] = rng.choice(np.array([0, 0.1, 0.24, 0.3], dtype=F), (n, nf))
    x["last_contacts0"] = rng.random((n, nf)) < 0.5
    x.update(feet=list(feet), num_bodies=nb, dt=dt, max_contact_force=100.0)
    return x


def golden_case(g, tag):
    """The block `tag` of tests/golden/teleop_rewards.npz in the layout of random_case."""
    p = lambda k: g[f"{tag}/{k}"]
    x = dict(dof_limits_lower=p("limits_lower"), dof_limits_upper=p("limits_upper"), torque_limits=p("torque_limits"),
             dof_state=np.ascontiguousarray(np.stack([p("dof_pos"), p("dof_vel")], axis=-1)), dof_force=p("torques"), actions=p("actions"),
             contact_force=p("contact_forces"), ref_root_vel=p("ref_root_vel"), rew_in=p("rew_in"), reward_im=p("reward_im"),
             feet_air_time0=p("feet_air_time0"), last_contacts0=p("last_contacts0"), feet=[int(f) for f in p("feet")], dt=float(g["dt"]))
    S, n, nb = p("body_vel").shape[:3]
    rbs = np.zeros((S, n, nb, 13), dtype=F)
    rbs[..., 3:7], rbs[..., 7:10] = p("body_rot"), p("body_vel")
    specs = dict(zip((str(s) for s in g["spec_names"]), (float(v) for v in g["spec_values"])))
    x.update(rigid_body_state=rbs, num_bodies=nb, max_contact_force=specs["max_contact_force"])
    return x


class Runner:
    """State and arguments of phc_teleop_rewards over the steps of a case, in host memory (`to` = identity) or on the device (`to` = numpy -> torch tensor,
    `back` = tensor -> numpy); `launch(lib_struct, args)` is the host build or the entry point."""

    def __init__(self, x, launch, terms, scales=None, to=lambda a: np.array(a, copy=True), back=lambda a: a, push_interval=0, recovery_steps=3, im_cols=5,
                 null_unused=True, with_state=True):
        self.x, self.launch, self.terms, self.to, self.back = x, launch, list(terms), to, back
        S, n, d = x["dof_state"].shape[:3]
        self.n, self.d, self.S, self.C = n, d, S, im_cols
        nf = len(x["feet"])
        self.state = dict(last_actions=to(np.zeros((n, d), F)), last_dof_vel=to(np.zeros((n, d), F)), feet_air_time=to(x["feet_air_time0"].astype(F)),
                          last_contacts=to(x["last_contacts0"].astype(np.uint8)), recovery_counter=to(np.zeros(n, np.int32)))
        self.dr_k = np.zeros(n, np.int32)
        self.progress = None   # [n] int64 per step when set; default: step + 1
        self.scales = scales or {t: 1.0 for t in terms}
        self.push_interval, self.recovery_steps, self.null_unused, self.with_state = push_interval, recovery_steps, null_unused, with_state
        self.lib, self._lib_keep = lib_struct(velocity_lib(x["ref_root_vel"], x["dt"]), to=lambda a: to(a))
        self.constant = {k: to(x[k]) for k in ("dof_limits_lower", "dof_limits_upper", "torque_limits")}

    def used(self):
        need = set()
        for t in self.terms:
            need |= set(NEEDS[t])
        if self.with_state:
            need |= {"last_actions", "actions", "last_dof_vel", "dof_state"}
        if self.push_interval > 0:
            need |= {"dr_k", "recovery_counter"}
        if "feet_air_time_teleop" in self.terms:
            need.add("recovery_counter")
        return need

    def step(self, s):
        """Launch step s -> (rew_buf [n], reward_raw [n, C + R]) as numpy."""
        x, to = self.x, self.to
        n = self.n
        R = len(self.terms)
        progress = np.full(n, s + 1, np.int64) if self.progress is None else np.asarray(self.progress[s], np.int64)
        per_step = dict(dof_state=x["dof_state"][s], dof_force=x["dof_force"][s], actions=x["actions"][s], contact_force=x["contact_force"][s],
                        rigid_body_state=x["rigid_body_state"][s], progress_buf=progress, motion_start_times=np.zeros(n, F), motion_start_times_offset=np.zeros(n, F),
                        dr_k=self.dr_k)
        arrays = {k: to(np.ascontiguousarray(v)) for k, v in per_step.items()}
        arrays.update(self.constant)
        arrays.update(self.state)
        if self.null_unused:
            need = self.used()
            arrays = {k: v for k, v in arrays.items() if k in need}
        rew = to(x["rew_in"][s].astype(F))
        im = to(np.ascontiguousarray(x["reward_im"][s][:, :self.C])) if self.C else None
        raw = to(np.full((n, self.C + R), np.nan, F))
        a = abi.teleop_args_struct(n, self.d, rew, raw, reward_im=im, terms=self.terms, scales=self.scales, dt=x["dt"], num_bodies=x["num_bodies"], feet=x["feet"],
                                   max_contact_force=x["max_contact_force"], push_interval=self.push_interval, recovery_steps=self.recovery_steps, **arrays)
        self.last_args, self._keep = a, (arrays, rew, im, raw)
        rc = self.launch(self.lib, a)
        assert rc == 0, rc
        return self.back(rew), self.back(raw)

    def state_np(self):
        return {k: np.array(self.back(v), copy=True) for k, v in self.state.items()}


def host_launch(lib, a):
    return shim().teleop_rewards_host(C.byref(lib), C.byref(a))


# ---- the terms as torch statements (the end-to-end test's restatement; scripts/probes/teleop_step_ab.py times it) ----------------------------------
def restate(task, st, ref_vel_xy):
    """The active terms as the torch statements a user would write, from the task's own tensors; `st`: the test's own copy of the state.  -> {name: [N]}"""
    import torch
    dt, feet = task.dt, task.feet_indices
    q, qd, tau, a = task._dof_pos, task._dof_vel, task.dof_force_tensor, task.actions
    Ff, vf = task._contact_forces[:, feet], task._rigid_body_vel[:, feet]
    out = {}
    lim = task.dof_pos_limits
    out["dof_pos_limits"] = (-(q - lim[:, 0]).clip(max=0.0) + (q - lim[:, 1]).clip(min=0.0)).sum(dim=1)
    out["torque_limits"] = (tau.abs() - task.torque_limits).clip(min=0.0).sum(dim=1)
    out["torques"] = tau.square().sum(dim=1)
    out["dof_vel"] = qd.square().sum(dim=1)
    out["dof_acc"] = ((st["last_dof_vel"] - qd) / dt).square().sum(dim=1)
    out["action_rate"] = (st["last_actions"] - a).square().sum(dim=1)
    out["slippage"] = (vf.norm(dim=-1) * (Ff.norm(dim=-1) > 1.0)).sum(dim=1)
    out["feet_contact_forces"] = (Ff.norm(dim=-1) - task.max_contact_force).clip(min=0.0).sum(dim=1)
    out["stumble"] = (Ff[..., :2].norm(dim=2) > 5 * Ff[..., 2].abs()).any(dim=1).float()
    contact = Ff[..., 2] > 1.0
    filt = contact | st["last_contacts"]
    st["last_contacts"] = contact
    first = (st["feet_air_time"] > 0.0) & filt
    st["feet_air_time"] = st["feet_air_time"] + dt
    air = ((st["feet_air_time"] - 0.25) * first).sum(dim=1) * (ref_vel_xy.norm(dim=1) > 0.1)
    st["feet_air_time"] = st["feet_air_time"] * ~filt
    out["feet_air_time_teleop"] = air
    g = torch.zeros(task.num_envs, device=q.device)
    for f in (0, 1):
        quat = task._rigid_body_rot[:, feet[f]]
        w, v = quat[:, 3:4], quat[:, :3]
        grav = torch.tensor([0.0, 0.0, -1.0], device=q.device).expand_as(v)
        rot = grav * (2.0 * w ** 2 - 1.0) - torch.cross(v, grav, dim=-1) * w * 2.0 + v * (v * grav).sum(-1, keepdim=True) * 2.0
        g = g + rot[:, :2].square().sum(dim=1) ** 0.5
    out["feet_ori"] = g
    st["last_actions"], st["last_dof_vel"] = a.clone(), qd.clone()
    return out
