"""Domain randomisation (config group `domain_rand`, e.g. `domain_rand=h1_dr`): per-env physics for sim-to-real training of the robots, after the reference's
schedule phc/data/cfg/domain_rand/h1_dr.yaml and its draws in phc/env/tasks/humanoid_teleop.py:309-406.

    randomize_friction     per-env ground friction from 64 buckets of U(friction_range)          -> phc_sim_dr_t.env_friction
    randomize_link_mass    mass (and inertia about the CoM) of the listed links x U(link_mass_range)   \\
    randomize_base_com     CoM of `base_com_body` (torso_link) += U(base_com_range) per axis            > K = num_buckets model variants, one per env
    randomize_pd_gain      kp, kd of every DoF x U(kp_range), U(kd_range)                               /   (phc_model_t blocks + env_shape)
    randomize_torque_rfi   torque noise of amplitude rfi_lim (x U(rfi_lim_range)) x effort limit   -> phc_sim_dr_t.torque_noise
    randomize_ctrl_delay   the action applied is the one of `delay` env steps ago, delay ~ randint(ctrl_delay_step_range), redrawn at every reset   \\  phc_dr_advance
    push_robots            every push_interval_s the root's xy velocity is set to U(-max_push_vel_xy, max_push_vel_xy)                              /
    seed (default: the run's seed), num_buckets (default 64), base_com_body (default torso_link): phc_amd's own keys

Everything drawn at construction is a counter hash of (seed, stream, GLOBAL index): the sampler is deterministic, variant v and bucket b are the same on every
rank, and env i of a rank with `env_offset` o draws what env o + i of a single-rank run draws.  Nothing goes into checkpoints.  The sampler is numpy on the host
(`DomainRand`); `upload()` makes the device tensors and the two argument structs, `advance()` is the phc_dr_advance launch."""
import copy

import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
STREAMS = {"friction_bucket": 1, "friction_id": 2, "variant_id": 3, "link_mass": 4, "base_com": 5, "kp": 6, "kd": 7, "rfi_lim": 8}
APPLIED_KEYS = {"has_domain_rand", "push_robots", "push_interval_s", "max_push_vel_xy", "randomize_friction", "friction_range", "randomize_base_mass",
                "randomize_base_com", "base_com_range", "randomize_link_mass", "link_mass_range", "randomize_link_body_names", "randomize_pd_gain", "kp_range",
                "kd_range", "randomize_torque_rfi", "rfi_lim", "randomize_rfi_lim", "rfi_lim_range", "randomize_ctrl_delay", "ctrl_delay_step_range",
                "seed", "num_buckets", "base_com_body"}


def _splitmix64(z):
    """splitmix64 of csrc/phc_rng.h on uint64 arrays."""
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return z ^ (z >> np.uint64(31))


def stream_key(seed):
    """The 64-bit key of a run's domain randomisation; the tag keeps it apart from the reset launch's and the push schedule's keys of the same seed."""
    return int(_splitmix64(_splitmix64(np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)) ^ np.uint64(0x646F6D61696E7264)))   # ("domainrd")


def uniform01(key, stream, index):
    """U[0, 1) doubles at the integer `index` array of stream `stream` under `key`: 53 bits of splitmix64(splitmix64(key + stream) ^ index * odd)."""
    idx = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = _splitmix64(np.uint64(key) + np.uint64(STREAMS[stream]) * np.uint64(0xD1B54A32D192ED03))
        h = _splitmix64(k ^ (idx * np.uint64(0x9E6C63D0876A9A47)))
    return (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _range(v, name):
    lo, hi = (float(x) for x in v)
    if not lo <= hi:
        raise ValueError(f"domain_rand.{name} must be [low, high] with low <= high, not {v!r}")
    return lo, hi


def shift_com(model, body, delta):
    """CoM of `body` += delta with the inertia about the CoM kept: inertia_origin re-derived by the parallel-axis term (model.pack() does the same for the
    solver reference point)."""
    m, c = model.mass[body], model.com[body].copy()
    icom = model.inertia_origin[body] - m * (c @ c * np.eye(3) - np.outer(c, c))
    c2 = c + np.asarray(delta, dtype=np.float64)
    model.com[body] = c2
    model.inertia_origin[body] = icom + m * (c2 @ c2 * np.eye(3) - np.outer(c2, c2))


def scale_mass(model, body, factor):
    """Mass of `body` x factor, the inertia about the CoM scaled with it (so the inertia about the origin scales too: both of its terms are linear in the mass)."""
    model.mass[body] *= factor
    model.inertia_origin[body] = model.inertia_origin[body] * factor


class DomainRand:
    """What `cfg.domain_rand` asks for, sampled for `num_envs` envs of `model` (an ArticulationModel with its gains applied).  Host attributes (numpy):
    env_friction [N] | None, models (K variants, models[0] is `model`), env_shape int32 [N] | None, torque_noise [N, D] | None, delay_range (lo, hi) | None,
    push_interval (env steps, 0 = none), max_push_vel_xy, key, env_offset, ignored (the keys read and not applied)."""

    def __init__(self, cfg, num_envs, model, plane_friction=1.0, dt=1 / 50, default_seed=0, env_offset=0, is_robot=True, explicit_pd=True):
        cfg = dict(cfg)
        if cfg.get("randomize_base_mass", False):
            raise ValueError("domain_rand.randomize_base_mass: replaced by randomize_link_mass (the reference raises for it too, humanoid_teleop.py)")
        if cfg.get("randomize_torque_rfi", False) and not (is_robot and explicit_pd):
            raise NotImplementedError("domain_rand.randomize_torque_rfi: the torque noise enters as a PD-target shift of the explicit `pd` drive of the revolute "
                                      "robots (control.control_mode=pd); it is not built for the SMPL family or control_mode=isaac_pd")
        self.num_envs, self.num_dof, self.env_offset = int(num_envs), int(model.num_dof), int(env_offset)
        self.seed = int(cfg.get("seed", default_seed))
        self.key = stream_key(self.seed)
        self.ignored = sorted(k for k in cfg if k not in APPLIED_KEYS)
        N, D = self.num_envs, self.num_dof
        genv = np.arange(N, dtype=np.uint64) + np.uint64(self.env_offset)
        u = lambda stream, index: uniform01(self.key, stream, index)

        # ---- friction: 64 buckets of U(friction_range), one per env (humanoid_teleop.py:_process_rigid_shape_props); the stepper's single coefficient is PhysX's
        # default "average" combine of the shape's and the plane's, clamped at 0 ----
        self.env_friction = None
        if cfg.get("randomize_friction", False):
            lo, hi = _range(cfg["friction_range"], "friction_range")
            buckets = lo + (hi - lo) * u("friction_bucket", np.arange(64))
            ids = np.minimum((u("friction_id", genv) * 64).astype(np.int64), 63)
            self.friction_buckets = buckets
            self.env_friction = np.maximum(0.0, 0.5 * (float(plane_friction) + buckets[ids])).astype(np.float32)

        # ---- model variants: variant 0 is the nominal model ----
        mass_on, com_on, gain_on = (bool(cfg.get(k, False)) for k in ("randomize_link_mass", "randomize_base_com", "randomize_pd_gain"))
        K = int(cfg.get("num_buckets", 64)) if (mass_on or com_on or gain_on) else 1
        if K < 1:
            raise ValueError("domain_rand.num_buckets must be >= 1")
        self.models = [model]
        names = list(cfg.get("randomize_link_body_names", [])) if mass_on else []
        missing = [b for b in names if b not in model.body_names]
        if missing:
            raise ValueError(f"domain_rand.randomize_link_body_names: no such body {missing}; the model has {model.body_names}")
        com_body = str(cfg.get("base_com_body", "torso_link"))
        if com_on and com_body not in model.body_names:
            raise ValueError(f"domain_rand.base_com_body={com_body!r}: no such body; the model has {model.body_names}")
        for v in range(1, K):
            m = copy.copy(model)   # (topology and geometry shared; what a variant changes is its own)
            m.mass, m.com, m.inertia_origin, m.dof_kp, m.dof_kd = (np.array(a, copy=True) for a in (model.mass, model.com, model.inertia_origin, model.dof_kp, model.dof_kd))
            if mass_on:
                lo, hi = _range(cfg["link_mass_range"], "link_mass_range")
                for b in names:
                    j = model.body_names.index(b)
                    scale_mass(m, j, lo + (hi - lo) * float(u("link_mass", v * 64 + j)))
            if com_on:
                r = cfg["base_com_range"]
                d = [_range(r[ax], f"base_com_range.{ax}") for ax in ("x", "y", "z")]
                shift_com(m, model.body_names.index(com_body), [lo + (hi - lo) * float(u("base_com", v * 3 + a)) for a, (lo, hi) in enumerate(d)])
            if gain_on:
                (plo, phi), (dlo, dhi) = _range(cfg["kp_range"], "kp_range"), _range(cfg["kd_range"], "kd_range")
                dofs = np.arange(D) + v * D
                m.dof_kp = m.dof_kp * (plo + (phi - plo) * u("kp", dofs))
                m.dof_kd = m.dof_kd * (dlo + (dhi - dlo) * u("kd", dofs))
            self.models.append(m)
        self.env_shape = np.minimum((u("variant_id", genv) * K).astype(np.int64), K - 1).astype(np.int32) if K > 1 else None

        # ---- torque noise ("rfi", humanoid.py:1597-1598): amplitude rfi_lim (x U(rfi_lim_range) per env and DoF) x effort limit ----
        self.torque_noise = None
        if cfg.get("randomize_torque_rfi", False):
            scale = np.ones((N, D))
            if cfg.get("randomize_rfi_lim", False):
                lo, hi = _range(cfg["rfi_lim_range"], "rfi_lim_range")
                scale = lo + (hi - lo) * u("rfi_lim", genv[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None])
            self.torque_noise = (float(cfg.get("rfi_lim", 0.1)) * scale * model.dof_effort[None]).astype(np.float32)

        # ---- per env step (phc_dr_advance): control delay in env steps, velocity push every ceil(push_interval_s / dt) env steps ----
        self.delay_range = None
        if cfg.get("randomize_ctrl_delay", False):
            lo, hi = (int(x) for x in cfg["ctrl_delay_step_range"])
            if not 0 <= lo <= hi <= 1023:
                raise ValueError(f"domain_rand.ctrl_delay_step_range must be [low, high] with 0 <= low <= high <= 1023, not {cfg['ctrl_delay_step_range']!r}")
            self.delay_range = (lo, hi)
        self.push_interval, self.max_push_vel_xy = 0, 0.0
        if cfg.get("push_robots", False):
            self.push_interval = int(np.ceil(float(cfg["push_interval_s"]) / float(dt)))
            self.max_push_vel_xy = float(cfg["max_push_vel_xy"])
            if self.push_interval < 1 or not self.max_push_vel_xy >= 0:
                raise ValueError("domain_rand.push_interval_s must be positive and max_push_vel_xy >= 0")
        self._dev = None

    def notice(self):
        """One line: the keys of the group that were read and are not applied (observation noise of the teleop layout, the unused mass range)."""
        return ("[phc_amd] domain_rand: accepted and NOT applied: " + (", ".join(self.ignored) if self.ignored else "(nothing)")
                + " -- they address HumanoidTeleop's observation layout or options that are off")

    def pack(self, kp_scale=1.0, kd_scale=1.0):
        """(ints [K, ni], floats [K, nf]) of the variants (model.pack_shapes), or the single model's (ints [ni], floats [nf]) for K == 1."""
        from .model import pack_shapes
        return pack_shapes(self.models, kp_scale, kd_scale) if len(self.models) > 1 else self.models[0].pack(kp_scale, kd_scale)

    # ---- device side ----
    def upload(self, device, root_states, kp_scale=1.0, kd_scale=1.0):
        """Device tensors, the K-block phc_model_t of the DR launch, phc_sim_dr_t and phc_dr_args_t.  `root_states`: the task's [N, 13] tensor (pushes write it)."""
        import torch

        from . import _lib as L
        from . import abi
        N, D, m0 = self.num_envs, self.num_dof, self.models[0]
        t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
        ints, floats = self.pack(kp_scale, kd_scale)
        d = self._dev = dict(ints=t(ints, torch.int32), floats=t(floats, torch.float32), env_shape=t(self.env_shape, torch.int32),
                             env_friction=t(self.env_friction, torch.float32), torque_noise=t(self.torque_noise, torch.float32))
        self.model_struct = abi.model_struct(d["ints"], d["floats"], m0.num_bodies, m0.num_dof, m0.max_level,
                                             max(len(m.contact_body) for m in self.models), num_shapes=len(self.models))
        lo, hi = self.delay_range or (0, 0)
        self.k = torch.zeros(N, dtype=torch.int32, device=device)
        self.delay = torch.zeros(N, dtype=torch.int32, device=device)
        self.action_queue = torch.zeros((hi + 1, N, D), dtype=torch.float32, device=device)
        self.delayed_actions = torch.zeros((N, D), dtype=torch.float32, device=device)
        s = self.sim_dr = L.SimDr()
        s.env_friction, s.torque_noise, s.k = abi.ptr(d["env_friction"]), abi.ptr(d["torque_noise"]), self.k.data_ptr()
        s.key, s.env_offset = self.key, self.env_offset
        a = self.args = L.DrArgs()
        a.num_envs, a.num_dof, a.delay_lo, a.delay_hi = N, D, lo, hi
        a.push_interval, a.max_push_vel_xy = self.push_interval, self.max_push_vel_xy
        a.key, a.env_offset = self.key, self.env_offset
        a.action_queue, a.delay, a.k, a.delayed_actions = self.action_queue.data_ptr(), self.delay.data_ptr(), self.k.data_ptr(), self.delayed_actions.data_ptr()
        a.root_states = root_states.data_ptr() if self.push_interval > 0 else None
        self._root_states = root_states
        self._lib, self._check, self._torch = L.load(), L.check, torch
        return self

    @property
    def env_shape_device(self):
        return self._dev["env_shape"]

    def advance(self, actions, progress_buf=None):
        """Once per env step, ahead of the stepper: phc_dr_advance on the current stream.  Afterwards `delayed_actions` is what the stepper is given and `k`
        counts the step."""
        torch = self._torch
        if actions.dtype != torch.float32 or tuple(actions.shape) != (self.num_envs, self.num_dof) or not actions.is_contiguous():
            raise ValueError("DomainRand.advance takes contiguous fp32 actions [num_envs, num_dof]")
        if progress_buf is not None and (progress_buf.dtype != torch.int64 or tuple(progress_buf.shape) != (self.num_envs,) or not progress_buf.is_contiguous()):
            raise ValueError("DomainRand.advance takes the task's progress_buf: a contiguous int64 [num_envs] tensor")
        self.args.actions = actions.data_ptr()
        self.args.progress_buf = None if progress_buf is None else progress_buf.data_ptr()
        self._check(self._lib.phc_dr_advance(self.args, torch.cuda.current_stream(self.k.device).cuda_stream), "phc_dr_advance")
