"""Thrown projectiles (config group `projectile`): spheres thrown at listed bodies of every env every few seconds, so that play, the evaluation sweep and
training see the disturbance the reference demonstrates with `flags.add_proj` (phc/env/tasks/humanoid.py:73-177, humanoid_im.py:562-593).  The reference's
blocks become spheres here, as boxes become capsules everywhere else in this package; PhysX moves its blocks as rigid bodies with friction and spin, this
model is a point mass with frictionless impacts.

    +projectile.mass=[1,5]              # kg, uniform per throw (required)
    +projectile.radius=0.1              # m
    +projectile.speed=[5,10]            # m/s along the line of sight
    +projectile.distance=[2,4]          # m from the target body's centre of mass
    +projectile.elevation_deg=[0,30]    # the start point's elevation above the target
    +projectile.bodies=[Pelvis,Torso,Head]   # one drawn per throw; default: the root body
    +projectile.interval_s=[2,4]        # pause between parking and the next throw, whole env steps
    +projectile.life_s=2                # a thrown projectile parks after this time
    +projectile.count=1                 # slots per env, at most 4
    +projectile.restitution=0.2
    +projectile.substeps=8              # sub-intervals of the env step
    +projectile.seed=<cfg.seed>

`ProjectileSchedule.advance()` is ONE launch (phc_proj_advance, include/phc_amd.h; rules line by line: csrc/phc_proj.h): flight, ground bounce, collision test
against every collision capsule and the impulse of a hit, written as `force` / `torque` [N, NB, 3] that `HumanoidIm` hands to phc_sim_step_wrench -- on a
shadow copy of the simulator tensors, whose rows it takes for the struck envs only (`shadow_of`, `snapshot`, `select`: phc_proj_rows), so that an env nothing
struck stays the env of a run without the group.  All state and all draws live on the device: capturable, a replayed capture draws anew.  There is one implementation and no torch twin."""
import math

import numpy as np
import torch

from .perturb import stream_key

STREAM_TAG = 0x70726F6A74687277   # ("projthrw") perturb.stream_key's tag of this schedule
OPTIONS = {"mass", "radius", "speed", "distance", "elevation_deg", "bodies", "interval_s", "life_s", "count", "restitution", "substeps", "seed"}


def _pair(v, name, positive=True):
    lo, hi = (v, v) if isinstance(v, (int, float)) else tuple(v)
    lo, hi = float(lo), float(hi)
    if not (lo <= hi and math.isfinite(lo) and math.isfinite(hi)) or (positive and not lo > 0.0):
        raise ValueError(f"projectile.{name} must be a number or [low, high] with {'0 < ' if positive else ''}low <= high, not {v!r}")
    return lo, hi


def model_tables(model):
    """The model's side of phc_proj_args_t as float32 / int32 numpy arrays: capsules [S, 7], owner [S], com [NB, 3], inverse mass [NB], inverse inertia about the
    centre of mass in the body frame [NB, 9]."""
    m, c = model.mass, model.com
    inv_inertia = np.zeros((model.num_bodies, 9))
    for i in range(model.num_bodies):
        about_com = model.inertia_origin[i] - m[i] * (c[i] @ c[i] * np.eye(3) - np.outer(c[i], c[i]))
        inv_inertia[i] = np.linalg.inv(about_com).reshape(9)
    return dict(capsules=np.ascontiguousarray(model.shape_capsules(), dtype=np.float32), owner=np.ascontiguousarray(model.shape_owner(), dtype=np.int32),
                com=c.astype(np.float32), inv_mass=(1.0 / m).astype(np.float32), inv_inertia=inv_inertia.astype(np.float32))


class ProjectileOptions:
    """The checked options of the `projectile` group (no device work: testable without a GPU)."""

    def __init__(self, cfg, body_names, dt, default_seed=0):
        from . import _lib as L
        cfg = dict(cfg)
        unknown = set(cfg) - OPTIONS
        if unknown:
            raise ValueError(f"unknown projectile option(s): {sorted(unknown)}")
        if "mass" not in cfg:
            raise ValueError("projectile.mass (kg, a number or [low, high]) is required")
        self.dt = float(dt)
        self.mass = _pair(cfg["mass"], "mass")
        self.speed = _pair(cfg.get("speed", [5.0, 10.0]), "speed")
        self.distance = _pair(cfg.get("distance", [2.0, 4.0]), "distance")
        self.elevation_deg = _pair(cfg.get("elevation_deg", [0.0, 30.0]), "elevation_deg", positive=False)
        if not -90.0 <= self.elevation_deg[0] <= self.elevation_deg[1] <= 90.0:
            raise ValueError(f"projectile.elevation_deg must lie in [-90, 90], not {cfg.get('elevation_deg')!r}")
        self.radius = float(cfg.get("radius", 0.1))
        if not (self.radius > 0.0 and math.isfinite(self.radius)):
            raise ValueError(f"projectile.radius must be positive, not {self.radius!r}")
        self.restitution = float(cfg.get("restitution", 0.2))
        if not 0.0 <= self.restitution <= 1.0:
            raise ValueError(f"projectile.restitution must lie in [0, 1], not {self.restitution!r}")
        self.count = int(cfg.get("count", 1))
        if not 1 <= self.count <= L.PROJ_MAX_SLOTS:
            raise ValueError(f"projectile.count must lie in [1, {L.PROJ_MAX_SLOTS}], not {self.count}")
        self.substeps = int(cfg.get("substeps", 8))
        if not 1 <= self.substeps <= 64:
            raise ValueError(f"projectile.substeps must lie in [1, 64], not {self.substeps}")
        # a sub-interval may not carry the sphere further than its own radius: no capsule is stepped over
        if self.speed[1] * self.dt / self.substeps > self.radius:
            raise ValueError(f"projectile: speed {self.speed[1]} m/s moves the sphere {self.speed[1] * self.dt / self.substeps:.3f} m per sub-interval, more than its "
                             f"radius {self.radius} m (tunnelling): raise projectile.substeps or the radius, or lower the speed")
        names = cfg.get("bodies", None) or [body_names[0]]
        names = [names] if isinstance(names, str) else list(names)
        missing = [b for b in names if b not in body_names]
        if missing:
            raise ValueError(f"projectile.bodies: no such body {missing}; the model has {list(body_names)}")
        self.listed = [list(body_names).index(b) for b in names]
        lo, hi = _pair(cfg.get("interval_s", [2.0, 4.0]), "interval_s", positive=False)
        if lo < 0.0:
            raise ValueError(f"projectile.interval_s must not be negative, not {cfg.get('interval_s')!r}")
        self.pause_steps = (max(1, int(round(lo / self.dt))), max(1, int(round(hi / self.dt))))   # drawn in whole env steps, like the push schedule's pause
        life = float(cfg.get("life_s", 2.0))
        if not (life > 0.0 and math.isfinite(life)):
            raise ValueError(f"projectile.life_s must be positive, not {life!r}")
        self.life_steps = max(1, int(round(life / self.dt)))
        self.seed = int(cfg.get("seed", default_seed))

    def fill(self, a, gravity_z, friction):
        """The option fields of a phc_proj_args_t."""
        a.count, a.substeps, a.life_steps = self.count, self.substeps, self.life_steps
        a.pause_lo, a.pause_hi = self.pause_steps
        a.dt, a.gravity_z, a.radius, a.restitution, a.friction = self.dt, gravity_z, self.radius, self.restitution, friction
        a.mass_lo, a.mass_hi = self.mass
        a.speed_lo, a.speed_hi = self.speed
        a.dist_lo, a.dist_hi = self.distance
        a.elev_lo, a.elev_hi = (math.radians(e) for e in self.elevation_deg)
        a.num_listed = len(self.listed)
        a.key = stream_key(self.seed, STREAM_TAG)


class ProjectileSchedule:
    """`+projectile.*`: the projectiles of one task.  `rigid_body_state` is the task's [N * NB, 13] (or [N, NB, 13]) tensor: the launch reads it in place.
    `env_offset`: global index of this rank's env 0, so the ranks of one run draw disjoint streams from one seed."""
    capturable = True
    _INT = ("life", "countdown", "thrown", "hits", "last_hit")

    def __init__(self, cfg, num_envs, model, rigid_body_state, dt, device, gravity_z=-9.81, friction=1.0, default_seed=0, env_offset=0):
        from . import _lib as L
        self.opt = opt = ProjectileOptions(cfg, model.body_names, dt, default_seed)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"+projectile.* runs phc_proj_advance on the GPU and has no CPU fallback (device {self.device})")
        N, NB, P = int(num_envs), model.num_bodies, opt.count
        if model.num_shapes_collision > L.PROJ_MAX_SHAPES:
            raise ValueError(f"projectile: the model has {model.num_shapes_collision} collision shapes, the launch takes {L.PROJ_MAX_SHAPES}")
        if rigid_body_state.numel() != N * NB * 13 or rigid_body_state.dtype != torch.float32 or not rigid_body_state.is_contiguous():
            raise ValueError("projectile: rigid_body_state must be the task's contiguous float32 [N, NB, 13] tensor")
        self.num_envs, self.num_bodies, self.count, self.env_offset = N, NB, P, int(env_offset)
        dev = self.device
        self._tables = {k: torch.from_numpy(v).to(dev) for k, v in model_tables(model).items()}
        self.bodies = torch.tensor(opt.listed, dtype=torch.int32, device=dev)
        self.force = torch.zeros((N, NB, 3), dtype=torch.float32, device=dev)
        self.torque = torch.zeros((N, NB, 3), dtype=torch.float32, device=dev)
        self._istate = torch.zeros((len(self._INT), P, N), dtype=torch.int32, device=dev)   # rows: _INT (include/phc_amd.h phc_proj_args_t)
        self._istate[4].fill_(-1)
        self._k = torch.zeros(N, dtype=torch.int32, device=dev)
        self._fstate = torch.zeros((P, N, 7), dtype=torch.float32, device=dev).view(-1)    # pos [P, N, 3] | vel [P, N, 3] | mass [P, N]
        self.pos, self.vel = self._fstate[:3 * P * N].view(P, N, 3), self._fstate[3 * P * N:6 * P * N].view(P, N, 3)
        self.mass = self._fstate[6 * P * N:].view(P, N)
        self.pos[..., 2] = -1000.0
        self._rbs = rigid_body_state
        self.marker_cache = {}   # render.projectile_markers: the per-marker radii / colours of this task's frames, on the device
        a = L.ProjArgs()
        a.num_envs, a.num_bodies, a.num_shapes = N, NB, model.num_shapes_collision
        opt.fill(a, float(gravity_z), float(friction))
        a.env_offset = self.env_offset
        t = self._tables
        a.bodies, a.capsules, a.owner = self.bodies.data_ptr(), t["capsules"].data_ptr(), t["owner"].data_ptr()
        a.body_com, a.body_inv_mass, a.body_inv_inertia = t["com"].data_ptr(), t["inv_mass"].data_ptr(), t["inv_inertia"].data_ptr()
        a.rigid_body_state = rigid_body_state.data_ptr()
        for i, name in enumerate(self._INT):
            setattr(a, name, self._istate[i].data_ptr())
        a.k, a.pos, a.vel, a.mass = self._k.data_ptr(), self.pos.data_ptr(), self.vel.data_ptr(), self.mass.data_ptr()
        a.force, a.torque = self.force.data_ptr(), self.torque.data_ptr()
        self._args, self._lib, self._check = a, L.load(), L.check

    life = property(lambda self: self._istate[0])
    countdown = property(lambda self: self._istate[1])
    last_hit = property(lambda self: self._istate[4])

    @property
    def thrown(self):
        """Projectiles thrown so far, all envs and slots: a 0-dim device tensor."""
        return self._istate[2].sum()

    @property
    def hits(self):
        """Impacts on bodies so far, all envs and slots: a 0-dim device tensor."""
        return self._istate[3].sum()

    def advance(self, progress_buf=None):
        """Once per env step, in front of the physics.  `progress_buf` int64 [N] as the task holds it: an env at progress 0 was reset since the last step.
        Afterwards `force` / `torque` hold what acts during this step."""
        if progress_buf is not None and (progress_buf.dtype != torch.int64 or progress_buf.shape != (self.num_envs,) or not progress_buf.is_contiguous()
                                         or progress_buf.device != self.force.device):
            raise ValueError("ProjectileSchedule.advance takes the task's progress_buf: a contiguous int64 [num_envs] tensor on the schedule's device")
        self._args.progress_buf = None if progress_buf is None else progress_buf.data_ptr()
        self._check(self._lib.phc_proj_advance(self._args, torch.cuda.current_stream(self.device).cuda_stream), "phc_proj_advance")

    def shadow_of(self, tensors):
        """Shadow copies of the task's simulator tensors (each contiguous float32 with num_envs rows) and the two phc_proj_rows launches over them:
        `snapshot()` copies every row into the shadows, `select()` takes the shadows' rows back for the envs a projectile struck in this step.  -> the shadows."""
        from . import _lib as L
        if not 1 <= len(tensors) <= L.PROJ_MAX_ROWSETS:
            raise ValueError(f"projectile: 1 to {L.PROJ_MAX_ROWSETS} tensors can be shadowed, not {len(tensors)}")
        shadows = []
        for t in tensors:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() % self.num_envs or t.numel() == 0 or t.device != self.force.device:
                raise ValueError("projectile: a shadowed tensor is contiguous float32 on the schedule's device with num_envs rows")
            shadows.append(t.clone())
        self._rows = []
        for mode in (L.PROJ_SNAPSHOT, L.PROJ_SELECT):
            a = L.ProjRows()
            a.num_envs, a.count, a.num_sets, a.mode, a.last_hit = self.num_envs, self.count, len(tensors), mode, self._istate[4].data_ptr()
            for i, (t, s) in enumerate(zip(tensors, shadows)):
                a.base[i], a.shadow[i], a.width[i] = t.data_ptr(), s.data_ptr(), t.numel() // self.num_envs
            self._rows.append(a)
        self._shadowed = (list(tensors), shadows)   # (held: the launches keep raw pointers only)
        return shadows

    def snapshot(self):
        self._check(self._lib.phc_proj_rows(self._rows[0], torch.cuda.current_stream(self.device).cuda_stream), "phc_proj_rows")

    def select(self):
        self._check(self._lib.phc_proj_rows(self._rows[1], torch.cuda.current_stream(self.device).cuda_stream), "phc_proj_rows")

    def state_dict(self):
        """The device state for a checkpoint, as host tensors (a sync: not for use under stream capture)."""
        return {"int": self._istate.cpu(), "k": self._k.cpu(), "float": self._fstate.cpu(), "force": self.force.cpu(), "torque": self.torque.cpu()}

    def fits(self, sd):
        return all(k in sd for k in ("int", "k", "float", "force", "torque")) and tuple(sd["int"].shape) == tuple(self._istate.shape) and tuple(sd["force"].shape) == tuple(self.force.shape)

    def load_state_dict(self, sd):
        if not self.fits(sd):
            raise ValueError(f"projectile state of another size: {tuple(sd['int'].shape)}, this schedule has {tuple(self._istate.shape)}")
        self._istate.copy_(sd["int"])
        self._k.copy_(sd["k"])
        self._fstate.copy_(sd["float"])
        self.force.copy_(sd["force"])
        self.torque.copy_(sd["torque"])
