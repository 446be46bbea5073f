"""Scheduled pushes (config group `perturb`): a random force on one body of every env every few seconds, so that play and the evaluation sweep
measure recovery.  The reference has only the viewer's "apply_force" key for this (phc/env/tasks/base_task.py:372-381).

    +perturb.force=[200,400]        # N, magnitude uniform in the range
    +perturb.bodies=[Pelvis,Torso]  # body names; default: the root body; one drawn per push
    +perturb.interval_s=[2,4]       # pause between the end of a push and the next, uniform
    +perturb.duration_s=0.1         # max(1, round(duration / dt)) env steps, whole env steps
    +perturb.direction=horizontal   # uniform azimuth, z = 0  |  any: uniform on the sphere
    +perturb.seed=<cfg.seed>
    +perturb.rng=torch              # torch: `PushSchedule`, play and evaluation  |  device: `DevicePushSchedule`, training too

All state lives on the task's device and `advance()` is a fixed sequence of torch ops: no host sync, the same number of random draws in every step.  The
draws come from a generator of the schedule's own, so a configured schedule leaves every other random stream of the run untouched.  The force buffer
`force` [N, NB, 3] (env axes, at the bodies' centres of mass) keeps its address: `HumanoidIm` hands it to phc_sim_step_wrench in every step, zero between pushes.

`rng=device` is the same schedule as ONE HIP launch (phc_push_advance, include/phc_amd.h): its draws are counter-based hashes of (seed, env, the env's own
step count), so the learner's captured rollout step (IMAmpAgent.play_steps) draws anew on every replay -- a captured `torch.Generator` would repeat itself.
The two implementations follow the same rules and draw different numbers."""
import math

import torch

RNG_MODES = ("torch", "device")


def make_schedule(cfg, num_envs, body_names, dt, device, default_seed=0, env_offset=0):
    """The schedule `+perturb.rng` names (default: torch); the classes check the option's value."""
    if str(dict(cfg).get("rng", "torch")) == "device":
        return DevicePushSchedule(cfg, num_envs, body_names, dt, device, default_seed=default_seed, env_offset=env_offset)
    return PushSchedule(cfg, num_envs, body_names, dt, device, default_seed=default_seed)


def _pair(v, name):
    lo, hi = (v, v) if isinstance(v, (int, float)) else tuple(v)
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo <= hi):
        raise ValueError(f"perturb.{name} must be a number or [low, high] with 0 <= low <= high, not {v!r}")
    return lo, hi


class _Schedule:
    """What the two schedules share: the options of the `perturb` group."""
    rng = None           # the `perturb.rng` value the class implements
    capturable = False   # may `advance()` be captured in a hipGraph and replayed?  (the learner's whole-step rollout graph)

    def _configure(self, cfg, num_envs, body_names, dt, device, default_seed):
        """The options both schedules share -> attributes of `self`; returns the listed bodies' indices."""
        cfg = dict(cfg)
        unknown = set(cfg) - {"force", "bodies", "interval_s", "duration_s", "direction", "seed", "rng"}
        if unknown:
            raise ValueError(f"unknown perturb option(s): {sorted(unknown)}")
        rng = str(cfg.get("rng", self.rng))
        if rng not in RNG_MODES:
            raise ValueError(f"perturb.rng must be torch or device, not {rng!r}")
        if rng != self.rng:
            raise ValueError(f"perturb.rng={rng} is not {type(self).__name__}: perturb.make_schedule builds the schedule the option names")
        if "force" not in cfg:
            raise ValueError("perturb.force (newtons, a number or [low, high]) is required")
        self.force_range = _pair(cfg["force"], "force")
        names = cfg.get("bodies", None) or [body_names[0]]
        names = [names] if isinstance(names, str) else list(names)
        missing = [b for b in names if b not in body_names]
        if missing:
            raise ValueError(f"perturb.bodies: no such body {missing}; the model has {list(body_names)}")
        self.direction = str(cfg.get("direction", "horizontal"))
        if self.direction not in ("horizontal", "any"):
            raise ValueError(f"perturb.direction must be horizontal or any, not {self.direction!r}")
        self.dt = float(dt)
        lo, hi = _pair(cfg.get("interval_s", [2.0, 4.0]), "interval_s")
        self.pause_steps = (max(1, int(round(lo / self.dt))), max(1, int(round(hi / self.dt))))   # the pause is drawn in whole env steps
        self.duration_steps = max(1, int(round(float(cfg.get("duration_s", 0.1)) / self.dt)))
        self.num_envs, self.num_bodies, self.device = int(num_envs), len(body_names), torch.device(device)
        self.seed = int(cfg.get("seed", default_seed))
        return [body_names.index(b) for b in names]


class PushSchedule(_Schedule):
    rng = "torch"         # `advance()` draws from a torch.Generator: a captured hipGraph would freeze its state

    def __init__(self, cfg, num_envs, body_names, dt, device, default_seed=0):
        listed = self._configure(cfg, num_envs, body_names, dt, device, default_seed)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed)
        dev, N = self.device, self.num_envs
        self.bodies = torch.tensor(listed, dtype=torch.long, device=dev)
        self.force = torch.zeros((N, self.num_bodies, 3), dtype=torch.float32, device=dev)
        self.remaining = torch.zeros(N, dtype=torch.long, device=dev)      # env steps the running push still lasts (this one included)
        self.countdown = self._pause(torch.rand(N, generator=self.gen, device=dev))   # force-free env steps before the next push
        self.pushes = torch.zeros((), dtype=torch.long, device=dev)        # pushes started so far, all envs
        self._rows = torch.arange(N, device=dev)

    def _pause(self, u):
        lo, hi = self.pause_steps
        return (lo + torch.floor(u * (hi - lo + 1)).to(torch.long)).clamp_(max=hi)

    def advance(self, reset=None):
        """Once per env step, before the physics.  `reset` [N] bool: envs reset since the last step -- their push ends and a new pause is drawn.
        Afterwards `force` holds what acts during this step."""
        dev, N = self.device, self.num_envs
        u = torch.rand((5, N), generator=self.gen, device=dev)    # pause, magnitude, azimuth, height, body: drawn in every step, used where a push starts or ends
        pause = self._pause(u[0])
        if reset is not None:
            self.remaining = torch.where(reset, torch.zeros_like(self.remaining), self.remaining)
            self.countdown = torch.where(reset, pause, self.countdown)
        start = (self.remaining == 0) & (self.countdown <= 0)
        lo, hi = self.force_range
        mag = lo + u[1] * (hi - lo)
        az = u[2] * (2.0 * math.pi)
        if self.direction == "horizontal":
            z = torch.zeros_like(mag)
            r = torch.ones_like(mag)
        else:
            z = 2.0 * u[3] - 1.0
            r = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
        vec = torch.stack([r * torch.cos(az), r * torch.sin(az), z], dim=-1) * mag[:, None]
        body = self.bodies[torch.floor(u[4] * len(self.bodies)).to(torch.long).clamp_(max=len(self.bodies) - 1)]
        new = torch.zeros_like(self.force)
        new[self._rows, body] = vec
        self.remaining = torch.where(start, torch.full_like(self.remaining, self.duration_steps), self.remaining)
        active = self.remaining > 0
        self.force.copy_(torch.where(start[:, None, None], new, self.force) * active[:, None, None])   # (in place: the stepper holds the address)
        self.pushes += start.sum()
        ended = active & (self.remaining == 1)
        self.remaining = torch.clamp(self.remaining - 1, min=0)
        self.countdown = torch.where(ended, pause, torch.where(active, self.countdown, self.countdown - 1))


def _splitmix64(z):
    """splitmix64 of csrc/phc_rng.h on Python integers."""
    M = (1 << 64) - 1
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def stream_key(seed, tag=0x7075736873636864):   # ("pushschd")
    """The 64-bit stream key of a device schedule.  The tag keeps it apart from the key the reset launch derives from the same run seed for its
    start-time draws (phc_im_reset_done: splitmix64(splitmix64(seed) ^ counter * odd constant)), and the streams of one run apart from each other: the
    push schedule's is the default, the task's own draws (`+env.task_rng=device`) pass theirs."""
    return _splitmix64(_splitmix64(int(seed) & ((1 << 64) - 1)) ^ int(tag))


class DevicePushSchedule(_Schedule):
    """`+perturb.rng=device`: the schedule above with `advance()` as one phc_push_advance launch on the current stream -- no host sync, no host-side
    state, no generator.  `env_offset`: global index of this rank's env 0, so the ranks of one run draw disjoint streams from one seed."""
    rng, capturable = "device", True
    _STATE = ("remaining", "countdown", "body", "k", "started")

    def __init__(self, cfg, num_envs, body_names, dt, device, default_seed=0, env_offset=0):
        from . import _lib as L
        listed = self._configure(cfg, num_envs, body_names, dt, device, default_seed)
        if self.device.type != "cuda":
            raise RuntimeError(f"perturb.rng=device runs phc_push_advance on the GPU and has no CPU fallback (device {self.device}); use perturb.rng=torch")
        if not all(0 <= b < self.num_bodies for b in listed):   # (the launch trusts the device copy)
            raise ValueError(f"perturb.bodies: body indices {listed} outside [0, {self.num_bodies})")
        self.env_offset = int(env_offset)
        dev, N = self.device, self.num_envs
        self.bodies = torch.tensor(listed, dtype=torch.int32, device=dev)
        self.force = torch.zeros((N, self.num_bodies, 3), dtype=torch.float32, device=dev)
        self._state = torch.zeros((len(self._STATE), N), dtype=torch.int32, device=dev)   # rows: _STATE (include/phc_amd.h phc_push_args_t)
        self._state[2].fill_(-1)
        a = L.PushArgs()
        a.num_envs, a.num_bodies, a.num_listed = N, self.num_bodies, len(listed)
        a.pause_lo, a.pause_hi = self.pause_steps
        a.duration, a.direction = self.duration_steps, ("horizontal", "any").index(self.direction)
        a.force_lo, a.force_hi = self.force_range
        a.key, a.env_offset = stream_key(self.seed), self.env_offset
        a.bodies, a.force = self.bodies.data_ptr(), self.force.data_ptr()
        for i, name in enumerate(self._STATE):
            setattr(a, name, self._state[i].data_ptr())
        self._args, self._lib, self._check = a, L.load(), L.check

    remaining = property(lambda self: self._state[0])
    countdown = property(lambda self: self._state[1])

    @property
    def pushes(self):
        """Pushes started so far, all envs: a 0-dim device tensor (the sum of the per-env counts: nothing in the launch is order-dependent)."""
        return self._state[4].sum()

    def advance(self, progress_buf=None):
        """Once per env step, before the physics.  `progress_buf` int64 [N] as the task holds it: an env at progress 0 was reset since the last step."""
        if progress_buf is not None and (progress_buf.dtype != torch.int64 or progress_buf.shape != (self.num_envs,) or not progress_buf.is_contiguous()
                                         or progress_buf.device != self.force.device):
            raise ValueError("DevicePushSchedule.advance takes the task's progress_buf: a contiguous int64 [num_envs] tensor on the schedule's device")
        self._args.progress_buf = None if progress_buf is None else progress_buf.data_ptr()
        self._check(self._lib.phc_push_advance(self._args, torch.cuda.current_stream(self.device).cuda_stream), "phc_push_advance")

    def state_dict(self):
        """The device state for a checkpoint, as host tensors (a sync: not for use under stream capture)."""
        return {"state": self._state.cpu(), "force": self.force.cpu()}

    def fits(self, sd):
        """Is `sd` the state of a schedule of this one's sizes?"""
        return tuple(sd["state"].shape) == tuple(self._state.shape) and tuple(sd["force"].shape) == tuple(self.force.shape)

    def load_state_dict(self, sd):
        if not self.fits(sd):
            raise ValueError(f"push schedule state of another size: {tuple(sd['state'].shape)}, this schedule has {tuple(self._state.shape)}")
        self._state.copy_(sd["state"])
        self.force.copy_(sd["force"])
