"""Scheduled pushes (config group `perturb`): a random force on one body of every env every few seconds, so that play and the evaluation sweep
measure recovery.  The reference has only the viewer's "apply_force" key for this (phc/env/tasks/base_task.py:372-381).

    +perturb.force=[200,400]        # N, magnitude uniform in the range
    +perturb.bodies=[Pelvis,Torso]  # body names; default: the root body; one drawn per push
    +perturb.interval_s=[2,4]       # pause between the end of a push and the next, uniform
    +perturb.duration_s=0.1         # max(1, round(duration / dt)) env steps, whole env steps
    +perturb.direction=horizontal   # uniform azimuth, z = 0  |  any: uniform on the sphere
    +perturb.seed=<cfg.seed>

All state lives on the task's device and `advance()` is a fixed sequence of torch ops: no host sync, the same number of random draws in every step.  The
draws come from a generator of the schedule's own, so a configured schedule leaves every other random stream of the run untouched.  The force buffer
`force` [N, NB, 3] (env axes, at the bodies' centres of mass) keeps its address: `HumanoidIm` hands it to phc_sim_step_wrench in every step, zero between pushes."""
import math

import torch


def _pair(v, name):
    lo, hi = (v, v) if isinstance(v, (int, float)) else tuple(v)
    lo, hi = float(lo), float(hi)
    if not (0.0 <= lo <= hi):
        raise ValueError(f"perturb.{name} must be a number or [low, high] with 0 <= low <= high, not {v!r}")
    return lo, hi


class PushSchedule:
    def __init__(self, cfg, num_envs, body_names, dt, device, default_seed=0):
        cfg = dict(cfg)
        unknown = set(cfg) - {"force", "bodies", "interval_s", "duration_s", "direction", "seed"}
        if unknown:
            raise ValueError(f"unknown perturb option(s): {sorted(unknown)}")
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
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(self.seed)
        dev, N = self.device, self.num_envs
        self.bodies = torch.tensor([body_names.index(b) for b in names], dtype=torch.long, device=dev)
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
