"""HumanoidTeleop: the sim-to-real half of the robots' training task on top of HumanoidIm (reference: phc/env/tasks/humanoid_teleop.py:35-307).

  * regularisation rewards (:176-307): every `r_<term>` key of `env.reward_specs` with a non-zero scale adds `term * scale * dt` to the reward and a column
    to `reward_raw`, behind the imitation (and power) columns, in the dict's order.  Terms (`_lib.TELEOP_TERMS`): dof_pos_limits, torque_limits, torques,
    dof_vel, dof_acc, action_rate, slippage, feet_contact_forces (`reward_specs.max_contact_force`), stumble, feet_air_time_teleop, feet_ori;
  * recovery window (:95-101,167-174): for `env.push_recovery_steps` (60) steps from a velocity push of `domain_rand.push_robots` on, the env is neither
    reset nor is its motion clock advanced.

Both are ONE launch per env step, phc_teleop_rewards (include/phc_amd.h), issued right behind phc_im_post_physics through HumanoidIm's
`_post_physics_launch` hook: `post_physics_step` is not overridden, so the whole rollout step stays capturable.  The state the terms keep -- `last_actions`,
`last_dof_vel`, `feet_air_time`, `last_contacts` -- lives on the device and, as in the reference (:104-118), is NOT cleared when an env is reset: the first
dof_acc / action_rate of an episode compares against the last step of the previous one.

Not built (refused by name): `control.action_filter` (the Butterworth low-pass of :50-54,75-76), `env.cycle_motion` (its start-time rewrite moves the
reward's lookup time), r_torques / r_torque_limits outside `control.control_mode=pd` (the reference has no `self.torques` there).  The reference's
observation noise (`add_noise`, :424-437) is non-zero only for the teleop observation layouts, which are not built: nothing is applied."""
import numpy as np
import torch

from ... import _lib as L
from ... import abi
from .humanoid_im import HumanoidIm, _stream

_IM_REWARD_DEFAULTS = {"k_pos": 100, "k_rot": 10, "k_vel": 0.1, "k_ang_vel": 0.1, "w_pos": 0.5, "w_rot": 0.3, "w_vel": 0.1, "w_ang_vel": 0.1}   # humanoid_im.py:202


class HumanoidTeleop(HumanoidIm):

    # ---- host phase: options ----
    def _load_humanoid_configs(self):
        super()._load_humanoid_configs()
        env, control = self.cfg["env"], self.cfg["control"]
        specs = dict(env.get("reward_specs", {}) or {})
        self.reward_specs = {**_IM_REWARD_DEFAULTS, **specs}   # (a reward_specs that names only r_* keys keeps the imitation gains)
        self._teleop_specs = specs
        if control.get("action_filter", False):
            raise NotImplementedError("control.action_filter=True: HumanoidTeleop's Butterworth action filter (humanoid_teleop.py:50-54,75-76) is not built")
        if self.cycle_motion:
            raise NotImplementedError("env.cycle_motion=True with HumanoidTeleop: the clip restart rewrites the start times the reward terms look the reference up at")
        self._recovery_steps = int(env.get("push_recovery_steps", 60))   # humanoid_teleop.py:44,101 hard-codes 60
        if self._recovery_steps < 0:
            raise ValueError("env.push_recovery_steps must be >= 0")

    def _setup_im_options(self):
        super()._setup_im_options()
        self._prepare_reward_function()

    def _prepare_reward_function(self):
        """humanoid_teleop.py:176-199: the r_* keys with a non-zero scale, in the dict's order, each scale multiplied by dt."""
        self.reward_names, self.reward_scales = [], {}
        for key, scale in self._teleop_specs.items():
            if not str(key).startswith("r_"):
                continue
            if key[2:] not in L.TELEOP_TERMS:
                raise ValueError(f"env.reward_specs.{key}: no such reward term; built: {', '.join('r_' + t for t in L.TELEOP_TERMS)}")
            if float(scale) == 0:
                continue
            self.reward_names.append(key)
            self.reward_scales[key] = float(scale) * self.dt
        self.max_contact_force = float(self._teleop_specs.get("max_contact_force", 0.0))
        terms = [n[2:] for n in self.reward_names]
        for t in ("torques", "torque_limits"):
            if t in terms and self.control_mode != "pd":
                raise NotImplementedError(f"env.reward_specs.r_{t} needs control.control_mode=pd (the explicit-PD torque is what the reference's self.torques holds; "
                                          f"it has none under {self.control_mode!r})")
        if "feet_contact_forces" in terms and "max_contact_force" not in self._teleop_specs:
            raise ValueError("env.reward_specs.r_feet_contact_forces needs env.reward_specs.max_contact_force")
        feet = list(self.cfg["env"]["contact_bodies"])
        if "feet_ori" in terms and len(feet) < 2:
            raise ValueError("env.reward_specs.r_feet_ori needs two feet: env.contact_bodies has fewer than two bodies")
        if len(feet) > L.TELEOP_MAX_FEET:
            raise ValueError(f"HumanoidTeleop takes at most {L.TELEOP_MAX_FEET} env.contact_bodies")
        self._feet = [self._body_names.index(b) for b in feet]
        self.num_im_reward_columns = 5 if self.power_reward else 4
        self.num_reward_columns = self.num_im_reward_columns + len(self.reward_names)

    # ---- device phase ----
    def _allocate_im_state(self):
        super()._allocate_im_state()
        N, D, dev, F = self.num_envs, self.num_dof, self.device, len(self._feet)
        f32 = dict(device=dev, dtype=torch.float32)
        # phc_im_post_physics writes its columns with a row stride of their own count: it keeps a private tensor, the launch behind it fills the public one
        self._reward_raw_im = self.reward_raw
        self.reward_raw = torch.zeros((N, self.num_reward_columns), **f32)
        self._recovery_counter = torch.zeros(N, device=dev, dtype=torch.int)   # phc_im_buffers_t.recovery_counter: the gate of the post-physics launch
        self.last_actions = torch.zeros((N, self.num_actions), **f32)
        self.last_dof_vel = torch.zeros((N, D), **f32)
        self.feet_air_time = torch.zeros((N, F), **f32)
        self.last_contacts = torch.zeros((N, F), device=dev, dtype=torch.uint8)
        self.feet_indices = self._contact_body_ids
        lo, hi = (x.astype(np.float32).copy() for x in self.model.dof_limits())
        free = (lo == 0) & (hi == 0)       # humanoid.py:1012-1014: a DoF without limits gets +-pi
        lo[free], hi[free] = -np.pi, np.pi
        self.dof_pos_limits = torch.from_numpy(np.stack([lo, hi], axis=-1)).to(dev)
        self._dof_pos_limits_lo, self._dof_pos_limits_hi = self.dof_pos_limits[:, 0].contiguous(), self.dof_pos_limits[:, 1].contiguous()
        self._teleop_args = None

    def _buffer_tensors(self):
        return super()._buffer_tensors() + (self.__dict__.get("_reward_raw_im"),)

    def _buffers_uncached(self, amp_in, amp_out):
        b = super()._buffers_uncached(amp_in, amp_out)
        b.reward_raw = self._reward_raw_im.data_ptr()
        return b

    def _teleop_struct(self):
        """phc_teleop_args_t of this task; rebuilt when a tensor it points at was rebound (`actions` is the caller's tensor: set per launch)."""
        dr = self._dr if (self._dr is not None and self._dr.push_interval > 0) else None
        tensors = (self._dof_state, self.dof_force_tensor, self._contact_forces, self._rigid_body_state, self.progress_buf, self._motion_start_times,
                   self._motion_start_times_offset, self._recovery_counter, self.last_actions, self.last_dof_vel, self.feet_air_time, self.last_contacts,
                   self.rew_buf, self._reward_raw_im, self.reward_raw, self.torque_limits, None if dr is None else dr.k)
        hit = self._teleop_args
        if hit is None or any(a is not b for a, b in zip(hit[1], tensors)):
            terms = [n[2:] for n in self.reward_names]
            args = abi.teleop_args_struct(
                self.num_envs, self.num_dof, self.rew_buf, self.reward_raw, reward_im=self._reward_raw_im, terms=terms,
                scales={n[2:]: self.reward_scales[n] for n in self.reward_names}, dt=self.dt, num_bodies=self.num_bodies, feet=self._feet,
                max_contact_force=self.max_contact_force, push_interval=0 if dr is None else dr.push_interval, recovery_steps=self._recovery_steps,
                dof_state=self._dof_state, dof_limits_lower=self._dof_pos_limits_lo, dof_limits_upper=self._dof_pos_limits_hi,
                torque_limits=self.torque_limits, dof_force=self.dof_force_tensor, contact_force=self._contact_forces,
                rigid_body_state=self._rigid_body_state, progress_buf=self.progress_buf, motion_start_times=self._motion_start_times,
                motion_start_times_offset=self._motion_start_times_offset, dr_k=None if dr is None else dr.k, recovery_counter=self._recovery_counter,
                last_actions=self.last_actions, last_dof_vel=self.last_dof_vel, feet_air_time=self.feet_air_time, last_contacts=self.last_contacts)
            hit = self._teleop_args = (args, tensors)
        return hit[0]

    def _post_physics_launch(self):
        """HumanoidIm.post_physics_step's hook, right behind phc_im_post_physics on its stream."""
        a = self._teleop_struct()
        act = self.actions
        if act.dtype != torch.float32 or not act.is_contiguous() or tuple(act.shape) != (self.num_envs, self.num_dof):
            raise ValueError("HumanoidTeleop takes contiguous fp32 actions [num_envs, num_dof]")
        a.actions = act.data_ptr()
        a.sampled_motion_ids = None if self._motion_ids_are_identity() else self._sampled_motion_ids.data_ptr()
        L.check(self._lib.phc_teleop_rewards(self._motion_lib.struct, a, _stream()), "phc_teleop_rewards")
