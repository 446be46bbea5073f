"""HumanoidImGetup: fall-recovery episodes on top of HumanoidIm (reference: phc/env/tasks/humanoid_im_getup.py:42-216).

A reset env becomes, with the reference's probabilities,
  * a RECOVERY episode  -- it had terminated (fallen) and simply keeps its state for `recoverySteps` steps (:160-164),
  * a FALL episode      -- it is teleported to one of the pre-generated fall states (:166-183), or
  * a normal reference-state-init episode (HumanoidIm reset kernel).
While `_recovery_counter > 0` the env is neither reset nor does its motion clock advance (:203-216) -- that gating
runs inside the post-physics kernel (`phc_im_buffers_t.recovery_counter`).  Fall states come from the HIP stepper:
random root orientation, zero joint state, one random action held for 150 `simulate` calls (:83-129), in ONE launch.

`+env.task_rng=device`: `reset_done()` decides the kinds, assigns the fall-state slots and teleports on the device (phc_getup_assign, csrc/phc_getup.h) and
resets by masks -- four launches, no listing of the done envs on the host, so the step is capturable.  Same rules, other numbers.  `reset(env_ids)` keeps the
torch path below in either mode (it never runs inside a capture) and works on the same `availalbe_fall_states` / `fall_id_assignments` the launch reads.
"""
import torch

from ... import _lib as L
from ...utils.flags import flags
from ... import abi
from .humanoid_im import GETUP_DRAWS_TAG, HumanoidIm, _stream


class HumanoidImGetup(HumanoidIm):

    _use_reset_list = False   # episode kinds are decided on the host: the done envs are listed there

    def __init__(self, cfg, sim_params=None, physics_engine=None, device_type="cuda", device_id=0, headless=True):
        super().__init__(cfg=cfg, sim_params=sim_params, physics_engine=physics_engine, device_type=device_type, device_id=device_id,
                         headless=headless)
        self._generate_fall_states()

    def _load_humanoid_configs(self):
        env = self.cfg["env"]
        self._recovery_episode_prob_tgt = self._recovery_episode_prob = env["recoveryEpisodeProb"]
        self._recovery_steps_tgt = self._recovery_steps = env["recoverySteps"]
        self._fall_init_prob_tgt = self._fall_init_prob = env["fallInitProb"]
        if flags.server_mode:
            self._recovery_episode_prob_tgt = self._recovery_episode_prob = 1
            self._fall_init_prob_tgt = self._fall_init_prob = 0
        self.getup_udpate_epoch = env.get("getup_udpate_epoch", 10000)
        self._reset_fall_env_ids = []
        super()._load_humanoid_configs()

    def _allocate_im_state(self):
        super()._allocate_im_state()
        n, dev = self.num_envs, self.device
        self._recovery_counter = torch.zeros(n, device=dev, dtype=torch.int)  # (the kernel buffers point at it)
        self.availalbe_fall_states = torch.zeros(n, device=dev, dtype=torch.long)
        self.fall_id_assignments = torch.zeros(n, device=dev, dtype=torch.long)
        if self.task_rng == "device":
            # what phc_getup_assign reads and writes.  All of it, the fall states included, is allocated here once and overwritten in place
            # (_generate_fall_states, update_getup_schedule): a captured step holds the addresses across resample_motions()
            from ...perturb import stream_key
            self._getup_key = stream_key(self._task_seed, GETUP_DRAWS_TAG)
            self._getup_prob = torch.zeros(2, device=dev, dtype=torch.float32)      # p_recovery, p_fall
            self._getup_k = torch.zeros(n, device=dev, dtype=torch.int32)           # draws per env
            self._getup_count = torch.zeros(1, device=dev, dtype=torch.long)        # launches (the slot permutation's counter)
            self._getup_kind = torch.zeros(n, device=dev, dtype=torch.int32)        # 0 not done, 1 NORMAL, 2 RECOVERY, 3 FALL
            self._getup_normal = torch.zeros(n, device=dev, dtype=torch.long)       # stands in for reset_buf in the NORMAL envs' phc_im_reset_done
            self._getup_fall_list = torch.full((n,), n, device=dev, dtype=torch.long)
            self._getup_free_list = torch.zeros(n, device=dev, dtype=torch.int32)
            self._fall_root_states = torch.zeros((n, 13), device=dev, dtype=torch.float32)
            self._fall_dof_pos = torch.zeros((n, self.num_dof), device=dev, dtype=torch.float32)
            self._fall_dof_vel = torch.zeros((n, self.num_dof), device=dev, dtype=torch.float32)
            self._write_getup_prob()

    # ------------------------------------------------------------------ schedule (:71-78)
    def update_getup_schedule(self, epoch_num, getup_udpate_epoch=5000):
        warm = epoch_num > getup_udpate_epoch
        self._recovery_episode_prob = self._recovery_episode_prob_tgt if warm else 0
        self._fall_init_prob = self._fall_init_prob_tgt if warm else 1
        if self.task_rng == "device":
            self._write_getup_prob()

    def _write_getup_prob(self):
        """The two probabilities into the device array the (possibly captured) phc_getup_assign launch reads."""
        self._getup_prob.copy_(torch.tensor([float(self._recovery_episode_prob), float(self._fall_init_prob)], dtype=torch.float32))

    # ------------------------------------------------------------------ fall states (:83-129)
    def _generate_fall_states(self, max_steps=150):
        N = self.num_envs
        root = self._initial_humanoid_root_states.clone()
        root[:, 3:7] = torch.nn.functional.normalize(torch.randn(N, 4, device=self.device), dim=-1)  # random root orientation
        self._root_states.copy_(root)
        self._dof_state.zero_()
        rand_actions = torch.rand(N, self.get_dof_action_size(), device=self.device) - 0.5        # U(-0.5, 0.5)
        self.pre_physics_step(rand_actions)
        L.check(self._lib.phc_sim_step(self._model_struct, self._sim_params, self._sim_struct, self.actions.data_ptr(),
                                       self._pd_action_offset.data_ptr(), self._pd_action_scale.data_ptr(), self._freeze_mask.data_ptr(),
                                       max_steps, _stream()), "phc_sim_step")
        if self.task_rng == "device":   # in place: see _allocate_im_state
            self._fall_root_states.copy_(self._humanoid_root_states)
            self._fall_root_states[:, 7:13] = 0
            self._fall_dof_pos.copy_(self._dof_pos)
        else:
            self._fall_root_states = self._humanoid_root_states.clone()
            self._fall_root_states[:, 7:13] = 0
            self._fall_dof_pos = self._dof_pos.clone()
            self._fall_dof_vel = torch.zeros_like(self._dof_vel)
        self.availalbe_fall_states[:] = 0
        self.fall_id_assignments[:] = 0
        self._recovery_counter.zero_()

    def resample_motions(self):
        self._reload_motions()
        if not flags.test:
            self._generate_fall_states()
        self.reset()

    # ------------------------------------------------------------------ reset (:131-196)
    def _reset_envs(self, env_ids):
        if len(env_ids) == 0:
            return
        env_ids = torch.as_tensor(env_ids, device=self.device).to(torch.long)
        self.availalbe_fall_states[self.fall_id_assignments[env_ids]] = 0
        n = env_ids.shape[0]
        want_recovery = torch.bernoulli(torch.full((n,), float(self._recovery_episode_prob), device=self.device)) == 1.0
        recovery_mask = want_recovery & (self._terminate_buf[env_ids] == 1)    # only envs that really fell (:140-142)
        recovery_ids = env_ids[recovery_mask]
        rest = env_ids[~recovery_mask]
        fall_mask = torch.bernoulli(torch.full((rest.shape[0],), float(self._fall_init_prob), device=self.device)) == 1.0
        fall_ids, normal_ids = rest[fall_mask], rest[~fall_mask]
        self._reset_fall_env_ids = fall_ids
        if len(fall_ids) > 0:
            self._reset_fall_episode(fall_ids)
        if len(recovery_ids) > 0:
            self._reset_from_state(recovery_ids, refresh=False, fill_history=False)
        if len(normal_ids) > 0:
            super()._reset_envs(normal_ids)      # zeroes _recovery_counter of these envs (:155)
        if len(fall_ids) + len(recovery_ids) > 0:
            self._recovery_counter[torch.cat([fall_ids, recovery_ids])] = self._recovery_steps

    def _reset_fall_episode(self, env_ids):
        free = (self.availalbe_fall_states == 0).nonzero().squeeze(-1)
        assert free.shape[0] >= env_ids.shape[0]
        pick = free[torch.randperm(free.shape[0], device=self.device)][:env_ids.shape[0]]
        self._humanoid_root_states[env_ids] = self._fall_root_states[pick]
        self._dof_pos[env_ids] = self._fall_dof_pos[pick]
        self._dof_vel[env_ids] = self._fall_dof_vel[pick]
        self.availalbe_fall_states[pick] = 1
        self.fall_id_assignments[env_ids] = pick
        self._reset_from_state(env_ids, refresh=True, fill_history=True)

    def _reset_from_state(self, env_ids, refresh, fill_history):
        ids = env_ids.contiguous()
        n = ids.shape[0]
        if refresh:
            L.check(self._lib.phc_refresh_body_state_indexed(self._model_struct, self._sim_struct, n, ids.data_ptr(), _stream()),
                    "phc_refresh_body_state_indexed")
        L.check(self._lib.phc_im_reset_from_state(self._model_struct, self._motion_lib.struct, self._im_params, self._sim_struct,
                                                  self._reset_prologue(from_state=True), n, ids.data_ptr(), int(fill_history), _stream()),
                "phc_im_reset_from_state")

    def reset_done(self):
        """Three kinds of episode need host-side bookkeeping, so the done envs are listed (as the reference's rollout does)."""
        if self.task_rng == "device":
            return self._reset_done_device()
        ids = self.reset_buf.nonzero(as_tuple=False).flatten()
        if len(ids) > 0:
            self._reset_envs(ids)

    # ------------------------------------------------------------------ env.task_rng=device
    def _getup_args(self):
        """The phc_getup_args_t of the launch; rebuilt when any tensor it points at was rebound (as `_buffers` does)."""
        tensors = (self.reset_buf, self._terminate_buf, self._root_states, self._dof_state, self.availalbe_fall_states, self.fall_id_assignments,
                   self._recovery_counter, self._fall_root_states, self._fall_dof_pos)
        hit = self.__dict__.get("_getup_args_cache")
        if hit is None or any(a is not b for a, b in zip(hit[1], tensors)):
            a = abi.getup_args_struct(num_envs=self.num_envs, num_dof=self.num_dof, key=self._getup_key, env_offset=self._task_env_offset, prob=self._getup_prob,
                                      reset_buf=self.reset_buf, terminate_buf=self._terminate_buf, fall_root=self._fall_root_states,
                                      fall_dof_pos=self._fall_dof_pos, root_states=self._root_states, dof_state=self._dof_state,
                                      avail=self.availalbe_fall_states, assign=self.fall_id_assignments, recovery_counter=self._recovery_counter,
                                      k=self._getup_k, launch_count=self._getup_count, kind=self._getup_kind, normal_flag=self._getup_normal,
                                      fall_list=self._getup_fall_list, free_list=self._getup_free_list)
            hit = self.__dict__["_getup_args_cache"] = (a, tensors)
        hit[0].recovery_steps = int(self._recovery_steps)
        return hit[0]

    def _reset_done_device(self):
        """reset_done() as four launches and no host read: (1) phc_getup_assign -- kinds, slots, teleports, counters; (2) the body state of the FALL envs from
        their teleported joint state; (3) FALL (history filled) and RECOVERY (history kept) envs reset from their state, by `kind`; (4) the NORMAL envs
        through the base class's phc_im_reset_done in its masked-sweep form, with the launch's NORMAL flags in place of reset_buf in that one launch's
        buffers.  (zero_out_far_train adds its phc_task_draws in front of (4), where the torch path has its torch.rand.)"""
        s = _stream()
        L.check(self._lib.phc_getup_assign(self._getup_args(), s), "phc_getup_assign")
        L.check(self._lib.phc_refresh_body_state_masked(self._model_struct, self._sim_struct, self._getup_fall_list.data_ptr(), s),
                "phc_refresh_body_state_masked")
        L.check(self._lib.phc_im_reset_from_state_masked(self._model_struct, self._motion_lib.struct, self._im_params, self._sim_struct,
                                                         self._reset_prologue(from_state=True), self._getup_kind.data_ptr(), s),
                "phc_im_reset_from_state_masked")
        start_at_zero = (self._state_init == HumanoidIm.StateInit.Start) or flags.test
        buf = self._reset_prologue()
        flags_of_all, buf.reset_list, buf.reset_buf = buf.reset_buf, None, self._getup_normal.data_ptr()
        try:
            L.check(self._lib.phc_im_reset_done(self._model_struct, self._motion_lib.struct, self._im_params, self._sim_struct, buf,
                                                self._reset_seed, self._reset_counter + 1, int(bool(start_at_zero)), s), "phc_im_reset_done")
        finally:
            buf.reset_buf = flags_of_all   # (the struct is the cached one of `_buffers`)
        self._reset_done_host(False)
        self._obs_noise(reset_rows=True)

    def _reset_done_capturable(self):
        """In device mode this class's reset_done() is launches plus `_reset_done_host` only."""
        return self.task_rng == "device" and type(self).reset_done is HumanoidImGetup.reset_done

    def _task_rng_state(self):
        state = super()._task_rng_state()
        state.update(getup_k=self._getup_k.cpu(), getup_count=int(self._getup_count.item()))
        return state

    def _load_task_rng_state(self, saved):
        super()._load_task_rng_state(saved)
        if "getup_k" in saved:
            self._getup_k.copy_(saved["getup_k"])
            self._getup_count.fill_(int(saved["getup_count"]))
