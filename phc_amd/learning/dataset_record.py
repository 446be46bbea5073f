"""`collect_dataset=True`: record (observation, clean action, noisy action, reset flag) rows while the evaluation sweep runs -- the player's dataset dump
(phc/learning/im_amp_players.py:44-50,95-99,132-151,200-214 with humanoid.py:1530-1535, humanoid_im.py:683-690,950-953).

Per batch of the sweep the recorder owns `obs_prev` (the task's observation BEFORE the step: seeded after the batch's reset, refreshed after every step) and
a clip-major block on the task's device: env i with `rows[i] = num_steps[i] - 1` rows starting at `row_start[i]`.  On a HIP device every env step is ONE
launch (`phc_dataset_record`, issued behind the post-physics launch on the same stream) and the block is copied to the host once, when the batch ends;
`record_rows` is the torch statement of the same rule, used when the task's tensors are not on a HIP device."""
import ctypes as C
import os
from datetime import datetime

import numpy as np
import torch

BACKEND = None   # None: the launch on a HIP device, the torch statement elsewhere; "torch": the torch statement everywhere (tests compare the two)


def record_rows(step, rows, row_start, obs_prev, obs_buf, clean_actions, actions, reset_buf, block):
    """The row rule in torch: env i with step < rows[i] stores (obs_prev[i], clean_actions[i], actions[i], reset_buf[i]) at row row_start[i] + step of
    block = (obs, clean, env, reset); then obs_prev = obs_buf for every env."""
    sel = torch.nonzero(step < rows).flatten()
    r = row_start[sel] + step
    for dst, src in zip(block, (obs_prev, clean_actions, actions, reset_buf)):
        dst[r] = src[sel]
    obs_prev.copy_(obs_buf)


class DatasetRecorder:
    def __init__(self, task):
        self.task = task
        self.obs, self.clean, self.env, self.reset, self.keys, self.lengths = [], [], [], [], [], []   # per clip, in the order the sweep visits them
        self._block = None

    def begin_batch(self, num_steps, keys):
        """After the batch's `env.reset()`: `num_steps` [N] of the loaded clips (wrapped-around duplicates of the last batch included), their keys."""
        t = self.task
        dev = t.obs_buf.device
        rows = np.maximum(np.asarray(num_steps, dtype=np.int64) - 1, 0)
        start = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
        self._rows_host, self._start_host, self._keys, self._step, self._capacity = rows, start, [str(k) for k in keys], 0, max(int(rows.sum()), 1)
        self._rows, self._start = torch.from_numpy(rows).to(dev), torch.from_numpy(start).to(dev)
        self._block = None      # allocated by the first record(): the action width is the stepped task's (an MCP task composes num_dof actions from num_prim weights)
        self._obs_prev = t.obs_buf.detach().to(torch.float32).clone()
        self._launch = dev.type == "cuda" and BACKEND != "torch"

    def record(self):
        """After an env step of the sweep."""
        t = self.task
        f32 = lambda x: x.detach().to(torch.float32).contiguous()
        obs_buf, clean, act, reset = f32(t.obs_buf), f32(t.clean_actions), f32(t.actions), t.reset_buf.detach().to(torch.int64).contiguous()
        if self._block is None:
            R, dev = self._capacity, obs_buf.device
            self._block = (torch.empty((R, obs_buf.shape[1]), dtype=torch.float32, device=dev), torch.empty((R, clean.shape[1]), dtype=torch.float32, device=dev),
                           torch.empty((R, clean.shape[1]), dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int64, device=dev))
        if self._launch:
            from .. import _lib as L
            from ..abi import record_args_struct
            obs, cl, en, rs = self._block
            a = record_args_struct(obs_buf.shape[0], obs_buf.shape[1], clean.shape[1], self._step, self._capacity, obs_buf=obs_buf, obs_prev=self._obs_prev,
                                   clean_actions=clean, actions=act, reset_buf=reset, rows=self._rows, row_start=self._start, obs=obs, clean=cl, env=en, reset=rs)
            L.check(L.load().phc_dataset_record(C.byref(a), torch.cuda.current_stream(obs_buf.device).cuda_stream), "phc_dataset_record")
        else:
            record_rows(self._step, self._rows, self._start, self._obs_prev, obs_buf, clean, act, reset, self._block)
        self._step += 1

    def end_batch(self):
        """One copy of the block to the host; every clip trimmed to min(T_batch, rows) (a batch may stop early: all envs terminated)."""
        if self._block is None:      # (a batch without a step)
            return
        host = [b.cpu().numpy() for b in self._block]
        for i, (n, s) in enumerate(zip(self._rows_host, self._start_host)):
            n = min(int(n), self._step)
            for dst, src in zip((self.obs, self.clean, self.env, self.reset), host):
                dst.append(src[s:s + n].copy())
            self.lengths.append(n)
        self.keys += self._keys
        self._block = None

    def dataset(self, running_mean=None, config=None):
        """What the reference's player dumps (im_amp_players.py:205-214)."""
        return {"obs": self.obs, "clean_action": self.clean, "env_action": self.env, "key_names": np.array(self.keys), "motion_lengths": np.array(self.lengths),
                "reset": np.concatenate(self.reset) if self.reset else np.zeros(0, dtype=np.int64), "running_mean": running_mean, "config": config}

    def dump(self, output_path, running_mean=None, log=print):
        """-> <output_path>/phc_act/<motion file stem>/noise_<add_action_noise>_<action_noise_std>_<date>.pkl (the trainer's file sampler splits the name at `_`)."""
        import joblib
        t = self.task
        cfg = getattr(t, "cfg", None)
        motion_file = str(cfg["env"]["motion_file"]).split("/")[-1].split(".")[0] if cfg is not None else "motions"
        d = os.path.join(str(output_path), "phc_act", motion_file)
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"noise_{bool(getattr(t, '_add_action_noise', False))}_{getattr(t, '_action_noise_std', 0.0)}_{datetime.now().strftime('%Y-%m-%d-%H:%M:%S')}.pkl")
        if log is not None:
            log(f"Dumping to: {path}")
        joblib.dump(self.dataset(running_mean, cfg), path, compress=True)
        return path
