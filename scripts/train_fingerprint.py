"""Fingerprint of three training epochs from a fixed seed: one JSON line with the SHA-256 of the flat parameter, the Adam moments and every
normaliser buffer, the optimizer step count and the number of gradient all-reduces.  Runs are deterministic per seed, so
two commits that compute the same thing print the same line: the check behind a learner refactor.

  python scripts/train_fingerprint.py [--device cuda|cpu] [--rccl] [config overrides ...]

The overrides are `phc_amd.config.compose` overrides (existing config keys only), e.g. `+learning.params.config.hip_graph=False`,
`+learning.params.config.branch_streams=False`, `learning=im_pnn env=env_im_pnn`, `+learning.params.config.actor_precision=split_bf16`,
`+learning.params.config.wgrad=native`, `+learning.params.config.split_allreduce=True`.  `--rccl`: a one-rank RCCL process group with
`force_collectives=True` (the set-up of tests/two_rank_gpu_main.py).  On the device the recipe is the one of tests/graph_equivalence_main.py
(256 envs, `synthetic:2:3`, minibatch 2048).  `HumanoidIm` has no CPU path: `--device cpu` drives the agent with a small seeded stand-in env
(32 envs, fp32 GEMMs), as tests/test_learner_cpu.py does.  The script uses only what the agent has always had, so it runs on older commits too."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phc_amd.config import compose  # noqa: E402
from phc_amd.learning.amp_agent import IMAmpAgent  # noqa: E402

EPOCHS = 3


class StandInTask:
    """What the agent reads of a task, without physics: obs 20, AMP obs 18, every draw from one seeded generator."""
    device = "cpu"
    temp_running_mean = True
    shape_resampling_interval = 500

    def __init__(self, n, seed):
        self.num_envs = n
        self.g = torch.Generator().manual_seed(seed)
        self.obs_buf = torch.randn(n, 20, generator=self.g)
        self.reset_buf = torch.zeros(n, dtype=torch.long)

    def get_num_amp_obs(self):
        return 18

    def get_task_obs_size_detail(self):
        return {"num_prim": 2, "training_prim": 1, "has_lateral": False}

    def reset_done(self):
        self.reset_buf.zero_()


class StandInVecEnv:
    clip_obs = np.inf

    def __init__(self, n, seed=0):
        self.task = StandInTask(n, seed)
        self.num_envs, self.num_obs, self.num_actions = n, 20, 5

    def reset(self, env_ids=None):
        return self.task.obs_buf

    def step(self, actions):
        t = self.task
        t.obs_buf = 0.9 * t.obs_buf + 0.1 * torch.randn(t.num_envs, 20, generator=t.g)
        rew = torch.exp(-actions.pow(2).mean(-1))
        done = (torch.rand(t.num_envs, generator=t.g) < 0.1).long()
        t.reset_buf = done
        info = {"amp_obs": torch.randn(t.num_envs, 18, generator=t.g), "terminate": done * (torch.rand(t.num_envs, generator=t.g) < 0.5).long(),
                "reward_raw": torch.rand(t.num_envs, 5, generator=t.g)}
        return t.obs_buf, rew, done, info

    def fetch_amp_obs_demo(self, n):
        return torch.randn(n, 18, generator=self.task.g) + 0.5


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--rccl", action="store_true", help="one-rank RCCL group, force_collectives=True")
    ap.add_argument("overrides", nargs="*")
    a = ap.parse_args()
    dist = None
    over = list(a.overrides)
    if a.rccl:
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29600 + os.getpid() % 300), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        over.append("+learning.params.config.force_collectives=True")
    torch.manual_seed(0)
    if a.device == "cpu":
        cfg = compose(["learning.params.config.horizon_length=8", "learning.params.config.minibatch_size=64", "learning.params.config.mini_epochs=2",
                       "learning.params.config.amp_minibatch_size=32", "learning.params.config.amp_batch_size=16",
                       "learning.params.config.amp_obs_demo_buffer_size=256", "learning.params.config.amp_replay_buffer_size=256",
                       "learning.params.network.mlp.units=[32,16]", "learning.params.network.disc.units=[32,16]"] + over)
        env = StandInVecEnv(32)
        torch.manual_seed(11)
        agent = IMAmpAgent(env, cfg, dist=dist, bf16=False)
    else:
        from phc_amd.env.tasks.vec_task import parse_task
        cfg = compose(["env.num_envs=256", "env.motion_file=synthetic:2:3", "learning.params.config.minibatch_size=2048",
                       "learning.params.config.amp_minibatch_size=1024", "learning.params.config.amp_obs_demo_buffer_size=4096",
                       "learning.params.config.amp_replay_buffer_size=4096"] + over)
        task, env = parse_task(cfg)
        torch.manual_seed(11)
        agent = IMAmpAgent(env, cfg, dist=dist)
    agent.init_train()
    infos = [agent.train_epoch() for _ in range(EPOCHS)]
    st = agent.optimizer.state[agent.grads.flat_param]
    parts = {"flat_param": sha(agent.grads.flat_param), "exp_avg": sha(st["exp_avg"]), "exp_avg_sq": sha(st["exp_avg_sq"])}
    for name, mod in (("running_mean_std", agent.running_mean_std), ("value_mean_std", agent.value_mean_std), ("amp_input_mean_std", agent._amp_input_mean_std)):
        if mod is not None:
            for k, b in mod.named_buffers():
                parts[f"{name}.{k}"] = sha(b)
    total = hashlib.sha256("".join(f"{k}={v};" for k, v in sorted(parts.items())).encode()).hexdigest()
    print(json.dumps({"sha256": total, "optimizer_steps": int(st["step"]), "expected_steps": EPOCHS * agent.mini_epochs_num * agent.num_minibatches,
                      "num_collectives": agent.num_collectives, "device": a.device, "rccl": a.rccl, "overrides": a.overrides,
                      "last_info": {k: infos[-1][k] for k in ("actor_loss", "critic_loss", "disc_loss", "kl")}, "parts": parts}))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
