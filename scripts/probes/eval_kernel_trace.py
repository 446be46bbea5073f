"""Workload for a kernel trace of `phc_eval_accumulate` (profiles/eval_device/README.md): the benchmark's task (4096 envs, one synthetic clip) stepped
`--steps` times in evaluation mode with an open device accumulation, so that `k_eval_accumulate` appears once per env step next to the stepper and
the post-physics launch.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/probes/eval_kernel_trace.py [--envs 4096] [--steps 50]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from phc_amd.config import compose                              # noqa: E402
from phc_amd.env.tasks.vec_task import parse_task               # noqa: E402
from phc_amd.utils.flags import flags                           # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    torch.manual_seed(0)
    task, env = parse_task(compose([f"env.num_envs={args.envs}", "env.motion_file=synthetic:1:0"]))
    env.reset()
    flags.test, flags.im_eval = True, True
    task.begin_eval_accumulation(task._motion_lib.get_motion_num_steps(), args.envs)
    actions = torch.zeros(args.envs, task.num_actions, device=task.device)
    for _ in range(args.steps):
        env.step(actions)
        alive, longest = task.eval_status()
    failed, sums, count = task.end_eval_accumulation()
    flags.test, flags.im_eval = False, False
    print(f"{args.steps} steps, {alive} envs alive, longest clip {longest} steps, frames counted {int(count.min())}..{int(count.max())}")


if __name__ == "__main__":
    main()
