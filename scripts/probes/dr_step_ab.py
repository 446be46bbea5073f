"""A/B: what `domain_rand=h1_dr` costs per env step.  Unitree H1 at 4096 envs (the bench's H1 configuration), one task with the group and one without in
ONE process, stepped alternately in blocks, warmed up, timed with HIP events; at least a second of steps per task and repeat, three repeats.

    python scripts/probes/dr_step_ab.py [--envs 4096] [--block 50] [--seconds 1.0] [--repeats 3]

Prints one JSON line: per task the mean env-step time in microseconds of every repeat, their mean and spread, and the difference."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--block", type=int, default=50, help="env steps per timed block; the two tasks alternate block by block")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed stepping per task and repeat, at least")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=60)
    args = ap.parse_args()
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    over = ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control", f"env.num_envs={args.envs}", "env.motion_file=synthetic:1:0"]
    tasks = {}
    for name, extra in (("plain", []), ("h1_dr", ["domain_rand=h1_dr"])):
        torch.manual_seed(0)
        task, env = parse_task(compose(over + extra))
        env.reset()
        tasks[name] = (task, env)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    act = (torch.rand(args.envs, 19, device="cuda", generator=g) * 2 - 1) * 0.3

    def block(name, n):
        task, env = tasks[name]
        for _ in range(n):
            task.reset_done()
            env.step(act)
    for name in tasks:
        block(name, args.warmup)
    torch.cuda.synchronize()
    out = {name: [] for name in tasks}
    for _ in range(args.repeats):
        ms, steps = {name: 0.0 for name in tasks}, 0
        while min(ms.values()) < args.seconds * 1e3:
            for name in tasks:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                block(name, args.block)
                b.record()
                b.synchronize()
                ms[name] += a.elapsed_time(b)
            steps += args.block
        for name in tasks:
            out[name].append(1e3 * ms[name] / steps)
    mean = {k: sum(v) / len(v) for k, v in out.items()}
    print(json.dumps({"probe": "dr_step_ab", "envs": args.envs, "steps_per_block": args.block, "repeats": args.repeats, "env_step_us": out,
                      "mean_us": mean, "spread_us": {k: max(v) - min(v) for k, v in out.items()}, "h1_dr_minus_plain_us": mean["h1_dr"] - mean["plain"],
                      "h1_dr_over_plain": mean["h1_dr"] / mean["plain"]}))


if __name__ == "__main__":
    main()
