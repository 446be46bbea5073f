"""A/B: what `+env.task_rng=device` does to the env step and the rollout of a task with `env.add_obs_noise=True`.  Sides live in ONE process and run alternately
in blocks, warmed up; a block is timed by HIP events around it (recorded on the stream, read after a synchronise), at least `--seconds` per side and repeat.

    python scripts/probes/obs_aug_ab.py step    [--envs 4096] [--block 50]   # (a) reset_done() + step() of HumanoidIm, eager: torch mode (the parent's path) / device mode
    python scripts/probes/obs_aug_ab.py launch  [--envs 4096]                # (b) phc_obs_augment alone on the task's observation buffer, all rows, back to back
    python scripts/probes/obs_aug_ab.py rollout [--envs 4096]                # (c) play_steps() of IMAmpAgent, horizon 32: torch mode (segment graphs), device mode eager
                                                                             #     (PHC_NO_ROLLOUT_GRAPH), device mode with whole-step graphs
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
NOISE = ["env.add_obs_noise=True"]
DEVICE = ["+env.task_rng=device"]
HBM_MEASURED_TBS = 6.29   # float4 copy on an MI355X


def timed(fn):
    """fn() between two HIP events -> milliseconds."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(run, seconds, repeats, unit):
    """run[side](): one block of `unit` steps -> per side the microseconds per step of every repeat."""
    out = {side: [] for side in run}
    for _ in range(repeats):
        spent, blocks = {side: 0.0 for side in run}, 0
        while min(spent.values()) < seconds * 1e3:
            for side in run:
                spent[side] += timed(run[side])
            blocks += 1
        for side in run:
            out[side].append(1e3 * spent[side] / (blocks * unit))
    return out


def report(probe, args, us, **more):
    mean = {k: sum(v) / len(v) for k, v in us.items()}
    print(json.dumps(dict(probe=probe, envs=args.envs, repeats=args.repeats, step_us=us, mean_us=mean, spread_us={k: max(v) - min(v) for k, v in us.items()}, **more)))


def make(args, extra, motion="synthetic:3:2"):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    task, env = parse_task(compose([f"env.num_envs={args.envs}", f"env.motion_file={motion}", *NOISE, *extra]))
    return task, env


def step_ab(args):
    tasks = {}
    for side, extra in (("torch", []), ("device", DEVICE)):
        task, env = make(args, extra)
        env.reset()
        tasks[side] = (task, env)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    act = (torch.rand(args.envs, 69, device="cuda", generator=g) - 0.5) * 0.6

    def block(side, n=args.block):
        task, env = tasks[side]
        for _ in range(n):
            task.reset_done()
            env.step(act)
    for side in tasks:
        block(side, args.warmup)
    torch.cuda.synchronize()
    us = alternate({side: (lambda side=side: block(side)) for side in tasks}, args.seconds, args.repeats, args.block)
    report("obs_aug_ab/step", args, us, steps_per_block=args.block, num_obs=int(tasks["device"][0].obs_buf.shape[1]))


def launch_alone(args):
    task, env = make(args, DEVICE)
    env.reset()

    def block(n=200):
        for _ in range(n):
            task._obs_augment()
    block(50)
    torch.cuda.synchronize()
    us = [1e3 * timed(block) / 200 for _ in range(args.repeats)]
    nbytes = 8 * task.obs_buf.numel()
    report("obs_aug_ab/launch", args, {"phc_obs_augment": us}, num_obs=int(task.obs_buf.shape[1]), bytes=nbytes,
           tb_per_s=[nbytes / (t * 1e-6) / 1e12 for t in us], fraction_of_measured_hbm=[nbytes / (t * 1e-6) / 1e12 / HBM_MEASURED_TBS for t in us])


def rollout_ab(args):
    from phc_amd.learning.amp_agent import IMAmpAgent
    agents = {}
    for side, extra, no_graph in (("torch_segments", [], False), ("device_eager", DEVICE, True), ("device_whole_steps", DEVICE, False)):
        task, env = make(args, [*extra, "learning=im", "+learning.params.config.hip_graph=True"], motion="synthetic:2:5:1.5")
        agent = IMAmpAgent(env, task.cfg)
        agent.init_train()
        agents[side] = (agent, no_graph)

    def rollout(side):
        agent, no_graph = agents[side]
        os.environ.pop("PHC_NO_ROLLOUT_GRAPH", None)
        if no_graph:
            os.environ["PHC_NO_ROLLOUT_GRAPH"] = "1"
        with torch.no_grad(), agent.grads.shadow_scope():
            agent.play_steps()
    for side in agents:
        for i in range(4):   # eager, as a run's first epoch; then: segment graphs, whole steps captured, replayed
            agents[side][0].epoch_num = 1 if i == 0 else 2
            rollout(side)
            torch.cuda.synchronize()
    horizon = agents["torch_segments"][0].horizon_length
    us = alternate({side: (lambda side=side: rollout(side)) for side in agents}, args.seconds, args.repeats, horizon)
    kinds = {side: sorted({k[0] for k in agents[side][0]._roll_graphs}) for side in agents}
    report("obs_aug_ab/rollout", args, us, horizon=horizon, graph_kinds=kinds,
           whole_step_capturable={side: bool(agents[side][0].task.whole_step_capturable()) for side in agents})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("step", "launch", "rollout"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--block", type=int, default=50, help="env steps per timed block of `step`; the sides alternate block by block")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed device work per side and repeat, at least")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=60)
    a = ap.parse_args()
    {"step": step_ab, "launch": launch_alone, "rollout": rollout_ab}[a.part](a)
