"""A/B: what `+env.task_rng=device` does to the getup task's env step and to the composer's rollout.  Two tasks (agents) in ONE process -- one without the
option, which is the parent's path launch for launch, and one with it -- run alternately in blocks, warmed up; at least `--seconds` of work per side and repeat.

    python scripts/probes/getup_step_ab.py step    [--envs 4096] [--block 50] [--seconds 1.0] [--repeats 3]   # (a) reset_done() + step() of HumanoidImGetup, eager
    python scripts/probes/getup_step_ab.py rollout [--envs 4096] [--seconds 2.0] [--repeats 3]                # (b) play_steps() of env_im_getup_mcp + im_mcp:
                                                                                                              #     segment graphs (torch) / whole-step graphs (device)
Both end with (c): the host-side launch calls of one step / one rollout step per side, counted by the profiler in a pass of its own.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GETUP = ["env.task=HumanoidImGetup", "env.recoveryEpisodeProb=0.5", "env.recoverySteps=90", "env.fallInitProb=0.5"]
MCP_GETUP = ["env=env_im_getup_mcp", "learning=im_mcp", "env.num_prim=3", "+learning.params.config.hip_graph=True"]
SIDES = (("torch", []), ("device", ["+env.task_rng=device"]))


def launch_calls(fn):
    """Host-side launch calls (kernel and graph launches) of fn(), by API name."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    calls = {}
    for e in prof.events():
        if "Launch" in e.name and e.name.startswith(("hip", "cuda")):
            calls[e.name] = calls.get(e.name, 0) + 1
    return calls


def alternate(run, seconds, repeats, unit):
    """run[side](): one block of `unit` steps, ending in a synchronise -> per side the microseconds per step of every repeat."""
    out = {side: [] for side in run}
    for _ in range(repeats):
        spent, blocks = {side: 0.0 for side in run}, 0
        while min(spent.values()) < seconds:
            for side in run:
                t0 = time.perf_counter()
                run[side]()
                spent[side] += time.perf_counter() - t0
            blocks += 1
        for side in run:
            out[side].append(1e6 * spent[side] / (blocks * unit))
    return out


def report(probe, args, us, calls, **more):
    mean = {k: sum(v) / len(v) for k, v in us.items()}
    print(json.dumps(dict(probe=probe, envs=args.envs, repeats=args.repeats, step_us=us, mean_us=mean, spread_us={k: max(v) - min(v) for k, v in us.items()},
                          device_over_torch=mean["device"] / mean["torch"], launch_calls_per_step=calls, **more)))


def step_ab(args):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    tasks = {}
    for side, extra in SIDES:
        torch.manual_seed(0)
        task, env = parse_task(compose([f"env.num_envs={args.envs}", "env.motion_file=synthetic:3:2", *GETUP, *extra]))
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
        torch.cuda.synchronize()
    for side in tasks:
        block(side, args.warmup)
    us = alternate({side: (lambda side=side: block(side)) for side in tasks}, args.seconds, args.repeats, args.block)
    calls = {side: launch_calls(lambda side=side: block(side, 1)) for side in tasks}
    done = {side: float((tasks[side][0].progress_buf == 0).float().mean()) for side in tasks}
    report("getup_step_ab/step", args, us, calls, steps_per_block=args.block, share_of_envs_at_progress_0=done)


def rollout_ab(args):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    from phc_amd.learning.amp_agent import IMAmpAgent
    from phc_amd.learning.network import PNN
    agents = {}
    for side, extra in SIDES:
        torch.manual_seed(0)
        task, env = parse_task(compose([f"env.num_envs={args.envs}", "env.motion_file=synthetic:2:5:1.5", *MCP_GETUP, *extra]))
        pnn = PNN(task.num_obs, [64, 32], "silu", task.num_dof, 3)
        task.load_primitives({"model": {f"a2c_network.pnn.{k}": v.clone() for k, v in pnn.state_dict().items()},
                              "running_mean_std": {"running_mean": torch.zeros(task.num_obs, dtype=torch.float64), "running_var": torch.ones(task.num_obs, dtype=torch.float64)}})
        agent = IMAmpAgent(env, task.cfg)
        agent.init_train()
        agents[side] = agent

    def rollout(side):
        agent = agents[side]
        with torch.no_grad(), agent.grads.shadow_scope():
            agent.play_steps()
        torch.cuda.synchronize()
    for side in agents:
        for i in range(4):   # eager, as a run's first epoch (the BLAS library initialises outside any capture); then: segment graphs, whole steps captured, replayed
            agents[side].epoch_num = 1 if i == 0 else 2
            print(f"[getup_step_ab] warm-up rollout {i} of side {side}", file=sys.stderr, flush=True)
            rollout(side)
    horizon = agents["torch"].horizon_length
    us = alternate({side: (lambda side=side: rollout(side)) for side in agents}, args.seconds, args.repeats, horizon)
    calls = {side: {k: v / horizon for k, v in launch_calls(lambda side=side: rollout(side)).items()} for side in agents}
    kinds = {side: sorted({k[0] for k in agents[side]._roll_graphs}) for side in agents}
    report("getup_step_ab/rollout", args, us, calls, horizon=horizon, graph_kinds=kinds,
           whole_step_capturable={side: bool(agents[side].task.whole_step_capturable()) for side in agents})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("step", "rollout"))
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--block", type=int, default=50, help="env steps per timed block of `step`; the two sides alternate block by block")
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per side and repeat, at least")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=60)
    a = ap.parse_args()
    (step_ab if a.part == "step" else rollout_ab)(a)
