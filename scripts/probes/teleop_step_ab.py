"""What HumanoidTeleop's reward launch costs.  Unitree H1 at 4096 envs under `domain_rand=h1_dr`, all eleven reward terms on.

    python scripts/probes/teleop_step_ab.py --mode step      HumanoidIm and HumanoidTeleop in ONE process, stepped alternately in blocks, HIP events
    python scripts/probes/teleop_step_ab.py --mode torch     the terms as the ~25 torch statements of the end-to-end test (tests/teleop_util.py: restate),
                                                             HIP events around a whole restatement: its launches' summed duration, gaps included
    python scripts/probes/teleop_step_ab.py --mode kernel    200 HumanoidTeleop steps and nothing else: the run to put behind `rocprofv3 --kernel-trace --stats --`

Each mode prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SPECS = {"r_feet_ori": -1.0, "r_torques": -1e-5, "r_dof_pos_limits": -10.0, "r_feet_air_time_teleop": 10.0, "r_torque_limits": -5.0, "r_dof_vel": -1e-3,
         "r_stumble": -2.0, "r_dof_acc": -2.5e-7, "r_action_rate": -0.01, "r_slippage": -1.0, "r_feet_contact_forces": -0.01, "max_contact_force": 200.0}


def make(name, envs):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    over = ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control", f"env.num_envs={envs}", "env.motion_file=synthetic:1:0",
            "domain_rand=h1_dr", f"env.task={name}"]
    if name == "HumanoidTeleop":
        over += [f"+env.reward_specs.{k}={v}" for k, v in SPECS.items()]
    torch.manual_seed(0)
    task, env = parse_task(compose(over))
    env.reset()
    return task, env


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "torch", "kernel"], default="step")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=60)
    args = ap.parse_args()
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    act = (torch.rand(args.envs, 19, device="cuda", generator=g) * 2 - 1) * 0.3
    names = ["HumanoidIm", "HumanoidTeleop"] if args.mode == "step" else ["HumanoidTeleop"]
    tasks = {n: make(n, args.envs) for n in names}

    def block(name, n):
        task, env = tasks[name]
        for _ in range(n):
            task.reset_done()
            env.step(act)
    for name in tasks:
        block(name, args.warmup)
    torch.cuda.synchronize()
    if args.mode == "kernel":
        block("HumanoidTeleop", 200)
        torch.cuda.synchronize()
        print(json.dumps({"probe": "teleop_step_ab", "mode": "kernel", "envs": args.envs, "steps": 200 + args.warmup}))
        return
    if args.mode == "torch":
        import teleop_util as tu
        task = tasks["HumanoidTeleop"][0]
        st = {k: getattr(task, k).clone() for k in ("last_actions", "last_dof_vel", "feet_air_time")}
        st["last_contacts"] = task.last_contacts.bool()
        ref = task.ref_body_vel[:, 0, :2].clone()
        scales = {n[2:]: float(task.reward_scales[n]) for n in task.reward_names}

        def once():
            terms = tu.restate(task, st, ref)
            rew = task.rew_buf.clone()
            cols = []
            for n, s in scales.items():
                c = terms[n] * s
                rew += c
                cols.append(c[:, None])
            return rew, torch.cat([task._reward_raw_im] + cols, dim=-1)
        for _ in range(20):
            once()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(200):
                once()
            b.record()
            b.synchronize()
            out.append(1e3 * a.elapsed_time(b) / 200)
        print(json.dumps({"probe": "teleop_step_ab", "mode": "torch", "envs": args.envs, "restatement_us": out, "mean_us": sum(out) / len(out)}))
        return
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
    print(json.dumps({"probe": "teleop_step_ab", "mode": "step", "envs": args.envs, "steps_per_block": args.block, "repeats": args.repeats, "env_step_us": out,
                      "mean_us": mean, "spread_us": {k: max(v) - min(v) for k, v in out.items()},
                      "teleop_minus_im_us": mean["HumanoidTeleop"] - mean["HumanoidIm"]}))


if __name__ == "__main__":
    main()
