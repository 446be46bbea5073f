"""What tracking a keypoint stream costs.  SMPL humanoid at 4096 envs, 24 tracked bodies, obs_v 7, `+stream.motion=synthetic:3:1`.

    python scripts/probes/stream_track_ab.py --mode launch   phc_stream_track alone (mode advance) on a warmed task: HIP events around blocks of 200 launches
    python scripts/probes/stream_track_ab.py --mode torch    the same frame as the torch statements a user would write on the device (root-relative limb scale,
                                                             ring push, the folded filters as einsums, frame matrix, velocity, gating, obs_v 7): events around 200
    python scripts/probes/stream_track_ab.py --mode step     HumanoidIm and HumanoidImDemo in ONE process, stepped alternately in blocks, HIP events

Each mode prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make(name, envs):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    over = [f"env.num_envs={envs}", "env.motion_file=synthetic:3:1", "env.obs_v=7", f"env.task={name}"]
    if name == "HumanoidImDemo":
        over += ["+stream.motion=synthetic:3:1"]
    torch.manual_seed(0)
    task, env = parse_task(compose(over))
    env.reset()
    return task, env


def timed(fn, n, repeats):
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / n)
    return out


def quat_rotate(q, v):
    w, qv = q[..., 3:4], q[..., :3]
    return v * (2 * w * w - 1) + 2 * w * torch.cross(qv.expand_as(v), v, dim=-1) + 2 * qv * (qv * v).sum(-1, keepdim=True)


def torch_restatement(task):
    """-> a closure that processes the task's staged frame like the launch does, as torch statements on the device (state of its own)."""
    o, dev, N, NB = task._stream_opts, task.device, task.num_envs, task.num_bodies
    W = o["window"]
    fold = task._stream_fold.float()   # [4, W, W] (fp32: what a user would write)
    pairs = torch.tensor(o["limb_pairs"], device=dev)
    lengths = torch.tensor(o["limb_lengths"], device=dev)
    M = torch.tensor(o["frame_mat"], device=dev, dtype=torch.float32)
    st = dict(body=torch.zeros(N, W, NB, 3, device=dev), root=torch.zeros(N, W, 3, device=dev), prev=torch.zeros(N, NB, 3, device=dev))
    track, ns = task._track_bodies_id, task.get_self_obs_size()
    obs_out = torch.zeros_like(task.obs_buf)

    def once():
        p = task._stream_cur
        trans = p[:, :1]
        q = p - trans
        scale = ((q[:, pairs[:, 0]] - q[:, pairs[:, 1]]).norm(dim=-1) / lengths).mean(dim=-1)
        q = q / scale[:, None, None]
        st["body"] = torch.cat([st["body"][:, 1:], q[:, None]], dim=1)           # (full rings: the steady state)
        st["root"] = torch.cat([st["root"][:, 1:], trans], dim=1)
        t = torch.einsum("cw,nwc->nc", fold[:3, W - 1], st["root"])
        ref = (torch.einsum("w,nwbc->nbc", fold[3, W - 1], st["body"]) + t[:, None]) @ M.T
        vel = (ref - st["prev"]) / o["dt"]
        st["prev"] = ref
        rbs = task._rigid_body_state.view(N, NB, 13)
        bp, bv, root_pos, root_rot = rbs[:, track, :3], rbs[:, track, 7:10], rbs[:, 0, :3], rbs[:, 0, 3:7]
        rp, rv = ref[:, track].clone(), vel[:, track].clone()
        dist = (root_pos - rp[:, 0]).norm(dim=-1)
        z, f = dist > task.close_distance, dist > task.far_distance
        rp[:, 1:] = torch.where(z[:, None, None], bp[:, 1:], rp[:, 1:])
        rv = torch.where(z[:, None, None], bv, rv)
        rp[:, 0] = torch.where(f[:, None], (rp[:, 0] - bp[:, 0]) / dist[:, None] * task.far_distance + bp[:, 0], rp[:, 0])
        x = quat_rotate(root_rot, torch.tensor([1.0, 0.0, 0.0], device=dev).expand(N, 3))
        half = -0.5 * torch.atan2(x[:, 1], x[:, 0])
        hinv = torch.stack([torch.zeros_like(half), torch.zeros_like(half), torch.sin(half), torch.cos(half)], dim=-1)[:, None]
        obs_out[:, ns:] = torch.cat([quat_rotate(hinv, rp - bp).flatten(1), quat_rotate(hinv, rv - bv).flatten(1),
                                     quat_rotate(hinv, rp - root_pos[:, None]).flatten(1)], dim=-1)
        task.reset_buf.zero_()
        task._terminate_buf.zero_()
        return (bp - ref[:, track]).norm(dim=-1).mean(dim=-1)
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["launch", "torch", "step"], default="launch")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--block", type=int, default=50)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=60)
    args = ap.parse_args()
    names = ["HumanoidIm", "HumanoidImDemo"] if args.mode == "step" else ["HumanoidImDemo"]
    tasks = {n: make(n, args.envs) for n in names}
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    act = (torch.rand(args.envs, 69, device="cuda", generator=g) * 2 - 1) * 0.3

    def block(name, n):
        task, env = tasks[name]
        for _ in range(n):
            task.reset_done()
            env.step(act)
    for name in tasks:
        block(name, args.warmup)   # (also fills the rings: the launch's steady state is the full window)
    torch.cuda.synchronize()
    if args.mode == "launch":
        from phc_amd import _lib as L
        task = tasks["HumanoidImDemo"][0]
        out = timed(lambda: task._stream_launch(L.STREAM_ADVANCE), 200, args.repeats)
        obs = timed(lambda: task._stream_launch(L.STREAM_OBSERVE), 200, args.repeats)
        print(json.dumps({"probe": "stream_track_ab", "mode": "launch", "envs": args.envs, "advance_us": out, "advance_mean_us": sum(out) / len(out),
                          "advance_spread_us": max(out) - min(out), "observe_us": obs, "observe_mean_us": sum(obs) / len(obs)}))
        return
    if args.mode == "torch":
        once = torch_restatement(tasks["HumanoidImDemo"][0])
        for _ in range(40):
            once()
        torch.cuda.synchronize()
        out = timed(once, 200, args.repeats)
        print(json.dumps({"probe": "stream_track_ab", "mode": "torch", "envs": args.envs, "restatement_us": out, "mean_us": sum(out) / len(out),
                          "spread_us": max(out) - min(out)}))
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
    print(json.dumps({"probe": "stream_track_ab", "mode": "step", "envs": args.envs, "steps_per_block": args.block, "repeats": args.repeats, "env_step_us": out,
                      "mean_us": mean, "spread_us": {k: max(v) - min(v) for k, v in out.items()}, "demo_minus_im_us": mean["HumanoidImDemo"] - mean["HumanoidIm"]}))


if __name__ == "__main__":
    main()
