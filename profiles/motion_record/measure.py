"""Measurements of the motion recorder on an MI355X (profiles/motion_record/README.md):  python profiles/motion_record/measure.py --out <file.json>

At 4096 envs of the default SMPL task, variants taking turns in one process:
  launch_us            phc_motion_record alone (HIP events around a window of launches that ends in a synchronise; no frame is refused inside a window)
  launch_ref_us        the same with ref_body_pos (`+record.ref=True`)
  torch_statement_us   the recorder's torch statement of the same rule on the device (`BACKEND = "torch"`)
  reference_copies_us  what the reference's `_record_states` does per env step: `.cpu().clone()` of root_states, dof_pos, the body rotations, progress_buf and
                       ref_body_pos (base_task.py:242-246, humanoid.py:445-453, humanoid_im.py:401-405)
  step_us              reset_done() + step(): the env step without the switch (the code of the parent commit: the recorder adds a launch behind it, no file of
                       the step changed)
  step_record_us       reset_done() + step() + the recorder's launch
  step_copies_us       reset_done() + step() + the reference's copies
There is no CPU path: without a device it fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(fn, iters, before=None):
    if before is not None:
        before()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters      # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no device: these are measurements on the MI355X, there is no CPU path")
    from phc_amd import motion_record as mr
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    task, env = parse_task(compose([f"env.num_envs={a.envs}", "env.motion_file=synthetic:1:0"]))
    env.reset()
    N, cap = task.num_envs, a.iters + 56
    actions = (torch.rand(N, task.num_actions, device=task.device) * 2 - 1) * 0.2
    recs = {}
    for name, ref, backend in (("launch", False, None), ("launch_ref", True, None), ("torch", False, "torch")):
        mr.BACKEND = backend
        recs[name] = mr.MotionRecorder(task, max_frames=cap, ref=ref)
        recs[name].begin_play()
    mr.BACKEND = None

    def rewind(r):
        def go():
            r._state["len"].zero_()
            r._held = 0
        return go

    def env_step():
        task.reset_done()
        task.step(actions)

    def copies():
        return (task._root_states.cpu().clone(), task._dof_pos.cpu().clone(), task._rigid_body_rot.cpu().clone(), task.progress_buf.cpu().clone(),
                task.ref_body_pos.cpu().clone())

    def both(f, g):
        def go():
            f()
            g()
        return go
    variants = {"launch_us": (recs["launch"]._append, rewind(recs["launch"])), "launch_ref_us": (recs["launch_ref"]._append, rewind(recs["launch_ref"])),
                "torch_statement_us": (recs["torch"]._append, rewind(recs["torch"])), "reference_copies_us": (copies, None), "step_us": (env_step, None),
                "step_record_us": (both(env_step, recs["launch"]._append), rewind(recs["launch"])), "step_copies_us": (both(env_step, copies), None)}
    for fn, before in variants.values():       # warm up every shape
        timed(fn, 10, before)
    out = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (fn, before) in variants.items():
            out[k].append(timed(fn, a.iters, before))
    assert all(int(r._state["dropped"].sum()) == 0 for r in recs.values()), "a frame was refused inside a timed window"
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "envs": N, "iters_per_window": a.iters, "rounds": a.rounds,
           "row_floats": recs["launch"].W, "row_floats_ref": recs["launch_ref"].W, "block_bytes_at_cap_1024": N * 1024 * recs["launch"].W * 4,
           "bytes_stored_per_launch": N * (recs["launch"].W * 4 + 16 + 4), "us_per_call": out,
           "summary_us": {k: {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v))} for k, v in out.items()}}
    print(json.dumps(res["summary_us"], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
