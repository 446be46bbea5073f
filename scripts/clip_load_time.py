"""Time `task.resample_motions()` with `clip_processing` host and device on one task, in one process (what `bench.py --config 3` measures as
`resample_motions_s`; bench.py cannot switch the option on).

    python scripts/clip_load_time.py [--envs 8192] [--clips 11313] [--runs 3] [--host-workers N] [--robot smpl|h1|g1] [--alternate] [--out FILE.json]

One task is built with the default (host) path; the option is then switched on the task's own motion library, so both paths load from the same library,
device and process.  Every timing is `time.perf_counter()` around a call that ends in `torch.cuda.synchronize()`.  The device path's first call (pinned
staging and device buffers are allocated) is reported apart from the timed runs.  The split of the device path between upload and launches comes from HIP
events around each chunk's copy and its launches (`motion_lib.CLIP_TIMING`).  `--robot h1 | g1` builds the robot's task (MotionLibReal, a synthetic robot
library) instead of the SMPL one; `--alternate` times host, device, host, device, ... instead of all host runs first.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


ROBOT = {"smpl": [], "h1": ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"],
         "g1": ["robot=unitree_g1", "env=env_im_g1_phc", "sim=robot_sim", "control=robot_control"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--clips", type=int, default=11313)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--host-workers", type=int, default=0, help="worker processes of the host path (0: the library's default for this machine)")
    ap.add_argument("--robot", choices=sorted(ROBOT), default="smpl")
    ap.add_argument("--alternate", action="store_true", help="alternate host and device runs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    from phc_amd import motion_lib as ML
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    t0 = time.perf_counter()
    task, env = parse_task(compose(ROBOT[args.robot] + [f"env.num_envs={args.envs}", f"env.motion_file=synthetic:{args.clips}:0"]))
    env.reset()
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    lib = task._motion_lib
    if args.host_workers:
        lib.m_cfg["num_workers"] = args.host_workers

    def timed():
        torch.cuda.synchronize()
        t = time.perf_counter()
        task.resample_motions()
        torch.cuda.synchronize()
        return time.perf_counter() - t

    def draw():
        ids, nf = lib._curr_motion_ids.cpu().tolist(), lib._motion_num_frames.cpu().tolist()
        per_clip = dict(zip(ids, nf))   # (one tree: a clip is processed once, whatever the number of envs that drew it)
        return {"distinct_clips": len(per_clip), "distinct_frames": int(sum(per_clip.values())), "env_frames": int(lib.frames.shape[0])}

    out = {"envs": args.envs, "robot": args.robot, "alternate": args.alternate, "library_clips": int(lib._num_unique_motions), "task_build_s": build_s,
           "host_workers": int(lib.m_cfg.get("num_workers", 0)) or ML.default_pool_workers(), "cpus": len(os.sched_getaffinity(0))}

    def timed_device(split):
        ML.CLIP_TIMING = []
        t = timed()
        ev = ML.CLIP_TIMING
        ML.CLIP_TIMING = None
        split.append({"chunks": len(ev), "upload_ms": sum(a.elapsed_time(b) for a, b, _ in ev), "launches_ms": sum(b.elapsed_time(c) for _, b, c in ev)})
        return t

    timed()   # (the pool's workers are up, as in a run that resamples repeatedly)
    host, dev, split, draws = [], [], [], {}
    if not args.alternate:
        host = [timed() for _ in range(args.runs)]
        draws["host"] = draw()
    lib.m_cfg["clip_processing"] = "device"
    out["device_first_call_s"] = timed()
    for _ in range(args.runs):
        if args.alternate:
            lib.m_cfg["clip_processing"] = "host"
            host.append(timed())
            draws["host"] = draw()
            lib.m_cfg["clip_processing"] = "device"
        dev.append(timed_device(split))
    out["host"] = {"runs_s": host, "min_s": min(host), "median_s": statistics.median(host), **draws["host"]}
    out["device"] = {"runs_s": dev, "min_s": min(dev), "median_s": statistics.median(dev), "split": split, **draw()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
