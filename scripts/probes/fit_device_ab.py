"""A/B of the two retargeting backends on a synthetic library (profiles/fit_device/README.md): `fit_clips(backend="device")` (phc_fit_iterate over the whole
library) against `fit_clips(backend="host", device="cuda:0")` (torch autograd per clip on the device: the path that existed before), alternated in one process.

    python scripts/probes/fit_device_ab.py --robot unitree_h1 --out fit_ab_h1.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/probes/fit_device_ab.py --robot unitree_h1 --profile

The library: `--clips` clips of 60-600 frames from `make_robot_clip` (seeded), handed over as "SMPL joints" the way tests/test_fit_robot_motion.py does.
Device fit: the whole library, `--iterations` iterations; wall time = host clock around `fit_clips` (which ends in a download, i.e. a synchronise) and the
time between two events around phc_fit_iterate alone.  Host-backend fit: the first `--host-clips` clips at `--host-iterations` iterations, clip by clip until
`--host-seconds` have passed; reported per clip and iteration (its cost per iteration does not depend on the iteration).  `--profile`: the device fit alone,
20 iterations after a warm-up, for a kernel trace.  No GPU: an error."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def make_library(model, rc, num_clips, seed):
    from scipy.spatial.transform import Rotation as sRot
    from phc_amd.utils.fit_robot_motion import SMPL_BONE_ORDER_NAMES, RobotFK
    from phc_amd.utils.synthetic_motion import make_robot_clip
    ext = list(rc["extend_config"])
    fk = RobotFK(model, ext, dtype=torch.float64)
    rng = np.random.default_rng(seed)
    clips = {}
    for i in range(num_clips):
        T = int(rng.integers(60, 601))
        gt = make_robot_clip(rng, model, T, num_extend=len(ext))
        pos, _ = fk(torch.from_numpy(gt["pose_aa"]), torch.from_numpy(gt["root_trans_offset"]))
        joints = np.zeros((T, 24, 3))
        for rname, sname in rc["joint_matches"]:
            joints[:, SMPL_BONE_ORDER_NAMES.index(sname)] = pos[:, fk.names.index(rname)].numpy()
        root_aa = (sRot.from_rotvec(gt["pose_aa"][:, 0]) * sRot.from_quat([0.5, 0.5, 0.5, 0.5])).as_rotvec()
        clips[f"clip_{i:04d}"] = (joints, joints[:, 0].copy(), root_aa)
    return clips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="unitree_h1", choices=["unitree_h1", "unitree_g1"])
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=500)
    ap.add_argument("--host-clips", type=int, default=32)
    ap.add_argument("--host-iterations", type=int, default=100)
    ap.add_argument("--host-seconds", type=float, default=40.0)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("fit_device_ab: no HIP device; this probe measures nothing without one")
    from phc_amd import robots
    from phc_amd.cfg_defaults import GROUPS
    from phc_amd.model import load_model
    from phc_amd.utils import fit_robot_motion as F
    rc = GROUPS["robot"][a.robot]
    model = load_model(f"{rc['humanoid_type']}_humanoid")
    robots.apply_robot_gains(model, robots.ROBOTS[rc["humanoid_type"]])
    clips = make_library(model, rc, a.clips, a.seed)
    frames = sum(c[0].shape[0] for c in clips.values())
    keys = list(clips)
    dev = "cuda:0"
    print(f"{a.robot}: {len(clips)} clips, {frames} frames", flush=True)
    F.fit_clips(model, rc, clips, iterations=5, backend="device", device=dev)                      # warm-up: code objects, allocator
    if a.profile:
        F.fit_clips(model, rc, clips, iterations=20, backend="device", device=dev)
        torch.cuda.synchronize()
        print("profiled 20 iterations", flush=True)
        return
    F.fit_clip(model, rc, *clips[keys[0]], iterations=5, device=dev)                                # warm-up of the host backend
    res = dict(robot=a.robot, clips=len(clips), frames=frames, iterations=a.iterations, host_iterations=a.host_iterations, rounds=[])
    for r in range(a.rounds):
        F.FIT_TIMING = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = F.fit_clips(model, rc, clips, iterations=a.iterations, backend="device", device=dev)
        wall = time.perf_counter() - t0
        kernel_ms = sum(t[3] for t in F.FIT_TIMING)
        F.FIT_TIMING = None
        err = float(np.mean([o["fit_keypoint_error"] for o in out.values()]))
        done, host_err, t0 = 0, [], time.perf_counter()
        for k in keys[:a.host_clips]:
            o = F.fit_clip(model, rc, *clips[k], iterations=a.host_iterations, device=dev)           # (ends in .cpu(): a synchronise)
            host_err.append(o["fit_keypoint_error"])
            done += 1
            if time.perf_counter() - t0 > a.host_seconds:
                break
        host_wall = time.perf_counter() - t0
        host_frames = sum(clips[k][0].shape[0] for k in keys[:done])
        row = dict(device_wall_s=wall, device_iterate_ms=kernel_ms, device_ms_per_iteration=kernel_ms / a.iterations,
                   device_frames_per_s=frames * a.iterations / (kernel_ms * 1e-3), device_mean_keypoint_error_m=err,
                   host_clips=done, host_frames=host_frames, host_wall_s=host_wall, host_ms_per_clip_iteration=host_wall * 1e3 / (done * a.host_iterations),
                   host_frames_per_s=host_frames * a.host_iterations / host_wall, host_mean_keypoint_error_m=float(np.mean(host_err)))
        res["rounds"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
