"""A/B of the two keypoint-fit backends on a synthetic library (profiles/fit_keypoints/README.md): `fit_keypoint_clips(backend="device")`
(phc_fit_sph_iterate over whole chunks) against `fit_keypoint_clips(backend="host", device="cuda:0")` (torch autograd per clip on the same HIP device),
alternated in one process and warmed up.

    python scripts/probes/fit_keypoints_ab.py --out fit_kp_ab.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/probes/fit_keypoints_ab.py --profile

The library: `--clips` clips of 60-600 frames (seeded): smooth random joint rotation vectors, a turning root and a drifting root position, through the
statement's own FK -> keypoints [T, 24, 3] of `smpl_humanoid`.
Device backend, library: the whole library, `--iterations` iterations; wall time = host clock around `fit_keypoint_clips`, `iterate` = the time between two
events around phc_fit_sph_iterate alone (FIT_TIMING).
The comparison the design asks for, on the SAME clips: the first `--sample` clips as one chunk on the device backend (events, per iteration) against the host
backend clip by clip at `--host-iterations` iterations (host clock around each fit, which ends in a download; per clip and iteration, summed over the
sample).  Both report their final `fit_keypoint_error` at `--sample-iterations` iterations when `--errors` is given (the host backend then runs that long).
`--profile`: the device fit alone, 20 iterations after a warm-up, for a kernel trace.  No GPU: an error."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def make_library(model, num_clips, seed):
    from phc_amd.utils.fit_keypoints import sph_fk, sph_model_arrays
    marr = sph_model_arrays(model, list(range(model.num_bodies)))
    nb = model.num_bodies
    rng = np.random.default_rng(seed)
    clips = {}
    for i in range(num_clips):
        T = int(rng.integers(60, 601))
        t = np.arange(T)[:, None, None] / 30.0
        freq, phase, amp = rng.uniform(0.2, 1.5, (1, nb - 1, 3)), rng.uniform(0, 2 * np.pi, (1, nb - 1, 3)), rng.uniform(0.0, 0.35, (1, nb - 1, 3))
        rot = amp * np.sin(2 * np.pi * freq * t + phase)
        root_rot = np.zeros((T, 3))
        root_rot[:, 2] = rng.uniform(-np.pi, np.pi) + rng.uniform(-0.5, 0.5) * t[:, 0, 0]
        root_rot[:, :2] = 0.1 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0, (1, 2)) * t[:, 0] + rng.uniform(0, 6.28, (1, 2)))
        root_pos = np.array([0.0, 0.0, 0.92]) + np.cumsum(rng.normal(scale=0.01, size=(T, 3)) * np.array([1.0, 1.0, 0.1]), axis=0)
        pos, _ = sph_fk(marr, torch.from_numpy(root_rot), torch.from_numpy(rot), torch.from_numpy(root_pos))
        clips[f"clip_{i:04d}"] = pos.numpy()
    return clips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=512)
    ap.add_argument("--iterations", type=int, default=500)
    ap.add_argument("--sample", type=int, default=8)
    ap.add_argument("--host-iterations", type=int, default=50)
    ap.add_argument("--sample-iterations", type=int, default=500)
    ap.add_argument("--errors", action="store_true", help="also run the host backend on the sample for --sample-iterations and report both final errors")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available() or torch.version.hip is None:
        raise SystemExit("fit_keypoints_ab: no HIP device; this probe measures nothing without one")
    from phc_amd.model import load_model
    from phc_amd.utils import fit_keypoints as F
    model = load_model("smpl_humanoid")
    clips = make_library(model, a.clips, a.seed)
    keys = list(clips)
    sample = {k: clips[k] for k in keys[:a.sample]}
    frames, sample_frames = sum(len(c) for c in clips.values()), sum(len(c) for c in sample.values())
    dev = "cuda:0"
    print(f"smpl_humanoid: {len(clips)} clips, {frames} frames; sample: {len(sample)} clips, {sample_frames} frames", flush=True)
    F.fit_keypoint_clips(model, clips, iterations=5, backend="device", device=dev)                       # warm-up: code objects, allocator
    if a.profile:
        F.fit_keypoint_clips(model, clips, iterations=20, backend="device", device=dev)
        torch.cuda.synchronize()
        print("profiled 20 iterations", flush=True)
        return
    F.fit_keypoint_clips(model, {keys[0]: clips[keys[0]]}, iterations=5, backend="host", device=dev)      # warm-up of the host backend
    res = dict(clips=len(clips), frames=frames, iterations=a.iterations, sample=len(sample), sample_frames=sample_frames, host_iterations=a.host_iterations, rounds=[])

    def device_fit(which, iterations):
        F.FIT_TIMING = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = F.fit_keypoint_clips(model, which, iterations=iterations, backend="device", device=dev)
        wall = time.perf_counter() - t0
        ms = sum(t[3] for t in F.FIT_TIMING)
        F.FIT_TIMING = None
        return out, wall, ms

    for r in range(a.rounds):
        out, wall, ms = device_fit(clips, a.iterations)
        err = [o["fit_keypoint_error"] for o in out.values()]
        s_out, _, s_ms = device_fit(sample, a.sample_iterations)
        host_ms = []
        for k in sample:                                  # clip by clip: the host backend's own granularity
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            F.fit_keypoint_clips(model, {k: sample[k]}, iterations=a.host_iterations, backend="host", device=dev)      # (ends in .cpu(): a synchronise)
            host_ms.append((time.perf_counter() - t0) * 1e3 / a.host_iterations)
        row = dict(device_wall_s=wall, device_iterate_ms=ms, device_ms_per_iteration=ms / a.iterations, device_frames_per_s=frames * a.iterations / (ms * 1e-3),
                   device_keypoint_error_m=dict(mean=float(np.mean(err)), median=float(np.median(err)), max=float(np.max(err))),
                   sample_device_ms_per_iteration=s_ms / a.sample_iterations, sample_host_ms_per_iteration_summed=float(np.sum(host_ms)),
                   sample_host_ms_per_clip_iteration=dict(min=float(np.min(host_ms)), median=float(np.median(host_ms)), max=float(np.max(host_ms))),
                   sample_device_keypoint_error_m=float(np.mean([o["fit_keypoint_error"] for o in s_out.values()])))
        if a.errors and r == 0:
            h_out = F.fit_keypoint_clips(model, sample, iterations=a.sample_iterations, backend="host", device=dev)
            row["sample_host_keypoint_error_m"] = float(np.mean([o["fit_keypoint_error"] for o in h_out.values()]))
        res["rounds"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
