"""Measurements of profiles/video/README.md, one process:  python profiles/video/measure.py [out.json]

For one 640 x 480 view and for a 2 x 2 grid (1280 x 960) of a 4-env SMPL task after a few env steps:
  * the time of one phc_jpeg_encode call (its four launches) by HIP events, for F = 1 and for a viewer chunk (64 views: 64 / 16 frames), 30 repeats after a
    warm-up; the frames are the rendered frame repeated;
  * host time per recorded frame, TaskRecorder.record() end to end (root read-back, render, tiling, then PNG: frame read-back, zlib, file -- or AVI: encode,
    scan read-back, file), png and avi alternated in blocks of 30 frames, 3 repeats;
  * bytes per frame of both, and what the default restart interval adds over one segment per frame."""
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]

FRAMES, REPEATS, CALLS, WARMUP = 30, 3, 30, 5


def encode_time_us(lib, L, video, frames, ri, calls=CALLS):
    F, H, W = (int(v) for v in frames.shape[:3])
    bound, need = lib.phc_jpeg_frame_bound(W, H, ri), lib.phc_jpeg_scratch_bytes(F, W, H, ri)
    out = torch.empty(F * bound, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    length = torch.empty(F, dtype=torch.int32, device="cuda")
    qt = video.quant_tables(90)
    a = L.JpegArgs()
    a.num_frames, a.width, a.height, a.restart_interval, a.row_stride, a.frame_stride = F, W, H, ri, 4 * W, 4 * W * H
    a.rgba, a.qtab, a.out, a.out_stride, a.length = frames.data_ptr(), qt.ctypes.data, out.data_ptr(), bound, length.data_ptr()
    a.coef, a.scratch, a.scratch_bytes = None, scratch.data_ptr(), need
    stream = torch.cuda.current_stream().cuda_stream
    t = []
    for r in range(WARMUP + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        assert lib.phc_jpeg_encode(C.byref(a), stream) == 0
        e1.record()
        e1.synchronize()
        if r >= WARMUP:
            t.append(e0.elapsed_time(e1) * 1e3)
    return {"median": float(np.median(t)), "min": float(np.min(t)), "max": float(np.max(t)), "scan_bytes_per_frame": float(length.float().mean()),
            "scratch_MiB": need / 2 ** 20}


def main():
    from phc_amd import _lib as L
    from phc_amd import render as R
    from phc_amd import video
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    lib = L.load()
    torch.manual_seed(0)
    task, env = parse_task(compose(["env.num_envs=4", "env.motion_file=synthetic:4:0"]))
    env.reset()
    for _ in range(10):
        env.step(torch.zeros(task.num_envs, task.num_actions, device=task.device))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, label in ((1, "640x480, one tile"), (4, "1280x960, four tiles")):
            res = out[label] = {}
            recs = {fmt: R.TaskRecorder(task, {"video": os.path.join(tmp, f"{fmt}{k}"), "envs": k, "format": fmt, "markers": True}) for fmt in ("png", "avi")}
            for rec in recs.values():
                for _ in range(WARMUP):
                    rec.record()
            per = {fmt: [] for fmt in recs}
            for _ in range(REPEATS):
                for fmt, rec in recs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(FRAMES):
                        rec.record()
                    torch.cuda.synchronize()
                    per[fmt].append((time.perf_counter() - t0) / FRAMES * 1e3)
            for rec in recs.values():
                rec.close()
            res["host_ms_per_frame"] = {fmt: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for fmt, v in per.items()}
            d = recs["png"].recorder.dir
            pngs = [os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".png")]
            n = recs["avi"].recorder.count
            res["bytes_per_frame"] = {"png": float(np.mean(pngs)), "avi": os.path.getsize(recs["avi"].recorder.avi_path) / n, "raw": 4 * k * 640 * 480}
            rec = recs["avi"]
            frame = R.tile(R.render_envs(task, range(k), rec.cameras, 640, 480, markers=True, capsules=rec.capsules), int(np.ceil(np.sqrt(k))))
            chunk = max(1, 64 // k)
            res["encode_us"] = {"F=1": encode_time_us(lib, L, video, frame[None].contiguous(), video.DEFAULT_RESTART_INTERVAL),
                                f"F={chunk}": encode_time_us(lib, L, video, frame[None].repeat(chunk, 1, 1, 1).contiguous(), video.DEFAULT_RESTART_INTERVAL),
                                "F=1, one segment": encode_time_us(lib, L, video, frame[None].contiguous(), 1 << 20, calls=3)}
            print(label, json.dumps(res), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
