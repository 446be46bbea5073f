"""Kernel-level comparison of the two weight-gradient paths of a fused-ReLU bf16 layer (profiles/wgrad_native/README.md):

  library: phc_colsum_relu_bf16 (mask + bias gradient) -> batched GEMM over SPLIT_K row chunks (bf16 slabs) -> phc_sum_slabs_bf16
  native:  ONE phc_wgrad_bf16 launch (mask, weight gradient, bias gradient, masked gradient written for the input-gradient GEMM)

Both produce gz, gw (fp32, stored) and gb on the same operands.  HIP events around `--iters` back-to-back calls, the two versions alternated
`--reps` times in one process after a warm-up; one JSON line per shape: median and spread of the per-call time, TFLOP/s from 2 rows n k, share of the
2.5 PFLOP/s bf16 peak, the HBM floor from the bytes the product needs (gy, y, x read once; gz, gw, gb written once) at 8 TB/s, and the error of
each path against float64 at one shape-independent sample of the output.

    python scripts/probes/wgrad_native_bench.py [--iters 20] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from phc_amd import _lib as L                                   # noqa: E402
from phc_amd.learning import fast_ops as fo                     # noqa: E402

PEAK_TFLOPS, PEAK_TBS = 2500.0, 8.0
SHAPES = [("actor/critic layer 1 (K-padded)", 16384, 1024, 1024), ("actor/critic layer 2", 16384, 512, 1024), ("actor head", 16384, 69, 512),
          ("discriminator layer 1 (K-padded)", 12288, 1024, 2048)]


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters     # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured off the device")
    lib = L.load()
    dev = torch.device("cuda")
    for name, rows, n, k in SHAPES:
        g = torch.Generator().manual_seed(rows + n + k)
        gy = (0.01 * torch.randn(rows, n, generator=g)).to(torch.bfloat16).to(dev)
        y = torch.relu(torch.randn(rows, n, generator=g)).to(torch.bfloat16).to(dev)
        x = torch.relu(torch.randn(rows, k, generator=g)).to(torch.bfloat16).to(dev)
        gw_l, gw_n = torch.empty(n, k, device=dev), torch.empty(n, k, device=dev)
        gb_l, gb_n = torch.empty(n, device=dev), torch.empty(n, device=dev)
        gz_n = torch.empty_like(gy)

        def library():
            gm, _ = fo.colsum_relu_bf16(gy, y, out=gb_l)
            fo.wgrad_split_k(gm, x, out=gw_l)

        def native():
            fo.wgrad_native(gy, y, x, gw_n, gz=gz_n, gb=gb_n)

        for _ in range(5):
            library()
            native()
        torch.cuda.synchronize()
        t_l, t_n = [], []
        for _ in range(args.reps):
            t_l.append(_time(library, args.iters))
            t_n.append(_time(native, args.iters))
        # accuracy at the first 64 output rows against float64 (same masked gradient for both)
        gz = torch.where(y > 0, gy, torch.zeros_like(gy)).double()
        ref = gz[:, :64].t() @ x.double()
        scale = float(ref.abs().max())
        flops = 2.0 * rows * n * k
        bytes_ = 2.0 * rows * (3 * n + k) + 4.0 * n * (k + 1)
        out = {"shape": name, "rows": rows, "n": n, "k": k, "slices": lib.phc_wgrad_bf16_slices(rows, n, k), "iters": args.iters, "reps": args.reps}
        for tag, t, gw in (("library", t_l, gw_l), ("native", t_n, gw_n)):
            med = statistics.median(t)
            out[tag] = {"us_median": round(med, 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2), "tflops": round(flops / med * 1e-6, 1),
                        "share_of_bf16_peak": round(flops / med * 1e-6 / PEAK_TFLOPS, 4), "max_err_over_max_abs": float((gw[:64].double() - ref).abs().max()) / scale}
        out["mfma_floor_us"] = round(flops / PEAK_TFLOPS * 1e-6, 2)
        out["hbm_floor_us"] = round(bytes_ / PEAK_TBS * 1e-6, 2)
        out["nearer_bound"] = "mfma" if out["mfma_floor_us"] >= out["hbm_floor_us"] else "hbm"
        out["native_over_library"] = round(out["native"]["us_median"] / out["library"]["us_median"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
