"""Measurements of the distillation stage on an MI355X (profiles/distill/README.md):  python profiles/distill/measure.py --out <file.json>

  record  -- the recorder's launch per env step at 4096 envs x 934 columns x 69 actions against the three device-to-host copies it replaces (observation,
             two action tensors, plus the reset flags), alternated in one loop;
  step    -- one optimizer step at the reference's shape (16384 x 934 -> 2048 -> 1024 -> 512 -> 69): the trainer's kernels against the same layers and GEMMs
             with torch's own nn.SiLU / nn.MSELoss in their place, alternated in one process;
  epoch   -- one epoch over a dataset recorded from a 64-clip synthetic library by an untrained agent.
Times are device events around windows that end in a synchronise; every shape is warmed up first.  There is no CPU path: without a device it fails."""
import argparse
import json
import os
import sys
import tempfile

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters      # us per call


def alternate(fns, iters, rounds):
    """-> {name: [us per call, one figure per round]} with the variants taking turns."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            out[k].append(timed(f, iters))
    return out


def measure_record(N=4096, D=934, A=69, steps=64):
    import ctypes as C
    from phc_amd import _lib as L
    from phc_amd.abi import record_args_struct
    dev = "cuda"
    rows = torch.full((N,), steps, dtype=torch.int64, device=dev)
    start = torch.cumsum(rows, 0) - rows
    R = N * steps
    obs_buf, prev = torch.randn(N, D, device=dev), torch.randn(N, D, device=dev)
    clean, act, reset = torch.randn(N, A, device=dev), torch.randn(N, A, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
    blk = (torch.empty(R, D, device=dev), torch.empty(R, A, device=dev), torch.empty(R, A, device=dev), torch.empty(R, dtype=torch.int64, device=dev))
    lib, st = L.load(), torch.cuda.current_stream().cuda_stream
    step = [0]

    def launch():
        a = record_args_struct(N, D, A, step[0] % steps, R, obs_buf=obs_buf, obs_prev=prev, clean_actions=clean, actions=act, reset_buf=reset, rows=rows,
                               row_start=start, obs=blk[0], clean=blk[1], env=blk[2], reset=blk[3])
        L.check(lib.phc_dataset_record(C.byref(a), st), "phc_dataset_record")
        step[0] += 1

    def copies():      # what the reference's loop does per env step (humanoid_im.py:683-690)
        return obs_buf.cpu().numpy(), act.cpu().numpy(), clean.cpu().numpy(), reset.cpu().numpy()
    t = alternate({"record_launch_us": launch, "device_to_host_copies_us": copies}, 200, 5)
    t["bytes_moved_by_the_launch"] = N * (D * 4 * 4 + A * 4 * 4 + 16)      # obs: prev read, row written, obs_buf read, prev written; two action rows read + written
    return t


def measure_step(B=16384, rows=65536, D=934, A=69, units=(2048, 1024, 512)):
    from phc_amd import distill
    from phc_amd.learning.fast_ops import adam_clip_step, deferred_colsums
    g = torch.Generator().manual_seed(0)
    obs, act = torch.randn(rows, D, generator=g).numpy(), torch.randn(rows, A, generator=g).numpy()
    mean, var = torch.zeros(D, dtype=torch.float64), torch.ones(D, dtype=torch.float64)
    ours = distill.Trainer(obs, act, mean, var, units, "silu", B, 2e-5, 0, "cuda")
    theirs = distill.Trainer(obs, act, mean, var, units, "silu", B, 2e-5, 0, "cuda")
    for i, m in enumerate(theirs.model.model):      # the same layers and GEMMs, torch's own SiLU modules behind them
        if isinstance(m, nn.SiLU):
            theirs.model.model[i] = nn.SiLU()
        elif hasattr(m, "fuse_silu"):
            m.fuse_silu = False
    crit = nn.MSELoss()
    idx = torch.randperm(rows, generator=g)[:B].cuda().contiguous()

    def torch_step():
        x = theirs._input(idx)
        theirs.grads.zero()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            pred = theirs.model(x)
        loss = crit(pred.float(), theirs.act[idx])
        with deferred_colsums():
            loss.backward()
        adam_clip_step(theirs.optimizer, theirs.grads.flat_param, theirs.grads.flat, None, shadow=theirs.grads.shadow)
    with ours.grads.shadow_scope(), theirs.grads.shadow_scope():
        t = alternate({"kernels_step_us": lambda: ours.step(idx), "torch_silu_mse_step_us": torch_step}, 20, 5)
    return t


def measure_epoch(clips=64):
    from phc_amd import distill
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    from phc_amd.learning.amp_agent import IMAmpAgent
    small = ["learning.params.config.minibatch_size=64", "learning.params.config.amp_obs_demo_buffer_size=512", "learning.params.config.amp_replay_buffer_size=512"]
    torch.manual_seed(0)
    task, env = parse_task(compose([f"env.num_envs={clips}", f"env.motion_file=synthetic:{clips}:0", "collect_dataset=True", "env.add_action_noise=True",
                                    "+env.action_noise_std=0.05", "+learning.params.config.eval_metrics=device"] + small))
    agent = IMAmpAgent(env, task.cfg)
    with tempfile.TemporaryDirectory() as d:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        agent.eval(output_dir=d, log=None)
        e1.record()
        torch.cuda.synchronize()
        merged, meta = distill.merge(os.path.join(d, "phc_act", f"synthetic:{clips}:0"), log=None)
        obs, act = distill.load_rows(merged)
    rms = agent.running_mean_std
    tr = distill.Trainer(obs, act, rms.running_mean.cpu(), rms.running_var.cpu(), (2048, 1024, 512), "silu", 16384, 2e-5, 0, "cuda")
    tr.run_epoch()
    torch.cuda.synchronize()
    t = [timed(tr.run_epoch, 5) for _ in range(5)]
    return {"rows": int(obs.shape[0]), "clips_recorded": len(agent.last_dataset.keys), "recording_sweep_ms": e0.elapsed_time(e1), "epoch_us": t}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="record,step,epoch")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no device: these are measurements on the MI355X, there is no CPU path")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    for name, fn in (("record", measure_record), ("step", measure_step), ("epoch", measure_epoch)):
        if name in a.only.split(","):
            res[name] = fn()
            print(name, json.dumps(res[name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
