"""Wall time of the evaluation sweep with the metrics formed on the host and on the device (profiles/eval_device/README.md):

  host:   every env step a second reference lookup, two [N, NB, 3] copies to the host, the arrays kept until the batch ends, numpy metrics per clip
  device: every env step ONE phc_eval_accumulate launch and an 8-byte status read; one copy of the totals per batch

`evaluate()` of an untrained agent on `synthetic:<clips>:0` at `--envs` envs (two batches by default), the two settings alternated `--reps` times in one
process after one untimed sweep.  Prints per sweep: wall time, the time inside the batch loops alone (the rest is loading the batch's clips, the same for
both), env steps and the process's peak RSS so far; writes the table as markdown into `--out`, between its two `sweep-table` marker lines (the
rest of that file -- the reading, the kernel's register report and its trace -- is kept).

    python scripts/probes/eval_sweep_time.py [--clips 8192] [--envs 4096] [--reps 3] [--out profiles/eval_device/README.md]
"""
import argparse
import os
import resource
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BEGIN, END = "<!-- sweep-table: written by scripts/probes/eval_sweep_time.py -->\n", "<!-- sweep-table: end -->\n"
sys.path.insert(0, ROOT)
from phc_amd.config import compose                              # noqa: E402
from phc_amd.env.tasks.vec_task import parse_task               # noqa: E402
from phc_amd.learning import im_eval                            # noqa: E402
from phc_amd.learning.amp_agent import IMAmpAgent               # noqa: E402


def write_table(path, text):
    """Put `text` between the marker lines of `path`; a file without them (or none) gets them appended."""
    doc = open(path).read() if os.path.exists(path) else ""
    if BEGIN in doc and END in doc.split(BEGIN, 1)[1]:
        head, rest = doc.split(BEGIN, 1)
        doc = head + BEGIN + text + END + rest.split(END, 1)[1]
    else:
        doc += ("\n" if doc else "") + BEGIN + text + END
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(doc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8192)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="device,host", help="order of the settings inside one repetition")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_device", "README.md"))
    args = ap.parse_args()
    torch.manual_seed(0)
    task, env = parse_task(compose([f"env.num_envs={args.envs}", f"env.motion_file=synthetic:{args.clips}:0"]))
    agent = IMAmpAgent(env, task.cfg)
    steps, loop_time = [0], [0.0]
    real_step = env.step

    def counted(actions):
        steps[0] += 1
        return real_step(actions)
    env.step = counted
    for name in ("_run_batch_host", "_run_batch_device"):   # time inside the batch loops (incl. their final copy and metric pass)
        def timed(*a, _fn=getattr(im_eval, name), **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = _fn(*a, **k)
            torch.cuda.synchronize()
            loop_time[0] += time.perf_counter() - t0
            return out
        setattr(im_eval, name, timed)

    def sweep(mode):
        agent.config["eval_metrics"] = mode
        steps[0], loop_time[0] = 0, 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info, _ = agent.eval(log=None)
        torch.cuda.synchronize()
        return dict(mode=mode, wall=time.perf_counter() - t0, loops=loop_time[0], steps=steps[0], rss=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024,
                    mpjpe=info["eval/mpjpe_all"], success=info["eval/success_rate"])

    modes = args.modes.split(",")
    warm = sweep(modes[0])
    rows = [sweep(m) for _ in range(args.reps) for m in modes]
    lines = [f"`evaluate()` on `synthetic:{args.clips}:0`, {args.envs} envs ({(args.clips + args.envs - 1) // args.envs} batches), untrained agent; untimed first sweep: "
             f"`{warm['mode']}`, peak RSS after it {warm['rss']:.0f} MiB.", "",
             "| sweep | eval_metrics | wall s | in the batch loops s | env steps | ms per env step (loops) | peak RSS so far MiB | eval/mpjpe_all mm |", "|---|---|---|---|---|---|---|---|"]
    for i, r in enumerate(rows):
        lines.append(f"| {i + 1} | {r['mode']} | {r['wall']:.3f} | {r['loops']:.3f} | {r['steps']} | {1e3 * r['loops'] / max(r['steps'], 1):.3f} | {r['rss']:.0f} | {r['mpjpe']:.4f} |")
    lines.append("")
    for m in modes:
        sel = [r for r in rows if r["mode"] == m]
        lines.append(f"* `{m}`: median wall {statistics.median(r['wall'] for r in sel):.3f} s, median in the batch loops {statistics.median(r['loops'] for r in sel):.3f} s "
                     f"(min {min(r['loops'] for r in sel):.3f}, max {max(r['loops'] for r in sel):.3f}), {sel[0]['steps']} env steps.")
    text = "\n".join(lines) + "\n"
    print(text)
    write_table(args.out, text)


if __name__ == "__main__":
    main()
