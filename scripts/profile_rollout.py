"""Where does the rollout (`play_steps`, 32 steps) spend its time?  Runs IMAmpAgent.play_steps with eager launches (PHC_NO_ROLLOUT_GRAPH=1: a replayed
graph has no inside to time) and HIP events around the agent's own pieces of a step -- `_rollout_reset`, `_rollout_policy`, `vec_env.step`, `_rollout_after` --
(device time) and perf_counter around the whole call (wall): python scripts/profile_rollout.py [num_envs]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from phc_amd.config import compose  # noqa: E402
from phc_amd.env.tasks.vec_task import parse_task  # noqa: E402
from phc_amd.learning.amp_agent import IMAmpAgent  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
cfg = compose([f"env.num_envs={n}", "env.motion_file=synthetic:1:0", "+learning.params.config.hip_graph=True"])
task, env = parse_task(cfg)
agent = IMAmpAgent(env, cfg)
agent.init_train()
for _ in range(3):
    agent.train_epoch()
torch.cuda.synchronize()
os.environ["PHC_NO_ROLLOUT_GRAPH"] = "1"
# a step records 8 events, one before and one behind each piece: a segment runs from event a to event b
SEG = {"reset + observation row": (0, 2), "policy segment": (2, 4), "env.step": (4, 5), "AMP copy": (5, 6), "after segment": (6, 7)}
marks = []


def timed(obj, name):
    f = getattr(obj, name)

    def g(*a, **k):
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        out = f(*a, **k)
        marks.append(torch.cuda.Event(enable_timing=True))
        marks[-1].record()
        return out
    setattr(obj, name, g)


for obj, name in ((agent, "_rollout_reset"), (agent, "_rollout_policy"), (agent.vec_env, "step"), (agent, "_rollout_after")):
    timed(obj, name)
acc, reps, wall = np.zeros(len(SEG)), 3, 0.0
for rep in range(reps):
    del marks[:]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad(), agent.grads.shadow_scope():
        agent.play_steps()
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    wall += time.perf_counter() - t0
    assert len(marks) == 8 * agent.horizon_length
    for s in range(0, len(marks), 8):
        for i, (a, b) in enumerate(SEG.values()):
            acc[i] += marks[s + a].elapsed_time(marks[s + b])
    print(f"rep {rep}: host issue time {t_issue * 1e3:.2f} ms, wall {1e3 * (time.perf_counter() - t0):.2f} ms (with the batch assembly behind the steps)")
acc /= reps
print(f"rollout of {agent.horizon_length} steps, {n} envs: wall {wall / reps * 1e3:.2f} ms; event time per segment (ms per rollout, includes launch gaps):")
for nm, v in zip(SEG, acc):
    print(f"  {nm:36s} {v:7.3f}  ({v / agent.horizon_length * 1e3:6.1f} us / step)")
print(f"  {'sum':36s} {acc.sum():7.3f}")
