"""-m gpu: the three device regimes of the learner's rollout -- eager launches, segment graphs, whole-step graphs -- fill the same experience buffer."""
import pytest
import torch

from test_env_gpu import make_task

pytestmark = pytest.mark.gpu

REGIMES = (("eager", "PHC_NO_ROLLOUT_GRAPH"), ("segments", "PHC_NO_STEP_GRAPH"), ("steps", None))
HORIZON, ROLLOUTS = 4, 3


@pytest.fixture(autouse=True)
def _training_flags():
    """The process-global flags as a training run has them (an in-process play or sweep of an earlier test module may have left its own behind)."""
    from phc_amd.utils.flags import flags
    old = (flags.test, flags.im_eval, flags.no_collision_check)
    flags.test = flags.im_eval = flags.no_collision_check = False
    yield
    flags.test, flags.im_eval, flags.no_collision_check = old


def _rollouts(monkeypatch, switch):
    """Three rollouts of a fresh (task, agent) pair under one regime -> (what each rollout left behind, the keys of the agent's graph store)."""
    from phc_amd.learning.amp_agent import IMAmpAgent
    for _, s in REGIMES:
        if s is not None:
            monkeypatch.delenv(s, raising=False)
    if switch is not None:
        monkeypatch.setenv(switch, "1")
    over = {"learning.params.config.horizon_length": HORIZON, "learning.params.config.amp_obs_demo_buffer_size": 512,
            "learning.params.config.amp_replay_buffer_size": 512, "+learning.params.config.hip_graph": True}
    task, env = make_task(64, motion="synthetic:2:1", seed=3, **over)
    assert task.whole_step_capturable()
    torch.manual_seed(5)
    agent = IMAmpAgent(env, task.cfg)
    torch.manual_seed(7)
    agent.init_train()
    agent.epoch_num = 2    # rollout graphs are admitted from here on; the first rollout still runs eagerly (it creates the reward accumulator)
    seen = []
    for _ in range(ROLLOUTS):
        with torch.no_grad(), agent.grads.shadow_scope():
            batch = agent.play_steps()
        torch.cuda.synchronize()
        out = {f"exp.{k}": v for k, v in agent.exp.items()}
        out.update(terminated_flags=batch["terminated_flags"], reward_raw=batch["reward_raw"], current_rewards=agent.current_rewards,
                   current_lengths=agent.current_lengths, progress_buf=task.progress_buf, reset_rng=task._reset_rng_dev)
        seen.append({k: v.clone() for k, v in out.items()})
    return seen, list(agent._roll_graphs)


def test_eager_segment_and_whole_step_rollouts_fill_the_same_experience_buffer(monkeypatch):
    """Twin (task, agent) pairs, 64 envs, horizon 4, same seeds, sampling noise replaced by zeros (actions = mu: the draw is the one thing a capture may
    number differently).  Three rollouts each: the first creates the reward accumulator eagerly, the second captures, the third only replays; the horizon
    crosses step 0 (no reset), step 1 (the reset carried over from the previous rollout) and a replay of every key.  After each rollout every tensor of the
    experience buffer, the batch's terminated flags and reward means, the episode statistics, the task's progress counters and its reset RNG counter are
    compared between the regimes.  Bound: bit equality -- the regimes issue the same launches on the same inputs, and the commit before the rollout moved
    into `rollout_graph.CapturedRollout` showed no difference in any tensor, rollout or pair of regimes (334 episode ends in the twelve steps)."""
    monkeypatch.setattr(torch, "randn", lambda *size, **kw: torch.zeros(*size, **kw))
    runs = {name: _rollouts(monkeypatch, switch) for name, switch in REGIMES}
    # the regime ran: no graph / segment graphs only / a whole-step graph for every step (next to the segment graphs of the first rollout, which has no accumulator yet)
    kinds = {name: {k[0] for k in keys} for name, (_, keys) in runs.items()}
    print("graph keys:", {name: sorted(k[:2] for k in keys) for name, (_, keys) in runs.items()})
    assert kinds["eager"] == set(), kinds
    assert kinds["segments"] == {"policy", "after"}, kinds
    assert {k[1] for k in runs["steps"][1] if k[0] == "step"} == set(range(HORIZON)), runs["steps"][1]
    ref = runs["eager"][0]
    dones = sum(int(r["exp.dones"].sum()) for r in ref)
    print(f"episode ends over {ROLLOUTS} rollouts: {dones}; reset RNG counter {int(ref[-1]['reset_rng'])}")
    worst = {}
    for name in ("segments", "steps"):
        for r, (a, b) in enumerate(zip(runs[name][0], ref)):
            for k in b:
                if not torch.equal(a[k], b[k]):
                    worst[(name, r, k)] = float((a[k].double() - b[k].double()).abs().max())
    print("differences from the eager rollout:", worst or "none")
    assert dones > 0, "no episode ended: the reset rule was not exercised"
    assert not worst, worst
