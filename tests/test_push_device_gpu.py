"""-m gpu: the device push schedule (`+perturb.rng=device`): phc_push_advance through the C ABI against the host build of phc_amd/csrc/phc_push.h
(tests/push_shim.cpp), a captured launch against eager ones, training under pushes with whole-step graphs, resuming, play and the evaluation sweep."""
import numpy as np
import pytest
import torch

import push_util as pu

pytestmark = pytest.mark.gpu
FORCE_TOL = 1e-3   # newtons: one fp32 ulp at 400 N is 3e-5 N, the device's cosf / sinf against glibc's differ by a few ulp
STEPS = 40


class DevPush:
    """Caller-side state of phc_push_advance in device memory, laid out like pu.HostPush; `force` and the state are followed by guard words."""
    def __init__(self, host, pad=64):
        from phc_amd import _lib as L
        n, nb = host.n, host.nb
        self.n, self.nb, self.L, self.PAD = n, nb, L, pad
        self.bodies = torch.zeros(len(host.bodies) + pad, dtype=torch.int32, device="cuda")
        self.bodies[:len(host.bodies)] = torch.from_numpy(host.bodies).cuda()
        self.state_buf = torch.full((5 * n + self.PAD,), pu.GUARD, dtype=torch.int32, device="cuda")
        self.state = self.state_buf[:5 * n].view(5, n)
        self.state.copy_(torch.from_numpy(host.state))
        self.force_buf = torch.full((n * nb * 3 + self.PAD,), pu.GUARD, dtype=torch.int32, device="cuda").view(torch.float32)
        self.force = self.force_buf[:n * nb * 3].view(n, nb, 3)
        self.force.zero_()
        self.progress = torch.zeros(n, dtype=torch.int64, device="cuda")
        a = L.PushArgs()
        for f, _ in L.PushArgs._fields_[:11]:   # the sizes, ranges, key and env_offset
            setattr(a, f, getattr(host.args, f))
        a.bodies, a.force = self.bodies.data_ptr(), self.force.data_ptr()
        for i, name in enumerate(("remaining", "countdown", "body", "k", "started")):
            setattr(a, name, self.state[i].data_ptr())
        self.args = a

    def advance(self, progress=None):
        if progress is not None:
            self.progress.copy_(torch.from_numpy(progress))
        self.args.progress_buf = None if progress is None else self.progress.data_ptr()
        return self.L.load().phc_push_advance(self.args, torch.cuda.current_stream().cuda_stream)

    def guards_intact(self):
        return bool((self.state_buf[5 * self.n:] == pu.GUARD).all()) and bool((self.force_buf.view(torch.int32)[self.n * self.nb * 3:] == pu.GUARD).all())


@pytest.mark.parametrize("direction", [0, 1], ids=["horizontal", "any"])
@pytest.mark.parametrize("n", [1, 70, 257])   # a single lane, a partial wavefront, one lane past a 256-thread block
def test_kernel_equals_the_host_build(n, direction):
    nb, listed = 24, [5, 23]                    # (the last body: the corner row of `force`)
    host = pu.HostPush(n, nb, listed, pause=(2, 5), duration=3, direction=direction, env_offset=1000)
    dev = DevPush(host)
    rng = np.random.default_rng(n)
    worst, pushes = 0.0, 0
    for t in range(STEPS):
        progress = None if t % 7 == 6 else rng.integers(0, 6, size=n).astype(np.int64)   # (zeros: envs reset since the last step; None: the nullable pointer)
        host.advance(progress)
        assert dev.advance(progress) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(dev.state.cpu().numpy(), host.state, err_msg=f"integer state, step {t}")
        got = dev.force.cpu().numpy()
        worst = max(worst, float(np.abs(got - host.force).max()))
        active = np.zeros((n, nb), dtype=bool)
        rows = host.body >= 0
        active[np.nonzero(rows)[0], host.body[rows]] = True
        assert (got[~active] == 0).all(), f"step {t}: force outside the active rows"
        assert (np.linalg.norm(got[active], axis=-1) >= 200 - 1e-3).all()
        assert dev.guards_intact(), f"step {t}"
    pushes = int(host.started.sum())
    print(f"N = {n}, direction {direction}: max |kernel - host build| force = {worst:.3e} N over {STEPS} steps, {pushes} pushes")
    assert pushes >= 3 * n and worst <= FORCE_TOL
    assert (host.state[3] == STEPS).all()


def test_entry_point_refuses_bad_arguments():
    """The value checks of `phc_push_advance` itself (null pointers: the host checker it calls, tests/test_push_device_cpu.py).  Every pointer is device
    memory with room behind it for the largest sizes tried, so that a check that stopped refusing would show as a failed assertion and nothing else."""
    from test_push_device_cpu import BAD_ARGS
    dev = DevPush(pu.HostPush(4, 4, [0, 2]), pad=4096)
    fn, stream = dev.L.load().phc_push_advance, torch.cuda.current_stream().cuda_stream
    for f, bad in BAD_ARGS:
        keep = getattr(dev.args, f)
        setattr(dev.args, f, bad)
        assert fn(dev.args, stream) == -1, (f, bad)
        setattr(dev.args, f, keep)
    torch.cuda.synchronize()
    assert (dev.state[3] == 0).all() and (dev.force == 0).all() and dev.guards_intact(), "a refused call launches nothing"
    dev.args.num_envs = 0
    assert fn(dev.args, stream) == 0
    torch.cuda.synchronize()
    assert (dev.state[3] == 0).all(), "no envs: nothing to launch"
    dev.args.num_envs = 4
    assert dev.advance() == 0
    torch.cuda.synchronize()
    assert (dev.state[3] == 1).all() and dev.guards_intact()


NAMES = [f"b{i}" for i in range(24)]
CFG = dict(force=[200, 400], bodies=["b0", "b23"], interval_s=[0.1, 0.2], duration_s=0.1, direction="any", seed=11, rng="device")


def _schedule(n=70, **kw):
    from phc_amd.perturb import make_schedule
    return make_schedule(dict(CFG, **kw), n, NAMES, 1 / 30, "cuda")


def test_graph_replay_draws_anew():
    """One captured `advance`, replayed 40 times, against 40 eager launches of a twin: equal bit for bit -- a stream frozen at capture would repeat a step."""
    a, b = _schedule(), _schedule()
    assert a.capturable and a.pause_steps == (3, 6) and a.duration_steps == 3
    progress = torch.ones(70, dtype=torch.int64, device="cuda")
    for s in (a, b):            # (the first launch loads the code object: outside the capture)
        s.advance(progress)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.advance(progress)
    torch.cuda.synchronize()
    assert torch.equal(a._state, b._state), "a capture launches nothing"
    forces = []
    for t in range(STEPS):
        progress.fill_(1)
        progress[t % 70] = 0    # one env reset per step
        g.replay()
        b.advance(progress)
        torch.cuda.synchronize()
        assert torch.equal(a._state, b._state) and torch.equal(a.force, b.force), t
        forces.append(a.force.clone())
    assert int(a.pushes) == int(b.pushes) > 70 and a.pushes.dim() == 0
    assert len({f.cpu().numpy().tobytes() for f in forces}) > STEPS // 2, "the replays must move on"
    assert (a._state[3] == STEPS + 1).all()
    other = _schedule(seed=12)
    for _ in range(STEPS + 1):
        other.advance(None)
    assert not torch.equal(other.force, b.force) or not torch.equal(other._state, b._state)
    with pytest.raises(ValueError, match="progress_buf"):
        a.advance(progress == 0)


def test_state_dict_round_trip_and_env_offset():
    a = _schedule()
    for _ in range(15):
        a.advance()
    sd = a.state_dict()
    assert not sd["state"].is_cuda
    b = _schedule()
    b.load_state_dict(sd)
    for _ in range(15):
        a.advance()
        b.advance()
    assert torch.equal(a._state, b._state) and torch.equal(a.force, b.force) and int(a.pushes) > 0
    with pytest.raises(ValueError, match="another size"):
        _schedule(n=71).load_state_dict(sd)
    # the ranks of one run: rank 1's envs continue rank 0's global numbering
    from phc_amd.perturb import DevicePushSchedule
    big, r1 = _schedule(n=140), DevicePushSchedule(CFG, 70, NAMES, 1 / 30, "cuda", env_offset=70)
    for _ in range(20):
        big.advance()
        r1.advance()
    assert torch.equal(big.force[70:], r1.force) and torch.equal(big._state[:, 70:], r1._state) and not torch.equal(big.force[:70], r1.force)


# ---- the task, the learner, play and the sweep ---------------------------------------------------------------------------------------------------------------------
SMALL = ["learning.params.config.minibatch_size=64", "learning.params.config.amp_obs_demo_buffer_size=512", "learning.params.config.amp_replay_buffer_size=512"]
PUSH = ["+perturb.force=[200,400]", "+perturb.bodies=[Pelvis,Torso]", "+perturb.interval_s=[0.1,0.2]", "+perturb.duration_s=0.1", "+perturb.seed=3", "+perturb.rng=device"]


def _task(extra=(), num_envs=4, motion="synthetic:4:0"):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    return parse_task(compose([f"env.num_envs={num_envs}", f"env.motion_file={motion}"] + list(extra)))


def test_training_under_pushes_replays_whole_steps():
    """64 envs, horizon 8, one clip, three epochs (the third replays captured whole steps): pushes in every epoch, `("step", n, ...)` graphs, finite parameters."""
    from phc_amd.learning.amp_agent import IMAmpAgent
    from phc_amd.perturb import DevicePushSchedule
    task, env = _task(["learning.params.config.horizon_length=8", "learning.params.config.minibatch_size=512", "learning.params.config.mini_epochs=2",
                       "learning.params.config.amp_obs_demo_buffer_size=512", "learning.params.config.amp_replay_buffer_size=512",
                       "+learning.params.config.hip_graph=True", "+perturb.force=[200,400]", "+perturb.interval_s=[0.067,0.133]", "+perturb.duration_s=0.067",
                       "+perturb.rng=device"], num_envs=64, motion="stand:4")
    assert type(task._push) is DevicePushSchedule and task._push.pause_steps == (2, 4) and task._push.duration_steps == 2
    assert task.whole_step_capturable()
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    infos, real = [], agent.train_epoch

    def recorded():
        infos.append(real())
        return infos[-1]
    agent.train_epoch = recorded
    agent.train(3, log=None)
    torch.cuda.synchronize()
    pushes = [i["perturb/pushes"] for i in infos]
    print("perturb/pushes per epoch:", pushes, "graph keys:", sorted(k[:2] for k in agent._roll_graphs))
    assert len(pushes) == 3 and all(p > 0 for p in pushes), pushes
    assert sum(pushes) == int(task._push.pushes)
    steps = {k[1] for k in agent._roll_graphs if k[0] == "step"}
    assert steps == set(range(8)), "whole-step graphs in use"
    assert (task._push._state[3] == 24).all(), "one launch per env step, captured ones included"
    assert all(torch.isfinite(p).all() for p in agent.model.parameters())
    assert "perturb/pushes" in agent.assemble_train_info(infos[-1])


RESUME = ["+perturb.force=[1,2]", "+perturb.bodies=[Pelvis,Torso]", "+perturb.interval_s=[0.1,0.2]", "+perturb.duration_s=0.1", "+perturb.rng=device"]


def test_resumed_run_continues_its_pushes():
    """The state after 10 steps into a fresh task, then the same 10 steps in both: equal force histories.  A resumed run resets every env (restore, then
    `train()`), so the first run does that too where the state is taken.  A small force on the stand clip with zero actions: nothing falls."""
    def steps(task, count):
        act = torch.zeros(task.num_envs, task.num_dof, device=task.device)
        out = []
        for _ in range(count):
            task.step(act)
            out.append((task._push.force.clone(), task.progress_buf.clone(), task._push._state.clone()))
        return out

    def restart(env):
        torch.manual_seed(5)
        env.reset()
    task, env = _task(RESUME, num_envs=8, motion="stand:4")
    restart(env)
    steps(task, 10)
    torch.cuda.synchronize()
    saved = task.get_env_rng_state()
    assert "push_schedule" in saved and int(task._push.pushes) > 0 and int(saved["push_schedule"]["state"][3, 0]) == 10
    restart(env)
    want = steps(task, 10)
    fresh, fenv = _task(RESUME, num_envs=8, motion="stand:4")
    fresh.set_env_rng_state(saved)
    restart(fenv)
    got = steps(fresh, 10)
    for t, ((fw, pw, sw), (fg, pg, sg)) in enumerate(zip(want, got)):
        assert torch.equal(pw, pg), f"step {t}: progress"
        assert torch.equal(sw, sg) and torch.equal(fw, fg), f"step {t}"
    assert any(float(f.abs().sum()) > 0 for f, _, _ in want) and len({f.cpu().numpy().tobytes() for f, _, _ in want}) > 1
    again, aenv = _task(RESUME, num_envs=8, motion="stand:4")    # without the state the same steps push elsewhere: the draws go on from k = 10
    restart(aenv)
    assert any(not torch.equal(f, g[0]) for (f, _, _), g in zip(want, steps(again, 10)))
    fresh.set_env_rng_state({"reset_rng_counter": 3, "reset_counter": 1})   # a checkpoint without the key loads as before
    assert int(fresh._reset_rng_dev.item()) == 3 and int(fresh._push._state[3, 0]) == 20


def test_checkpoint_restores_the_schedule_for_a_same_size_training_run_only(tmp_path, capsys):
    """Through `agent.save` / `agent.restore`, what `python -m phc_amd.run` does: the same env count continues the schedule; another env count and play /
    the sweep (`flags.test`) restore the policy and leave the schedule as configured."""
    from phc_amd.learning.amp_agent import IMAmpAgent
    from phc_amd.utils.flags import flags

    def agent_of(num_envs):
        task, env = _task(SMALL + RESUME, num_envs=num_envs, motion="stand:4")
        torch.manual_seed(1)
        return IMAmpAgent(env, task.cfg), task, env
    agent, task, env = agent_of(8)
    env.reset()
    act = torch.zeros(8, task.num_dof, device=task.device)
    for _ in range(12):
        task.step(act)
    path = str(tmp_path / "Humanoid.pth")
    agent.save(path)
    torch.cuda.synchronize()
    want_state, want_force = task._push._state.clone(), task._push.force.clone()
    assert int(task._push.pushes) > 0
    same, t_same, _ = agent_of(8)
    same.restore(path)
    assert torch.equal(t_same._push._state, want_state) and torch.equal(t_same._push.force, want_force)
    capsys.readouterr()
    other, t_other, e_other = agent_of(4)
    other.restore(path)                                          # (before: ValueError, push schedule state of another size)
    assert "push schedule state not restored" in capsys.readouterr().out
    assert (t_other._push._state[3] == 0).all() and (t_other._push.force == 0).all()
    for a, b in zip(agent.model.parameters(), other.model.parameters()):
        assert torch.equal(a, b)
    e_other.reset()
    for _ in range(12):                                          # ... and the schedule runs
        t_other.step(torch.zeros(4, t_other.num_dof, device=t_other.device))
    assert int(t_other._push.pushes) > 0
    play, t_play, _ = agent_of(8)
    flags.test = True
    try:
        play.restore(path, load_optimizer=False)
    finally:
        flags.test = False
    assert (t_play._push._state[3] == 0).all(), "play and the sweep start the configured schedule, not the training run's"


def _sweep(mode):
    from phc_amd.learning.amp_agent import IMAmpAgent
    task, env = _task(SMALL + PUSH + [f"+learning.params.config.eval_metrics={mode}"])
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    info, failed = agent.eval(log=None)
    torch.cuda.synchronize()
    return info, agent, task, env


def test_play_and_evaluation_under_device_pushes():
    from phc_amd.run import play
    host, agent, task, env = _sweep("host")
    device = _sweep("device")[0]
    print(host, device)
    assert host["perturb_pushes"] > 0 and host["perturb_pushes"] == device["perturb_pushes"]
    assert all(np.isfinite(v) for v in host.values()) and all(np.isfinite(v) for v in device.values())
    out = play(agent, task, env, steps=30)
    assert out["perturb_pushes"] > 0 and np.isfinite(out["mean_episode_reward"])
