"""HumanoidTeleop on the MI355X: the phc_teleop_rewards kernel against the host build of phc_amd/csrc/phc_teleop.h (tests/teleop_shim.cpp), the task end to end
against HumanoidIm plus a torch restatement of the active terms, the recovery window after a velocity push, and captured whole rollout steps."""
import numpy as np
import pytest
import torch

import teleop_util as tu
from phc_amd import _lib as L

pytestmark = pytest.mark.gpu
F = np.float32
SPECS = {"r_feet_ori": -1.0, "r_torques": -1e-5, "r_dof_pos_limits": -10.0, "r_feet_air_time_teleop": 10.0, "r_torque_limits": -5.0, "r_dof_vel": -1e-3,
         "r_stumble": -2.0, "r_dof_acc": -2.5e-7, "r_action_rate": -0.01, "r_slippage": -1.0, "r_feet_contact_forces": -0.01, "max_contact_force": 200.0}
SPEC_ARGS = [f"+env.reward_specs.{k}={v}" for k, v in SPECS.items()]


@pytest.fixture(autouse=True)
def _training_flags():
    """The process-global flags as a training run has them (an in-process play or sweep of an earlier test module may have left its own behind)."""
    from phc_amd.utils.flags import flags
    old = (flags.test, flags.im_eval, flags.no_collision_check)
    flags.test = flags.im_eval = flags.no_collision_check = False
    yield
    flags.test, flags.im_eval, flags.no_collision_check = old


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _back(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _device_launch(lib, a):
    return L.load().phc_teleop_rewards(lib, a, torch.cuda.current_stream().cuda_stream)


def _pair(x, terms, **kw):
    return tu.Runner(x, tu.host_launch, terms, **kw), tu.Runner(x, _device_launch, terms, to=_to, back=_back, **kw)


def _compare(host, dev, steps, what):
    for s in range(steps):
        (rh, rawh), (rd, rawd) = host.step(s), dev.step(s)
        tu.close(rawd, rawh, f"{what} step {s} reward_raw")
        tu.close(rd, rh, f"{what} step {s} rew_buf")
        sh, sd = host.state_np(), dev.state_np()
        for k in ("last_contacts", "recovery_counter", "last_actions", "last_dof_vel"):
            np.testing.assert_array_equal(sd[k], sh[k], err_msg=f"{what} step {s}: {k}")
        tu.close(sd["feet_air_time"], sh["feet_air_time"], f"{what} step {s} feet_air_time")


# one env / a partial block plus one group / two blocks plus two groups; one DoF, H1's, G1's (two passes over the row), SMPL's (three); two and four feet
SHAPES = [(1, 1, 2), (1, 19, 4), (65, 19, 2), (65, 69, 4), (130, 37, 4), (130, 69, 2)]


@pytest.mark.parametrize("n,d,nf", SHAPES)
def test_kernel_equals_the_host_build(n, d, nf):
    feet = [3, 1, 4, 0][:nf]
    x = tu.random_case(n, d, feet, nb=6, steps=2, seed=n + d)
    scales = {t: 0.5 + 0.1 * i for i, t in enumerate(tu.TERMS)}
    order = list(tu.TERMS[::-1])
    host, dev = _pair(x, order, scales=scales, push_interval=2, recovery_steps=3)
    for r in (host, dev):
        r.dr_k = np.array([(e % 3) * 2 for e in range(n)], np.int32)   # k = 0: nothing; 2, 4: the next step pushes
        r.progress = [np.full(n, 1, np.int64), np.full(n, 1, np.int64)]  # (step 1: every env whose counter was written is gated: lookup at progress + 1)
    _compare(host, dev, 2, f"all terms n={n} d={d} feet={nf}")
    assert (dev.state_np()["recovery_counter"] == np.where(np.arange(n) % 3 > 0, 4, 0)).all()
    for t in tu.TERMS:
        _compare(*_pair(x, [t], with_state=t in ("dof_acc", "action_rate")), 2, f"{t} alone n={n} d={d} feet={nf}")
    # R = 0: the imitation columns copied (4 of them here), rew_buf unchanged
    dev0 = tu.Runner(x, _device_launch, [], to=_to, back=_back, with_state=False, im_cols=4)
    rew, raw = dev0.step(0)
    np.testing.assert_array_equal(raw, x["reward_im"][0][:, :4])
    np.testing.assert_array_equal(rew, x["rew_in"][0])


def test_two_launches_are_bit_identical_and_the_bits_do_not_depend_on_the_env_count():
    x = tu.random_case(130, 69, [0, 1, 2, 3], nb=5, steps=1, seed=9)
    terms = list(tu.TERMS)
    outs = [tu.Runner(x, _device_launch, terms, to=_to, back=_back).step(0) for _ in range(2)]
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
    small = {k: (v[:, :65] if isinstance(v, np.ndarray) and v.ndim >= 2 and v.shape[1] == 130 else v) for k, v in x.items()}
    small["feet_air_time0"], small["last_contacts0"] = x["feet_air_time0"][:65], x["last_contacts0"][:65]
    rew, raw = tu.Runner(small, _device_launch, terms, to=_to, back=_back).step(0)
    assert rew.tobytes() == outs[0][0][:65].tobytes() and raw.tobytes() == outs[0][1][:65].tobytes()
    rew_h, raw_h = tu.Runner(x, tu.host_launch, terms).step(0)
    tu.close(raw_h, outs[0][1], "host build")


# ---- the task ----------------------------------------------------------------------------------------------------------------------------------------------
def _task(*extra, task="HumanoidTeleop", n=8, seed=0):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(seed)
    return parse_task(compose([f"env.num_envs={n}", "env.motion_file=armswing:10", f"env.task={task}", *tu.H1_OVER, *extra]))


def _actions(t, n=8):
    g = torch.Generator().manual_seed(100 + t)
    return ((torch.rand(n, 19, generator=g) * 2 - 1) * 0.3).cuda()


def test_end_to_end_equals_humanoid_im_plus_the_torch_restatement():
    """H1, 8 envs, armswing, 6 steps, same seed and actions: the imitation columns are HumanoidIm's bit for bit, the reward is HumanoidIm's plus the restated
    terms (the reference speed of the air-time gate read from ref_body_vel BEFORE each step), the state is the restatement's."""
    im, env_im = _task(task="HumanoidIm")
    tele, env_t = _task(*SPEC_ARGS)
    names = [n for n in SPECS if n.startswith("r_")]
    C = im.reward_raw.shape[1]
    assert tele.reward_names == names and tele.reward_raw.shape == (8, C + 11) and tele.whole_step_capturable()
    for e in (env_im, env_t):   # (the reset draws its start phases from torch's generator)
        torch.manual_seed(5)
        e.reset()
    st = dict(last_actions=torch.zeros(8, 19, device="cuda"), last_dof_vel=torch.zeros(8, 19, device="cuda"), feet_air_time=torch.zeros(8, 2, device="cuda"),
              last_contacts=torch.zeros(8, 2, dtype=torch.bool, device="cuda"))
    seen = {n: [] for n in names}
    for t in range(6):
        im.reset_done()
        tele.reset_done()
        ref_xy = tele.ref_body_vel[:, 0, :2].clone()
        act = _actions(t)
        env_im.step(act.clone())
        env_t.step(act.clone())
        torch.cuda.synchronize()
        assert torch.equal(tele._rigid_body_state, im._rigid_body_state) and torch.equal(tele.progress_buf, im.progress_buf)
        assert torch.equal(tele.reward_raw[:, :C], im.reward_raw) and torch.equal(tele.reset_buf, im.reset_buf)
        terms = tu.restate(tele, st, ref_xy)
        total = im.rew_buf.double()
        for c, name in enumerate(names):
            col = terms[name[2:]].double() * float(np.float32(tele.reward_scales[name]))
            tu.close(tele.reward_raw[:, C + c].cpu().numpy(), col.cpu().numpy(), f"step {t} {name}")
            total = total + col
            seen[name].append(col.abs().max().item())
        tu.close(tele.rew_buf.cpu().numpy(), total.cpu().numpy(), f"step {t} rew_buf")
        assert torch.equal(tele.last_actions, st["last_actions"]) and torch.equal(tele.last_dof_vel, st["last_dof_vel"])
        assert torch.equal(tele.last_contacts.bool(), st["last_contacts"])
        tu.close(tele.feet_air_time.cpu().numpy(), st["feet_air_time"].cpu().numpy(), f"step {t} feet_air_time")
        assert tele.extras["reward_raw"].shape == (8, C + 11) and not tele._recovery_counter.any()
    print({n: max(v) for n, v in seen.items()})
    for name in ("r_torques", "r_dof_vel", "r_dof_acc", "r_action_rate"):   # (what a standing robot with moving arms certainly produces)
        assert max(seen[name]) > 0, name


PUSH_ONLY = ["domain_rand=h1_dr", "domain_rand.randomize_friction=False", "domain_rand.randomize_base_com=False", "domain_rand.randomize_link_mass=False",
             "domain_rand.randomize_pd_gain=False", "domain_rand.randomize_torque_rfi=False", "domain_rand.randomize_ctrl_delay=False"]


def test_recovery_window_after_a_push():
    """Pushes every 5 env steps, a window of 3, a termination distance every env exceeds: an episode lasts two steps (the reset test waits for progress > 1),
    so the envs end at steps 1 and 3; the launch of step 4 sees k = 5 and arms the counter; the push of step 5 finds envs 0, 1, 3 .. 7 at progress 1 and they
    are held -- no reset, no termination, progress unchanged -- for steps 5, 6, 7 and end at step 8.  Env 2 is reset right before step 5: it is neither pushed
    (phc_dr_advance skips an env at progress 0) nor held, and ends at step 6."""
    task, env = _task(*PUSH_ONLY, "domain_rand.push_interval_s=0.1", "env.push_recovery_steps=3", "env.terminationDistance=0.00001",
                      "env.enableEarlyTermination=True", "env.stateInit=Start", "+env.reward_specs.r_action_rate=-0.01")
    assert task._dr.push_interval == 5 and task._recovery_steps == 3 and task._dr.delay_range is None
    env.reset()
    others = torch.tensor([0, 1, 3, 4, 5, 6, 7], device="cuda")
    log = []
    for t in range(9):
        task.reset_done()
        if t == 5:
            task.reset(torch.tensor([2], device="cuda"))
            assert int(task._recovery_counter[2]) == 0 and int(task.progress_buf[2]) == 0
        env.step(_actions(t))
        torch.cuda.synchronize()
        log.append({k: getattr(task, k).clone() for k in ("progress_buf", "reset_buf", "_terminate_buf", "_recovery_counter")})
    for t in (1, 3):
        assert (log[t]["_terminate_buf"] == 1).all() and (log[t]["progress_buf"] == 2).all(), "the premise: every env ends after two steps"
    assert (log[3]["_recovery_counter"] == 0).all() and (log[4]["_recovery_counter"] == 4).all() and (log[4]["progress_buf"] == 1).all()
    for t, left in ((5, 3), (6, 2), (7, 1)):
        for k in ("reset_buf", "_terminate_buf"):
            assert (log[t][k][others] == 0).all(), (t, k)
        assert (log[t]["progress_buf"][others] == 1).all() and (log[t]["_recovery_counter"][others] == left).all(), t
    assert (log[8]["_terminate_buf"][others] == 1).all() and (log[8]["reset_buf"][others] == 1).all() and (log[8]["progress_buf"][others] == 2).all()
    assert [int(log[t]["progress_buf"][2]) for t in (5, 6)] == [1, 2] and int(log[6]["_terminate_buf"][2]) == 1
    assert all(int(log[t]["_recovery_counter"][2]) == 0 for t in (5, 6, 7))
    assert (task._dr.k == 9).all()


def test_captured_rollout_step_equals_the_eager_one():
    """Under domain_rand=h1_dr a captured reset_done + step, replayed, moves on like eager steps of a twin: physics, rewards, columns, the terms' state and
    the recovery counter, bit for bit."""
    extra = ["domain_rand=h1_dr", "domain_rand.push_interval_s=0.1", "env.enableEarlyTermination=False", "env.stateInit=Start", *SPEC_ARGS]
    (a, env_a), (b, env_b) = _task(*extra, n=4), _task(*extra, n=4)
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    assert a.whole_step_capturable() and type(a).post_physics_step is HumanoidIm.post_physics_step
    for task, env in ((a, env_a), (b, env_b)):
        env.reset()
        for t in range(3):
            task.reset_done()
            env.step(_actions(t, 4))
    torch.cuda.synchronize()
    names = ("_root_states", "_dof_state", "rew_buf", "reward_raw", "last_actions", "last_dof_vel", "feet_air_time", "last_contacts", "_recovery_counter",
             "progress_buf")
    for name in names:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    act = _actions(50, 4)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.reset_done()
        a.step(act)
    torch.cuda.synchronize()
    assert torch.equal(a.last_actions, b.last_actions) and torch.equal(a._dr.k, b._dr.k), "a capture launches nothing"
    seen = []
    for t in range(4):
        g.replay()
        b.reset_done()
        b.step(act)
        torch.cuda.synchronize()
        for name in names:
            assert torch.equal(getattr(a, name), getattr(b, name)), (t, name)
        seen.append(int(a._recovery_counter.max()))
    assert (a._dr.k == 7).all() and max(seen) == 61, seen   # the launch of the step that made k = 5 armed the default window of 60 (+ 1)


def test_training_under_h1_dr_replays_whole_steps():
    from phc_amd.learning.amp_agent import IMAmpAgent
    task, env = _task("domain_rand=h1_dr", "+env.reward_specs.r_action_rate=-0.01", "+env.reward_specs.r_torques=-1e-5",
                      "learning.params.config.horizon_length=8", "learning.params.config.minibatch_size=512", "learning.params.config.mini_epochs=2",
                      "learning.params.config.amp_obs_demo_buffer_size=512", "learning.params.config.amp_replay_buffer_size=512",
                      "+learning.params.config.hip_graph=True", n=64)
    assert task.whole_step_capturable() and task.reward_raw.shape[1] == task.num_im_reward_columns + 2
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    infos, real = [], agent.train_epoch

    def recorded():
        infos.append(real())
        return infos[-1]
    agent.train_epoch = recorded
    agent.train(3, log=None)
    torch.cuda.synchronize()
    steps = {k[1] for k in agent._roll_graphs if k[0] == "step"}
    assert steps == set(range(8)), "whole-step graphs in use"
    assert (task._dr.k == 24).all(), "one launch per env step, captured ones included"
    assert all(torch.isfinite(p).all() for p in agent.model.parameters())
    raw = np.asarray(infos[-1]["reward_raw"], dtype=np.float64)
    assert raw.shape == (task.reward_raw.shape[1],) and np.isfinite(raw).all() and raw[-2] < 0 and raw[-1] < 0
