"""-m gpu: `+env.task_rng=device` with add_obs_noise / fut_tracks_dropout / occl_training -- phc_obs_augment / phc_occl_advance against the host build of
phc_obs_aug.h and the fp64 oracle, the task in device mode against a twin without the option, capturability, whole-step graphs against eager rollouts, the
checkpoint round trip, and the untouched default path."""
import numpy as np
import pytest
import torch

import obs_aug_util as ou
from test_env_gpu import make_task

pytestmark = pytest.mark.gpu

DEVICE = {"+env.task_rng": "device"}
NOISE = {"env.add_obs_noise": True}
DROPOUT = {"env.fut_tracks": True, "env.numTrajSamples": 3, "env.obs_v": 6, "+env.fut_tracks_dropout": True}
OCCL = {"+env.occl_training": True}
MCP_GETUP = {"env": "env_im_getup_mcp", "learning": "im_mcp", "env.num_prim": 3}
STD = float(np.float32(0.1))


@pytest.fixture(autouse=True)
def _training_flags():
    """The process-global flags as a training run has them (an in-process play or sweep of an earlier test module may have left its own behind)."""
    from phc_amd.utils.flags import flags
    old = (flags.test, flags.im_eval, flags.no_collision_check)
    flags.test = flags.im_eval = flags.no_collision_check = False
    yield
    flags.test, flags.im_eval, flags.no_collision_check = old


def _stream():
    return torch.cuda.current_stream().cuda_stream


class DeviceCopy:
    """The backing buffers of an obs_aug_util state on the device, guard elements included."""

    def __init__(self, s):
        self.s = s
        self.t = {name: torch.from_numpy(b.copy()).cuda() for name, b in s.back.items()}

    def pointers(self):
        return {name: t.data_ptr() for name, t in self.t.items()}

    def fetch(self):
        out = self.s.clone()
        for name, t in self.t.items():
            out.back[name][...] = t.cpu().numpy()
        return out


def _augment(dev):
    from phc_amd import _lib as L
    rc = L.load().phc_obs_augment(dev.s.args(dev.pointers()), _stream())
    torch.cuda.synchronize()
    return rc


def _selections(n):
    yield "all", None
    for done in ou.DONE_SETS:
        yield "flag", done
    yield "ids", np.random.default_rng(n).permutation(np.arange(0, n, 2))   # a permuted list
    yield "ids", np.array([n - 1])                                          # one element
    yield "ids", np.array([], dtype=np.int64)                               # empty


# ---- C ABI against the host build and the fp64 oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ou.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_obs_augment_equals_the_host_build(case):
    """Every shape of obs_aug_util.CASES x every selection form (all rows; row_flag over five done sets; env_ids permuted / one element / empty).  Counters, flags,
    id lists, guard elements, untouched rows and -- without noise -- the whole observation are bit-equal to the host build's; with noise every element is within
    E = 2^-23 |o'| + noise_std r 2^-19 of the fp64 oracle (obs_aug_util.check_call), and the dropout decisions under the noise are the host build's (a dropped
    column is noise alone).  Measured on an MI355X: see profiles/obs_device/README.md."""
    worst = 0.0
    for form, select in _selections(case[0]):
        s = ou.AugState(*case, form=form, select=select, seed=case[1])
        what = f"{case} {form} {select}: "
        dev = DeviceCopy(s)
        assert _augment(dev) == 0, what
        got = dev.fetch()
        worst = max(worst, ou.check_call(s, got, what))
        host = s.clone()
        host.run_host()
        ou.assert_bytes_equal(got, host, ("k", "row_flag", "env_ids") + (() if s.noise_std > 0 else ("obs",)), what)
    print(f"{case}: largest error / bound on the device = {worst:.3f}")


@pytest.mark.parametrize("n", ou.OCCL_N)
def test_occl_advance_equals_the_host_build_bit_for_bit(n):
    from phc_amd import _lib as L
    for J in ou.OCCL_J:
        s = ou.OcclState(n, J, seed=n + J)
        dev = DeviceCopy(s)
        for call in range(3):
            assert s.call(L.load().phc_occl_advance, dev.pointers(), _stream()) == 0
            s.run_host()
        torch.cuda.synchronize()
        got = dev.fetch()
        assert got.guards_intact() and (got["k"] == s["k"]).all()
        ou.assert_bytes_equal(got, s, ("k", "count", "mask"), f"n={n} J={J}: ")


def test_a_second_launch_draws_anew_and_restored_counters_give_the_same_bits():
    s = ou.AugState(65, 513, 0, 3, 0.1, 0.1, form="flag", select="alternate", seed=9)
    dev = DeviceCopy(s)
    assert _augment(dev) == 0
    one = dev.fetch()
    dev.t["obs"].copy_(torch.from_numpy(s.back["obs"]))
    assert _augment(dev) == 0
    two = dev.fetch()
    rows = s.rows()
    assert np.array_equal(two["k"][rows], s["k"][rows] + 2) and not np.array_equal(two["obs"][rows], one["obs"][rows])
    assert np.abs(two["obs"][rows] - one["obs"][rows]).max() > 0.1
    dev.t["obs"].copy_(torch.from_numpy(s.back["obs"]))
    dev.t["k"].copy_(torch.from_numpy(s.back["k"]))
    assert _augment(dev) == 0
    ou.assert_bytes_equal(dev.fetch(), one, ("obs", "k", "row_flag"), "restored counters: ")


# ---- the task in device mode ---------------------------------------------------------------------------------------------------------------------------
def _actions(task, g, scale=2.0):
    return (torch.rand(task.num_envs, 69, device=task.device, generator=g) - 0.5) * scale


def _twins(n, seed, option, **over):
    pair = []
    for opt in (option, {}):
        task, env = make_task(n, motion="synthetic:3:1", seed=seed, **opt, **DEVICE, **over)
        torch.manual_seed(seed + 1)
        env.reset()
        pair.append((task, env))
    return pair


def _noise_ratio(task, rows, k_before, noisy, clean):
    """max over the rows of |noisy - (clean + noise_std * the host build's normals)| / E."""
    genv = task._task_env_offset + rows
    z = ou.normals(task._obs_aug_key, genv, k_before[rows], noisy.shape[1]).astype(np.float64)
    _, r = ou.normals_f64(task._obs_aug_key, genv, k_before[rows], noisy.shape[1])
    err = np.abs(noisy[rows].astype(np.float64) - (clean[rows].astype(np.float64) + STD * z))
    return float((err / ou.noise_bound(noisy[rows].astype(np.float64), r, STD)).max())


def test_noise_of_the_task_is_the_host_builds_on_the_steps_rows_and_on_the_reset_rows():
    """64 envs; a twin task with the same seed and the option off receives the same actions, so its observation is the clean one.  After every step
    noisy - clean == noise_std * the host build's normals of (key, env, k) within E on every row; after reset_done() on the reset rows only -- every other row
    and counter is untouched."""
    n = 64
    (noisy, nenv), (clean, cenv) = _twins(n, 2, NOISE)
    assert noisy._obs_aug_k is not None and clean._obs_aug_k is None and noisy._occl_k is None
    assert (noisy._obs_aug_k == 2).all()   # reset(): two reset launches over every env
    every = np.arange(n)
    worst = _noise_ratio(noisy, every, np.ones(n, np.int32), noisy.obs_buf.cpu().numpy(), clean.obs_buf.cpu().numpy())
    g = torch.Generator(device=noisy.device).manual_seed(3)
    resets = 0
    for _ in range(10):
        a = _actions(noisy, g)
        k0 = noisy._obs_aug_k.cpu().numpy().copy()
        nenv.step(a), cenv.step(a)
        assert torch.equal(noisy._root_states, clean._root_states) and torch.equal(noisy.reset_buf, clean.reset_buf)
        obs_n, obs_c = noisy.obs_buf.cpu().numpy().copy(), clean.obs_buf.cpu().numpy()
        worst = max(worst, _noise_ratio(noisy, every, k0, obs_n, obs_c))
        assert np.array_equal(noisy._obs_aug_k.cpu().numpy(), k0 + 1)
        done = np.flatnonzero(noisy.reset_buf.cpu().numpy() != 0)
        noisy.reset_done(), clean.reset_done()
        after, k1 = noisy.obs_buf.cpu().numpy(), noisy._obs_aug_k.cpu().numpy()
        rest = np.setdiff1d(every, done)
        assert np.array_equal(after[rest].view(np.uint32), obs_n[rest].view(np.uint32)) and np.array_equal(k1[rest], k0[rest] + 1)
        assert np.array_equal(k1[done], k0[done] + 2)
        if len(done):
            worst = max(worst, _noise_ratio(noisy, done, k0 + 1, after, clean.obs_buf.cpu().numpy()))
            resets += len(done)
    print(f"noise against the host build's normals: largest error / E = {worst:.3f}; reset rows checked: {resets}")
    assert resets > 0, "no episode ended: the reset rows were not exercised"
    assert worst <= 1.0, worst


def test_dropout_of_the_task_zeroes_exactly_the_host_builds_blocks():
    """fut_tracks (numTrajSamples 3, obs_v 6) with fut_tracks_dropout and no noise: after every step the zeroed blocks are those of the host build's uniforms,
    every other column is the clean twin's, bit for bit."""
    n = 64
    (drop, denv), (clean, cenv) = _twins(n, 4, {"+env.fut_tracks_dropout": True}, **{k: v for k, v in DROPOUT.items() if k != "+env.fut_tracks_dropout"})
    assert drop._fut_tracks_dropout and not clean._fut_tracks_dropout and drop._obs_aug_k is not None and clean._obs_aug_k is None
    so, T, width = drop.get_self_obs_size(), 3, drop.obs_buf.shape[1]
    W, P = (width - so) // T, (width + 1) // 2
    g = torch.Generator(device=drop.device).manual_seed(5)
    zeroed = 0
    for _ in range(6):
        a = _actions(drop, g, 0.5)
        k0 = drop._obs_aug_k.cpu().numpy().copy()
        denv.step(a), cenv.step(a)
        dropped = ou.uniforms(drop._obs_aug_key, drop._task_env_offset + np.arange(n), k0, P, T)[:, :, 0] < np.float32(0.1)
        want = clean.obs_buf.cpu().numpy().copy()
        want[:, so:].reshape(n, T, W)[dropped] = 0.0
        assert np.array_equal(drop.obs_buf.cpu().numpy().view(np.uint32), want.view(np.uint32))
        zeroed += int(dropped.sum())
        drop.reset_done(), clean.reset_done()
    assert 0 < zeroed < 0.3 * 6 * n * T, zeroed


def test_occlusion_schedule_of_the_task_is_the_host_builds_and_torchs_generator_stays():
    """occl_training + add_obs_noise in device mode: after three steps random_occlu_count equals three calls of the host build from zeros, the mask is the
    reference's (bodies 9 .. 23 visible), random_occlu_idx reads it -- and torch.cuda.get_rng_state() is unchanged by reset_done() + step()."""
    n = 64
    task, env = make_task(n, motion="synthetic:3:1", seed=6, **OCCL, **NOISE, **DEVICE)
    env.reset()
    J = task._occl_mask.shape[1]
    ref = ou.OcclState(n, J, prob=task._occl_training_prob, key=task._occl_key, env_offset=task._task_env_offset)
    ref["k"][:], ref["count"][...] = 0, 0
    assert (task._occl_k == 0).all() and (task.random_occlu_count == 0).all() and J == 24
    count_ptr = task.random_occlu_count.data_ptr()
    g = torch.Generator(device=task.device).manual_seed(7)
    for _ in range(3):
        a = _actions(task, g, 0.5)
        torch.cuda.synchronize()
        rng = torch.cuda.get_rng_state()
        task.reset_done()
        env.step(a)
        torch.cuda.synchronize()
        assert torch.equal(torch.cuda.get_rng_state(), rng)
        ref.run_host()
    assert np.array_equal(task.random_occlu_count.cpu().numpy(), ref["count"]) and np.array_equal(task._occl_k.cpu().numpy(), ref["k"]) and ref["count"].max() >= 29
    assert task.random_occlu_count.data_ptr() == count_ptr
    visible = (np.arange(J) >= 9) & (np.arange(J) < 24)
    assert np.array_equal(task._occl_mask.cpu().numpy(), np.broadcast_to(~visible, (n, J)).astype(np.uint8))
    assert np.array_equal(task.random_occlu_idx.cpu().numpy(), np.broadcast_to(~visible, (n, J))) and task.random_occlu_idx.dtype == torch.bool
    assert torch.isfinite(task.obs_buf).all() and torch.isfinite(task.rew_buf).all()


CAPTURE_CASES = {"noise": NOISE, "dropout": DROPOUT, "occl": OCCL, "noise+dropout": {**NOISE, **DROPOUT}, "noise+occl": {**NOISE, **OCCL}}


@pytest.mark.parametrize("switches", sorted(CAPTURE_CASES))
@pytest.mark.parametrize("name", ("HumanoidIm", "HumanoidImMCPGetup"))
def test_capturability_follows_the_option(name, switches):
    """Each of the three switches alone, and together as far as the task admits them (occl_training excludes fut_tracks: noise + dropout, noise + occlusion), on
    HumanoidIm and on HumanoidImMCPGetup (env_im_getup_mcp; its zero_out_far excludes fut_tracks, so the dropout cases switch that off): capturable with
    `+env.task_rng=device`, not without.  The first half fails on the commit before phc_obs_augment / phc_occl_advance."""
    over = dict(CAPTURE_CASES[switches], **(MCP_GETUP if name == "HumanoidImMCPGetup" else {}))
    if name == "HumanoidImMCPGetup" and "dropout" in switches:
        over["env.zero_out_far"] = False
    for device in (True, False):
        task, _ = make_task(64, motion="synthetic:2:1", **over, **(DEVICE if device else {}))
        assert type(task).__name__ == name and task.task_rng == ("device" if device else "torch")
        assert task.whole_step_capturable() is device, (name, switches, device)
        assert (task._obs_aug_k is not None) == (device and switches != "occl")
        assert (task._occl_k is not None) == (device and "occl" in switches)


# ---- graphs against eager ------------------------------------------------------------------------------------------------------------------------------
EPOCHS = 4


def _train(monkeypatch, eager):
    from phc_amd.learning.amp_agent import IMAmpAgent
    for sw in ("PHC_NO_ROLLOUT_GRAPH", "PHC_NO_STEP_GRAPH", "PHC_NO_GRAPH"):
        monkeypatch.delenv(sw, raising=False)
    if eager:
        monkeypatch.setenv("PHC_NO_ROLLOUT_GRAPH", "1")
    over = {"learning": "im", "learning.params.config.horizon_length": 4, "learning.params.config.minibatch_size": 256,
            "learning.params.config.amp_obs_demo_buffer_size": 512, "learning.params.config.amp_replay_buffer_size": 512, "+learning.params.config.hip_graph": True}
    task, env = make_task(64, motion="synthetic:2:1", seed=3, **NOISE, **DEVICE, **over)
    assert task.whole_step_capturable() and type(task).__name__ == "HumanoidIm"
    torch.manual_seed(5)
    agent = IMAmpAgent(env, task.cfg)
    torch.manual_seed(7)
    agent.init_train()
    agent.epoch_num = 1    # rollout graphs are admitted from epoch 2 on; the first rollout still runs without whole-step graphs (it creates the reward accumulator)
    seen = []
    for e in range(EPOCHS):
        if e == 3:
            torch.manual_seed(11)
            task.resample_motions()   # drops the graphs
        agent.train_epoch()
        torch.cuda.synchronize()
        out = {f"exp.{k}": v for k, v in agent.exp.items()}
        out.update(progress_buf=task.progress_buf, obs_k=task._obs_aug_k, reset_rng=task._reset_rng_dev, obs_buf=task.obs_buf)
        out.update({f"param.{k}": v for k, v in agent.model.state_dict().items()})
        seen.append({k: v.detach().clone() for k, v in out.items()})
    return seen, list(agent._roll_graphs)


def test_whole_step_graphs_equal_eager_rollouts_with_observation_noise(monkeypatch):
    """Plain HumanoidIm + learning=im with env.add_obs_noise=True and `+env.task_rng=device`, 64 envs, horizon 4, the policy's sampling noise replaced by zeros.
    Four epochs each: the first creates the reward accumulator, the second captures a whole-step graph per step, the third only replays, a resample_motions()
    drops the graphs and the fourth captures again.  After every epoch the experience buffers, the noise counters and every parameter are compared.  Bound: bit
    equality -- both regimes issue the same launches on the same inputs, and a replayed phc_obs_augment reads its counters from device memory.  The eager leg
    runs and is checked first: a failed capture can abort the process."""
    real_randn = torch.randn
    # the sampling noise of phc_policy_sample -- torch.randn((N, D), ...), the one call with a shape tuple -- is zeros: the draw is the one thing a capture may
    # number differently
    monkeypatch.setattr(torch, "randn", lambda *size, **kw: torch.zeros(*size, **kw) if len(size) == 1 and isinstance(size[0], tuple) else real_randn(*size, **kw))
    ref, keys = _train(monkeypatch, eager=True)
    assert {k[0] for k in keys} == set(), keys
    dones = sum(int(r["exp.dones"].sum()) for r in ref)
    print(f"eager: episode ends over {EPOCHS} epochs: {dones}; noise draws {int(ref[-1]['obs_k'].sum())}")
    assert int(ref[-1]["obs_k"].min()) >= EPOCHS * 4 and all(torch.isfinite(v).all() for k, v in ref[-1].items() if k.startswith("param.") and v.is_floating_point())
    got, keys = _train(monkeypatch, eager=False)
    assert {k[1] for k in keys if k[0] == "step"} == set(range(4)), keys
    worst = {}
    for e, (a, b) in enumerate(zip(got, ref)):
        for k in b:
            if not torch.equal(a[k], b[k]):
                worst[(e, k)] = float((a[k].double() - b[k].double()).abs().max())
    print("differences from the eager run:", worst or "none")
    assert not worst, worst


# ---- checkpoints ---------------------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_of_the_counters(capsys):
    """The noise counters, the occlusion counters and random_occlu_count travel in get_env_rng_state() / set_env_rng_state(); a task with another env count
    starts afresh, and so does a checkpoint written without them."""
    n = 64
    task, env = make_task(n, motion="synthetic:3:1", seed=8, **OCCL, **NOISE, **DEVICE)
    env.reset()
    g = torch.Generator(device=task.device).manual_seed(9)
    for _ in range(3):
        task.reset_done()
        env.step(_actions(task, g, 0.5))
    state = task.get_env_rng_state()
    saved = state["task_rng"]
    assert torch.equal(saved["obs_k"], task._obs_aug_k.cpu()) and torch.equal(saved["occl_k"], task._occl_k.cpu()) and int(saved["occl_k"].min()) == 3
    assert torch.equal(saved["occl_count"], task.random_occlu_count.cpu()) and int(saved["occl_count"].max()) >= 27 and int(saved["obs_k"].min()) >= 5
    twin, _ = make_task(n, motion="synthetic:3:1", seed=8, **OCCL, **NOISE, **DEVICE)
    assert (twin._obs_aug_k == 0).all()
    twin.set_env_rng_state(state)
    assert torch.equal(twin._obs_aug_k, task._obs_aug_k) and torch.equal(twin._occl_k, task._occl_k) and torch.equal(twin.random_occlu_count, task.random_occlu_count)
    other, _ = make_task(32, motion="synthetic:3:1", seed=8, **OCCL, **NOISE, **DEVICE)
    other.set_env_rng_state(state)
    assert (other._obs_aug_k == 0).all() and (other._occl_k == 0).all() and (other.random_occlu_count == 0).all()
    assert "start afresh" in capsys.readouterr().out
    old = dict(state, task_rng={"draw_k": saved["draw_k"]})   # a checkpoint from before these counters
    twin._obs_aug_k.fill_(7)
    twin.set_env_rng_state(old)
    assert "start afresh" in capsys.readouterr().out and (twin._obs_aug_k == 7).all()


# ---- the default path ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over", [{**NOISE, **OCCL}, {**NOISE, **DROPOUT}], ids=["noise+occl", "noise+dropout"])
def test_default_path_steps_bit_identically_and_issues_no_new_launch(over):
    """Two torch-mode tasks with the options on, same seeds: 8 reset_done() + step() leave bit-equal buffers, neither new entry point is called (each is
    replaced by a function that fails the test), and neither counter exists."""
    n = 64
    runs = []
    for _ in range(2):
        task, env = make_task(n, motion="synthetic:3:1", seed=6, **over)
        assert task.task_rng == "torch" and not task.whole_step_capturable() and task._obs_aug_k is None and task._occl_k is None and task._aug_streams == {}

        class Guard:
            def __init__(self, lib):
                self._lib = lib

            def __getattr__(self, name):
                assert name not in ("phc_obs_augment", "phc_occl_advance"), name
                return getattr(self._lib, name)
        task._lib = Guard(task._lib)
        torch.manual_seed(8)
        env.reset()
        for _ in range(8):
            task.reset_done()
            env.step((torch.rand(n, 69, device=task.device) - 0.5) * 2.0)
        torch.cuda.synchronize()
        out = dict(obs=task.obs_buf.clone(), rew=task.rew_buf.clone(), root=task._root_states.clone(), progress=task.progress_buf.clone())
        if task._occl_training:
            out.update(count=task.random_occlu_count.clone(), mask=task._occl_mask.clone())
        runs.append(out)
    assert all(torch.equal(runs[0][k], runs[1][k]) for k in runs[0]), [k for k in runs[0] if not torch.equal(runs[0][k], runs[1][k])]
