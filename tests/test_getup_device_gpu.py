"""-m gpu: `+env.task_rng=device` -- phc_getup_assign / phc_task_draws against the host build of phc_getup.h, the masked resets against the listed ones, the
getup task in device mode, capturability, whole-step graphs against eager rollouts, and the untouched default path."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import getup_util as gu
from test_env_gpu import _pnn_checkpoint, make_task

pytestmark = pytest.mark.gpu

GETUP = {"env.task": "HumanoidImGetup", "env.recoveryEpisodeProb": 0.5, "env.recoverySteps": 8, "env.fallInitProb": 0.5}
MCP_GETUP = {"env": "env_im_getup_mcp", "learning": "im_mcp", "env.num_prim": 3}
DEVICE = {"+env.task_rng": "device"}


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
    """The backing buffers of a getup_util.GetupState on the device, guard words included."""

    def __init__(self, s):
        self.s = s
        self.t = {name: torch.from_numpy(b.copy()).cuda() for name, b in s.back.items()}

    def launch(self):
        from phc_amd import _lib as L
        a = self.s.args({name: t.data_ptr() for name, t in self.t.items()})
        rc = L.load().phc_getup_assign(a, _stream())
        torch.cuda.synchronize()
        return rc

    def fetch(self):
        """-> a GetupState holding what the device holds now."""
        out = self.s.clone()
        for name, t in self.t.items():
            out.back[name][...] = t.cpu().numpy()
        return out


# ---- C ABI against the host build --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", gu.SIZES)
def test_getup_assign_equals_the_host_build_bit_for_bit(n):
    """The CPU cases through the C ABI: every N x done set x three probability pairs x terminate patterns, drawn uniforms and the launch's own permutation;
    every array equal to the host build's byte for byte, guard words included."""
    for done, (prob, term) in itertools.product(gu.DONE_SETS, (((0.5, 0.5), "mixed"), ((0.0, 1.0), "zeros"), ((1.0, 0.0), "ones"), ((0.5, 1.0), "mixed"))):
        s = gu.GetupState(n, seed=n + 1, prob=prob, done=done, terminate=term)
        dev = DeviceCopy(s)
        assert dev.launch() == 0
        s.run_host()
        got = dev.fetch()
        assert got.guards_intact()
        gu.assert_equal_states(got, s, f"n={n} done={done} p={prob} terminate={term}: ")


@pytest.mark.parametrize("n,case", [(65, "tight"), (1025, "tight"), (65, "assign"), (65, "slot0"), (65, "demote")])
def test_getup_assign_edge_pools_equal_the_host_build(n, case):
    """The tight pool (F == n_f), assign entries outside [0, N), the slot-0 release and a pool that cannot serve its fallers: as the host build, guards intact."""
    s = gu.GetupState(n, seed=11, prob=(0.0, 1.0), holders=2.0 if case == "tight" else 0.5, done="alternate")
    if case == "assign":
        s["assign"][::2] = np.resize(np.array([-1, n, 1 << 40, -(1 << 40)]), len(s["assign"][::2]))
    elif case == "slot0":
        s["assign"][:], s["avail"][:] = 0, 0
        s["avail"][0], s["prob"][1] = 1, 0.0
    elif case == "demote":
        s["avail"][:], s["assign"][:] = 1, -1
    dev = DeviceCopy(s)
    assert dev.launch() == 0
    s.run_host()
    got = dev.fetch()
    assert got.guards_intact()
    gu.assert_equal_states(got, s, f"{case} n={n}: ")
    if case == "tight":
        assert (got["avail"] == 1).all() and len(set(got["assign"].tolist())) == n and (got["kind"][::2] == 3).all()
    if case == "slot0":
        assert got["avail"][0] == 0
    if case == "demote":
        assert (got["kind"][::2] == 1).all() and (got["fall_list"] == n).all()


def test_task_draws_equals_the_host_build():
    from phc_amd import _lib as L
    for n in (1, 65, 257, 1025):
        k = np.arange(n, dtype=np.int32)
        phase, offs = np.zeros(n + 16, np.float32), np.zeros(2 * n + 16, np.float32)
        phase[n:], offs[2 * n:] = 7.0, 7.0    # guard words
        kd, pd, od = (torch.from_numpy(x.copy()).cuda() for x in (k, phase, offs))
        for outs in ((pd, od), (None, od), (pd, None)):
            assert L.load().phc_task_draws(n, gu.KEY, 5, kd.data_ptr(), *(None if t is None else t.data_ptr() for t in outs), _stream()) == 0
            gu.shim().task_draws_host(n, gu.KEY, 5, k.ctypes.data, None if outs[0] is None else phase.ctypes.data, None if outs[1] is None else offs.ctypes.data)
        torch.cuda.synchronize()
        assert np.array_equal(kd.cpu().numpy(), k) and (k == np.arange(n) + 3).all()
        assert np.array_equal(pd.cpu().numpy(), phase) and np.array_equal(od.cpu().numpy(), offs) and (phase[n:] == 7).all() and (offs[2 * n:] == 7).all()


def test_a_second_launch_draws_anew_and_the_same_counters_give_the_same_bits():
    s = gu.GetupState(256, seed=13, prob=(0.5, 0.5), holders=0.3, done="all", terminate="ones")
    a, b = DeviceCopy(s), DeviceCopy(s)
    assert a.launch() == 0 and b.launch() == 0
    one, twin = a.fetch(), b.fetch()
    gu.assert_equal_states(one, twin, "same counters: ")
    # the same inputs again (flags, terminations, pool, states), only the counters moved on
    for name in ("reset_buf", "terminate_buf", "avail", "assign", "root_states", "dof_state", "recovery_counter"):
        a.t[name].copy_(torch.from_numpy(s.back[name]))
    assert a.launch() == 0
    two = a.fetch()
    assert (two["k"] == s["k"] + 2).all() and two["launch_count"][0] == s["launch_count"][0] + 2
    assert not np.array_equal(two["kind"], one["kind"])
    both = (one["kind"] == 3) & (two["kind"] == 3)
    assert both.sum() > 0 and not np.array_equal(two["assign"][both], one["assign"][both])
    # the permutation alone: same kinds (p_fall = 1), same free list, another launch count
    s2 = gu.GetupState(256, seed=13, prob=(0.0, 1.0), holders=0.0, done="all")
    c = DeviceCopy(s2)
    assert c.launch() == 0
    first = c.fetch()["assign"].copy()
    for name in ("avail", "assign"):
        c.t[name].copy_(torch.from_numpy(s2.back[name]))
    assert c.launch() == 0
    second = c.fetch()["assign"]
    assert np.array_equal(np.sort(first), np.arange(256)) and np.array_equal(np.sort(second), np.arange(256)) and not np.array_equal(first, second)


# ---- the task ----------------------------------------------------------------------------------------------------------------------------------------
def _state_tensors(task):
    t = {f"buf{i}": x for i, x in enumerate(task._buffer_tensors()) if x is not None}
    t.update(root=task._root_states, dof=task._dof_state, body=task._rigid_body_state, contact=task._contact_forces, dof_force=task.dof_force_tensor,
             pd_target=task._pd_target)
    return {k: v for k, v in t.items() if v is not None}


def test_masked_resets_equal_the_listed_ones():
    """128 envs of HumanoidImGetup after a few steps; kinds 0 .. 3 dealt at random, the FALL envs teleported to fall states.  Masked: refresh over the fall
    list, phc_im_reset_from_state_masked on `kind`, phc_im_reset_done (start at zero) on the NORMAL flags in place of reset_buf.  Listed, on a restored copy of
    the state: the existing phc_refresh_body_state_indexed + phc_im_reset_from_state (fill 1 / fill 0) + phc_im_reset with the id lists taken from `kind`.
    Every task and simulator buffer bit-equal; envs of kind 0 untouched."""
    from phc_amd import _lib as L
    n = 128
    task, env = make_task(n, motion="synthetic:3:2", seed=2, **GETUP)
    env.reset()
    for _ in range(5):
        env.step((torch.rand(n, 69, device=task.device) - 0.5) * 0.6)
    g = torch.Generator().manual_seed(4)
    kind = torch.randint(0, 4, (n,), generator=g).to(torch.int32)
    kind[-1], kind[0] = 3, 2
    ids = {k: torch.nonzero(kind == k).flatten().to(task.device) for k in (0, 1, 2, 3)}
    assert all(len(v) > 8 for v in ids.values())
    task._humanoid_root_states[ids[3]] = task._fall_root_states[ids[3]]
    task._dof_pos[ids[3]] = task._fall_dof_pos[ids[3]]
    task._dof_vel[ids[3]] = 0
    task._recovery_counter[:] = 5
    task.reset_buf[:] = (kind > 0).to(task.reset_buf.dtype)
    tensors = _state_tensors(task)
    saved = {k: v.clone() for k, v in tensors.items()}
    lib, s, kind_d = task._lib, _stream(), kind.to(task.device)
    fall_list = torch.full((n,), n, dtype=torch.long, device=task.device)
    fall_list[:len(ids[3])] = ids[3]
    normal = (kind_d == 1).to(torch.long)
    # masked
    L.check(lib.phc_refresh_body_state_masked(task._model_struct, task._sim_struct, fall_list.data_ptr(), s), "refresh masked")
    L.check(lib.phc_im_reset_from_state_masked(task._model_struct, task._motion_lib.struct, task._im_params, task._sim_struct,
                                               task._reset_prologue(from_state=True), kind_d.data_ptr(), s), "reset masked")
    buf = task._reset_prologue()
    keep, buf.reset_list, buf.reset_buf = buf.reset_buf, None, normal.data_ptr()
    L.check(lib.phc_im_reset_done(task._model_struct, task._motion_lib.struct, task._im_params, task._sim_struct, buf, 1, 1, 1, s), "reset done")
    buf.reset_buf = keep
    torch.cuda.synchronize()
    masked = {k: v.clone() for k, v in tensors.items()}
    for k, v in tensors.items():
        v.copy_(saved[k])
    # listed
    task._reset_from_state(ids[3], refresh=True, fill_history=True)
    task._reset_from_state(ids[2], refresh=False, fill_history=False)
    L.check(lib.phc_im_reset(task._model_struct, task._motion_lib.struct, task._im_params, task._sim_struct, task._reset_prologue(), len(ids[1]),
                             ids[1].contiguous().data_ptr(), None, 1, s), "reset listed")
    torch.cuda.synchronize()
    diff = [k for k, v in tensors.items() if not torch.equal(v, masked[k])]
    # (the listed phc_im_reset clears the reset flag of its envs, the masked sweep leaves it to the next post-physics launch: the flags of the NORMAL envs apart)
    flags_name = next(k for k, v in tensors.items() if v is task.reset_buf)
    if flags_name in diff:
        a, b = masked[flags_name], tensors[flags_name]
        assert torch.equal(a[ids[0]], b[ids[0]]) and torch.equal(a[ids[2]], b[ids[2]]) and torch.equal(a[ids[3]], b[ids[3]])
        diff.remove(flags_name)
    assert not diff, diff
    for k, v in masked.items():
        if v.shape[0] == n:
            assert torch.equal(v[ids[0]], saved[k][ids[0]]), k   # kind 0: untouched
    assert (masked[flags_name][ids[2]] == 0).all() and (task.progress_buf[kind_d > 0] == 0).all() and (task._recovery_counter[ids[1]] == 0).all()


def test_getup_task_in_device_mode():
    """64 envs, recoverySteps 8, probabilities 0.5, 24 steps of random actions.  After every reset_done(), against a host model of who holds which slot (a
    release frees the slot whoever holds it, as the rules say): held slots distinct, avail == the held set, FALL envs stand on their fall-state rows, RECOVERY
    envs kept their state, counters recoverySteps / 0; then the kinds follow update_getup_schedule exactly at p = 0 / 1."""
    n = 64
    task, env = make_task(n, motion="synthetic:3:2", seed=1, **GETUP, **DEVICE)
    assert task.task_rng == "device" and task.whole_step_capturable()
    env.reset()
    held = {int(s): int(i) for i, s in enumerate(task.fall_id_assignments.tolist()) if task._recovery_counter[i] > 0 and task.availalbe_fall_states[s] == 1}
    assert sorted(held) == torch.nonzero(task.availalbe_fall_states).flatten().tolist()
    seen = np.zeros(4, dtype=int)

    def reset_and_check(expect=None):
        before = {k: v.clone() for k, v in dict(root=task._root_states, dof=task._dof_state, assign=task.fall_id_assignments, done=task.reset_buf,
                                                term=task._terminate_buf).items()}
        task.reset_done()
        torch.cuda.synchronize()
        kind = task._getup_kind.cpu().numpy()
        assert np.array_equal(kind > 0, before["done"].cpu().numpy() != 0)
        assign, avail = task.fall_id_assignments.cpu().numpy(), task.availalbe_fall_states.cpu().numpy()
        for i in np.flatnonzero(kind > 0):
            held.pop(int(before["assign"][i]), None)
        for i in np.flatnonzero(kind == 3):
            assert int(assign[i]) not in held, "a slot was handed out twice"
            held[int(assign[i])] = int(i)
        assert np.array_equal(np.flatnonzero(avail), np.array(sorted(held), dtype=np.int64))
        fall, rec, normal = (torch.from_numpy(np.flatnonzero(kind == k)).to(task.device) for k in (3, 2, 1))
        pick = task.fall_id_assignments[fall]
        assert torch.equal(task._humanoid_root_states[fall], task._fall_root_states[pick]) and torch.equal(task._dof_pos[fall], task._fall_dof_pos[pick])
        assert (task._dof_vel[fall] == 0).all()
        assert torch.equal(task._root_states[rec], before["root"][rec]) and torch.equal(task._dof_state.view(n, -1)[rec], before["dof"].view(n, -1)[rec])
        rc = task._recovery_counter
        assert (rc[fall] == 8).all() and (rc[rec] == 8).all() and (rc[normal] == 0).all()
        assert (task.progress_buf[torch.from_numpy(kind > 0).to(task.device)] == 0).all()
        if expect is not None:
            want = expect(before["term"].cpu().numpy())
            sel = kind > 0
            assert np.array_equal(kind[sel], want[sel]), (kind[sel], want[sel])
        np.add.at(seen, kind, 1)
        return kind

    g = torch.Generator(device=task.device).manual_seed(3)
    act = lambda: (torch.rand(n, 69, device=task.device, generator=g) - 0.5) * 2.0
    for _ in range(16):
        reset_and_check()
        env.step(act())
    print("kinds over 16 steps at p = (0.5, 0.5) [not done, NORMAL, RECOVERY, FALL]:", seen)
    assert seen[1] > 0 and seen[2] > 0 and seen[3] > 0
    task.update_getup_schedule(1, getup_udpate_epoch=5)        # before the warm-up epoch: p = (0, 1) -- every done env falls
    for _ in range(4):
        reset_and_check(lambda term: np.full(n, 3))
        env.step(act())
    task._recovery_episode_prob_tgt, task._fall_init_prob_tgt = 1, 0   # past it, with targets (1, 0): RECOVERY where terminated, NORMAL otherwise
    task.update_getup_schedule(6, getup_udpate_epoch=5)
    assert task._recovery_episode_prob == 1 and task._fall_init_prob == 0 and task._getup_prob.tolist() == [1.0, 0.0]
    for _ in range(4):
        reset_and_check(lambda term: np.where(term == 1, 2, 1))
        env.step(act())
    assert torch.isfinite(task.obs_buf).all() and torch.isfinite(task.rew_buf).all()
    # reset(env_ids) keeps working (torch draws) and leaves the bookkeeping the launch reads consistent; the fall buffers stay where they are
    task._recovery_episode_prob_tgt, task._fall_init_prob_tgt = 0.5, 0.5
    task.update_getup_schedule(6, getup_udpate_epoch=5)
    ptrs = (task._fall_root_states.data_ptr(), task._fall_dof_pos.data_ptr(), task.availalbe_fall_states.data_ptr(), task._getup_prob.data_ptr())
    task.resample_motions()
    assert ptrs == (task._fall_root_states.data_ptr(), task._fall_dof_pos.data_ptr(), task.availalbe_fall_states.data_ptr(), task._getup_prob.data_ptr())
    avail, assign, rc = task.availalbe_fall_states.cpu().numpy(), task.fall_id_assignments.cpu().numpy(), task._recovery_counter.cpu().numpy()
    holders = np.flatnonzero(avail)   # (every held slot is the slot of an env in a FALL episode)
    assert 0 < len(holders) <= (rc > 0).sum() and set(holders.tolist()) <= set(assign[rc > 0].tolist())
    state = task.get_env_rng_state()
    assert state["task_rng"]["getup_count"] == int(task._getup_count.item()) == 24 and int(state["task_rng"]["getup_k"].sum()) == int(seen[1:].sum())


def test_capturability_follows_the_option():
    """env_im_getup_mcp + im_mcp (cycle_motion, zero_out_far, the getup reset, the composer's step): capturable with `+env.task_rng=device`, not without.  The
    same for plain HumanoidIm with cycle_motion, and for HumanoidImGetup alone."""
    for over, name in ((MCP_GETUP, "HumanoidImMCPGetup"), ({"env.cycle_motion": True}, "HumanoidIm"), (GETUP, "HumanoidImGetup")):
        for device in (False, True):
            task, _ = make_task(64, motion="synthetic:2:1", **over, **(DEVICE if device else {}))
            assert type(task).__name__ == name and task.task_rng == ("device" if device else "torch")
            assert task.whole_step_capturable() is device, (name, device)
    task, _ = make_task(64, motion="synthetic:2:1")
    assert task.whole_step_capturable() and task.task_rng == "torch"   # the default task: as before


def test_cycle_motion_draws_come_from_the_launch_in_device_mode():
    """HumanoidIm with cycle_motion: in device mode a step leaves phc_task_draws' numbers in `_cycle_phase` (the host build's, bit for bit) and does not touch
    torch's generator; in torch mode it advances it."""
    n = 64
    task, env = make_task(n, motion="synthetic:2:1", seed=4, **{"env.cycle_motion": True}, **DEVICE)
    env.reset()
    k0 = task._task_draw_k.cpu().numpy().copy()
    rng = torch.cuda.get_rng_state()
    task.reset_done()
    task.step(torch.zeros(n, 69, device=task.device))
    torch.cuda.synchronize()
    assert torch.equal(torch.cuda.get_rng_state(), rng)
    k, phase = k0.copy(), np.zeros(n, np.float32)
    gu.shim().task_draws_host(n, task._task_draw_key, task._task_env_offset, k.ctypes.data, phase.ctypes.data, None)
    assert np.array_equal(task._task_draw_k.cpu().numpy(), k) and np.array_equal(task._cycle_phase.cpu().numpy(), phase)
    twin, tenv = make_task(n, motion="synthetic:2:1", seed=4, **{"env.cycle_motion": True})
    tenv.reset()
    rng = torch.cuda.get_rng_state()
    twin.step(torch.zeros(n, 69, device=task.device))
    assert not torch.equal(torch.cuda.get_rng_state(), rng)


# ---- graphs against eager ----------------------------------------------------------------------------------------------------------------------------
EPOCHS = 4


def _train(monkeypatch, eager):
    from phc_amd.learning.amp_agent import IMAmpAgent
    for sw in ("PHC_NO_ROLLOUT_GRAPH", "PHC_NO_STEP_GRAPH", "PHC_NO_GRAPH"):
        monkeypatch.delenv(sw, raising=False)
    if eager:
        monkeypatch.setenv("PHC_NO_ROLLOUT_GRAPH", "1")
    over = {"learning.params.config.horizon_length": 4, "learning.params.config.minibatch_size": 256, "learning.params.config.amp_obs_demo_buffer_size": 512,
            "learning.params.config.amp_replay_buffer_size": 512, "+learning.params.config.hip_graph": True, "env.recoverySteps": 4}
    task, env = make_task(64, motion="synthetic:2:1", seed=3, **MCP_GETUP, **DEVICE, **over)
    assert task.whole_step_capturable()
    task.load_primitives(_pnn_checkpoint(task, 3)[0])
    torch.manual_seed(5)
    agent = IMAmpAgent(env, task.cfg)
    torch.manual_seed(7)
    agent.init_train()
    agent.epoch_num = 1    # rollout graphs are admitted from epoch 2 on; the first rollout still runs without whole-step graphs (it creates the reward accumulator)
    seen, kinds = [], np.zeros(4, dtype=int)
    for e in range(EPOCHS):
        if e == 3:
            torch.manual_seed(11)
            task.resample_motions()   # drops the graphs; the fall buffers keep their addresses
        agent.train_epoch()
        torch.cuda.synchronize()
        out = {f"exp.{k}": v for k, v in agent.exp.items()}
        out.update(progress_buf=task.progress_buf, recovery=task._recovery_counter, assign=task.fall_id_assignments, avail=task.availalbe_fall_states,
                   getup_k=task._getup_k, getup_count=task._getup_count, draw_k=task._task_draw_k, reset_rng=task._reset_rng_dev)
        out.update({f"param.{k}": v for k, v in agent.model.state_dict().items()})
        seen.append({k: v.detach().clone() for k, v in out.items()})
    return seen, list(agent._roll_graphs)


def test_whole_step_graphs_equal_eager_rollouts_on_the_getup_composer(monkeypatch):
    """env_im_getup_mcp + im_mcp with `+env.task_rng=device`, 64 envs, horizon 4, sampling noise replaced by zeros (as in tests/test_rollout_regimes_gpu.py;
    here only the sampling call's).
    Four epochs each: the first creates the reward accumulator, the second captures a whole-step graph per step, the third only replays, a
    resample_motions() drops the graphs and the fourth captures again.  After every epoch the experience buffers, the task's counters and slot bookkeeping
    and every parameter are compared.  Bound: bit equality -- both regimes issue the same launches on the same inputs.  The eager leg runs and is checked
    first: a failed capture can abort the process."""
    real_randn = torch.randn
    # the sampling noise of phc_policy_sample -- torch.randn((N, D), ...), the one call with a shape tuple -- is zeros: the draw is the one thing a capture may
    # number differently.  Every other torch.randn (the fall states' random orientations) stays
    monkeypatch.setattr(torch, "randn", lambda *size, **kw: torch.zeros(*size, **kw) if len(size) == 1 and isinstance(size[0], tuple) else real_randn(*size, **kw))
    ref, keys = _train(monkeypatch, eager=True)
    assert {k[0] for k in keys} == set(), keys
    dones = sum(int(r["exp.dones"].sum()) for r in ref)
    print(f"eager: episode ends over {EPOCHS} epochs: {dones}; getup launches {int(ref[-1]['getup_count'])}, draws {int(ref[-1]['getup_k'].sum())}")
    assert dones > 0 and int(ref[-1]["getup_k"].sum()) > 0, "no episode ended: the getup reset was not exercised"
    assert all(torch.isfinite(v).all() for k, v in ref[-1].items() if k.startswith("param.") and v.is_floating_point())
    got, keys = _train(monkeypatch, eager=False)
    assert {k[1] for k in keys if k[0] == "step"} == set(range(4)), keys
    worst = {}
    for e, (a, b) in enumerate(zip(got, ref)):
        for k in b:
            if not torch.equal(a[k], b[k]):
                worst[(e, k)] = float((a[k].double() - b[k].double()).abs().max())
    print("differences from the eager run:", worst or "none")
    assert not worst, worst


# ---- the default path --------------------------------------------------------------------------------------------------------------------------------
def test_default_path_steps_bit_identically_and_issues_no_new_launch(monkeypatch):
    """Two HumanoidImGetup tasks built without the option, same seeds: 12 reset_done() + step() leave bit-equal buffers, and none of the new entry points is
    called (each is replaced by a function that fails the test)."""
    n = 64
    tasks = []
    for _ in range(2):
        task, env = make_task(n, motion="synthetic:3:2", seed=6, **GETUP)
        assert task.task_rng == "torch" and not task.whole_step_capturable() and not hasattr(task, "_getup_kind") and task._task_draw_k is None

        class Guard:
            def __init__(self, lib):
                self._lib = lib

            def __getattr__(self, name):
                assert name not in ("phc_getup_assign", "phc_task_draws", "phc_im_reset_from_state_masked", "phc_refresh_body_state_masked"), name
                return getattr(self._lib, name)
        task._lib = Guard(task._lib)
        torch.manual_seed(8)
        env.reset()
        for _ in range(12):
            task.reset_done()
            env.step((torch.rand(n, 69, device=task.device) - 0.5) * 2.0)
        torch.cuda.synchronize()
        tasks.append({k: v.clone() for k, v in _state_tensors(task).items()})
        tasks[-1].update(avail=task.availalbe_fall_states.clone(), assign=task.fall_id_assignments.clone())
    assert all(torch.equal(tasks[0][k], tasks[1][k]) for k in tasks[0]), [k for k in tasks[0] if not torch.equal(tasks[0][k], tasks[1][k])]
    assert int(tasks[0]["avail"].sum()) > 0
