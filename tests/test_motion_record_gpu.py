"""-m gpu: phc_motion_record through the C ABI against the host build of csrc/phc_record.h (tests/record_shim.cpp), the launch against the torch statement on a
stepping task, and `+record.motion` end to end: the sweep, the round trip through the motion library, play.

Every device array is a view in front of (the block: also behind) sentinel elements; after each call they must be unchanged.  Tolerances are those of
tests/record_util.py (the CPU tests'): headers, counters and copied floats bit-equal; the root's exp map and the robots' axis x angle rows within their bounds
of the fp64 statement."""
import ctypes as C

import numpy as np
import pytest
import torch

import record_util as ru

pytestmark = pytest.mark.gpu
F = np.float32
SMALL = {"learning.params.config.minibatch_size": 64, "learning.params.config.amp_obs_demo_buffer_size": 512, "learning.params.config.amp_replay_buffer_size": 512}
# published body positions against FK of the joint state: the bound tests/test_env_gpu.py::test_body_state_is_fk_of_joint_state holds the stepper to
FK_ATOL = 1e-4


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel against the host build
@pytest.mark.parametrize("name", ["smpl", "h1", "g1"])
@pytest.mark.parametrize("N", [1, 5, 33, 65])
@pytest.mark.parametrize("offset", [0, 1])
def test_kernel_equals_the_host_build(name, N, offset):
    """cap 3, six calls: a seed call and a call in one-segment mode (the flagged envs close), the envs re-opened, four calls in segment mode (every env
    overflows); ref_body_pos on; `offset` 1 starts the block one float into its allocation (no row is 16-byte aligned the same way twice).  After every call the
    device block, headers and counters against the host build's: bit-equal but for the computed columns, which stay within the CPU test's bounds of the fp64
    statement.  SMPL / H1 take 32 lanes per env, G1 64; N = 33 and 65 put envs 7 / 8 in the second half / the next wavefront and the last env in a partly
    filled workgroup."""
    from phc_amd import _lib as L
    from phc_amd import abi
    fam = ru.family(name)
    cap, flags0 = 3, ru.REF
    W = ru.width(fam, flags0)
    assert ru.shim().record_group_of(fam["NB"], fam["E"]) == (64 if name == "g1" else 32)
    st, wholes = ru.make_block(N, cap, W, offset=offset)
    dev_wholes = [torch.from_numpy(w.copy()).cuda() for w in wholes]
    n = N * cap * W
    dst = dict(frames=dev_wholes[0][offset:offset + n].view(N, cap, W), header=dev_wholes[1][:N * cap * 4].view(N, cap, 4),
               **{k: dev_wholes[2 + i][:N] for i, k in enumerate(("len", "seg", "closed", "dropped"))})
    assert dst["frames"].data_ptr() % 16 == (4 * offset) % 16
    limit = (1 + np.arange(N) % 4).astype(np.int32)
    dlimit = torch.from_numpy(limit).cuda()
    ints, floats = torch.from_numpy(fam["ints"]).cuda(), torch.from_numpy(fam["floats"]).cuda()
    dm = ru.host_model(fam)
    dm.ints, dm.floats = ints.data_ptr(), floats.data_ptr()
    hm = ru.host_model(fam)
    comp, _ = ru.columns(fam, flags0)
    for c in range(6):
        if c == 2:      # re-open
            st["closed"][:] = 0
            dst["closed"].zero_()
        flags = flags0 | (ru.ONE if c < 2 else 0) | (ru.SEED if c == 0 else 0)
        src, _ = ru.make_sources(fam, N, seed=900 + c)
        sw = [torch.from_numpy(np.concatenate([v.reshape(-1), np.full(ru.GUARD, ru.sentinel(v.dtype), v.dtype)])).cuda() for v in src.values()]
        dsrc = {k: w[:v.size].view(v.shape) for (k, v), w in zip(src.items(), sw)}
        before = {k: v.cpu().numpy() for k, v in dst.items()}      # (the device's own rows: an earlier call's computed columns differ from the host build's)
        ha = ru.args_of(fam, src, st, cap, flags, limit)
        ru.shim().motion_record_host_of(C.byref(hm), C.byref(ha))
        da = abi.motion_record_args_struct(N, fam["NB"], fam["E"], fam["D"], cap, ru.DT, ref=True, seed=bool(flags & ru.SEED), one_segment=bool(flags & ru.ONE),
                                           limit=dlimit, **dsrc, **dst)
        assert L.load().phc_motion_record(C.byref(dm), C.byref(da), stream()) == 0
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in dst.items()}
        for k in ("header", "len", "seg", "closed", "dropped"):
            assert np.array_equal(got[k], st[k]), (k, c)
        assert got["frames"][..., ~comp].tobytes() == st["frames"][..., ~comp].tobytes(), c
        ru.check_call(fam, src, before, got, cap, flags, limit)
        for w, h in zip(dev_wholes, wholes):
            tail = w[-ru.GUARD:].cpu().numpy()
            assert (tail == ru.sentinel(h.dtype)).all()
        assert (dev_wholes[0][:offset].cpu().numpy() == ru.sentinel(F)).all()
        for w, v in zip(sw, src.values()):
            assert (w[-ru.GUARD:].cpu().numpy() == ru.sentinel(v.dtype)).all()
    assert (st["dropped"] > 0).all() and st["seg"].any()
    for e in sorted({0, min(7, N - 1), min(8, N - 1), N - 1}):      # placement in the batch
        assert got["frames"][e, :st["len"][e]][:, ~comp].tobytes() == st["frames"][e, :st["len"][e]][:, ~comp].tobytes()
        assert np.array_equal(got["header"][e, :st["len"][e]], st["header"][e, :st["len"][e]])


# ------------------------------------------------------------------------------------------------------------------ 2. the launch against the torch statement
def make_task(num_envs, motion="synthetic:3:1", seed=0, **over):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(seed)
    return parse_task(compose([f"env.num_envs={num_envs}", f"env.motion_file={motion}"] + [f"{k}={v}" for k, v in over.items()]))


def _same_clips(a, b, fam, ref):
    comp, tol = ru.columns(fam, ru.REF if ref else 0)
    assert [c["key"] for c in a.clips] == [c["key"] for c in b.clips] and a.dropped == b.dropped
    for x, y in zip(a.clips, b.clips):
        assert np.array_equal(x["header"], y["header"]), x["key"]
        assert x["frames"][:, ~comp].tobytes() == y["frames"][:, ~comp].tobytes(), x["key"]
        assert (np.abs(x["frames"][:, comp].astype(np.float64) - y["frames"][:, comp]) <= 2 * tol[comp]).all(), x["key"]


def test_launch_equals_the_torch_statement_on_a_stepping_task(monkeypatch):
    """8 envs of synthetic:3:1, 6 steps with random actions, two recorders on the same task -- the launch and `BACKEND = "torch"` --, cap 4 (one flush on the
    way), ref_body_pos on: the same segments, headers and copied floats; computed floats within twice the bound (two fp32 evaluations)."""
    from phc_amd import motion_record as mr
    task, env = make_task(8, "synthetic:3:1", **{"env.episode_length": 4})
    env.reset()
    a = mr.MotionRecorder(task, max_frames=4, ref=True)
    monkeypatch.setattr(mr, "BACKEND", "torch")
    b = mr.MotionRecorder(task, max_frames=4, ref=True)
    assert a._launch and not b._launch
    a.begin_play()
    b.begin_play()
    fired = 0
    for _ in range(6):
        env.step((torch.rand(8, 69, device=task.device) * 2 - 1) * 0.3)
        a.record()
        b.record()
        ids = task.reset_buf.nonzero().flatten()
        fired += len(ids)
        if len(ids):
            env.reset(ids)
    ra, rb = a.close(), b.close()
    assert ra == rb and fired > 0 and ra["record_clips"] > 8 and ra["record_dropped"] == 0 and sum(len(c["frames"]) for c in a.clips) == 8 * 7
    _same_clips(a, b, ru.family("smpl"), True)
    rows = np.concatenate([c["frames"] for c in a.clips])
    assert np.isfinite(rows).all()


# ------------------------------------------------------------------------------------------------------------------ 3. the sweep, end to end
_sweeps = {}


def _sweep(mode, record, collect=False, tmp=None):
    """One evaluation sweep of an untrained agent: 2 envs, synthetic:3:1 (two batches, the second one wrapping); computed once per setting.  Per batch the
    reference state at time 0 right after the reset, every step's body positions and terminate flags are kept."""
    key = (mode, record, collect)
    if key in _sweeps:
        return _sweeps[key]
    import joblib
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    from phc_amd.learning.amp_agent import IMAmpAgent
    from phc_amd.utils.flags import flags
    over = dict(SMALL, **{"+learning.params.config.eval_metrics": mode, "learning.params.config.minibatch_size": 2})
    if collect:
        over["collect_dataset"] = True
    path = None
    if record:
        path = str(tmp / f"rec_{mode}_{int(collect)}.pkl")
        over.update({"+record.motion": path, "+record.ref": True})
    torch.manual_seed(0)
    task, env = parse_task(compose(["env.num_envs=2", "env.motion_file=synthetic:3:1"] + [f"{k}={v}" for k, v in over.items()]))
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    batches, real_reset, real_step = [], env.reset, env.step

    def reset(*a):      # (the sweep resets once per batch)
        out = real_reset(*a)
        lib = task._motion_lib
        ref0 = lib.get_motion_state(task._sampled_motion_ids, torch.zeros(2, device=task.device), task._global_offset)
        batches.append(dict(keys=[str(k) for k in lib.curr_motion_keys], num_steps=lib.get_motion_num_steps().cpu().numpy().copy(),
                            ref_pos=ref0["rg_pos"].cpu().numpy(), ref_rot=ref0["rb_rot"].cpu().numpy(), pos=[task._rigid_body_pos.cpu().numpy().copy()], root=[task._root_states[:, 0:3].cpu().numpy().copy()], term=[]))
        return out

    def step(actions):
        out = real_step(actions)
        batches[-1]["pos"].append(task._rigid_body_pos.cpu().numpy().copy())
        batches[-1]["root"].append(task._root_states[:, 0:3].cpu().numpy().copy())
        batches[-1]["term"].append(task._terminate_buf.cpu().numpy().copy())
        return out
    env.reset, env.step = reset, step
    saved = (flags.test, flags.im_eval)
    try:
        torch.manual_seed(2)
        info, failed = agent.eval(log=None)
    finally:
        env.reset, env.step = real_reset, real_step
        flags.test, flags.im_eval = saved
    torch.cuda.synchronize()
    out = dict(info=info, failed=[str(k) for k in failed], batches=batches, task=task, rec=agent.last_motion_record, dataset=agent.last_dataset,
               sim={k: getattr(task, k).cpu().numpy().copy() for k in ("_root_states", "_dof_state", "_rigid_body_state")},
               lib=joblib.load(path) if record else None, states=joblib.load(path.replace(".pkl", "_states.pkl")) if record else None)
    _sweeps[key] = out
    return out


@pytest.fixture(scope="module")
def sweep_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("motion_record")


@pytest.mark.parametrize("mode", ["host", "device"])
def test_sweep_end_to_end(mode, sweep_dir):
    """Three clips, two batches of two envs (the second wraps).  The export holds each clip once, under the source clip's key; frame 0 is the library's frame at
    time 0 (rotations up to sign, root translation); a clip that fails ends at its terminating frame; eval dict and simulation tensors are bit-identical with
    and without the switch, and with `collect_dataset=True` beside it."""
    plain, rec = _sweep(mode, False), _sweep(mode, True, tmp=sweep_dir)
    assert plain["rec"] is None and plain["lib"] is None
    assert set(plain["info"]) == set(rec["info"]) and plain["failed"] == rec["failed"]
    for k, v in plain["info"].items():
        assert (np.isnan(v) and np.isnan(rec["info"][k])) or v == rec["info"][k], k
    for k, v in plain["sim"].items():
        assert v.tobytes() == rec["sim"][k].tobytes(), k
    assert len(plain["batches"]) == len(rec["batches"]) == 2
    for bp, br in zip(plain["batches"], rec["batches"]):
        assert len(bp["pos"]) == len(br["pos"]) and all(x.tobytes() == y.tobytes() for x, y in zip(bp["pos"], br["pos"]))
    lib, states, task = rec["lib"], rec["states"], rec["task"]
    keys = rec["batches"][0]["keys"] + rec["batches"][1]["keys"][:1]
    assert rec["batches"][1]["keys"][1] == keys[0] and list(lib) == keys == list(states) and len(set(keys)) == 3
    for n, key in enumerate(keys):
        b, i = rec["batches"][n // 2], n % 2
        clip, s = lib[key], states[key]
        T = len(clip["root_trans_offset"])
        source = task._motion_train_lib._motion_data_load[key]
        copied = [k for k in ("beta", "gender") if k in source]
        assert sorted(clip) == sorted(["fps", "pose_aa", "pose_quat_global", "root_trans_offset"] + copied) and clip["fps"] == 30
        assert all(np.array_equal(clip[k], source[k]) for k in copied)
        assert clip["pose_quat_global"].shape == (T, 24, 4) and clip["pose_aa"].shape == (T, 72) and s["frames"] == T and s["ref_body_pos_full"].shape == (T, 24, 3)
        np.testing.assert_allclose(clip["root_trans_offset"][0], b["ref_pos"][i, 0], rtol=0, atol=1e-5)
        unit = lambda q: q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=-1, keepdims=True)     # (neither side is unit to better than ~1e-4)
        dots = np.abs((unit(clip["pose_quat_global"][0]) * unit(b["ref_rot"][i])).sum(-1))
        print(f"{key}: frame 0 against the library at time 0: 1 - |q . q_ref| <= {float((1 - dots).max()):.3e}, quaternion norms within "
              f"{float(np.abs(np.linalg.norm(clip['pose_quat_global'][0], axis=-1) - 1).max()):.3e} / {float(np.abs(np.linalg.norm(b['ref_rot'][i], axis=-1) - 1).max()):.3e} of 1")
        np.testing.assert_allclose(dots, 1, rtol=0, atol=1e-5)
        term = np.array([t[i] for t in b["term"]]) != 0
        steps = len(term)
        first = int(np.flatnonzero(term)[0]) if term.any() else None
        want = min(int(b["num_steps"][i]), steps + 1 if first is None else first + 2)
        assert T == want, (key, T, want)
        assert s["failed"] == (first is not None and first + 2 <= int(b["num_steps"][i])) and (not s["failed"] or key in rec["failed"])
        np.testing.assert_allclose(s["motion_time"], np.arange(T, dtype=F) * F(task.dt), rtol=0, atol=1e-6)
        # the recorded root is the simulated one, frame by frame
        sim_root = np.stack([b["root"][k][i] for k in range(T)])
        assert clip["root_trans_offset"].tobytes() == sim_root.tobytes()
    both = _sweep(mode, True, collect=True, tmp=sweep_dir)
    assert both["dataset"] is not None and len(both["dataset"].keys) == 4 and list(both["lib"]) == keys
    for key in keys:
        assert both["lib"][key]["pose_quat_global"].tobytes() == lib[key]["pose_quat_global"].tobytes(), key


def test_round_trip_through_the_motion_library(sweep_dir):
    """The export loaded with MotionLibSMPL on the task's skeletons: `get_motion_state` at the recorded frame times returns the simulated body positions of
    those steps within the bound test_body_state_is_fk_of_joint_state holds the stepper to (the FK is the library's, the rotations are fp32 copies)."""
    from phc_amd.config import EasyDict
    from phc_amd.motion_lib import MotionLibSMPL
    from phc_amd.utils.flags import flags
    rec = _sweep("device", True, tmp=sweep_dir)
    task, lib_dict = rec["task"], rec["lib"]
    keys = list(lib_dict)
    cfg = EasyDict(dict(task._motion_train_lib.m_cfg))
    cfg.motion_file, cfg.im_eval, cfg.randomrize_heading = lib_dict, False, False
    ml = MotionLibSMPL(cfg)
    saved = flags.test
    flags.test = True      # (no random heading, no crop)
    try:
        ml.load_motions(skeleton_trees=task.skeleton_trees[:1] * 3, gender_betas=task.humanoid_shapes.cpu()[:1].repeat(3, 1),
                        limb_weights=task.humanoid_limb_and_weights.cpu()[:1].repeat(3, 1), random_sample=False, start_idx=0)
    finally:
        flags.test = saved
    assert [str(k) for k in ml.curr_motion_keys] == keys
    worst = 0.0
    for n, key in enumerate(keys):
        b, i = rec["batches"][n // 2], n % 2
        T = len(lib_dict[key]["root_trans_offset"])
        times = torch.arange(T, device=task.device, dtype=torch.float32) / 30.0
        got = ml.get_motion_state(torch.full((T,), n, device=task.device, dtype=torch.long), times)["rg_pos"].cpu().numpy()
        sim = np.stack([b["pos"][k][i] for k in range(T)])
        err = np.abs(got - sim).max(axis=(1, 2))
        print(f"{key}: {T} frames, worst |library FK - simulated body position| {err.max():.3e} (reset frame {err[0]:.3e})")
        worst = max(worst, float(err.max()))
        np.testing.assert_allclose(got, sim, rtol=0, atol=FK_ATOL, err_msg=key)
    assert np.isfinite(worst)


def test_round_trip_robot():
    """H1 in play: 6 steps recorded, exported, loaded with MotionLibReal (fix_height=no_fix); the library's FK of the recorded pose_aa returns the simulated body
    positions within the same bound."""
    from phc_amd import motion_record as mr
    from phc_amd.config import EasyDict
    from phc_amd.motion_lib import FixHeightMode, MotionLibReal
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    task, env = parse_task(compose(list(ru.OVER["h1"]) + ["env.num_envs=3", "env.motion_file=synthetic:3:1", "env.enableEarlyTermination=False"]))
    env.reset()
    rec = mr.MotionRecorder(task)
    rec.begin_play()
    pos = [task._rigid_body_pos.cpu().numpy().copy()]
    for _ in range(6):
        env.step(torch.zeros(3, task.num_actions, device=task.device))
        rec.record()
        pos.append(task._rigid_body_pos.cpu().numpy().copy())
        assert not task.reset_buf.any()
    rec.close()
    lib_dict = rec.library()
    assert list(lib_dict) == ["0_0", "1_0", "2_0"] and all(len(c["dof"]) == 7 for c in lib_dict.values())
    cfg = EasyDict(dict(task._motion_train_lib.m_cfg))
    cfg.motion_file, cfg.fix_height, cfg.im_eval = lib_dict, FixHeightMode.no_fix, False
    ml = MotionLibReal(cfg)
    ml.load_motions(skeleton_trees=task.skeleton_trees[:3], gender_betas=task.humanoid_shapes.cpu()[:3], limb_weights=task.humanoid_limb_and_weights.cpu()[:3],
                    random_sample=False, start_idx=0)
    fps = float(lib_dict["0_0"]["fps"])
    for n in range(3):
        times = torch.arange(7, device=task.device, dtype=torch.float32) / fps
        got = ml.get_motion_state(torch.full((7,), n, device=task.device, dtype=torch.long), times)["rg_pos"].cpu().numpy()
        sim = np.stack([p[n] for p in pos])
        print(f"h1 env {n}: worst |library FK - simulated body position| {np.abs(got - sim).max():.3e}")
        np.testing.assert_allclose(got, sim, rtol=0, atol=FK_ATOL)


# ------------------------------------------------------------------------------------------------------------------ 4. play
def _play(backend, tmp, monkeypatch):
    import joblib
    from phc_amd import motion_record as mr
    from phc_amd import run
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    from phc_amd.learning.amp_agent import IMAmpAgent
    monkeypatch.setattr(mr, "BACKEND", backend)
    path = str(tmp / f"play_{backend}.pkl")
    over = dict(SMALL, **{"+record.motion": path, "+record.max_frames": 4, "env.episode_length": 4, "learning.params.config.minibatch_size": 3})
    torch.manual_seed(0)
    task, env = parse_task(compose(["env.num_envs=3", "env.motion_file=synthetic:3:1"] + [f"{k}={v}" for k, v in over.items()]))
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    resets, real_step = [], env.step

    def step(actions):
        out = real_step(actions)
        resets.append(task.reset_buf.cpu().numpy().copy() != 0)
        return out
    env.step = step
    torch.manual_seed(2)
    out = run.play(agent, task, env, steps=10)
    torch.cuda.synchronize()
    return out, np.array(resets), joblib.load(path), agent.last_motion_record


def test_play_mode(tmp_path, monkeypatch):
    """N = 3, cap 4, 10 steps: 11 frames per env (the reset state and one per step) in segments split where reset_buf fired; the segment count, the frames and
    `record_dropped` equal what the torch backend gives on a second, identically seeded run."""
    out, resets, lib, rec = _play(None, tmp_path, monkeypatch)
    out_t, resets_t, lib_t, rec_t = _play("torch", tmp_path, monkeypatch)
    assert np.array_equal(resets, resets_t) and resets.any() and resets.shape == (10, 3)
    assert out["record_dropped"] == out_t["record_dropped"] == 0 and out["record_clips"] == out_t["record_clips"] == len(lib)
    assert {k: v for k, v in out.items() if not k.startswith("record_")} == {k: v for k, v in out_t.items() if not k.startswith("record_")}
    want = {}
    for i in range(3):
        seg, n = 0, 1                      # frame 0: the reset state
        for s in range(10):
            n += 1                         # the frame of step s belongs to the segment it ends
            if resets[s, i]:
                want[f"{i}_{seg}"], seg, n = n, seg + 1, 0
        if n:
            want[f"{i}_{seg}"] = n
    assert {k: len(v["root_trans_offset"]) for k, v in lib.items()} == want and sum(want.values()) == 33
    _same_clips(rec, rec_t, ru.family("smpl"), False)
