"""Recording the simulated motion (phc_amd/motion_record.py, csrc/phc_record.h / .hip): everything that runs without a GPU.

  1. the row rule and the counters: the host build (tests/record_shim.cpp) against a numpy statement, exactly
  2. the row contents on constructed states of the three model families; `body_quat` of the state dump against the reference's own exp_map_to_quat
  3. the bindings: struct size, the width, the argument check through the shim and through the library
  4. the torch statement of the rule against the host build
  5. the export: keys, shapes, trimming, fps, and the motion libraries take the dict back
  6. the refusals
  7. the stand-alone sanitizer program (tests/record_asan_main.cpp)"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import record_util as ru
from phc_amd import _lib as L
import host_build

F = np.float32


def call(fam, src, st, cap, flags=0, limit=None):
    a = ru.args_of(fam, src, st, cap, flags, limit)
    m = ru.host_model(fam)
    assert ru.shim().motion_record_check_of(C.byref(m), C.byref(a)) == 0
    ru.shim().motion_record_host_of(C.byref(m), C.byref(a))


# ---- 1. the row rule -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("cap", [1, 2, 5])
def test_row_rule_and_counters(N, cap):
    """Every flag set x both segment modes x limit null / per-env, `cap + 2` calls each (the last ones overflow), a seed call in front: counters, headers and
    the place of every row equal the numpy statement; the guard elements behind every array stay."""
    fam = ru.family("smpl")
    W = ru.width(fam)
    for fi, flag_set in enumerate(ru.FLAG_SETS):
        for one in (0, ru.ONE):
            for with_limit in (False, True):
                limit = ((np.arange(N) % (cap + 2)).astype(np.int32)) if with_limit else None      # 0 (never a row) .. cap + 1 (cap binds)
                st, gw = ru.make_block(N, cap, W)
                wholes = list(gw)
                for c in range(cap + 3):
                    src, sw = ru.make_sources(fam, N, seed=100 * fi + c, flag_set=flag_set)
                    flags = one | (ru.SEED if c == 0 else 0)
                    before = ru.snapshot(st)
                    call(fam, src, st, cap, flags, limit)
                    ru.check_call(fam, src, before, st, cap, flags, limit)
                    assert ru.guards_intact(wholes + sw)
                if flag_set == "none":
                    room = np.full(N, cap) if limit is None else np.minimum(limit, cap)
                    assert np.array_equal(st["len"], room) and np.array_equal(st["dropped"], cap + 3 - room) and not st["closed"].any() and not st["seg"].any()


def test_every_env_overflows():
    """cap 2, six calls, no flag: every env refuses four frames, `dropped` counts each of them, rows 0 and 1 keep what the first two calls wrote."""
    fam = ru.family("smpl")
    N, cap, W = 65, 2, ru.width(fam)
    st, wholes = ru.make_block(N, cap, W)
    kept = None
    for c in range(6):
        src, sw = ru.make_sources(fam, N, seed=c, flag_set="none")
        call(fam, src, st, cap)
        if c == 1:
            kept = st["frames"].copy()
        assert ru.guards_intact(wholes + sw)
    assert (st["len"] == 2).all() and (st["dropped"] == 4).all() and st["frames"].tobytes() == kept.tobytes()


# ---- 2. the row contents ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nb,ne,nd", [("smpl", 24, 0, 69), ("h1", 20, 3, 19), ("g1", 38, None, 37)])
@pytest.mark.parametrize("ref", [0, ru.REF])
def test_row_contents(name, nb, ne, nd, ref):
    """Copied fields bit-equal (the quaternions of both hemispheres as they are), the root's exp map and the robots' axis x angle rows within their bounds
    of the fp64 statement, extended bodies' rows zero; roots from tests/rotation_cases.py (angle near 0 and near pi, w < 0, |w| = 1 to rounding)."""
    fam = ru.family(name)
    assert (fam["NB"], fam["D"]) == (nb, nd) and (ne is None or fam["E"] == ne) and fam["E"] >= (0 if name == "smpl" else 1)
    assert ru.shim().record_group_of(fam["NB"], fam["E"]) == (64 if name == "g1" else 32)
    N, cap, W = 80, 2, ru.width(fam, ref)
    assert W == ru.shim().record_width_of(fam["NB"], fam["E"], fam["D"], ref) and (name != "smpl" or ref or W == 247)
    st, wholes = ru.make_block(N, cap, W)
    for c in range(2):
        src, sw = ru.make_sources(fam, N, seed=7 + c)
        assert (src["root_states"][:, 6] < 0).any() and (np.abs(src["root_states"][:, 6]) > 0.9999).any()
        before = ru.snapshot(st)
        call(fam, src, st, cap, ref)
        ru.check_call(fam, src, before, st, cap, ref)
        assert ru.guards_intact(wholes + sw)
    o = 3 + 4 * fam["NB"] + 3 * fam["NB"]
    assert fam["E"] == 0 or not st["frames"][:, :, o:o + 3 * fam["E"]].any()
    if name == "smpl":     # the joints' rows are dof_pos as it is
        aa = st["frames"][:, 1, 3 + 96:3 + 96 + 72]
        assert aa[:, 3:].tobytes() == np.ascontiguousarray(src["dof_state"][..., 0]).tobytes()


def test_state_dump_body_quat_is_the_references(golden):
    """`body_quat = [root, exp_map_to_quat(dof_pos)]` of the state dump against the reference's own torch_utils.exp_map_to_quat
    (tests/gen_golden_motion_record.py), at the bound test_quat_kat holds exp_map_to_quat to."""
    from phc_amd.motion_record import exp_map_to_quat
    g = golden("motion_record")
    np.testing.assert_allclose(exp_map_to_quat(g["dof_pos"].reshape(len(g["dof_pos"]), -1, 3)), g["body_quat"][:, 1:], atol=2e-6, rtol=0)
    assert g["body_quat"][:, 0].tobytes() == g["root_quat"].tobytes()


# ---- 3. the bindings -------------------------------------------------------------------------------------------------------------------------------------
def test_struct_and_argument_check():
    fam = ru.family("smpl")
    assert C.sizeof(L.MotionRecordArgs) == ru.shim().record_sizeof_args() == 8 * 4 + 16 * C.sizeof(C.c_void_p)
    lib = L.load()
    assert lib.phc_motion_record(None, None, None) == -1 and lib.phc_motion_record_width(24, 0, 69, 0) == 247 and lib.phc_motion_record_width(24, 0, 69, 1) == 319
    assert lib.phc_motion_record_width(60, 5, 59, 0) == -2 and lib.phc_motion_record_width(0, 0, 69, 0) == -1
    src, _ = ru.make_sources(fam, 4, seed=0)
    st, _ = ru.make_block(4, 2, ru.width(fam))
    m = ru.host_model(fam)
    check = lambda a, model=m: ru.shim().motion_record_check_of(C.byref(model) if model is not None else None, C.byref(a) if a is not None else None)
    assert check(ru.args_of(fam, src, st, 2)) == 0 and check(None) == -1 and check(ru.args_of(fam, src, st, 2), None) == -1
    for name, _ in L.MotionRecordArgs._fields_[8:]:
        a = ru.args_of(fam, src, st, 2, ru.REF if name == "ref_body_pos" else 0)
        if name == "ref_body_pos":
            a.width = ru.width(fam, ru.REF)
        setattr(a, name, None)
        assert check(a) == (0 if name == "limit" else -1), name
        if name != "limit":
            assert lib.phc_motion_record(C.byref(m), C.byref(a), None) == -1, name     # returns before any launch
    for field, bad, code in (("num_envs", 0, -1), ("num_envs", -3, -1), ("num_bodies", 0, -1), ("num_dof", 0, -1), ("cap", 0, -1), ("num_ext", -1, -1), ("width", 246, -1),
                             ("flags", 8, -1), ("dt", 0.0, -1), ("dt", float("nan"), -1), ("num_ext", 41, -2), ("num_bodies", 23, -1)):
        a = ru.args_of(fam, src, st, 2)
        setattr(a, field, bad)
        assert check(a) == code, (field, bad)
        assert lib.phc_motion_record(C.byref(m), C.byref(a), None) == code, (field, bad)     # returns before any launch
    empty = L.Model()
    assert check(ru.args_of(fam, src, st, 2), empty) == -1


# ---- 4. the torch statement ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smpl", "h1"])
def test_torch_statement_equals_the_host_build(name):
    from phc_amd import motion_record as mr
    fam = ru.family(name)
    N, cap, W = 9, 3, ru.width(fam, ru.REF)
    limit = np.array([3, 1, 0, 2, 3, 9, 3, 3, 2], np.int32)
    st, _ = ru.make_block(N, cap, W)
    st["frames"][:] = 0
    st["header"][:] = 0
    ts = {k: torch.from_numpy(v.copy()) for k, v in st.items()}
    ts["limit"] = torch.from_numpy(limit)
    tables = (torch.from_numpy(fam["jt"].astype(np.int64)), torch.from_numpy(fam["ds"].astype(np.int64)), torch.from_numpy(fam["axis"]))
    for one in (0, ru.ONE):
        for c in range(5):
            src, _ = ru.make_sources(fam, N, seed=40 + c)
            flags = ru.REF | one | (ru.SEED if c == 0 else 0)
            call(fam, src, st, cap, flags, limit)
            tsrc = {k: torch.from_numpy(v.copy()) for k, v in src.items()}
            mr.record_rows(mr.frame_rows(tsrc, tables, fam["E"], ru.DT, True), tsrc, ts, cap, seed=bool(flags & ru.SEED), one_segment=bool(one))
            for k in ("header", "len", "seg", "closed", "dropped"):
                assert np.array_equal(ts[k].numpy(), st[k]), (k, c)
            _, comp, tol = ru.rows_f64(fam, src, ru.REF)
            got, want = ts["frames"].numpy(), st["frames"]
            assert got[..., ~comp].tobytes() == want[..., ~comp].tobytes()
            assert (np.abs(got[..., comp].astype(np.float64) - want[..., comp]) <= 2 * tol[comp]).all()


# ---- 5. the export ---------------------------------------------------------------------------------------------------------------------------------------
def _host_task(name):
    from phc_amd.config import compose
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    t = HumanoidIm.host_only(compose(["env.num_envs=2", *ru.OVER[name]]))
    t.device = "cpu"
    return t


def _hand_made(name, monkeypatch):
    """A recorder over hand-made blocks: play segments of length 1, 2 and cap, then a sweep batch with a failed clip and a duplicate."""
    from phc_amd import motion_record as mr
    monkeypatch.setattr(mr, "BACKEND", "torch")
    t = _host_task(name)
    rec = mr.MotionRecorder(t, ref=True)
    fam, cap = ru.family(name), 4
    W = ru.width(fam, ru.REF)
    assert rec.W == W
    rng = np.random.default_rng(3)

    def block(lens, segs_of, flags_of):
        N = len(lens)
        fr = rng.standard_normal((N, cap, W)).astype(F)
        q = fr[:, :, 3:3 + 4 * fam["NB"]].reshape(N, cap, fam["NB"], 4)
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        hd = np.zeros((N, cap, 4), np.int32)
        for i in range(N):
            hd[i, :, 0], hd[i, :, 3] = segs_of[i], flags_of[i]
        return dict(frames=torch.from_numpy(fr), header=torch.from_numpy(hd), len=torch.tensor(lens, dtype=torch.int32), seg=torch.zeros(N, dtype=torch.int32),
                    closed=torch.zeros(N, dtype=torch.int32), dropped=torch.tensor([0] * (N - 1) + [2], dtype=torch.int32))
    return rec, block, cap, fam


@pytest.mark.parametrize("name", ["smpl", "h1"])
def test_export_play_segments(name, monkeypatch, tmp_path):
    import joblib
    rec, block, cap, fam = _hand_made(name, monkeypatch)
    rec._state, rec._one_segment, rec._open_segments, rec._cap, rec._held = block([4, 4], [[0, 1, 1, 2], [0, 0, 0, 0]], [[1, 0, 1, 0], [0, 0, 0, 0]]), False, {}, cap, cap
    first = rec._state["frames"].numpy().copy()
    rec.flush()
    rec._state.update(block([1, 0], [[2, 0, 0, 0], [0, 0, 0, 0]], [[1, 0, 0, 0], [0, 0, 0, 0]]))      # segment 2 of env 0 goes on across the flush
    out = rec.close()
    assert out == {"record_dropped": 4, "record_clips": 4}
    path, spath = rec.export(str(tmp_path / "out" / "motion.pkl"), log=None)
    lib, states = joblib.load(path), joblib.load(spath)
    assert spath.endswith("motion_states.pkl") and list(lib) == ["0_0", "0_1", "0_2", "1_0"] == list(states)
    NB, E, D = fam["NB"], fam["E"], fam["D"]
    assert [len(c["root_trans_offset"]) for c in lib.values()] == [1, 2, 2, 4] and [s["frames"] for s in states.values()] == [1, 2, 2, 4]
    assert [s["failed"] for s in states.values()] == [True, True, True, False]
    fps = int(round(1 / rec.task.dt))      # 30 for the SMPL task, 50 for the robots'
    assert fps == (30 if name == "smpl" else 50)
    for c in lib.values():
        T = len(c["root_trans_offset"])
        assert c["fps"] == fps and c["root_trans_offset"].shape == (T, 3)
        if name == "smpl":
            assert sorted(c) == ["fps", "pose_aa", "pose_quat_global", "root_trans_offset"] and c["pose_quat_global"].shape == (T, NB, 4) and c["pose_aa"].shape == (T, 3 * NB)
        else:
            assert sorted(c) == ["dof", "fps", "pose_aa", "root_rot", "root_trans_offset"] and c["pose_aa"].shape == (T, NB + E, 3) and c["dof"].shape == (T, D) and c["root_rot"].shape == (T, 4)
    assert lib["1_0"]["root_trans_offset"].tobytes() == first[1, :, 0:3].tobytes()
    quat = first[0, 1:3, 3:3 + 4 * NB].reshape(2, NB, 4)
    assert (lib["0_1"]["pose_quat_global"] if name == "smpl" else lib["0_1"]["root_rot"]).tobytes() == (quat if name == "smpl" else quat[:, 0]).tobytes()
    s = states["1_0"]
    assert s["root_states_seg"].shape == (4, 13) and s["dof_pos"].shape == (4, D) and s["ref_body_pos_full"].shape == (4, NB, 3) and s["motion_time"].shape == (4,)
    assert abs(s["fps"] - fps) < 1e-9 and s["skeleton_parents"].shape == (NB,) and s["skeleton_local_translation"].shape == (NB, 3)
    assert ("body_quat" in s) == (name == "smpl") and (name != "smpl" or s["body_quat"].shape == (4, NB, 4))
    # the motion libraries take the export back (the constructor and the clip reader: what runs without a device)
    from phc_amd.config import EasyDict
    from phc_amd.motion_lib import MotionLibReal, MotionLibSMPL
    t = rec.task
    cfg = EasyDict(dict(motion_file=lib, device="cpu", step_dt=t.dt))
    if name == "smpl":
        ml = MotionLibSMPL(cfg)
    else:
        cfg["robot"], cfg["robot_model"] = t.cfg["robot"], t.model
        ml = MotionLibReal(cfg)
    assert ml._num_unique_motions == 4 and list(ml._motion_data_keys) == list(lib)
    _, a, trans, clip_fps = ml._clip_payload(ml._motion_data_list[3], 0, -1, None)
    assert len(a) == len(trans) == 4 and clip_fps == fps


def test_export_sweep_trims_fails_and_drops_duplicates(monkeypatch, tmp_path):
    import joblib
    rec, block, cap, fam = _hand_made("smpl", monkeypatch)
    source = {"a": {"beta": np.arange(10.0), "gender": "neutral"}, "b": {}, "c": {"beta": np.ones(10)}}
    rec.task._motion_lib = types.SimpleNamespace(_motion_data_load=source)
    for keys, lens, flags in ((["a", "b"], [4, 2], [[0, 0, 0, 0], [0, 1, 0, 0]]), (["c", "a"], [1, 3], [[0] * 4, [0] * 4])):      # the second batch wraps: "a" again
        rec._state, rec._one_segment, rec._keys = block(lens, [[0] * 4] * 2, flags), True, keys
        rec.end_batch()
        assert rec._state is None
    assert [c["key"] for c in rec.clips] == ["a", "b", "c"] and [len(c["frames"]) for c in rec.clips] == [4, 2, 1] and [c["failed"] for c in rec.clips] == [False, True, False]
    assert rec.dropped == 4
    path, spath = rec.export(str(tmp_path / "sweep.pkl"), log=None)
    lib, states = joblib.load(path), joblib.load(spath)
    assert list(lib) == ["a", "b", "c"] and np.array_equal(lib["a"]["beta"], np.arange(10.0)) and lib["a"]["gender"] == "neutral" and "beta" not in lib["b"]
    assert [states[k]["failed"] for k in lib] == [False, True, False] and states["b"]["frames"] == 2


# ---- 6. the refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path):
    from phc_amd import motion_record as mr
    from phc_amd.config import compose
    from phc_amd.learning import im_eval
    from phc_amd.learning.amp_agent import IMAmpAgent
    cfg = compose(["env.num_envs=2", "+record.motion=" + str(tmp_path / "m.pkl")])
    assert mr.options(cfg) == dict(path=str(tmp_path / "m.pkl"), ref=False, max_frames=None) and mr.options(compose(["env.num_envs=2"])) is None
    agent = IMAmpAgent.__new__(IMAmpAgent)
    agent.task = types.SimpleNamespace(cfg=cfg)
    with pytest.raises(NotImplementedError, match="record.motion"):
        agent.train(1)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_frames"):
            mr.check_max_frames(bad)
    with pytest.raises(ValueError, match="max_frames"):
        mr.options(compose(["env.num_envs=2", "+record.motion=x.pkl", "+record.max_frames=0"]))
    dist = types.SimpleNamespace(is_initialized=lambda: True, get_world_size=lambda: 2, get_rank=lambda: 0)
    task = types.SimpleNamespace(cfg=cfg, collect_dataset=False, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="one process"):
        im_eval.evaluate(types.SimpleNamespace(task=task, dist=dist, config={}), log=None)
    # a device that is not a HIP device with the default backend: an error, not a fallback
    t = _host_task("smpl")
    with pytest.raises(RuntimeError, match="HIP device"):
        mr.MotionRecorder(t)
    assert not (tmp_path / "m.pkl").exists()


def test_without_the_switch_nothing_is_recorded(tmp_path):
    import test_distill_cpu as td
    import gen_golden_distill as gg
    from phc_amd.learning import im_eval
    agent, _ = td._scripted_agent(gg.make_script(), collect=False)
    im_eval.evaluate(agent, output_dir=str(tmp_path), log=None)
    assert agent.last_motion_record is None and agent.last_dataset is None


# ---- 7. the sanitizer program ----------------------------------------------------------------------------------------------------------------------------
def test_host_build_runs_clean_under_the_address_and_undefined_sanitizers():
    """tests/record_asan_main.cpp (its own main; nothing is loaded into Python): the overflow and N = 65 cases on heap arrays of exact size."""
    returncode, stdout, stderr = host_build.run_sanitized("record_asan_main.cpp")
    print(stdout[-2000:], stderr)
    assert returncode == 0 and stdout.strip().endswith("ok"), stdout + stderr
