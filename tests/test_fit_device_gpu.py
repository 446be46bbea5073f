"""The device retargeting fit on the GPU: phc_fit_iterate against the fp64 oracle at the bounds of tests/test_fit_device_cpu.py (the device's sin / cos / sqrt
differ from libm: no bit-equality with the host build, except for the integer bookkeeping), guard words, refusals through the entry itself, the bits under
placement, segmenting and chunking, `fit_clips(backend="device")` end to end, and a captured graph."""
import numpy as np
import pytest
import torch

import fit_util as U
import test_fit_device_cpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", T.NAMES)
def test_one_iteration_against_the_oracle(name):
    """The bounds of CPU tests 3 and 4 hold for the kernels: gradient 4 E + floor; update a few roundings from Adam on the device's own moments."""
    case = U.make_batch(name)
    st = U.zero_state(case)
    got, host = U.run(case, st, 1, device=DEV), U.run(case, st, 1)
    oracle = U.oracle_step(case, st)
    T.check_gradient(case, got, oracle, f"{name} device")
    T.check_regimes(case, got, oracle)
    assert np.array_equal(got["step"], host["step"]) and np.array_equal(got["step"], case["step"] + 1)
    np.testing.assert_allclose(got["loss"], host["loss"], rtol=1e-5)
    rng = np.random.RandomState(7)
    for k in ("dof", "root_rot", "root_off"):
        st[k + "_m"] = rng.normal(scale=0.01, size=st[k].shape).astype(np.float32)
        st[k + "_v"] = (rng.uniform(0.2, 2.0, size=st[k].shape) * 1e-4).astype(np.float32)
    T.check_update(case, st, U.run(case, st, 1, device=DEV), f"{name} device")


@pytest.mark.parametrize("name", ["unitree_h1", "unitree_g1"])
def test_ten_iterations_against_fit_clip_fp64(name):
    """The bound of CPU test 5; the step counter is exact, and the deviation from the host build is printed."""
    case = U.clip_case(name)
    got, host = U.run(case, U.zero_state(case), 10, device=DEV), U.run(case, U.zero_state(case), 10)
    assert got["step"].tolist() == [10] == host["step"].tolist()
    T.check_trajectory(name, got, f"{name} device")
    for k in ("dof", "root_rot", "root_off", "loss"):
        print(f"{name} device vs host build, {k}: max |difference| {np.abs(got[k].astype(np.float64) - host[k]).max():.3e}")
    batch = U.make_batch(name)
    got, host = U.run(batch, U.zero_state(batch), 10, device=DEV), U.run(batch, U.zero_state(batch), 10)
    assert np.array_equal(got["step"], host["step"]) and np.isfinite(got["loss"]).all() and np.isfinite(got["dof"]).all()


def test_scratch_size_is_exact_and_guards_hold():
    """`run` checks the guard words behind every state array and the scratch (all tests here go through it); the entry takes exactly
    phc_fit_scratch_bytes and refuses one byte less."""
    from phc_amd import _lib as L
    lib = L.load()
    for name in ("chain3", "unitree_g1"):
        case = U.make_batch(name)
        nb, ne, nd, M = U.dims(case["marr"])
        args, mem = U.place(case, U.zero_state(case), DEV, scratch_fill=0x7FC00000)
        assert args.scratch_bytes == lib.phc_fit_scratch_bytes(case["dof"].shape[0], len(case["start"]) - 1, nb + ne) == (mem["scratch"].numel() - U.GUARD_WORDS) * 4
        stream = torch.cuda.current_stream().cuda_stream
        args.scratch_bytes -= 1
        assert lib.phc_fit_iterate(args, 2, stream) == U.EINVAL
        args.scratch_bytes += 1
        assert lib.phc_fit_iterate(args, 2, stream) == 0
        got = U.collect(mem)
        assert got["step"].tolist() == (case["step"] + 2).tolist() and np.isfinite(got["dof"]).all()


ENTRY_REFUSALS = [r for r in T.REFUSALS if r[0] in ("null dof", "null scratch", "null clip_start_host", "iterations < 0", "num_bodies + num_ext > 64",
                                                    "more than 32 matched", "scratch one byte short", "clip_start: an empty clip", "clip_start: descending",
                                                    "clip_start: does not end at num_frames", "misaligned dof")]


@pytest.mark.parametrize("what,override,iterations,code", ENTRY_REFUSALS, ids=[r[0] for r in ENTRY_REFUSALS])
def test_entry_refuses_and_leaves_the_state(what, override, iterations, code):
    from phc_amd import _lib as L
    case = U.make_batch("chain3")
    st = {k: np.full_like(v, 7) for k, v in U.zero_state(case).items()}
    args, mem = U.place(case, st, DEV)
    keep = []
    for k, v in override.items():
        if callable(v):
            keep.append(T._starts(case, v))
            setattr(args, k, keep[-1].ctypes.data)
        elif k == "scratch_bytes":
            args.scratch_bytes += v
        elif k == "dof_offset":
            args.dof += v
        else:
            setattr(args, k, v)
    assert L.load().phc_fit_iterate(args, iterations, torch.cuda.current_stream().cuda_stream) == code
    torch.cuda.synchronize()
    got = U.collect(mem)
    for k in U.STATE:
        assert (got[k] == 7).all(), k


@pytest.mark.parametrize("name", ["chain3", "unitree_g1"])
def test_segmenting_and_placement_keep_the_bits_on_the_device(name):
    T.check_segmenting_and_placement(name, device=DEV)


def _library(name, lengths, seed=3):
    return {f"clip_{i:02d}": U.robot_clip_inputs(name, seed=seed + i, T=t) for i, t in enumerate(lengths)}


def test_fit_clips_chunks_keep_the_bits():
    from phc_amd.utils.fit_robot_motion import fit_clips
    rc, model = U.robot("unitree_h1")
    clips = _library("unitree_h1", (20, 45, 7, 33, 64, 1, 30))
    one = fit_clips(model, rc, clips, iterations=5, backend="device", device=DEV)
    logged = []
    many = fit_clips(model, rc, clips, iterations=5, backend="device", device=DEV, chunk_frames=64, log=logged.append)
    assert list(one) == list(many) == list(clips) and len(logged) >= 4          # (at least four chunks, one line each)
    for k in clips:
        for f in ("root_trans_offset", "pose_aa", "dof", "root_rot", "smpl_joints", "fit_loss", "fit_keypoint_error"):
            assert np.array_equal(np.asarray(one[k][f]), np.asarray(many[k][f])), (k, f)


@pytest.mark.parametrize("name", ["unitree_h1", "unitree_g1"])
def test_fit_clips_device_end_to_end(name):
    """The gates of tests/test_fit_robot_motion.py on the device fit, and the host fit's final error next to it."""
    from phc_amd.utils.fit_robot_motion import RobotFK, fit_clip, fit_clips
    rc, model = U.robot(name)
    ext = list(rc["extend_config"])
    clip = U.robot_clip_inputs(name)
    out = fit_clips(model, rc, {"fit_00000": clip}, iterations=300, backend="device", device=DEV)["fit_00000"]
    torch.manual_seed(0)
    host = fit_clip(model, rc, *clip, iterations=300)
    print(f"{name}: fit_keypoint_error after 300 iterations: device {out['fit_keypoint_error'] * 1000:.3f} mm, host fit {host['fit_keypoint_error'] * 1000:.3f} mm")
    Tn = clip[0].shape[0]
    assert set(out) >= {"root_trans_offset", "pose_aa", "dof", "root_rot", "smpl_joints", "fps"}
    assert out["pose_aa"].shape == (Tn, model.num_bodies + len(ext), 3) and out["dof"].shape == (Tn, model.num_dof)
    assert out["fit_keypoint_error"] < 0.03, out["fit_keypoint_error"]
    lo, hi = model.dof_limits()
    assert (out["dof"] >= lo - 1e-6).all() and (out["dof"] <= hi + 1e-6).all()
    pos0, rot0 = RobotFK(model, ext)(torch.from_numpy(out["pose_aa"][:1]), torch.from_numpy(out["root_trans_offset"][:1]))
    z = pos0[0, model.contact_body, 2].numpy() + np.einsum("kj,kj->k", rot0[0].numpy()[model.contact_body][:, 2, :], model.contact_pos) - model.contact_radius
    assert abs(float(z.min())) < 1e-4
    from phc_amd.config import EasyDict
    from phc_amd.env.tasks.humanoid_im import SkeletonTree
    from phc_amd.motion_lib import FixHeightMode, MotionLibReal
    cfg = EasyDict({"motion_file": {"fit_00000": out}, "device": DEV, "fix_height": FixHeightMode.full_fix, "min_length": -1, "max_length": -1,
                    "im_eval": False, "multi_thread": False, "smpl_type": rc["humanoid_type"], "randomrize_heading": False, "step_dt": 1 / 50, "robot": rc,
                    "robot_model": model})
    lib = MotionLibReal(cfg)
    lib.load_motions(skeleton_trees=[SkeletonTree(model.body_names, model.parent, model.local_translation)] * 2, random_sample=False)
    assert lib._motion_num_frames.tolist() == [Tn, Tn]


def test_captured_graph_replays_the_iterations():
    """One phc_fit_iterate(iterations = 5) captured into a torch.cuda.graph (one stream, no parallel branches) and replayed twice = 10 eager iterations."""
    from phc_amd import _lib as L
    lib = L.load()
    case = U.make_batch("unitree_h1")
    st = U.zero_state(case)
    eager = U.run(case, st, 10, device=DEV)
    args, mem = U.place(case, st, DEV)
    first = {k: mem[k].clone() for k in U.STATE}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # (a warm-up outside the capture; the state is put back below)
        assert lib.phc_fit_iterate(args, 5, side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.phc_fit_iterate(args, 5, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for k in U.STATE:
        mem[k].copy_(first[k])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    got = U.collect(mem)
    for k in U.STATE:
        assert np.array_equal(got[k], eager[k]), k
