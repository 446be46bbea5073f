"""The spherical-joint keypoint fit on the GPU: phc_fit_sph_iterate against the fp64 oracle at the bounds of tests/test_fit_keypoints_cpu.py (the device's
sin / cos / sqrt differ from libm: no bit-equality with the host build, except for the integer bookkeeping), the exact regimes, guard words, refusals through
the entry itself, the bits under placement, segmenting and chunking, a captured graph, and `fit_keypoint_clips(backend="device")` end to end."""
import numpy as np
import pytest
import torch

import fit_sph_util as S
import test_fit_keypoints_cpu as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", S.NAMES)
def test_one_iteration_against_the_oracle(name):
    """The bounds of CPU tests 3 and 4 hold for the kernels: gradient 4 E + floor; update a few roundings from Adam on the device's own moments."""
    case = S.make_batch(name)
    st = S.zero_state(case)
    got, host = S.run(case, st, 1, device=DEV), S.run(case, st, 1)
    oracle = S.oracle_step(case, st)
    T.check_gradient(case, got, oracle, f"{name} device")
    T.check_regimes(case, got, oracle)
    assert np.array_equal(got["step"], host["step"]) and np.array_equal(got["step"], case["step"] + 1)
    np.testing.assert_allclose(got["loss"], host["loss"], rtol=1e-5)
    np.testing.assert_allclose(got["loss"], oracle["loss"], rtol=1e-5)
    st = T.fit_moments(st)
    T.check_update_and_clamp(case, st, S.run(case, st, 1, device=DEV), f"{name} device")


def test_unmatched_hands_stay_exactly_zero_on_the_device():
    T.check_hands_stay_zero(device=DEV)


@pytest.mark.parametrize("noise", T.NOISES)
def test_ten_iterations_against_the_host_fit_fp64(noise):
    """The bound of CPU test 5; the step counter is exact, and the deviation from the host build is printed."""
    case = S.clip_case(1.0, noise)
    got, host = S.run(case, S.zero_state(case), 10, device=DEV), S.run(case, S.zero_state(case), 10)
    assert got["step"].tolist() == [10] == host["step"].tolist()
    T.check_trajectory(got, f"device, noise {noise}", noise=noise)
    for k in ("dof", "root_rot", "root_off", "loss"):
        print(f"device vs host build, {k}: max |difference| {np.abs(got[k].astype(np.float64) - host[k]).max():.3e}")


def test_scratch_size_is_exact_and_guards_hold():
    """`run` checks the guard words behind every state array and the scratch (all tests here go through it); the entry takes exactly
    phc_fit_sph_scratch_bytes and refuses one byte less."""
    from phc_amd import _lib as L
    lib = L.load()
    for name in ("chain4s", "smpl24"):
        case = S.make_batch(name)
        nb, nd, M = S.dims(case["marr"])
        args, mem = S.place(case, S.zero_state(case), DEV, scratch_fill=0x7FC00000)
        assert args.scratch_bytes == lib.phc_fit_sph_scratch_bytes(case["dof"].shape[0], len(case["start"]) - 1, nb) == (mem["scratch"].numel() - S.GUARD_WORDS) * 4
        stream = torch.cuda.current_stream().cuda_stream
        args.scratch_bytes -= 1
        assert lib.phc_fit_sph_iterate(args, 2, stream) == S.EINVAL
        args.scratch_bytes += 1
        assert lib.phc_fit_sph_iterate(args, 2, stream) == 0
        got = S.collect(mem)
        assert got["step"].tolist() == (case["step"] + 2).tolist() and np.isfinite(got["dof"]).all()


ENTRY_REFUSALS = [r for r in T.REFUSALS if r[0] in ("null dof", "null scratch", "null clip_start_host", "iterations < 0", "33 bodies", "an extended body",
                                                    "33 matched", "scratch one byte short", "NaN lr", "clip_start: an empty clip",
                                                    "clip_start: does not end at num_frames", "misaligned dof")]


@pytest.mark.parametrize("what,override,iterations,code", ENTRY_REFUSALS, ids=[r[0] for r in ENTRY_REFUSALS])
def test_entry_refuses_and_leaves_the_state(what, override, iterations, code):
    from phc_amd import _lib as L
    case = S.make_batch("chain4s")
    st = {k: np.full_like(v, 7) for k, v in S.zero_state(case).items()}
    args, mem = S.place(case, st, DEV)
    stream = torch.cuda.current_stream().cuda_stream
    assert L.load().phc_fit_sph_iterate(args, 0, stream) == 0          # a no-op
    keep = []
    T.apply_override(case, args, override, keep)
    assert L.load().phc_fit_sph_iterate(args, iterations, stream) == code
    torch.cuda.synchronize()
    got = S.collect(mem)
    for k in S.STATE:
        assert (got[k] == 7).all(), k


@pytest.mark.parametrize("name", ["chain4s", "smpl24"])
def test_segmenting_and_placement_keep_the_bits_on_the_device(name):
    T.check_segmenting_and_placement(name, device=DEV)


def test_chunks_keep_the_bits():
    from phc_amd.utils.fit_keypoints import fit_keypoint_clips
    kp = S.walk_keypoints(2.0)
    lengths, clips, at = (20, 45, 7, 33, 64, 1, 30), {}, 0
    for i, t in enumerate(lengths):                       # windows of the walk (wrapping), each moved a little
        rows = (at + np.arange(t)) % len(kp)
        clips[f"clip_{i:02d}"] = kp[rows] + np.array([0.1 * i, 0.0, 0.0])
        at += 11
    m = S.smpl_model()
    one = fit_keypoint_clips(m, clips, iterations=5, backend="device", device=DEV)
    logged = []
    many = fit_keypoint_clips(m, clips, iterations=5, backend="device", device=DEV, chunk_frames=64, log=logged.append)
    assert list(one) == list(many) == list(clips) and len(logged) >= 4          # (at least four chunks, one line each)
    for k in clips:
        for f in ("pose_quat_global", "root_trans_offset", "pose_aa", "keypoints", "fit_loss", "fit_keypoint_error"):
            assert np.array_equal(np.asarray(one[k][f]), np.asarray(many[k][f])), (k, f)


def test_captured_graph_replays_the_iterations():
    """One phc_fit_sph_iterate(iterations = 5) captured into a torch.cuda.graph (one stream, no parallel branches) and replayed twice = 10 eager iterations."""
    from phc_amd import _lib as L
    lib = L.load()
    case = S.make_batch("smpl24")
    st = S.zero_state(case)
    eager = S.run(case, st, 10, device=DEV)
    args, mem = S.place(case, st, DEV)
    first = {k: mem[k].clone() for k in S.STATE}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # (a warm-up outside the capture; the state is put back below)
        assert lib.phc_fit_sph_iterate(args, 5, side.cuda_stream) == 0
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = lib.phc_fit_sph_iterate(args, 5, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    for k in S.STATE:
        mem[k].copy_(first[k])
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    got = S.collect(mem)
    for k in S.STATE:
        assert np.array_equal(got[k], eager[k]), k


def test_device_backend_end_to_end():
    """300 iterations on the 61-frame walk: the error against both host precisions, the layout, `MotionLibSMPL` loads it and `get_motion_state` at the frame
    times gives the input keypoints back at the same mean error."""
    from phc_amd.env.tasks.humanoid_im import SkeletonTree
    from phc_amd.utils.fit_keypoints import fit_keypoint_clips
    m = S.smpl_model()
    kp = S.walk_keypoints(2.0)
    out = fit_keypoint_clips(m, {"walk": kp}, iterations=300, backend="device", device=DEV)["walk"]
    T.check_clip(out, kp, 300, "device backend")
    from phc_amd.config import EasyDict
    from phc_amd.motion_lib import MotionLibSMPL
    lib = MotionLibSMPL(EasyDict({"motion_file": {"walk": out}, "device": DEV, "min_length": -1, "max_length": -1, "im_eval": False, "multi_thread": False,
                                  "randomrize_heading": False, "step_dt": 1 / 30}))
    lib.load_motions(skeleton_trees=[SkeletonTree(m.body_names, m.parent, m.local_translation)], random_sample=False)
    assert lib._motion_num_frames.tolist() == [len(kp)]
    ids = torch.zeros(len(kp), dtype=torch.int64, device=DEV)
    times = torch.arange(len(kp), dtype=torch.float32, device=DEV) / 30.0
    pos = lib.get_motion_state(ids, times)["rg_pos"].cpu().numpy().astype(np.float64)
    back = float(np.linalg.norm(pos - kp, axis=-1).mean())
    print(f"device backend: keypoints through get_motion_state: {back * 1000:.3f} mm")
    assert abs(back - out["fit_keypoint_error"]) <= 1e-4, (back, out["fit_keypoint_error"])
