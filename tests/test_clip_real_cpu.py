"""Device clip processing for the robots (`clip_processing: device` on MotionLibReal, phc_clip_process_real) on a machine without a GPU:
phc_amd/csrc/phc_clip_real.h built for the host with g++ (tests/clip_real_shim.cpp) against the robot branch of `_run_clip_job` -- the existing host path --
field by field, the height fix alone, guard words, the argument checks, the binding and the host-side errors.  The launches themselves:
tests/test_clip_real_gpu.py."""
import numpy as np
import pytest

import clip_real_util as ru

EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("fix", [True, False], ids=["height_fix", "no_fix"])
@pytest.mark.parametrize("name", ru.TREES)
def test_lane_functions_equal_the_host_path(name, fix):
    """Clips of 3 .. 40 frames concatenated in ONE call, 30 and 60 fps: every field within one fp32 rounding (gavs: plus the acos floor), the pad floats 0;
    guard words behind `frames` and the scratch intact and every float written (clip_real_util.host_process)."""
    want, fps_frame, _ = ru.oracle(name, fix)
    got, _ = ru.host_process(name, fix)
    _, n = ru.arrays(name, fix)
    ru.compare(got, want, fps_frame, n["NB"], n["E"], what=f"{name} fix={fix} host build vs _run_clip_job:")


@pytest.mark.parametrize("name", ru.TREES)
def test_height_fix_alone(name):
    """clip_dz of every clip against `fix_trans_height`'s diff, to 1e-12 relative; without the fix it is 0."""
    _, _, want = ru.oracle(name, True)
    _, dz = ru.host_process(name, True)
    err = np.abs(dz - want) / np.maximum(np.abs(want), 1e-300)
    print(f"{name} clip_dz: worst relative error {err.max():.3e} (|dz| {np.abs(want).min():.3f} .. {np.abs(want).max():.3f})")
    assert (np.abs(want) > 1e-3).all() and err.max() <= 1e-12
    assert (ru.host_process(name, False)[1] == 0).all()


def test_a_leak_across_a_clip_boundary_would_show():
    """The inputs' own property: across every clip boundary the root velocity jumps so far that even the filter's smallest tap (exp(-8) / 5.01 = 6.7e-5) reaching
    into the neighbour would miss the tolerance by more than a factor of ten."""
    want, _, _ = ru.oracle("chain")
    root_v = want[:, ru.fields(3, 1)[0]["gvs"]][:, :3].astype(np.float64)
    ends = np.cumsum(ru.LENGTHS)[:-1]
    jump = np.abs(root_v[ends] - root_v[ends - 1]).max(axis=1)
    assert (6.7e-5 * jump > 10 * ru.EPS32 * np.abs(root_v).max()).all(), jump


def test_row_sum_order_and_last_frame_quirk():
    """dof_pos is numpy's three-term row sum, bit for bit before the one rounding, and the clip's last dvs is the difference of frames T-3 and T-2."""
    want, _, _ = ru.oracle("h1")
    got, _ = ru.host_process("h1")
    fl, _ = ru.fields(20, 3)
    assert np.array_equal(got[:, fl["dof_pos"]], want[:, fl["dof_pos"]])
    _, poses, _, fps = ru.case("h1")
    ends = np.cumsum(ru.LENGTHS) - 1
    for u, e in enumerate(ends):
        d = poses[u].sum(-1)[:, 1:20]
        assert np.array_equal(got[e, fl["dvs"]], ((d[-2] - d[-3]) / (1.0 / fps[u])).astype(np.float32))


def _small_args(fix=True):
    _, n = ru.arrays("chain", fix)
    sb = int(ru.shim().clip_real_scratch_bytes_of(n["F"], n["NB"], n["U"]))
    keep = [np.zeros((n["F"], 52), dtype=np.float32), np.zeros(sb // 8, dtype=np.float64)]
    a, _ = ru.host_args("chain", fix, keep[0], keep[1], keep)
    return a, keep, sb


def test_argument_checks():
    """`clip_real_args_check` (phc_clip_real.h), the function `phc_clip_process_real` asks before it launches, through the host build: nothing here reaches a
    launch."""
    check = ru.shim().clip_real_args_check_of
    a, keep, sb = _small_args()
    assert sb == 115 * 3 * 48 + 8 * 8 + 464 and check(a) == 0 and check(None) == EINVAL
    for f in ru.POINTERS:
        old = getattr(a, f)
        setattr(a, f, None)
        assert check(a) == EINVAL, f
        setattr(a, f, old)
    misaligned = tuple((f, getattr(a, f) + 4, EINVAL) for f in ("offsets", "rest_mat", "pose_aa", "trans", "clip_start", "clip_dt", "contact_pos", "contact_radius", "scratch"))
    misaligned += tuple((f, getattr(a, f) + 2, EINVAL) for f in ("parents", "contact_body", "frames"))
    for f, bad, code in ru.BAD_ARGS + (("scratch_bytes", sb - 1, EINVAL),) + misaligned:
        old = getattr(a, f)
        setattr(a, f, bad)
        if f == "num_frames" and bad > 115:
            a.scratch_bytes = 1 << 62
        assert check(a) == code, (f, bad)
        setattr(a, f, old)
        a.scratch_bytes = sb
    for f, good in (("scratch_bytes", sb + 8), ("num_frames", 24)):
        old = getattr(a, f)
        setattr(a, f, good)
        assert check(a) == 0, (f, good)
        setattr(a, f, old)
    a.num_bodies, a.num_ext, a.frame_stride, a.scratch_bytes = 60, 4, 928, 1 << 40
    assert check(a) == 0 and ru.shim().clip_real_stride_of(60, 4) == 928, "64 bodies including the extended ones is the limit"
    a.num_ext = 5
    assert check(a) == EUNSUPPORTED, "NB + E = 65"
    # without the height fix the contact arrays are not asked for
    a, keep, sb = _small_args(fix=False)
    a.num_contacts, a.contact_body, a.contact_pos, a.contact_radius = 0, None, None, None
    assert check(a) == 0
    a.fix_height = 1
    assert check(a) == EINVAL
    assert [ru.shim().clip_real_frames_per_block_of(*j) for j in ((1, 0), (20, 3), (38, 1), (64, 0))] == [16, 16, 14, 8]
    from phc_amd import abi
    assert all(ru.shim().clip_real_stride_of(nb, ne) == abi.frame_stride_for(nb, ne, 1) for nb in range(1, 65) for ne in range(0, 65 - nb))


def test_binding_and_struct_size():
    from phc_amd import _lib as L
    assert {"phc_clip_real_scratch_bytes", "phc_clip_process_real"} <= set(L.EXPORTED_SYMBOLS) and hasattr(L, "ClipRealArgs")
    lib = L.load()
    assert hasattr(lib, "phc_clip_real_scratch_bytes") and hasattr(lib, "phc_clip_process_real") and lib.phc_abi_version() == 37
    assert len(lib.phc_clip_process_real.argtypes) == 2 and lib.phc_clip_process_real.restype is L.c_i32 and lib.phc_clip_real_scratch_bytes.restype is L.c_i64
    assert lib.phc_clip_real_scratch_bytes(115, 3, 1, 8) == 115 * 3 * 48 + 64 + 464 == ru.shim().clip_real_scratch_bytes_of(115, 3, 8)
    assert [lib.phc_clip_real_scratch_bytes(*bad) for bad in ((-1, 3, 1, 8), (4, 0, 1, 8), (4, 3, -1, 8), (4, 3, 1, 0))] == [EINVAL] * 4
    # (phc_clip_real_args_t against its mirror: tests/test_abi_and_host.py)  the entry point refuses before any device work (no GPU is touched here)
    a, keep, sb = _small_args()
    a.scratch_bytes = sb - 1
    assert lib.phc_clip_process_real(a, None) == EINVAL and lib.phc_clip_process_real(None, None) == EINVAL
    a.scratch_bytes, a.num_ext = sb, 62
    assert lib.phc_clip_process_real(a, None) == EUNSUPPORTED


def test_validator_refusals():
    from phc_amd import motion_lib as ML
    consts, poses, trans, fps = ru.case("chain")
    short = [p[:2] if u == 5 else p for u, p in enumerate(poses)], [t[:2] if u == 5 else t for u, t in enumerate(trans)]
    with pytest.raises(ValueError, match="clip 5 has 2 frame"):
        ML.validate_robot_clip_inputs(consts, short[0], short[1], fps)
    with pytest.raises(ValueError, match="clip 5 has 2 frame"):
        ML.process_robot_clips_device(consts, short[0], short[1], fps, "cpu")
    with pytest.raises(ValueError, match="clip 2"):
        ML.validate_robot_clip_inputs(consts, [p[:, :3] if u == 2 else p for u, p in enumerate(poses)], trans, fps)   # narrower than NB + E
    with pytest.raises(ValueError, match="clip 1"):
        ML.validate_robot_clip_inputs(consts, poses, [t[:-1] if u == 1 else t for u, t in enumerate(trans)], fps)
    for bad_fps in ([30] * 7 + [0], [30] * 7 + [-1.0], [30] * 7):
        with pytest.raises(ValueError):
            ML.validate_robot_clip_inputs(consts, poses, trans, bad_fps)
    with pytest.raises(ValueError, match="precede"):
        ML.validate_robot_clip_inputs(dict(consts, parent=np.array([-1, 2, 1])), poses, trans, fps)
    many = dict(consts, parent=np.arange(-1, 63), local_translation=np.zeros((64, 3)), local_rotation=np.tile([1.0, 0, 0, 0], (64, 1)), num_bodies=64)
    with pytest.raises(ValueError, match="at most 64 bodies"):
        ML.validate_robot_clip_inputs(many, [np.zeros((3, 65, 3))], [np.zeros((3, 3))], [30])
    v = ML.validate_robot_clip_inputs(consts, [np.concatenate([p, np.ones((p.shape[0], 2, 3))], axis=1) for p in poses], trans, fps)   # wider is fine
    assert v["nf"].tolist() == list(ru.LENGTHS) and v["num_bodies"] == 3 and v["num_ext"] == 1 and v["rest_mat"].shape == (4, 3, 3)


@pytest.mark.parametrize("name", ["h1", "chain"])
def test_motion_lib_real_takes_the_option(name):
    """`clip_processing: device` on MotionLibReal: the constructor accepts it; on the CPU `load_motions` fails with the RuntimeError that names the HIP device
    (no fallback) and starts no worker pool."""
    from phc_amd import motion_lib as ML
    from phc_amd.env.tasks.humanoid_im import SkeletonTree
    lib = ru.library(name, clip_processing="device")
    _, model = ru.robot(name)
    tree = SkeletonTree(model.body_names, model.parent, model.local_translation)
    with pytest.raises(RuntimeError, match="HIP device only.*clip_processing=host"):
        lib.load_motions(skeleton_trees=[tree] * 2, random_sample=False)
    with pytest.raises(RuntimeError, match="clip_processing=host"):
        ML.process_robot_clips_device(*ru.case(name), device="cpu")
    assert not ML._POOL, "no worker pool for the device path"
    assert lib._job_fps(30.0) == 30 and isinstance(lib._job_fps(30.0), int)


def test_a_model_that_is_not_all_revolute_is_refused_at_construction():
    """The option on a MotionLibReal whose model has spherical joints (the SMPL humanoid: 69 DoF on 24 bodies), or on a config without a model, is a
    NotImplementedError that names `clip_processing=host`; with the default the same config is not refused for it."""
    import types
    from phc_amd import motion_lib as ML
    from phc_amd.model import load_model
    smpl = load_model("smpl_humanoid")
    assert smpl.num_dof != smpl.num_bodies - 1
    cfg = {"clip_processing": "device", "robot_model": smpl, "robot": {"extend_config": []}}
    with pytest.raises(NotImplementedError, match="all-revolute.*clip_processing=host"):
        ML.MotionLibReal(cfg)
    with pytest.raises(NotImplementedError, match="clip_processing=host"):
        ML.MotionLibReal({"clip_processing": "device", "robot": {"extend_config": []}})
    with pytest.raises(AttributeError):   # (the default goes on to the constructor's own needs: this plain dict is no full config)
        ML.MotionLibReal(dict(cfg, clip_processing="host"))
    _, chain = ru.robot("chain")
    assert chain.num_dof == chain.num_bodies - 1 and isinstance(chain, types.SimpleNamespace)
