"""Device clip processing (`clip_processing: device`, phc_clip_process) on a machine without a GPU: phc_amd/csrc/phc_clip.h built for the host with g++
(tests/clip_shim.cpp) against `process_clip` -- the existing host path -- field by field, the filter's weights against scipy, the argument checks, the
binding and the host-side errors.  The launches themselves: tests/test_clip_device_gpu.py."""
import numpy as np
import pytest
import torch

import clip_util as cu

EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("name", ["smpl", "chain3", "star5"])
def test_lane_functions_equal_process_clip(name):
    """Clips of 2 .. 40 frames concatenated in ONE call, 30 and 60 fps, two body shapes: every field at the tolerance of one fp32 rounding (angular fields:
    plus the acos floor); grs and the pad floats bit-equal."""
    want, fps_frame = cu.oracle(name)
    got = cu.host_process(name)
    cu.compare(got, want, fps_frame, what=f"{name} host build vs process_clip:")


def test_a_leak_across_a_clip_boundary_would_show():
    """The inputs' own property: across every clip boundary the root velocity jumps so far that even the filter's smallest tap (exp(-8) / 5.01 = 6.7e-5) reaching
    into the neighbour would miss the tolerance by more than a factor of ten."""
    want, _ = cu.oracle("chain3")
    root_v = want[:, cu.fields(3)["gvs"]][:, :3].astype(np.float64)
    ends = np.cumsum(cu.LENGTHS)[:-1]
    jump = np.abs(root_v[ends] - root_v[ends - 1]).max(axis=1)
    assert (6.7e-5 * jump > 10 * cu.EPS32 * np.abs(root_v).max()).all(), jump


def test_gaussian_weights_equal_scipys():
    from scipy.ndimage import gaussian_filter1d
    w = np.zeros(17)
    cu.shim().clip_weights(w.ctypes.data)
    impulse = np.zeros(33)
    impulse[16] = 1.0
    ref = gaussian_filter1d(impulse, 2, mode="nearest")
    assert ref[:8].max() == 0.0 and ref[25:].max() == 0.0, "radius 8"
    err = np.abs(w - ref[8:25]).max()
    print(f"max |weight - scipy| = {err:.3e}")
    assert err <= 1e-15 and abs(w.sum() - 1.0) <= 1e-15


def _small_args():
    c = cu.make_case("chain3")
    F_ = int(sum(cu.LENGTHS))
    sb = int(cu.shim().clip_scratch_bytes_of(F_, 3))
    keep = [np.zeros((F_, 60), dtype=np.float32), np.zeros(sb // 8, dtype=np.float64)]
    return cu.host_args(c, keep[0], keep[1], keep), keep, sb


def test_argument_checks():
    """`clip_args_check` (phc_clip.h), the function `phc_clip_process` asks before it launches, through the host build: nothing here reaches a launch."""
    check = cu.shim().clip_args_check_of
    a, keep, sb = _small_args()
    assert sb == 113 * 3 * 48 + 456 and check(a) == 0 and check(None) == EINVAL
    for f in ("parents", "local_translation", "clip_tree", "clip_start", "clip_dt", "quat", "trans", "scratch", "frames"):
        old = getattr(a, f)
        setattr(a, f, None)
        assert check(a) == EINVAL, f
        setattr(a, f, old)
    for f, bad, code in cu.BAD_ARGS + (("scratch_bytes", sb - 1, EINVAL), ("quat", a.quat + 4, EINVAL), ("scratch", a.scratch + 4, EINVAL), ("frames", a.frames + 2, EINVAL)):
        old = getattr(a, f)
        setattr(a, f, bad)
        if f == "num_frames" and bad > 113:
            a.scratch_bytes = 1 << 62
        assert check(a) == code, (f, bad)
        setattr(a, f, old)
        a.scratch_bytes = sb
    for f, good in (("scratch_bytes", sb + 8), ("num_frames", 16), ("num_trees", 7)):
        old = getattr(a, f)
        setattr(a, f, good)
        assert check(a) == 0, (f, good)
        setattr(a, f, old)
    a.num_bodies, a.frame_stride, a.scratch_bytes = 64, 1280, 1 << 40
    assert check(a) == 0, "64 bodies is the limit"
    assert [cu.shim().clip_frames_per_block_of(j) for j in (1, 24, 64)] == [16, 16, 6]


def test_binding_and_struct_size():
    from phc_amd import _lib as L
    assert {"phc_clip_scratch_bytes", "phc_clip_process"} <= set(L.EXPORTED_SYMBOLS) and hasattr(L, "ClipArgs")
    lib = L.load()
    assert hasattr(lib, "phc_clip_scratch_bytes") and hasattr(lib, "phc_clip_process") and lib.phc_abi_version() == 37
    assert len(lib.phc_clip_process.argtypes) == 2 and lib.phc_clip_process.restype is L.c_i32 and lib.phc_clip_scratch_bytes.restype is L.c_i64
    assert lib.phc_clip_scratch_bytes(113, 3) == 113 * 3 * 48 + 456 == cu.shim().clip_scratch_bytes_of(113, 3)
    assert lib.phc_clip_scratch_bytes(-1, 3) == EINVAL and lib.phc_clip_scratch_bytes(4, 0) == EINVAL
    # (phc_clip_args_t against its mirror: tests/test_abi_and_host.py)  the entry point refuses before any device work (no GPU is touched here)
    a, keep, sb = _small_args()
    a.scratch_bytes = sb - 1
    assert lib.phc_clip_process(a, None) == EINVAL and lib.phc_clip_process(None, None) == EINVAL
    a.scratch_bytes, a.num_bodies = sb, 65
    assert lib.phc_clip_process(a, None) == EUNSUPPORTED


def _smpl_lib(**over):
    from phc_amd.config import EasyDict
    from phc_amd.motion_lib import MotionLibSMPL
    c = cu.make_case("smpl")
    clips = {f"clip{u}": {"pose_quat_global": g, "root_trans_offset": t, "fps": f} for u, (g, t, f) in enumerate(zip(c["quats"], c["trans"], c["fps"]))}
    cfg = {"motion_file": clips, "device": "cpu", "min_length": -1, "im_eval": False, "step_dt": 1 / 30}
    cfg.update(over)
    return MotionLibSMPL(EasyDict(cfg))


def _smpl_tree():
    from phc_amd.env.tasks.humanoid_im import SkeletonTree
    from phc_amd.model import load_model
    m = load_model("smpl_humanoid")
    return SkeletonTree(m.body_names, m.parent, m.local_translation)


def test_host_side_errors():
    from phc_amd import motion_lib as ML
    with pytest.raises(ValueError, match="clip_processing"):
        _smpl_lib(clip_processing="nonsense")
    lib = _smpl_lib()
    lib.m_cfg["clip_processing"] = "nonsense"
    with pytest.raises(ValueError, match="clip_processing"):
        lib.load_motions(skeleton_trees=[_smpl_tree()] * 2, random_sample=False)
    c = cu.make_case("chain3")
    with pytest.raises(RuntimeError, match="clip_processing=host"):
        ML.process_clips_device(device="cpu", **c)
    with pytest.raises(RuntimeError, match="clip_processing=host"):
        _smpl_lib(clip_processing="device").load_motions(skeleton_trees=[_smpl_tree()] * 2, random_sample=False)
    assert not ML._POOL, "no worker pool for the device path"
    one = dict(c, quats=[q[:1] if u == 3 else q for u, q in enumerate(c["quats"])], trans=[t[:1] if u == 3 else t for u, t in enumerate(c["trans"])])
    with pytest.raises(ValueError, match="clip 3 has 1 frame"):
        ML.process_clips_device(device="cpu", **one)
    for bad in (dict(parents=np.array([-1, 2, 1])), dict(clip_tree=np.array([0, 1, 2, 0, 1, 0, 0, 1])), dict(fps=[30] * 7 + [0])):
        with pytest.raises(ValueError):
            ML.process_clips_device(device="cpu", **dict(c, **bad))
    with pytest.raises(NotImplementedError, match="clip_processing=host"):
        ML.MotionLibReal({"clip_processing": "device"})
    assert ML._clip_chunks([40, 2, 3, 8, 9, 16, 17, 18], 32) == [(0, 1), (1, 5), (5, 6), (6, 7), (7, 8)]
    assert ML._clip_chunks(list(cu.LENGTHS), 262144) == [(0, 8)]


def test_default_stays_host():
    """Without the option nothing changes: `load_motions` on the CPU takes the numpy path and its records are the oracle's."""
    lib = _smpl_lib()
    tree = _smpl_tree()
    from phc_amd.utils.flags import flags
    flags.test = True   # (no random heading)
    try:
        lib.load_motions(skeleton_trees=[tree] * 8, random_sample=False)
    finally:
        flags.test = False
    c = cu.make_case("smpl")
    from phc_amd import abi
    from phc_amd.motion_lib import process_clip
    recs = []
    for g, t, f in zip(c["quats"], c["trans"], c["fps"]):
        p = {k: v.astype(np.float32) for k, v in process_clip(tree.parent_indices.numpy(), tree.local_translation.numpy(), g, t, f).items()}
        recs.append(abi.pack_frames(p["gts"], p["grs"], p["gvs"], p["gavs"], p["lrs"], p["dvs"]))
    assert np.array_equal(lib.frames.numpy(), np.concatenate(recs)) and torch.equal(lib._motion_num_frames, torch.tensor(cu.LENGTHS))
