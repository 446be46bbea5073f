"""Device clip processing for the robots on the MI355X: `process_robot_clips_device` / phc_clip_process_real against the existing host path (the robot branch
of `_run_clip_job`, tests/clip_real_util.py) at the tolerance of one fp32 rounding, chunking, guard words, the entry point's refusals, and the option end to
end (`+env.clip_processing=device` on H1 and G1) against the same task built with the default."""
import numpy as np
import pytest
import torch

import clip_real_util as ru
from clip_util import ANG_FLOOR, EPS32, GUARD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("name", ru.TREES)
def test_process_robot_clips_device_equals_the_host_path(name):
    """The constructed clips (3 .. 40 frames in one call, 30 / 60 fps, height fix on) with the default chunk, and with chunk_frames = 32: the clips split
    over several chunks, the 40-frame clip is a chunk of its own, the two staging slots are re-used.  Chunking must not change a bit."""
    from phc_amd import motion_lib as ML
    want, fps_frame, _ = ru.oracle(name)
    c = ru.case(name)
    _, n = ru.arrays(name)
    whole = ML.process_robot_clips_device(*c, device=DEV)
    stage = ML._CLIP_STAGE[torch.device(DEV)]
    uses = stage.uses
    slots = [s.data_ptr() for s in stage.slots if s is not None]
    parts = ML.process_robot_clips_device(*c, device=DEV, chunk_frames=32)
    torch.cuda.synchronize()
    assert whole.device == torch.device(DEV) and whole.dtype == torch.float32 and tuple(whole.shape) == want.shape
    assert stage is ML._CLIP_STAGE[torch.device(DEV)] and stage.uses == uses + 1 and all(s is not None for s in stage.slots)
    assert slots[0] in [s.data_ptr() for s in stage.slots], "the staging buffers are kept and re-used"
    assert len(ML._clip_chunks(list(ru.LENGTHS), 32)) > 2
    ru.compare(whole.cpu().numpy(), want, fps_frame, n["NB"], n["E"], what=f"{name} device vs _run_clip_job:")
    assert torch.equal(whole, parts), "chunking changed the records"


def _device_args(name, fix=True):
    """phc_clip_real_args_t over device tensors, with guard words behind `frames` and behind the scratch."""
    from phc_amd import _lib as L
    from phc_amd import abi
    arrs, n = ru.arrays(name, fix)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in arrs.items()}
    stride = abi.frame_stride_for(n["NB"], n["E"], 1)
    sb = int(L.load().phc_clip_real_scratch_bytes(n["F"], n["NB"], n["E"], n["U"]))
    frames = torch.full((n["F"] * stride + 4,), 7.0, dtype=torch.float32, device=DEV)
    frames[-4:].view(torch.int32).fill_(GUARD)
    scratch = torch.zeros(sb // 8 + 2, dtype=torch.float64, device=DEV)
    scratch[-2:].view(torch.int64).fill_(GUARD)
    a = abi.clip_real_args_struct(n["U"], n["F"], n["NB"], n["E"], n["C"], n["fix"], scratch, sb, frames, **t)
    return a, dict(t, frames=frames, scratch=scratch), sb, n, stride


@pytest.mark.parametrize("fix", [True, False], ids=["height_fix", "no_fix"])
@pytest.mark.parametrize("name", ru.TREES)
def test_entry_point_guard_words_and_pad_floats(name, fix):
    from phc_amd import _lib as L
    want, fps_frame, dz = ru.oracle(name, fix)
    a, t, sb, n, stride = _device_args(name, fix)
    assert L.load().phc_clip_process_real(a, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert (t["frames"][-4:].view(torch.int32) == GUARD).all() and (t["scratch"][-2:].view(torch.int64) == GUARD).all()
    got = t["frames"][:-4].view(want.shape).cpu().numpy()
    assert (got[:, ru.fields(n["NB"], n["E"])[0]["pad"]] == 0).all() and not (got == 7.0).any(), "every float of every record is written, the pads as 0"
    ru.compare(got, want, fps_frame, n["NB"], n["E"], what=f"{name} fix={fix} phc_clip_process_real vs _run_clip_job:")
    got_dz = t["scratch"][n["F"] * 6 * n["NB"]:n["F"] * 6 * n["NB"] + n["U"]].cpu().numpy()
    assert np.abs(got_dz - (dz if fix else 0.0)).max() <= 1e-12 * max(1.0, float(np.abs(dz).max()))


def test_entry_point_refuses_before_any_launch():
    """The refusals of tests/test_clip_real_cpu.py through phc_clip_process_real itself: the code comes back and `frames` keeps its fill value."""
    from phc_amd import _lib as L
    fn, stream = L.load().phc_clip_process_real, torch.cuda.current_stream().cuda_stream
    a, t, sb, n, stride = _device_args("chain")
    assert fn(None, stream) == EINVAL
    for f in ru.POINTERS:
        old = getattr(a, f)
        setattr(a, f, None)
        assert fn(a, stream) == EINVAL, f
        setattr(a, f, old)
    for f, bad, code in ru.BAD_ARGS + (("scratch_bytes", sb - 1, EINVAL), ("pose_aa", a.pose_aa + 4, EINVAL), ("frames", a.frames + 2, EINVAL)):
        old = getattr(a, f)
        setattr(a, f, bad)
        if f == "num_frames" and bad > n["F"]:
            a.scratch_bytes = 1 << 62
        assert fn(a, stream) == code, (f, bad)
        setattr(a, f, old)
        a.scratch_bytes = sb
    torch.cuda.synchronize()
    assert (t["frames"][:-4] == 7.0).all(), "a refused call must not launch"


ROBOT = {"h1": ("robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"),
         "g1": ("robot=unitree_g1", "env=env_im_g1_phc", "sim=robot_sim", "control=robot_control")}


def _task(n, over, device_clips):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(3)
    return parse_task(compose(list(over) + [f"env.num_envs={n}", "env.motion_file=synthetic:6:2"] + (["+env.clip_processing=device"] if device_clips else [])))


def _close(got, want, floor_fps=None, scale=4.0):
    a, b = got.double().cpu().numpy(), want.double().cpu().numpy()
    tol = EPS32 * np.maximum(np.abs(b), 1.0) + (0.0 if floor_fps is None else ANG_FLOOR * floor_fps / 30.0)
    return float((np.abs(a - b) / (scale * tol)).max())


def _agree(lh, ld, nb, ne, what):
    """Same draw and shapes; records and lookups at 64 random (id, time) pairs within 4x the per-field tolerances."""
    assert torch.equal(lh._curr_motion_ids, ld._curr_motion_ids) and lh.frames.shape == ld.frames.shape
    assert torch.equal(lh._motion_num_frames, ld._motion_num_frames) and torch.equal(lh._motion_fps, ld._motion_fps)
    assert torch.equal(lh._motion_lengths, ld._motion_lengths) and torch.equal(lh.length_starts, ld.length_starts)
    fps_frame = torch.repeat_interleave(lh._motion_fps, lh._motion_num_frames).double().cpu().numpy()
    ru.compare(ld.frames.cpu().numpy(), lh.frames.cpu().numpy(), fps_frame, nb, ne, scale=4.0, what=f"{what} frames, device vs host:")
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 8, (64,), generator=g).to(DEV)
    times = (torch.rand(64, generator=g).to(DEV) * lh._motion_lengths[ids])
    sh, sd = lh.get_motion_state(ids, times), ld.get_motion_state(ids, times)
    fps = lh._motion_fps[ids].double().cpu().numpy()
    assert set(sh) == set(sd)
    for k in sorted(sh):
        if k == "motion_aa" or not torch.is_floating_point(sh[k]):
            assert torch.equal(sd[k], sh[k]), k
            continue
        floor = fps.reshape((-1,) + (1,) * (sh[k].dim() - 1)) if k in ("body_ang_vel", "root_ang_vel", "body_ang_vel_t") else None
        r = _close(sd[k], sh[k], floor)
        print(f"{what} get_motion_state {k}: worst |diff| / (4 x tolerance) = {r:.3e}")
        assert r <= 1.0, k


@pytest.mark.parametrize("name", ["h1", "g1"])
def test_option_end_to_end(name):
    """Two tasks of 8 envs on the same multi-clip synthetic robot library and seed, one with `+env.clip_processing=device`: same draw, same shapes, records and
    lookups within 4x the per-field tolerances; the same again after `load_motions(..., max_len=20)` under one seed (crops are drawn, the height fix uses each
    crop's first frame); the device task then resamples twice and steps."""
    from phc_amd import motion_lib as ML
    uses = lambda: getattr(ML._CLIP_STAGE.get(torch.device(DEV)), "uses", 0)
    th, _ = _task(8, ROBOT[name], False)
    before = uses()
    td, env_d = _task(8, ROBOT[name], True)
    assert uses() > before, "the device task's records come from phc_clip_process_real"
    lh, ld = th._motion_lib, td._motion_lib
    assert isinstance(ld, ML.MotionLibReal) and ld.m_cfg["clip_processing"] == "device" and lh.m_cfg["clip_processing"] == "host" and not ML._POOL
    nb, ne = ld.num_bodies, ld.num_ext_bodies
    assert len(set(lh._curr_motion_ids.tolist())) > 1 and ld._motion_fps.tolist() == [30.0] * 8
    _agree(lh, ld, nb, ne, f"{name} task")
    for lib, task in ((lh, th), (ld, td)):
        torch.manual_seed(11)
        lib._heading_rs = None          # (the crop stream restarts from the seed on both sides)
        lib.load_motions(skeleton_trees=task.skeleton_trees, random_sample=True, max_len=20)
    assert (ld._motion_num_frames == 20).all() and uses() > before + 1
    _agree(lh, ld, nb, ne, f"{name} cropped")
    epoch = ld.frames_epoch
    td.resample_motions()
    td.resample_motions()
    assert ld.frames_epoch == epoch + 2 and not ML._POOL
    env_d.step(torch.zeros(8, td.num_dof, device=DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(td.obs_buf).all() and torch.isfinite(ld.frames).all()
