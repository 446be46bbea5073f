"""Device clip processing on the MI355X: `process_clips_device` / phc_clip_process against the existing host path (`process_clip` + float32 +
`abi.pack_frames`, tests/clip_util.py) at the tolerance of one fp32 rounding, chunking, guard words, the entry point's refusals, and the option end to end
(`+env.clip_processing=device`) against the same task built with the default."""
import numpy as np
import pytest
import torch

import clip_util as cu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EUNSUPPORTED = -1, -2


@pytest.mark.parametrize("name", ["smpl", "chain3", "star5"])
def test_process_clips_device_equals_the_host_path(name):
    """The constructed clips (2 .. 40 frames in one call, 30 / 60 fps, two body shapes) with the default chunk, and with chunk_frames = 32: the clips split over
    five chunks, the 40-frame clip is a chunk of its own, the two staging slots are re-used.  Chunking must not change a bit."""
    from phc_amd import motion_lib as ML
    want, fps_frame = cu.oracle(name)
    c = cu.make_case(name)
    whole = ML.process_clips_device(device=DEV, **c)
    uses = ML._CLIP_STAGE[torch.device(DEV)].uses
    slots = [s.data_ptr() for s in ML._CLIP_STAGE[torch.device(DEV)].slots if s is not None]
    parts = ML.process_clips_device(device=DEV, chunk_frames=32, **c)
    torch.cuda.synchronize()
    assert whole.device == torch.device(DEV) and whole.dtype == torch.float32 and tuple(whole.shape) == want.shape
    stage = ML._CLIP_STAGE[torch.device(DEV)]
    assert stage.uses == uses + 1 and slots[0] in [s.data_ptr() for s in stage.slots], "the staging buffers are kept and re-used"
    cu.compare(whole.cpu().numpy(), want, fps_frame, what=f"{name} device vs process_clip:")
    assert torch.equal(whole, parts), "chunking changed the records"


def _device_args(c, frames_guard=4):
    """phc_clip_args_t over device tensors, with guard words behind `frames` and behind the scratch."""
    from phc_amd import _lib as L
    from phc_amd import abi
    J, nf = len(c["parents"]), np.array([q.shape[0] for q in c["quats"]], dtype=np.int64)
    F_ = int(nf.sum())
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEV)
    t = dict(parents=up(c["parents"], np.int32), lt=up(c["local_translations"], np.float64), tree=up(c["clip_tree"], np.int32),
             start=up(np.concatenate([[0], np.cumsum(nf)]), np.int64), dt=up(1.0 / np.asarray(c["fps"], dtype=np.float64), np.float64),
             quat=up(np.concatenate(c["quats"]), np.float64), trans=up(np.concatenate(c["trans"]), np.float64))
    sb = int(L.load().phc_clip_scratch_bytes(F_, J))
    t["frames"] = torch.full((F_ * 20 * J + frames_guard,), 7.0, dtype=torch.float32, device=DEV)
    t["frames"][-frames_guard:].view(torch.int32).fill_(cu.GUARD)
    t["scratch"] = torch.zeros(sb // 8 + 2, dtype=torch.float64, device=DEV)
    t["scratch"][-2:].view(torch.int64).fill_(cu.GUARD)
    a = abi.clip_args_struct(len(nf), F_, J, t["lt"].shape[0], t["parents"], t["lt"], t["tree"], t["start"], t["dt"], t["quat"], t["trans"], t["scratch"], sb, t["frames"])
    return a, t, sb


@pytest.mark.parametrize("name", ["smpl", "chain3"])
def test_guard_words_and_pad_floats(name):
    from phc_amd import _lib as L
    want, fps_frame = cu.oracle(name)
    a, t, sb = _device_args(cu.make_case(name))
    assert L.load().phc_clip_process(a, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert (t["frames"][-4:].view(torch.int32) == cu.GUARD).all() and (t["scratch"][-2:].view(torch.int64) == cu.GUARD).all()
    got = t["frames"][:-4].view(want.shape).cpu().numpy()
    assert (got[:, cu.fields(want.shape[1] // 20)["pad"]] == 0).all() and not (got == 7.0).any(), "every float of every record is written, the pads as 0"
    cu.compare(got, want, fps_frame, what=f"{name} phc_clip_process vs process_clip:")


def test_entry_point_refuses_before_any_launch():
    """The refusals of tests/test_clip_device_cpu.py through phc_clip_process itself: the code comes back and `frames` keeps its fill value."""
    from phc_amd import _lib as L
    fn, stream = L.load().phc_clip_process, torch.cuda.current_stream().cuda_stream
    a, t, sb = _device_args(cu.make_case("chain3"))
    assert fn(None, stream) == EINVAL
    for f in ("parents", "local_translation", "clip_tree", "clip_start", "clip_dt", "quat", "trans", "scratch", "frames"):
        old = getattr(a, f)
        setattr(a, f, None)
        assert fn(a, stream) == EINVAL, f
        setattr(a, f, old)
    for f, bad, code in cu.BAD_ARGS + (("scratch_bytes", sb - 1, EINVAL),):
        old = getattr(a, f)
        setattr(a, f, bad)
        if f == "num_frames" and bad > 113:
            a.scratch_bytes = 1 << 62
        assert fn(a, stream) == code, (f, bad)
        setattr(a, f, old)
        a.scratch_bytes = sb
    torch.cuda.synchronize()
    assert (t["frames"][:-4] == 7.0).all(), "a refused call must not launch"


def _task(n, over, device_clips):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(3)
    return parse_task(compose(list(over) + [f"env.num_envs={n}", "env.motion_file=synthetic:6:2"] + (["+env.clip_processing=device"] if device_clips else [])))


def _close(got, want, floor_fps=None, scale=4.0):
    a, b = got.double().cpu().numpy(), want.double().cpu().numpy()
    tol = cu.EPS32 * np.maximum(np.abs(b), 1.0) + (0.0 if floor_fps is None else cu.ANG_FLOOR * floor_fps / 30.0)
    return float((np.abs(a - b) / (scale * tol)).max())


@pytest.mark.parametrize("over", [(), ("robot=smpl_humanoid_shape",)], ids=["one_shape", "per_env_shapes"])
def test_option_end_to_end(over):
    """Two HumanoidIm tasks of 8 envs on the same multi-clip synthetic library and seed, one with `+env.clip_processing=device`: same draw, same shapes, records and
    lookups within 4x the per-field tolerances (the per-env heading is the same fp32 torch code on inputs at most one rounding apart); the device task then
    resamples twice and steps.  `per_env_shapes` is the real `robot=smpl_humanoid_shape` task (three compiled shapes, three skeleton trees: `clip_tree`)."""
    from phc_amd import motion_lib as ML
    (th, _), (td, env_d) = _task(8, over, False), _task(8, over, True)
    lh, ld = th._motion_lib, td._motion_lib
    assert ld.m_cfg["clip_processing"] == "device" and lh.m_cfg["clip_processing"] == "host" and not ML._POOL
    assert len(td.shape_models) == (3 if over else 1) and len({id(t) for t in td.skeleton_trees}) == len(td.shape_models)
    assert torch.equal(lh._curr_motion_ids, ld._curr_motion_ids) and lh.frames.shape == ld.frames.shape and len(set(lh._curr_motion_ids.tolist())) > 1
    assert torch.equal(lh._motion_num_frames, ld._motion_num_frames) and torch.equal(lh._motion_fps, ld._motion_fps)
    fps_frame = torch.repeat_interleave(lh._motion_fps, lh._motion_num_frames).double().cpu().numpy()
    cu.compare(ld.frames.cpu().numpy(), lh.frames.cpu().numpy(), fps_frame, scale=4.0, what=f"{'shapes' if over else 'plain'} task frames, device vs host:")
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 8, (64,), generator=g).to(DEV)
    times = (torch.rand(64, generator=g).to(DEV) * lh._motion_lengths[ids])
    sh, sd = lh.get_motion_state(ids, times), ld.get_motion_state(ids, times)
    fps = lh._motion_fps[ids].double().cpu().numpy()
    for k in ("root_pos", "root_rot", "rg_pos", "rb_rot", "body_vel", "root_vel", "dof_pos", "body_ang_vel", "root_ang_vel", "dof_vel"):
        floor = fps.reshape((-1,) + (1,) * (sh[k].dim() - 1)) if k in ("body_ang_vel", "root_ang_vel", "dof_vel") else None
        r = _close(sd[k], sh[k], floor)
        print(f"get_motion_state {k}: worst |diff| / (4 x tolerance) = {r:.3e}")
        assert r <= 1.0, k
    assert torch.equal(sd["motion_aa"], sh["motion_aa"])
    epoch = ld.frames_epoch
    td.resample_motions()
    td.resample_motions()
    assert ld.frames_epoch == epoch + 2 and not ML._POOL
    env_d.step(torch.zeros(8, td.num_dof, device=DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(td.obs_buf).all() and torch.isfinite(ld.frames).all()
