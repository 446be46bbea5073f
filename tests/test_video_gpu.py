"""Video output on the device: phc_jpeg_encode through the C ABI on the cases of tests/video_util.py, against the fp64 transform (a) and the entropy decoder (b)
under the rules of tests/test_video_cpu.py, and the product path -- `+render.format=avi` in play and in the clip viewer -- read back with the RIFF walker.
Whether the device's bytes equal the host build's is printed per case; they need not (the two builds may round a tie coefficient differently)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import video_util as vu

pytestmark = pytest.mark.gpu
PAD = 256


def _lib():
    from phc_amd import _lib as L
    return L, L.load()


class Guarded:
    """`nbytes` of device memory, 16-byte aligned, inside an allocation filled with a guard byte."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.base = torch.full((self.n + 2 * PAD + 16,), vu.GUARD, dtype=torch.uint8, device="cuda")
        self.off = PAD + (-(self.base.data_ptr() + PAD)) % 16
        self.ptr = self.base.data_ptr() + self.off

    def bytes(self):
        return self.base[self.off:self.off + self.n]

    def intact(self):
        return bool((self.base[:self.off] == vu.GUARD).all()) and bool((self.base[self.off + self.n:] == vu.GUARD).all())

    def untouched(self):
        return bool((self.base == vu.GUARD).all())


def device_args(rgba, quality, ri, want_coef=True, row_pad=0):
    """phc_jpeg_args_t over guarded device buffers for rgba uint8 [F, H, W, 4] (numpy) -> (args, buffers, things to keep alive)."""
    L, lib = _lib()
    F, H, W = rgba.shape[:3]
    src = np.full((F, H, 4 * W + row_pad), 0x3C, dtype=np.uint8)
    src[:, :, :4 * W] = rgba.reshape(F, H, 4 * W)
    dsrc = torch.from_numpy(src).cuda()
    q = np.ascontiguousarray(vu.qtables(quality), dtype=np.uint8)
    nm = ((W + 15) // 16) * ((H + 15) // 16)
    bound, need = lib.phc_jpeg_frame_bound(W, H, ri), lib.phc_jpeg_scratch_bytes(F, W, H, ri)
    bufs = dict(out=Guarded(F * bound), length=Guarded(4 * F), coef=Guarded(F * 6 * nm * 128), scratch=Guarded(need))
    a = L.JpegArgs()
    a.num_frames, a.width, a.height, a.restart_interval = F, W, H, ri
    a.row_stride, a.frame_stride = 4 * W + row_pad, (4 * W + row_pad) * H
    a.rgba, a.qtab, a.out, a.out_stride, a.length = dsrc.data_ptr(), q.ctypes.data, bufs["out"].ptr, bound, bufs["length"].ptr
    a.coef, a.scratch, a.scratch_bytes = (bufs["coef"].ptr if want_coef else None), bufs["scratch"].ptr, need
    return a, bufs, (dsrc, q)


def device_encode(rgba, quality, ri, want_coef=True, row_pad=0):
    """-> (scans, coef [F, 6 M, 64] or None, guards intact)"""
    L, lib = _lib()
    a, bufs, keep = device_args(rgba, quality, ri, want_coef, row_pad)
    rc = lib.phc_jpeg_encode(C.byref(a), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, rc
    F = rgba.shape[0]
    n = bufs["length"].bytes().cpu().numpy().view(np.int32)
    out = bufs["out"].bytes().cpu().numpy()
    assert (n >= 0).all() and (n <= a.out_stride).all()
    scans = [out[f * a.out_stride:f * a.out_stride + n[f]].tobytes() for f in range(F)]
    coef = bufs["coef"].bytes().cpu().numpy().view(np.int16).reshape(F, -1, 64) if want_coef else None
    if not want_coef:
        assert bufs["coef"].untouched()
    return scans, coef, all(b.intact() for b in bufs.values())


@pytest.mark.parametrize("name", list(vu.CASES))
def test_device_matches_both_oracles(name):
    img, quality, ri, expect = vu.CASES[name]
    rgb = img()
    rgba = vu.rgba_of(rgb)[None]
    scans, coef, intact = device_encode(rgba, quality, ri)
    assert intact, "guard bytes around out / length / coef / scratch"
    vu.check_frame(name, rgb, quality, ri, scans[0], coef[0], expect)
    host, hcoef, _ = vu.host_encode(rgba, quality, ri)
    print(f"{name}: device bytes {'equal' if host == scans else 'differ from'} the host build's; {int((hcoef != coef).sum())} coefficients differ")


def test_frames_strides_and_the_nullable_output_on_the_device():
    """F = 3 distinct frames in one call give what three calls give (offsets and lengths per frame); a padded row stride and coef = NULL change nothing;
    repeats are byte-identical."""
    imgs = [vu.scene(40, 24), vu.noise(40, 24, 7), vu.gradient(40, 24)]
    rgba = np.stack([vu.rgba_of(i, s) for s, i in enumerate(imgs)])
    scans, coef, intact = device_encode(rgba, 90, 2)
    assert intact and len({len(s) for s in scans}) == 3
    for f in range(3):
        one, c1, ok = device_encode(rgba[f:f + 1], 90, 2)
        assert ok and one[0] == scans[f] and (c1[0] == coef[f]).all()
        again, _, _ = device_encode(rgba[f:f + 1], 90, 2)
        assert again == one
        vu.check_frame(f"frame {f}", imgs[f], 90, 2, scans[f], coef[f])
    padded, _, ok = device_encode(rgba, 90, 2, row_pad=20)
    plain, none, ok2 = device_encode(rgba, 90, 2, want_coef=False)
    assert padded == scans and plain == scans and none is None and ok and ok2


def test_refused_arguments_launch_nothing():
    from test_video_cpu import EINVAL_CASES
    L, lib = _lib()
    rgba = vu.rgba_of(vu.noise(20, 12))[None].repeat(2, axis=0)
    for what, spoil in EINVAL_CASES.items():
        a, bufs, keep = device_args(rgba, 90, 2)
        qtab = {"q": keep[1].reshape(-1)}
        spoil(a, qtab)
        assert lib.phc_jpeg_encode(C.byref(a), torch.cuda.current_stream().cuda_stream) == -1, what
        torch.cuda.synchronize()
        assert all(b.untouched() for b in bufs.values()), what
    a, bufs, keep = device_args(rgba, 90, 2)
    a.num_frames = 0
    assert lib.phc_jpeg_encode(C.byref(a), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs.values())


def test_encode_frames_takes_strided_views():
    """phc_amd.video.encode_frames on a view into a larger device tensor (the renderer's tiles): complete files that decoder (b) reads back to the coefficients
    of the fp64 transform, equal to what the C ABI gives for the packed copy."""
    from phc_amd import video
    big = torch.from_numpy(vu.rgba_of(vu.scene(80, 48))).cuda()
    view = big[8:40, 16:64]                                              # [32, 48, 4], rows 320 bytes apart
    rgba = view.cpu().numpy()
    files = video.encode_frames(view, quality=75)
    scans, coef, _ = device_encode(np.ascontiguousarray(rgba)[None], 75, video.DEFAULT_RESTART_INTERVAL)
    assert files == [vu.header(48, 32, 75, video.DEFAULT_RESTART_INTERVAL) + scans[0] + b"\xff\xd9"]
    assert (vu.decode(files[0])["coef"] == coef[0]).all()
    with pytest.raises(RuntimeError, match="HIP device"):
        video.encode_frames(view.cpu())


# ---------------------------------------------------------------------------------------------------------------- the product path
W, H = 64, 48
BASE = ["test=True", "games=5", "env.num_envs=2", "env.motion_file=synthetic:2:0"]


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@pytest.fixture(scope="module")
def plays(tmp_path_factory):
    """phc_amd.run.main in player mode on 2 SMPL envs: without recording, with PNG frames by default and by name, as AVI, as both."""
    from phc_amd import run
    root = tmp_path_factory.mktemp("plays")
    out = {}
    for name, extra in (("none", None), ("default", []), ("png", ["+render.format=png"]), ("avi", ["+render.format=avi"]),
                        ("both", ["+render.format=both", "+render.quality=60"])):
        d = root / name
        rec = [] if extra is None else ["+render.video=" + str(d), "+render.envs=2", f"+render.width={W}", f"+render.height={H}"] + extra
        info = run.main(BASE + [f"output_path={root / ('out_' + name)}"] + rec)
        out[name] = (info, _files(d) if extra is not None else {})
    return out


def test_play_statistics_do_not_depend_on_recording(plays):
    for name in ("default", "png", "avi", "both"):
        assert plays[name][0] == plays["none"][0], name


def test_png_is_the_default_and_both_adds_to_it(plays):
    pngs = [f"frame_{i:06d}.png" for i in range(5)]
    assert sorted(plays["default"][1]) == pngs
    assert plays["png"][1] == plays["default"][1], "render.format=png writes what no key writes"
    both = plays["both"][1]
    assert {f: both[f] for f in pngs} == plays["default"][1] and len(both) == 6
    assert [f for f in plays["avi"][1] if not f.endswith(".avi")] == [] and len(plays["avi"][1]) == 1


@pytest.mark.parametrize("name,quality", [("avi", 90), ("both", 60)])
def test_play_avi_is_well_formed(plays, name, quality, tmp_path):
    from phc_amd import video
    (fname, data), = [(f, b) for f, b in plays[name][1].items() if f.endswith(".avi")]
    p = tmp_path / "play.avi"
    p.write_bytes(data)
    frames = vu.check_avi(str(p), 2 * W, H, 30, 5)                       # two envs side by side, fps = 1 / dt
    head = video.jpeg_header(2 * W, H, quality, video.DEFAULT_RESTART_INTERVAL)
    for f in frames:
        got = vu.decode(f)
        assert f.startswith(head) and (got["width"], got["height"]) == (2 * W, H) and got["ri"] == video.DEFAULT_RESTART_INTERVAL
        assert np.abs(got["coef"][:, 1:]).sum() > 0, "a rendered frame is not flat"
    assert len(set(frames)) > 1, "the humanoid moves"


def test_recording_avi_leaves_the_simulation_bit_identical(tmp_path):
    from test_render_gpu import _task
    runs = []
    for rec in (False, True):
        extra = ["+render.video=" + str(tmp_path / "v"), "+render.envs=2", f"+render.width={W}", f"+render.height={H}", "+render.format=avi"] if rec else []
        task, env = _task(2, extra)
        torch.manual_seed(1)
        env.reset()
        g = torch.Generator(device=task.device).manual_seed(7)
        out = []
        for _ in range(6):
            act = (torch.rand(task.num_envs, task.num_actions, device=task.device, generator=g) * 2 - 1) * 0.5
            obs, rew, done, _ = env.step(act)
            task.render()
            out.append((obs.clone(), rew.clone(), done.clone(), task.reset_buf.clone(), task._rigid_body_state_reshaped.clone()))
        torch.cuda.synchronize()
        task.close()
        runs.append(out)
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), f"step {k}"
    avis = [f for f in os.listdir(tmp_path / "v")]
    assert len(avis) == 1 and avis[0].endswith(".avi")
    vu.check_avi(str(tmp_path / "v" / avis[0]), 2 * W, H, 30, 6)


def test_viewer_codes_each_chunk_in_one_call(tmp_path):
    """view_motion with render.format=both on a synthetic library: the AVI's frames are the JPEG files of the PNG frames it wrote next to it, `video` names the
    file, and format=avi alone writes no PNG."""
    from phc_amd import video
    from phc_amd import view_motion as vm
    from test_render_gpu import _png_rgba
    argv = ["env.motion_file=synthetic:3:0", f"+render.width={W}", f"+render.height={H}", "+replay.clips=2", "+replay.frames=5",
            "+render.video=" + str(tmp_path / "b"), "+render.format=both"]
    task = vm.make_task(argv)
    out = vm.main(argv, task=task)
    assert out["frames"] == 5 and os.path.dirname(out["video"]) == str(tmp_path / "b") and out["video"].endswith(".avi")
    frames = vu.check_avi(out["video"], 2 * W, H, 30, 5)
    pngs = sorted(f for f in os.listdir(tmp_path / "b") if f.endswith(".png"))
    assert pngs == [f"frame_{i:06d}.png" for i in range(5)]
    imgs = np.stack([_png_rgba(tmp_path / "b" / f) for f in pngs])
    assert video.encode_frames(torch.from_numpy(imgs).cuda()) == frames
    for f in frames:
        assert vu.decode(f)["width"] == 2 * W
    # the same task under the other two settings of the key (the viewer reads them from the task's config on every call)
    task.cfg["render"]["video"], task.cfg["render"]["format"] = str(tmp_path / "a"), "avi"
    only = vm.main(argv, task=task)
    assert os.listdir(tmp_path / "a") == [os.path.basename(only["video"])] and vu.check_avi(only["video"], 2 * W, H, 30, 5) == frames
    task.cfg["render"]["video"] = str(tmp_path / "p")
    del task.cfg["render"]["format"]
    plain = vm.main(argv, task=task)
    assert "video" not in plain and _files(tmp_path / "p") == {f: open(tmp_path / "b" / f, "rb").read() for f in pngs}
