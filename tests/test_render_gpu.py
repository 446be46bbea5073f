"""phc_render (csrc/phc_render.hip) on the MI355X against the fp64 oracle of tests/render_oracle.py, on the non-excluded pixels:
  * hit_id bit-exact;
  * |depth - oracle| <= 1 mm (1 mm is about 1/20 of a pixel footprint at these cameras, so a larger error would be visible);
  * RGB within +-1 level (rounding at the .5 boundary is the only expected difference);
plus byte-identical repeat calls, sentinel padding around every output, PHC_EINVAL without a launch, and non-interference with the task.

The kernel's fp32 depth bound (U = 2^-24, the unit roundoff; scenes within |x| <= 8 m of the origin, camera-to-hit distances T <= 8 m,
capsule half-lengths and radii <= 0.3 m; every number below is a bound derived from the arithmetic, not a fit to the kernel's output):
  * inputs: body positions, capsule ends and cameras are fp32 in both (the oracle reads the same fp32 values).  Posing a capsule (quaternion
    rotation of an end of <= 0.3 m plus the body position <= 8 m) costs <= 8 m * 3 U + 0.3 m * 10 U ~ 1.6e-6 m in its centre / axis.
  * the ray: f, r, u and the pixel offsets are unit-size values with a few roundings each, so d carries <= ~10 U = 6e-7 of direction error;
    over T = 8 m that moves the ray by <= 4.8e-6 m sideways.
  * the shape-centred solve: tc = (c - o) . d has <= 3 * 8 m * 2 U + 8 m * 6e-7 ~ 6e-6 m of error along the ray, which t = tc + s inherits
    one to one; p = o + tc d - c has |p| <= R <= 0.6 m, so the quadratic's coefficients are products of numbers <= 0.6 m and its rounding
    moves the root by <= 4 U R^2 / (2 sqrt(disc)).  Off a silhouette by >= DELTA = 1e-4 m (the oracle's exclusion), sqrt(disc) >=
    sqrt(r DELTA) >= 1.4e-3 m (r >= 0.02 m): <= 4 U 0.36 / 2.8e-3 ~ 3e-5 m.  The lateral error eps = 4.8e-6 + 1.6e-6 m of the ray moves the
    root by <= eps * r / sqrt(r DELTA) = eps * sqrt(r / DELTA) <= eps * 55 (r <= 0.3 m) = 3.5e-4 m.
  * the ground: t = -o.z / d.z with |d.z| >= sin 5 degrees (the 5 degree rule of the committed cameras): relative error <= U + 10 U / sin 5
    = 116 U ~ 7e-6, times T <= 8 m: <= 6e-5 m.
  Total: <= 6e-6 + 3e-5 + 3.5e-4 (+ 6e-5 on the ground) ~ 4.5e-4 m < 1 mm.  (Solved from the camera origin instead, the quadratic's constant
  |o - c|^2 - r^2 would carry 64 m^2 * U ~ 4e-6 m^2 of rounding, i.e. up to ~2 mm of depth next to silhouettes: over the bound.)"""
import os

import numpy as np
import pytest
import torch

import render_oracle as ro

pytestmark = pytest.mark.gpu

PAD = 256   # sentinel elements in front of and behind every output (a multiple of 4 bytes: the kernel stores one 32-bit word per pixel)
SENT = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A, torch.float32: 0x7FC0DEAD}
VIEW = {torch.uint8: torch.uint8, torch.int32: torch.int32, torch.float32: torch.int32}


class SentBuf:
    """An output tensor inside a sentinel-filled allocation (uint8 / int32 / float32): `t` is the view the kernel writes, `check()` asserts
    that the padding came back unchanged."""

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.base = torch.empty(PAD + n + PAD, dtype=dtype, device="cuda")
        self.base.view(VIEW[dtype]).fill_(SENT[dtype])
        self.t = self.base[PAD:PAD + n].view(*shape)
        self.n = n

    @property
    def ptr(self):
        return self.base.data_ptr() + PAD * self.base.element_size()

    def check(self, what=""):
        bits = self.base.view(VIEW[self.base.dtype])
        s = SENT[self.base.dtype]
        assert bool((bits[:PAD] == s).all()) and bool((bits[PAD + self.n:] == s).all()), f"{what}: write outside the buffer"

    def untouched(self):
        return bool((self.base.view(VIEW[self.base.dtype]) == SENT[self.base.dtype]).all())


def _lib():
    from phc_amd import _lib as L
    return L, L.load()


def _upload(sc, markers=True):
    import phc_amd.render as R
    dev = "cuda"
    K = sc["capsules"].shape[0]
    tab = np.concatenate([sc["capsules"], sc["owner"][..., None].astype(np.float32)], axis=-1).reshape(K, -1)
    keep = dict(caps=torch.from_numpy(np.ascontiguousarray(tab, np.float32)).to(dev),
                bs=torch.from_numpy(sc["body_state"]).to(dev),
                env_shape=torch.from_numpy(sc["env_shape"]).to(dev) if sc["env_shape"] is not None else None,
                mk=torch.from_numpy(sc["markers"]).to(dev) if markers else None)
    scene = R.scene_struct(keep["caps"], sc["body_state"].shape[0], sc["body_state"].shape[1], keep["bs"], env_shape=keep["env_shape"],
                           markers=keep["mk"], marker_radius=R.MARKER_RADIUS)
    return scene, keep


def _cams(L, sc):
    cams = (L.Camera * len(sc["cameras"]))()
    for i, (env, (eye, tgt, up, fov)) in enumerate(sc["cameras"]):
        cams[i].env = env
        cams[i].eye[:], cams[i].target[:], cams[i].up[:] = [float(v) for v in eye], [float(v) for v in tgt], [float(v) for v in up]
        cams[i].fov_y = float(fov)
    return cams


def _run(sc, markers=True):
    L, lib = _lib()
    scene, keep = _upload(sc, markers)
    V, H, W = len(sc["cameras"]), sc["H"], sc["W"]
    rgba, dep, ids = SentBuf((V, H, W, 4), torch.uint8), SentBuf((V, H, W), torch.float32), SentBuf((V, H, W), torch.int32)
    rc = lib.phc_render(scene, _cams(L, sc), V, W, H, rgba.ptr, dep.ptr, ids.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for b, n in ((rgba, "rgba"), (dep, "depth"), (ids, "hit_id")):
        b.check(n)
    return rgba.t.cpu().numpy(), dep.t.cpu().numpy(), ids.t.cpu().numpy()


def _compare(name, sc, markers):
    rgba, dep, ids = _run(sc, markers)
    ref = ro.render_scene(sc, markers=markers)
    for v, o in enumerate(ref):
        keep, keep_rgb = ~o["excl"], ~o["excl_rgb"]
        bad_id = (ids[v] != o["id"]) & keep
        fin = np.isfinite(o["depth"])
        both = keep & fin & (ids[v] == o["id"])
        derr = np.zeros(o["depth"].shape)
        derr[both] = np.abs(dep[v][both].astype(np.float64) - o["depth"][both])
        rerr = np.where(keep_rgb[..., None], np.abs(rgba[v, ..., :3].astype(np.int64) - o["rgba"][..., :3].astype(np.int64)), 0)
        print(f"{name} view {v} markers {markers}: excluded {keep.size - keep.sum()} px, id mismatches {int(bad_id.sum())}, "
              f"max |depth err| {derr.max():.3e} m, max rgb err {int(rerr.max())}")
        assert not bad_id.any(), f"{name} view {v}: hit_id differs at {np.argwhere(bad_id)[:5].tolist()}"
        assert (np.isinf(dep[v]) == ~fin)[keep].all()
        assert derr.max() <= 1e-3
        assert rerr.max() <= 1
        assert (rgba[v, ..., 3] == 255).all()


@pytest.mark.parametrize("name,markers", [("smpl", True), ("smpl", False), ("h1", True), ("g1", True), ("smpl_shape", True)])
def test_render_matches_the_fp64_oracle(name, markers):
    sc = ro.make_scene(name)
    if name == "smpl":
        assert len(sc["cameras"]) == 8
    _compare(name, sc, markers)


def test_render_is_deterministic_and_covers_many_views():
    sc = ro.make_scene("g1")
    sc["cameras"] = sc["cameras"] * 9          # 36 views: three launches of up to 16
    a = _run(sc)
    b = _run(sc)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert all(np.array_equal(a[2][v], a[2][v % 4]) for v in range(36))


def test_invalid_arguments_return_einval_without_a_launch():
    L, lib = _lib()
    sc = ro.make_scene("h1")
    scene, keep = _upload(sc)
    cams = _cams(L, sc)
    V, H, W = len(sc["cameras"]), sc["H"], sc["W"]
    st = torch.cuda.current_stream().cuda_stream
    rgba, dep, ids = SentBuf((V, H, W, 4), torch.uint8), SentBuf((V, H, W), torch.float32), SentBuf((V, H, W), torch.int32)
    EINVAL = -1

    def call(scene_=scene, cams_=cams, v=V, w=W, h=H, out=rgba.ptr):
        return lib.phc_render(scene_, cams_, v, w, h, out, dep.ptr, ids.ptr, st)
    assert call(scene_=None) == EINVAL
    assert call(cams_=None) == EINVAL
    assert call(out=None) == EINVAL
    assert call(v=0) == EINVAL and call(v=-1) == EINVAL
    assert call(w=0) == EINVAL and call(h=-5) == EINVAL
    assert call(w=4097, h=4096) == EINVAL                    # W * H above PHC_RENDER_MAX_PIXELS
    assert call(out=rgba.ptr + 1) == EINVAL                  # not 4-byte aligned
    bad = _cams(L, sc)
    bad[1].env = sc["body_state"].shape[0]                   # env out of range
    assert call(cams_=bad) == EINVAL
    bad[1].env = -1
    assert call(cams_=bad) == EINVAL
    for field, value in (("body_state", None), ("capsules", None), ("num_capsules", 0), ("num_capsules", L.RENDER_MAX_SHAPES + 1),
                         ("num_markers", L.RENDER_MAX_MARKERS + 1), ("num_markers", -1), ("markers", None), ("num_bodies", 0),
                         ("num_bodies", 65), ("num_shape_blocks", 0), ("capsule_stride", 8), ("num_envs", 0)):
        s2, _ = _upload(sc)
        setattr(s2, field, value)
        assert call(scene_=s2) == EINVAL, field
    torch.cuda.synchronize()
    assert rgba.untouched() and dep.untouched() and ids.untouched()
    assert call() == 0                                        # and the same arguments, corrected, render
    torch.cuda.synchronize()
    assert not rgba.untouched()


def _task(n, extra=()):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    cfg = compose([f"env.num_envs={n}", "env.motion_file=synthetic:4:0"] + list(extra))
    return parse_task(cfg)


def test_recording_does_not_change_the_simulation(tmp_path):
    """A 4096-env VecEnv.step sequence with render() recording between steps gives bit-identical obs, reward and reset buffers to the same
    sequence without it."""
    runs = []
    for rec in (False, True):
        extra = ["+render.video=" + str(tmp_path / "frames"), "+render.envs=4", "+render.width=160", "+render.height=120",
                 "+render.markers=True"] if rec else []
        task, env = _task(4096, extra)
        torch.manual_seed(1)
        env.reset()
        g = torch.Generator(device=task.device).manual_seed(7)
        out = []
        for _ in range(12):
            act = (torch.rand(task.num_envs, task.num_actions, device=task.device, generator=g) * 2 - 1) * 0.5
            obs, rew, done, _ = env.step(act)
            task.render()
            out.append((obs.clone(), rew.clone(), done.clone(), task.reset_buf.clone()))
            ids = done.nonzero(as_tuple=False).flatten()
            if len(ids):
                env.reset(ids)
        torch.cuda.synchronize()
        task.close()
        runs.append(out)
        del task, env
    for k, (a, b) in enumerate(zip(*runs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), f"step {k}"
    frames = sorted(os.listdir(tmp_path / "frames"))
    assert len([f for f in frames if f.endswith(".png")]) == 12


def _png_rgba(path):
    import test_render_cpu as trc
    return trc._decode_png(path)


def test_player_records_frames_with_identical_statistics(tmp_path):
    """phc_amd.run.main(test=True games=20 +render.video=DIR) on an untrained agent: 20 PNGs of the requested size showing the humanoid,
    and the same statistics as the run without +render.video."""
    from phc_amd import run
    from phc_amd import render as R
    base = ["test=True", "games=20", "env.num_envs=16", "env.motion_file=synthetic:2:0", f"output_path={tmp_path / 'out'}"]
    ref = run.main(list(base))
    d = tmp_path / "video"
    got = run.main(base + ["+render.video=" + str(d), "+render.width=200", "+render.height=150"])
    assert got == ref
    pngs = sorted(f for f in os.listdir(d) if f.endswith(".png"))
    assert pngs == [f"frame_{i:06d}.png" for i in range(20)]
    # background colours: the two ground tones lit or in shadow (the ground's normal is +z: lit = L.z) and the sky
    st = R.STYLE
    bg = [np.floor(np.clip(np.asarray(c) * s, 0, 1) * 255 + 0.5) for c in st["ground_color"]
          for s in (st["ambient"], st["ambient"] + st["diffuse"] * st["light_dir"][2])] + [np.floor(np.asarray(st["sky_color"]) * 255 + 0.5)]
    for f in pngs:
        img = _png_rgba(d / f)
        assert img.shape == (150, 200, 4)
        rgb = img[..., :3].astype(np.int64)
        near_bg = np.zeros(rgb.shape[:2], bool)
        for c in bg:
            near_bg |= (np.abs(rgb - c).max(-1) <= 1)
        assert (~near_bg).sum() > 200, f"{f}: no humanoid pixels"
