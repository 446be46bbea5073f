"""CPU checks of the offscreen renderer's host side (phc_amd/render.py) and of its fp64 oracle (tests/render_oracle.py):
  * the oracle against closed forms (sphere / capsule head-on, a plane hit, a ground point in a capsule's shadow);
  * the exclusion cap (at most 2 % of a view's pixels) on every committed test scene, and the 5 degree rule of their cameras;
  * a write_png round trip decoded with zlib;
  * the follow camera against the reference's _init_camera / _update_camera (humanoid.py:1715-1743);
  * the values of the renderer's header limits (the struct layouts: tests/test_abi_and_host.py)."""
import math
import os
import struct
import tempfile
import zlib

import numpy as np
import pytest

import render_oracle as ro
import host_build


def _style():
    from phc_amd import render
    return render.STYLE, render.PALETTE


def _one_body(capsule, pos=(0.0, 0.0, 0.0)):
    """A one-body scene: capsule [7] in the body frame, body at pos with the identity rotation."""
    bs = np.zeros((1, 13))
    bs[0, 0:3] = pos
    bs[0, 6] = 1.0
    return np.asarray([capsule], np.float64), np.zeros(1, np.int64), bs


def test_oracle_closed_forms_head_on():
    style, pal = _style()
    # sphere (a = b) of radius 0.2 at (0, 0, 1), seen head-on from 4 m: the one-pixel view's ray is the optical axis
    cap, own, bs = _one_body([0, 0, 0, 0, 0, 0, 0.2], pos=(0.0, 0.0, 1.0))
    cam = ((0.0, -4.0, 1.0), (0.0, 0.0, 1.0), (0.0, 0.0, 1.0), math.radians(40.0))
    o = ro.render_view(style, pal, cap, own, bs, cam, 1, 1)
    assert o["id"][0, 0] == 0 and abs(o["depth"][0, 0] - (4.0 - 0.2)) < 1e-12
    # capsule along x (a = -0.3, b = +0.3), radius 0.07, seen across its axis: distance - r; and end-on along its axis: distance - 0.3 - r
    cap, own, bs = _one_body([-0.3, 0, 0, 0.3, 0, 0, 0.07], pos=(1.0, 2.0, 1.5))
    o = ro.render_view(style, pal, cap, own, bs, ((1.0, -1.0, 1.5), (1.0, 2.0, 1.5), (0, 0, 1), 0.5), 1, 1)
    assert abs(o["depth"][0, 0] - (3.0 - 0.07)) < 1e-12
    o = ro.render_view(style, pal, cap, own, bs, ((4.0, 2.0, 1.5), (1.0, 2.0, 1.5), (0, 0, 1), 0.5), 1, 1)
    assert o["id"][0, 0] == 0 and abs(o["depth"][0, 0] - (3.0 - 0.3 - 0.07)) < 1e-12
    # the normal at the head-on hit faces the camera: lit = n . L, rgb = C (ambient + diffuse lit)
    n = np.array([1.0, 0.0, 0.0])
    v = np.asarray(pal[0]) * (style["ambient"] + style["diffuse"] * max(n @ np.asarray(style["light_dir"]), 0.0))
    assert np.array_equal(o["rgba"][0, 0, :3], np.floor(np.clip(v, 0, 1) * 255 + 0.5).astype(np.uint8))


def test_oracle_plane_hit():
    style, pal = _style()
    cap, own, bs = _one_body([0, 0, 0, 0, 0, 0, 0.1], pos=(50.0, 50.0, 1.0))      # far away, out of view
    h, ang = 1.3, math.radians(35.0)
    cam = ((0.25, 0.25, h), (0.25, 0.25 + math.cos(ang), h - math.sin(ang)), (0, 0, 1), 0.3)
    o = ro.render_view(style, pal, cap, own, bs, cam, 1, 1)
    t = h / math.sin(ang)
    assert o["id"][0, 0] == -2 and abs(o["depth"][0, 0] - t) < 1e-12
    y = 0.25 + t * math.cos(ang)                                                      # hit at (0.25, y, 0): cell parity (0 + floor(y)) & 1
    tone = np.asarray(style["ground_color"][int(math.floor(y)) & 1])
    v = tone * (style["ambient"] + style["diffuse"] * style["light_dir"][2])
    assert np.array_equal(o["rgba"][0, 0, :3], np.floor(np.clip(v, 0, 1) * 255 + 0.5).astype(np.uint8))
    # a ray that rises meets nothing: sky, +inf
    o = ro.render_view(style, pal, cap, own, bs, ((0, 0, 1), (0, 1, 1.5), (0, 0, 1), 0.3), 1, 1)
    assert o["id"][0, 0] == -1 and np.isinf(o["depth"][0, 0]) and np.array_equal(o["rgba"][0, 0, :3], np.floor(np.asarray(style["sky_color"]) * 255 + 0.5).astype(np.uint8))


def test_oracle_ground_point_in_a_capsule_shadow():
    style, pal = _style()
    L = np.asarray(style["light_dir"])
    g = np.array([0.5, 0.5, 0.0])                                                      # ground point straight down-light of the capsule
    c = g + 0.8 * L
    cap, own, bs = _one_body([-0.15, 0, 0, 0.15, 0, 0, 0.08], pos=tuple(c))
    cam = (tuple(g + np.array([0.0, -2.0, 2.0])), tuple(g), (0, 0, 1), 0.3)
    o = ro.render_view(style, pal, cap, own, bs, cam, 1, 1)
    assert o["id"][0, 0] == -2 and not o["excl_rgb"][0, 0]
    tone = np.asarray(style["ground_color"][0])                                        # (0.5, 0.5) lies in cell (0, 0)
    assert np.array_equal(o["rgba"][0, 0, :3], np.floor(tone * style["ambient"] * 255 + 0.5).astype(np.uint8))
    bs[0, 0:3] += np.array([0.0, 0.0, 5.0]) + 3.0 * np.cross(L, [0, 0, 1]) / np.linalg.norm(np.cross(L, [0, 0, 1]))   # moved aside: lit
    o = ro.render_view(style, pal, cap, own, bs, cam, 1, 1)
    v = tone * (style["ambient"] + style["diffuse"] * L[2])
    assert np.array_equal(o["rgba"][0, 0, :3], np.floor(v * 255 + 0.5).astype(np.uint8))


@pytest.mark.parametrize("name", ro.SCENES)
def test_exclusion_cap_holds_on_every_scene(name):
    """At most 2 % of the pixels of any view may be excluded (a condition on the committed inputs, checked with the oracle alone); every
    ground ray descends at >= 5 degrees, every other ray climbs at >= 5 degrees (no grazing ground rays); each view shows the humanoid."""
    sc = ro.make_scene(name)
    for markers in (True, False):
        for (env, cam), o in zip(sc["cameras"], ro.render_scene(sc, markers=markers)):
            frac, frac_rgb = o["excl"].mean(), o["excl_rgb"].mean()
            print(f"{name} env {env} markers {markers}: excluded {100 * frac:.3f} % (rgb {100 * frac_rgb:.3f} %)")
            assert frac_rgb <= 0.02 and frac <= 0.02
            down, up = ro.ground_ray_angles(cam, sc["W"], sc["H"])
            assert down >= 5.0 and up >= 5.0, (down, up)
            assert ((o["id"] >= 0) & (o["id"] < ro.MARKER_ID)).sum() > 100
            if markers:
                assert (o["id"] >= ro.MARKER_ID).any()
    if name == "smpl":
        assert len(sc["cameras"]) == 8
    if name == "g1":
        assert sc["body_state"].shape[1] == 38 and sc["capsules"].shape[1] == 42
    if name == "smpl_shape":
        assert sorted(set(sc["env_shape"][[e for e, _ in sc["cameras"]]].tolist())) == [0, 1, 2]


def _decode_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    W, H, depth, ctype = ihdr[:4]
    assert depth == 8 and ctype == 6
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 4 * W)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(H, W, 4)


def test_write_png_round_trip():
    from phc_amd.render import tile, write_png
    import torch
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        write_png(os.path.join(d, "a.png"), img)
        assert np.array_equal(_decode_png(os.path.join(d, "a.png")), img)
        frames = torch.from_numpy(rng.integers(0, 256, (5, 6, 7, 4), dtype=np.uint8))
        grid = tile(frames, 3)
        assert grid.shape == (12, 21, 4)
        write_png(os.path.join(d, "b.png"), grid)
        g = _decode_png(os.path.join(d, "b.png"))
        assert np.array_equal(g[6:12, 7:14], frames[4].numpy()) and (g[6:12, 14:21] == 0).all()


def test_follow_camera_reproduces_the_reference_placement():
    from phc_amd.render import Camera
    cam = Camera()
    roots = [np.array([0.3, -1.2, 0.9]), np.array([0.5, -1.0, 0.85]), np.array([2.0, 1.0, 0.7])]
    cam.follow(roots[0])                                                      # _init_camera
    assert np.allclose(cam.eye, [0.3, -4.2, 1.0]) and np.allclose(cam.target, [0.3, -1.2, 1.0])
    cam.eye = np.array([0.1, -4.0, 1.4])                                      # (the viewer moved the camera)
    prev = roots[0]
    for r in roots[1:]:                                                       # _update_camera
        want_eye = np.array([r[0] + cam.eye[0] - prev[0], r[1] + cam.eye[1] - prev[1], cam.eye[2]])
        cam.follow(r)
        assert np.allclose(cam.eye, want_eye) and np.allclose(cam.target, [r[0], r[1], 1.0])
        prev = r
    assert np.allclose(cam.eye, [0.1 + 2.0 - 0.3, -4.0 + 1.0 + 1.2, 1.4])


def test_render_struct_sizes_match_the_header():
    """The layouts themselves: tests/test_abi_and_host.py.  Here: the values the renderer's oracle and its documented limits rest on."""
    from phc_amd import _lib
    assert _lib.RENDER_PALETTE == 16 and _lib.RENDER_MARKER_ID == ro.MARKER_ID
    assert host_build.header_values("PHC_RENDER_MAX_PIXELS", "PHC_RENDER_MAX_SHAPES", "PHC_RENDER_MAX_MARKERS", "PHC_RENDER_PALETTE",
                                    "PHC_RENDER_MARKER_ID") == [1 << 24, 128, 128, 16, 1000]
