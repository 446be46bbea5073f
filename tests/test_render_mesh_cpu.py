"""CPU checks of the mesh renderer's host side (phc_amd/render_mesh.py) and of its fp64 oracle (tests/render_mesh_oracle.py):
  * the BVH builder's invariants (every triangle in exactly one leaf, child boxes inside the parent's, the skip chain from the root visits
    every node once and in order, the permutation a bijection), for leaf sizes 1 / 2 / 4 / 8 and on a flat mesh (zero-thickness boxes);
  * the STL loader on a binary and an ASCII file; the MJCF reader on both visual forms and its ValueErrors;
  * what the oracle and the BVH builder assume of the ctypes mirrors and limits (their layouts against the header: tests/test_abi_and_host.py);
  * the oracle against the analytic ellipsoid: an inscribed icosphere lies between the ellipsoid and the ellipsoid shrunk by the sphere's
    own faceting factor (an affine map keeps containment), so every depth lies between the two closed forms;
  * the exclusion caps on every committed scene, with the oracle alone: at most 5 % of a view excluded from id / depth, at most 10 % of its
    mesh-hit pixels excluded from RGB / tri_id, at least 500 compared mesh-hit pixels, and the 5 degree rule of the ground rays."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest

import render_mesh_oracle as rmo
import render_oracle as ro


# ---------------------------------------------------------------------------------------------------------------- files written by the tests
def write_stl(path, vertices, faces, ascii=False):
    tri = np.asarray(vertices, np.float32)[np.asarray(faces)]
    if ascii:
        with open(path, "w") as f:
            f.write("solid t\n")
            for t in tri:
                f.write(" facet normal 0 0 0\n  outer loop\n" + "".join(f"   vertex {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for p in t)
                        + "  endloop\n endfacet\n")
            f.write("endsolid t\n")
    else:
        with open(path, "wb") as f:
            f.write(b"\0" * 80 + struct.pack("<I", len(tri)))
            for t in tri:
                f.write(struct.pack("<12fH", 0.0, 0.0, 0.0, *t.reshape(-1).tolist(), 0))


def write_robot_mjcf(directory, body_names, rgb):
    """An MJCF with one visual ellipsoid mesh (binary and ASCII STLs in turn, written next to it) and one collision sphere per body name,
    the visual geoms through a default class of colour rgb.  -> its path"""
    os.makedirs(os.path.join(directory, "meshes"), exist_ok=True)
    write_stl(os.path.join(directory, "meshes", "blob.stl"), *rmo.ellipsoid(2, (0.08, 0.08, 0.14)))
    write_stl(os.path.join(directory, "meshes", "blob_ascii.stl"), *rmo.ellipsoid(1, (0.07, 0.07, 0.1)), ascii=True)
    bodies = "".join(f'<body name="{n}"><geom class="visual" mesh="{"blob" if k % 2 else "blob_ascii"}"/><geom type="sphere" size="0.05"/></body>'
                     for k, n in enumerate(body_names))
    path = os.path.join(directory, "robot.xml")
    with open(path, "w") as f:
        f.write(f'<mujoco><compiler meshdir="meshes"/><default><default class="visual"><geom type="mesh" contype="0" conaffinity="0" '
                f'rgba="{rgb[0]} {rgb[1]} {rgb[2]} 1"/></default></default><asset><mesh name="blob" file="blob.stl"/>'
                f'<mesh name="blob_ascii" file="blob_ascii.stl"/></asset><worldbody>{bodies}</worldbody></mujoco>')
    return path


def in_colour(img, rgb):
    """Pixels of an RGBA image that show the colour rgb at some shade between the ambient and the fully lit level."""
    from phc_amd import render as R
    st = R.STYLE
    rgb = np.asarray(rgb, np.float64)
    c = img[..., :3].astype(np.float64)
    lo, hi = rgb * st["ambient"] * 255 - 1.5, rgb * (st["ambient"] + st["diffuse"]) * 255 + 1.5
    shade = c[..., int(np.argmax(rgb))] / (255 * rgb.max())
    return (np.abs(c - shade[..., None] * 255 * rgb).max(-1) <= 1.5) & (c >= lo).all(-1) & (c <= hi).all(-1)


def _same_triangles(v, f, v2, f2):
    return np.array_equal(np.asarray(v, np.float32)[np.asarray(f)], v2[f2])


# ---------------------------------------------------------------------------------------------------------------- BVH
def _check_bvh(v, f, leaf_size):
    from phc_amd.render_mesh import build_bvh
    b = build_bvh(v, f, leaf_size)
    nodes, order = b["nodes"], b["order"]
    NN, NT = len(nodes), len(f)
    assert sorted(order.tolist()) == list(range(NT))                                   # the permutation is a bijection
    corners = np.asarray(v, np.float32)[np.asarray(f)][order]                          # triangles in leaf order
    seen = np.zeros(NT, int)
    end = lambda n: NN if nodes["skip"][n] < 0 else int(nodes["skip"][n])
    first_expected = 0
    for n in range(NN):
        assert n < end(n) <= NN
        lf = int(nodes["leaf"][n])
        if lf >= 0:
            first, count = lf >> 4, lf & 15
            assert 1 <= count <= leaf_size and first == first_expected and end(n) == n + 1   # leaves in increasing `first`
            first_expected += count
            seen[first:first + count] += 1
            tri = corners[first:first + count].reshape(-1, 3)
            assert np.array_equal(nodes["lo"][n], tri.min(0)) and np.array_equal(nodes["hi"][n], tri.max(0))   # exact fp32 bounds
        else:
            left, right = n + 1, end(n + 1)
            assert right < end(n) and end(right) == end(n)                             # two children filling the subtree
            for c in (left, right):
                assert (nodes["lo"][c] >= nodes["lo"][n]).all() and (nodes["hi"][c] <= nodes["hi"][n]).all()
            assert np.array_equal(np.minimum(nodes["lo"][left], nodes["lo"][right]), nodes["lo"][n])
    assert (seen == 1).all()                                                           # every triangle in exactly one leaf
    # the miss chain from the root with every box "hit": node + 1 below an interior node, skip after a leaf -> 0, 1, 2, ... NN - 1
    visit, n = [], 0
    while n >= 0:
        visit.append(n)
        n = n + 1 if nodes["leaf"][n] < 0 else int(nodes["skip"][n])
    assert visit == list(range(NN))
    # and with every box "missed" the root's skip ends the walk
    assert nodes["skip"][0] == -1
    c = b["center"].astype(np.float64)
    assert np.linalg.norm(np.asarray(v, np.float64)[np.unique(f)] - c, axis=1).max() <= b["radius"] * (1 + 1e-12)
    return b


@pytest.mark.parametrize("leaf_size", [1, 2, 4, 8])
def test_bvh_invariants(leaf_size):
    for v, f in (rmo.tetrahedron(0.5), rmo.cube(0.3), rmo.ellipsoid(2, (0.1, 0.1, 0.2)), rmo.quad_grid(0.5, 5),
                 (np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32), np.array([(0, 1, 2)]))):
        _check_bvh(v, f, leaf_size)


def test_bvh_of_a_flat_mesh_has_zero_thickness_boxes_and_coincident_centroids_split():
    b = _check_bvh(*rmo.quad_grid(0.5, 4), 4)
    assert (b["nodes"]["lo"][:, 2] == b["nodes"]["hi"][:, 2]).all()
    v = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32)
    _check_bvh(v, np.array([(0, 1, 2)] * 9), 2)                                        # nine copies of one triangle: no axis separates them


def test_mesh_set_concatenates_meshes_with_global_indices():
    from phc_amd.render_mesh import MeshSet
    ms = MeshSet(leaf_size=2)
    m0 = ms.add_mesh(*rmo.cube(0.3))
    m1 = ms.add_mesh(*rmo.tetrahedron(0.4))
    ms.add_instance(m1, 3, pos=(0.1, 0.2, 0.3), rgb=(0.1, 0.2, 0.3))
    ms.add_instance(m0, 5)
    ms.add_instance(m1, 3)
    v, t, p, n = ms.arrays()
    assert len(v) == 12 and len(t) == 16 and sorted(p.tolist()) == list(range(16))
    faces = np.concatenate([rmo.cube(0.3)[1], rmo.tetrahedron(0.4)[1] + 8])
    assert np.array_equal(t, faces[p])                                                 # tri_perm maps leaf order back to the caller's order
    root1 = ms.meshes[m1][0]
    assert root1 == len(ms.nodes[0]) and n["skip"][root1] == -1 and n["skip"][0] == -1
    sub = n[root1:]
    assert ((sub["skip"] == -1) | (sub["skip"] > root1)).all() and (sub["leaf"][sub["leaf"] >= 0] >> 4).min() == 12
    arr = ms.instance_array()
    assert [arr[i].owner for i in range(3)] == [3, 5, 3] and [arr[i].root for i in range(3)] == [root1, 0, root1]
    assert list(arr[0].quat) == [0.0, 0.0, 0.0, 1.0] and arr[0].radius > 0


# ---------------------------------------------------------------------------------------------------------------- loaders
def test_stl_loader_reads_binary_and_ascii(tmp_path):
    from phc_amd.render_mesh import load_stl
    v, f = rmo.ellipsoid(1, (0.1, 0.15, 0.2))
    for ascii in (False, True):
        p = tmp_path / f"m{int(ascii)}.stl"
        write_stl(p, v, f, ascii=ascii)
        v2, f2 = load_stl(str(p))
        assert v2.dtype == np.float32 and f2.dtype == np.int32 and f2.shape == (len(f), 3)
        assert len(v2) == len(v)                                                       # duplicates merged
        assert _same_triangles(v, f, v2, f2)                                           # the same triangles, in file order
    (tmp_path / "bad.stl").write_text("solid x\nendsolid x\n")
    with pytest.raises(ValueError, match="bad.stl"):
        load_stl(str(tmp_path / "bad.stl"))


MJCF = """<mujoco model="t">
  <compiler angle="radian" meshdir="{meshdir}"/>
  <default>
    <geom rgba="0.1 0.2 0.3 1"/>
    <default class="visual"><geom type="mesh" contype="0" conaffinity="0" rgba="0.7 0.6 0.5 1"/></default>
    <default class="collision"><geom type="capsule"/></default>
  </default>
  <asset>{assets}</asset>
  <worldbody>
    <body name="pelvis" pos="0 0 1">
      <freejoint/>
      {pelvis}
      <body name="torso" pos="0 0 0.2">
        {torso}
      </body>
    </body>
  </worldbody>
</mujoco>
"""


def _write_mjcf(tmp_path, pelvis, torso, assets='<mesh name="a" file="a.stl"/><mesh name="b" file="b.STL" scale="2 2 2"/>', meshdir="meshes",
                stl=("a.stl", "b.STL")):
    os.makedirs(tmp_path / "meshes", exist_ok=True)
    for s in stl:
        write_stl(tmp_path / "meshes" / s, *rmo.tetrahedron(0.2))
    p = tmp_path / "robot.xml"
    p.write_text(MJCF.format(meshdir=meshdir, assets=assets, pelvis=pelvis, torso=torso))
    return str(p)


def test_mjcf_reader_finds_both_visual_forms(tmp_path):
    from phc_amd.render_mesh import read_mjcf_visuals
    path = _write_mjcf(tmp_path,
                       pelvis='<geom type="mesh" mesh="a" contype="0" conaffinity="0" pos="0.1 0.2 0.3" quat="0.5 0.5 -0.5 0.5" rgba="0.9 0.8 0.7 1"/>'
                              '<geom type="mesh" mesh="a"/> <geom type="sphere" size="0.1"/>',
                       torso='<geom class="visual" mesh="b"/> <geom class="collision" size="0.05" fromto="0 0 0 0 0 0.1"/>')
    vis = read_mjcf_visuals(path)
    assert [(g["body"], os.path.basename(g["file"])) for g in vis] == [("pelvis", "a.stl"), ("torso", "b.STL")]
    assert np.allclose(vis[0]["pos"], [0.1, 0.2, 0.3]) and np.allclose(vis[0]["quat"], [0.5, -0.5, 0.5, 0.5])   # wxyz -> xyzw
    assert np.allclose(vis[0]["rgba"], [0.9, 0.8, 0.7, 1]) and np.allclose(vis[1]["rgba"], [0.7, 0.6, 0.5, 1])
    assert np.allclose(vis[1]["scale"], 2) and np.allclose(vis[1]["quat"], [0, 0, 0, 1]) and os.path.dirname(vis[0]["file"]) == str(tmp_path / "meshes")


def test_mjcf_reader_errors_name_the_file_or_body(tmp_path):
    from phc_amd.render_mesh import read_mjcf_visuals, task_mesh_set
    path = _write_mjcf(tmp_path, pelvis='<geom type="mesh" mesh="a"/>', torso='<geom class="collision" size="0.05" fromto="0 0 0 0 0 0.1"/>')
    with pytest.raises(ValueError, match="robot.xml.*no visual mesh"):
        read_mjcf_visuals(path)
    path = _write_mjcf(tmp_path, pelvis='<geom class="visual" mesh="a"/>', torso='<geom class="visual" mesh="b"/>', stl=("a.stl",))
    os.remove(tmp_path / "meshes" / "b.STL")                                           # (the first call above wrote it)
    with pytest.raises(ValueError, match="b.STL.*torso"):
        read_mjcf_visuals(path)

    class Task:
        _body_names = ["pelvis", "chest"]
        has_shape_variation = False
        device = "cpu"
    path = _write_mjcf(tmp_path, pelvis='<geom class="visual" mesh="a"/>', torso='<geom class="visual" mesh="b"/>')
    with pytest.raises(ValueError, match="body torso"):
        task_mesh_set(Task(), path)
    Task.has_shape_variation = True
    with pytest.raises(ValueError, match="has_shape_variation"):
        task_mesh_set(Task(), path)
    Task.has_shape_variation = False
    with pytest.raises(ValueError, match="mesh_color"):
        task_mesh_set(Task(), path, color="blue")
    with pytest.raises(ValueError, match="nowhere.xml"):
        task_mesh_set(Task(), str(tmp_path / "nowhere.xml"))


# ---------------------------------------------------------------------------------------------------------------- ctypes mirrors
def test_mesh_struct_layouts_match_the_header():
    """The layouts and the macros against the header: tests/test_abi_and_host.py.  Here: what the oracle and the BVH builder assume of them."""
    from phc_amd import _lib
    assert _lib.RENDER_MESH_ID == rmo.MESH_ID and rmo.MIN_CROSS == _lib.RENDER_MESH_MIN_CROSS
    assert _lib.RENDER_MAX_INSTANCES >= 128 and _lib.RENDER_MAX_TRIANGLES >= 1 << 22
    assert C.sizeof(_lib.BvhNode) == 32 and C.sizeof(_lib.MeshInstance) == 64
    from phc_amd.render_mesh import build_bvh
    assert build_bvh(*rmo.cube(1.0))["nodes"].dtype.itemsize == 32


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _ellipsoid_depth(o, d, c, semi):
    """First entry of rays into the axis-aligned ellipsoid at c (nan on a miss): the unit-sphere solve in scaled coordinates."""
    q, e = (o - c) / semi, d / semi
    a, b, cc = np.einsum("nk,nk->n", e, e), np.einsum("nk,nk->n", q, e), np.einsum("nk,nk->n", q, q) - 1.0
    disc = b * b - a * cc
    with np.errstate(invalid="ignore"):
        return np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.nan)


def test_oracle_against_the_analytic_ellipsoid():
    from phc_amd import render
    semi = np.array([0.1, 0.1, 0.2])
    uv, uf = rmo.icosphere(3)
    shrink = np.abs(np.einsum("tk,tk->t", uv[uf[:, 0]], np.cross(uv[uf[:, 1]] - uv[uf[:, 0]], uv[uf[:, 2]] - uv[uf[:, 0]]))
                    / np.linalg.norm(np.cross(uv[uf[:, 1]] - uv[uf[:, 0]], uv[uf[:, 2]] - uv[uf[:, 0]]), axis=1)).min()
    assert 0.99 < shrink < 1.0                                                          # the unit icosphere contains the sphere of this radius
    mesh = rmo.ellipsoid(3, semi)
    bs = np.zeros((1, 13))
    bs[0, 0:3], bs[0, 6] = (0.5, 0.25, 1.0), 1.0
    c = bs[0, 0:3]
    caps, own = np.array([[0, 0, 0, 0, 0, 0, 0.1]]), np.zeros(1, np.int64)              # (body 0's capsule: suppressed by the instance)
    inst = [dict(mesh=0, owner=0, pos=np.zeros(3, np.float32), quat=np.array([0, 0, 0, 1], np.float32), rgb=np.array([0.5, 0.6, 0.7], np.float32))]
    cam = rmo.orbit(c, 1.5, 35.0, 25.0)
    W, H = 160, 120
    o = rmo.render_view(render.STYLE, render.PALETTE, caps, own, bs, cam, W, H, [mesh], inst)
    d = ro.camera_rays(*cam, W, H).reshape(-1, 3)
    eye = np.broadcast_to(np.asarray(cam[0], np.float64), d.shape)
    semi32 = np.abs(mesh[0]).max(0).astype(np.float64)                                  # (the fp32 vertices' own semi-axes)
    outer = _ellipsoid_depth(eye, d, c, semi32 * (1 + 1e-6)).reshape(H, W)
    inner = _ellipsoid_depth(eye, d, c, semi32 * shrink * (1 - 1e-6)).reshape(H, W)
    hit = o["id"] == rmo.MESH_ID
    assert hit.sum() > 300 and (o["id"][~hit] < 0).all()
    assert not (hit & np.isnan(outer)).any()                                            # a mesh hit lies inside the ellipsoid
    assert hit[~np.isnan(inner)].all()                                                  # the shrunk ellipsoid lies inside the mesh
    assert (o["depth"][hit] >= outer[hit]).all()
    m = hit & ~np.isnan(inner)
    assert (o["depth"][m] <= inner[m]).all()
    print(f"faceting: shrink {shrink:.5f}, max depth gap {np.nanmax((inner - outer)[m]):.2e} m")
    assert ((o["tri"] >= 0) == hit).all() and o["tri"].max() < 1280
    # flat shading: the colour of a lit, unshadowed hit is rgb * (ambient + diffuse * n . L) with the face normal of its triangle
    v, f = mesh
    L = np.asarray(render.STYLE["light_dir"])
    ys, xs = np.nonzero(hit & ~o["excl_rgb"])
    for y, x in list(zip(ys, xs))[::37]:
        t = v[f[o["tri"][y, x]]].astype(np.float64)
        n = np.cross(t[1] - t[0], t[2] - t[0])
        n /= np.linalg.norm(n)                                                           # outward: the camera is outside a convex mesh
        want = np.asarray(inst[0]["rgb"], np.float64) * (render.STYLE["ambient"] + render.STYLE["diffuse"] * max(n @ L, 0.0))
        assert np.array_equal(o["rgba"][y, x, :3], np.floor(np.clip(want, 0, 1) * 255 + 0.5).astype(np.uint8))


def test_oracle_single_triangle_closed_form_and_two_sidedness():
    from phc_amd import render
    tri = (np.array([(-0.5, -0.5, 0), (0.5, -0.5, 0), (0, 0.5, 0)], np.float32), np.array([(0, 1, 2)]))
    bs = np.zeros((1, 13))
    bs[0, 0:3], bs[0, 6] = (0.0, 0.0, 1.0), 1.0
    caps, own = np.array([[0, 0, 0, 0, 0, 0, 0.1]]), np.zeros(1, np.int64)
    inst = [dict(mesh=0, owner=0, pos=np.zeros(3, np.float32), quat=np.array([0, 0, 0, 1], np.float32), rgb=np.array([1.0, 1.0, 1.0], np.float32))]
    st = render.STYLE
    for eye_z, lit in ((3.0, st["light_dir"][2]), (0.2, 0.0)):                          # from above: lit by n = +z; from below: n = -z faces away
        o = rmo.render_view(st, render.PALETTE, caps, own, bs, ((0.0, 0.0, eye_z), (0.0, 0.0, 1.0), (0, 1, 0), 0.3), 1, 1, [tri], inst)
        assert o["id"][0, 0] == rmo.MESH_ID and o["tri"][0, 0] == 0 and abs(o["depth"][0, 0] - abs(eye_z - 1.0)) < 1e-12
        assert o["rgba"][0, 0, 0] == math.floor((st["ambient"] + st["diffuse"] * lit) * 255 + 0.5)
    # the ground under the triangle is in its shadow; a degenerate triangle is never hit
    g = np.array([0.0, 0.0, 0.0]) - 1.0 * np.asarray(st["light_dir"]) / st["light_dir"][2]   # the point the light sees through (0, 0, 1)
    o = rmo.render_view(st, render.PALETTE, caps, own, bs, ((g[0], g[1] - 1.0, 2.0), tuple(g), (0, 0, 1), 0.2), 1, 1, [tri], inst)
    assert o["id"][0, 0] == -2 and o["rgba"][0, 0, 0] == math.floor(st["ground_color"][int(math.floor(g[0]) + math.floor(g[1])) & 1][0] * st["ambient"] * 255 + 0.5)
    flat = (np.array([(-0.5, 0, 0), (0.5, 0, 0), (0, 0, 0)], np.float32), np.array([(0, 1, 2)]))
    o = rmo.render_view(st, render.PALETTE, caps, own, bs, ((0.0, 0.0, 3.0), (0.0, 0.0, 1.0), (0, 1, 0), 0.3), 1, 1, [flat], inst)
    assert o["id"][0, 0] == -2


@pytest.mark.parametrize("name", rmo.SCENES)
def test_exclusion_caps_hold_on_every_scene(name):
    """Conditions on the committed inputs, checked with the oracle alone (so the GPU comparison cannot hide a failure behind exclusions)."""
    sc = rmo.make_scene(name)
    for (env, cam), o in zip(sc["cameras"], rmo.render_scene(name)):
        mesh = o["id"] >= rmo.MESH_ID
        frac = o["excl"].mean()
        frac_mesh = (o["excl_rgb"] & mesh).sum() / max(1, mesh.sum())
        compared = (mesh & ~o["excl_rgb"]).sum()
        print(f"{name} env {env}: excluded {100 * frac:.2f} % of the view, {100 * frac_mesh:.2f} % of {mesh.sum()} mesh-hit pixels, compared {compared}")
        assert frac <= 0.05 and frac_mesh <= 0.10 and compared >= 500
        down, up = ro.ground_ray_angles(cam, sc["W"], sc["H"])
        assert down >= 5.0 and up >= 5.0, (down, up)
        assert cam[0][2] > 0.05
    ids = np.concatenate([o["id"].reshape(-1) for o in rmo.render_scene(name)])
    if name == "h1_mixed":
        own = sc["owner"][0]
        caps_seen = {int(own[i]) for i in np.unique(ids[(ids >= 0) & (ids < ro.MARKER_ID)])}
        assert caps_seen == {4} and len(sc["instances"]) == sc["body_state"].shape[1] - 1     # the one body left to its capsules shows them
    if name == "g1_all":
        assert len(sc["instances"]) == 39 and [i["owner"] for i in sc["instances"]].count(0) == 2 and not ((ids >= 0) & (ids < ro.MARKER_ID)).any()
        assert (ids == rmo.MESH_ID + 38).any()
    if name == "ico5":
        assert len(sc["meshes"][0][1]) == 20480
    if name == "frames_far":
        assert np.abs(sc["body_state"][1, 0, 0:2]).max() == 8.0 and len({i["mesh"] for i in sc["instances"]}) == 1
    if name == "axis":
        d = ro.camera_rays(*sc["cameras"][0][1], sc["W"], sc["H"])
        assert (sc["W"], sc["H"]) == (161, 121) and np.array_equal(d[60, 80], [0.0, 0.0, -1.0])
