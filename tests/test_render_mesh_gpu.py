"""phc_render_mesh (csrc/phc_render_mesh.hip) on the MI355X against the fp64 oracle of tests/render_mesh_oracle.py, on the non-excluded pixels:
  * hit_id and tri_id exact;  * |depth - oracle| <= 1 mm;  * RGB within +-1 level;
plus: no meshes = phc_render's bytes, byte-identical repeats over 36 views, sentinel padding around all four outputs, PHC_EINVAL without a
launch, and `+render.meshes` through phc_amd.run.main.

The kernel's fp32 depth bound for a triangle hit (U = 2^-24; scenes within |x| <= 10 m of the origin, camera-to-hit distances T <= 8 m, mesh
bounding radii and geom offsets <= 0.35 m, triangle corner angles between 30 and 150 degrees; every number is derived from the arithmetic, not
fitted to the kernel's output).  The capsule, marker and ground hits keep the bound of tests/test_render_gpu.py.
  * inputs: body states, geom frames, vertices and cameras are fp32 in both.
  * posing an instance: the frame origin p_body + rot(q_body, pos) is two additions at <= 10 m: <= 10 m * 2 U = 1.2e-6 m; the composed and
    normalised quaternion carries <= ~10 U of relative error, which moves a mesh point at an arm <= 0.35 m by <= 0.35 * 20 U = 4e-7 m.
  * the ray: d carries <= ~10 U = 6e-7 of direction error (test_render_gpu.py): over T = 8 m, <= 4.8e-6 m sideways.
  * the shape-centred origin: tc = (c - o) . d has <= 3 * 10 m * 2 U + 8 m * 6e-7 = 8.4e-6 m of error ALONG the ray, which t = tc + s inherits
    once; p = (o - c) + tc d is formed from differences of <= 8 m: <= ~1.5e-6 m in each direction; its rotation into the mesh frame and the
    added mesh-frame centre (numbers <= 0.35 m) add <= 0.35 m * 8 U = 2e-7 m.
  * so the mesh-frame ray is the true ray moved sideways by eps <= 1.2e-6 + 4e-7 + 4.8e-6 + 1.5e-6 + 2e-7 ~ 8e-6 m.  On the triangle's plane
    that moves the hit along the ray by eps * tan(incidence) <= eps / |d . n|.
  * the triangle solve s = e2 . (tv x e1) / det, det = -d . (e1 x e2): the numerator is a sum of products of three lengths <= |tv| |e1| |e2|
    with <= ~12 U of relative rounding, det >= |d . n| |e1| |e2| sin(corner angle): <= 12 U * 0.7 m / (|d . n| * 0.5) = 1e-6 m / |d . n|.
  Total: <= 8.4e-6 + (8e-6 + 1e-6) / |d . n|.  The oracle excludes hits with |d . n| < GRAZE; GRAZE = 0.02 gives 8.4e-6 + 4.5e-4 ~ 4.6e-4 m, under
  half of the 1 mm bound (GRAZE = 0.01 would give 9.1e-4 m: no room).  At GRAZE = 0.02 the excluded band is 0.04 % of a sphere's disc.
  (Solved with the camera origin taken into the mesh frame instead, tv would carry 8 m * U = 4.8e-7 m per component before the cancellation
  to a <= 0.7 m vector, and s would lose ~8 U * 8 m / |d . n|: 2.4e-4 m more at the threshold.)"""
import os

import numpy as np
import pytest
import torch

import render_mesh_oracle as rmo
import render_oracle as ro
from test_render_gpu import SentBuf, _cams, _lib, _png_rgba, _upload

pytestmark = pytest.mark.gpu
EINVAL = -1


def _mesh_set(sc, leaf_size=None):
    from phc_amd import render_mesh as RM
    ms = RM.MeshSet(**({"leaf_size": leaf_size} if leaf_size else {}))
    for v, f in sc["meshes"]:
        ms.add_mesh(v, f)
    for i in sc["instances"]:
        ms.add_instance(i["mesh"], i["owner"], i["pos"], i["quat"], i["rgb"])
    return ms.upload("cuda")


def _run(sc, ms, markers=True, tri=True):
    L, lib = _lib()
    scene, keep = _upload(sc, markers)
    V, H, W = len(sc["cameras"]), sc["H"], sc["W"]
    bufs = [SentBuf((V, H, W, 4), torch.uint8), SentBuf((V, H, W), torch.float32), SentBuf((V, H, W), torch.int32), SentBuf((V, H, W), torch.int32)]
    rc = lib.phc_render_mesh(scene, ms.struct if ms is not None else None, _cams(L, sc), V, W, H, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr,
                             bufs[3].ptr if tri else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    for b, n in zip(bufs, ("rgba", "depth", "hit_id", "tri_id")):
        b.check(n)
    if not tri:
        assert bufs[3].untouched()
    return [b.t.cpu().numpy() for b in bufs]


@pytest.mark.parametrize("name", rmo.SCENES)
def test_render_mesh_matches_the_fp64_oracle(name):
    sc = rmo.make_scene(name)
    rgba, dep, ids, tri = _run(sc, _mesh_set(sc))
    for v, o in enumerate(rmo.render_scene(name)):
        keep, keep_rgb = ~o["excl"], ~o["excl_rgb"]
        bad_id = (ids[v] != o["id"]) & keep
        bad_tri = (tri[v] != o["tri"]) & keep_rgb
        fin = np.isfinite(o["depth"])
        both = keep & fin & (ids[v] == o["id"])
        derr = np.zeros(o["depth"].shape)
        derr[both] = np.abs(dep[v][both].astype(np.float64) - o["depth"][both])
        rerr = np.where(keep_rgb[..., None], np.abs(rgba[v, ..., :3].astype(np.int64) - o["rgba"][..., :3].astype(np.int64)), 0)
        mesh = o["id"] >= rmo.MESH_ID
        print(f"{name} view {v}: excluded {keep.size - keep.sum()} px, mesh-hit {mesh.sum()} (compared {(mesh & keep_rgb).sum()}), id mismatches "
              f"{int(bad_id.sum())}, tri mismatches {int(bad_tri.sum())}, max |depth err| {derr.max():.3e} m (mesh {derr[mesh].max() if mesh.any() else 0:.3e}), "
              f"max rgb err {int(rerr.max())}")
        assert not bad_id.any(), f"{name} view {v}: hit_id differs at {np.argwhere(bad_id)[:5].tolist()}"
        assert not bad_tri.any(), f"{name} view {v}: tri_id differs at {np.argwhere(bad_tri)[:5].tolist()}"
        assert (np.isinf(dep[v]) == ~fin)[keep].all()
        assert derr.max() <= 1e-3
        assert rerr.max() <= 1
        assert (rgba[v, ..., 3] == 255).all()
        assert ((tri[v] >= 0) == (ids[v] >= rmo.MESH_ID)).all()                      # on every pixel: a triangle id exactly where a mesh is hit


@pytest.mark.parametrize("leaf_size", [1, 4, 8])
def test_other_leaf_sizes_give_the_same_ids(leaf_size):
    sc = rmo.make_scene("frames_far")
    a = _run(sc, _mesh_set(sc))
    b = _run(sc, _mesh_set(sc, leaf_size))
    keep = np.stack([~o["excl"] for o in rmo.render_scene("frames_far")])
    assert np.array_equal(a[2][keep], b[2][keep]) and np.array_equal(a[3][keep], b[3][keep])


def test_without_meshes_the_outputs_are_phc_renders():
    """meshes == NULL and a mesh set with zero instances: rgba / depth / hit_id byte-identical to phc_render's on the committed h1 scene."""
    from phc_amd import render_mesh as RM
    import test_render_gpu as trg
    sc = ro.make_scene("h1")
    ref = trg._run(sc)
    empty = RM.MeshSet()
    empty.add_mesh(*rmo.tetrahedron(0.3))
    empty.upload("cuda")
    assert empty.struct.num_instances == 0
    for ms in (None, empty):
        got = _run(sc, ms)
        for x, y in zip(ref, got[:3]):
            assert x.tobytes() == y.tobytes()
        assert (got[3] == -1).all()
    assert _run(sc, None, tri=False)[0].tobytes() == ref[0].tobytes()


def test_render_mesh_is_deterministic_and_covers_many_views():
    sc = dict(rmo.make_scene("g1_all"))
    sc["cameras"] = sc["cameras"] * 18          # 36 views: three launches of up to 16
    ms = _mesh_set(sc)
    a = _run(sc, ms)
    b = _run(sc, ms)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert all(np.array_equal(a[k][v], a[k][v % 2]) for v in range(36) for k in (2, 3))


def test_invalid_mesh_arguments_return_einval_without_a_launch():
    L, lib = _lib()
    sc = rmo.make_scene("tetra")
    scene, keep = _upload(sc)
    ms = _mesh_set(sc)
    cams = _cams(L, sc)
    V, H, W = len(sc["cameras"]), sc["H"], sc["W"]
    st = torch.cuda.current_stream().cuda_stream
    bufs = [SentBuf((V, H, W, 4), torch.uint8), SentBuf((V, H, W), torch.float32), SentBuf((V, H, W), torch.int32), SentBuf((V, H, W), torch.int32)]

    def call(scene_=scene, meshes_=ms.struct, cams_=cams, v=V, w=W, h=H, out=bufs[0].ptr, tri=bufs[3].ptr):
        return lib.phc_render_mesh(scene_, meshes_, cams_, v, w, h, out, bufs[1].ptr, bufs[2].ptr, tri, st)
    # everything phc_render refuses
    assert call(scene_=None) == EINVAL and call(cams_=None) == EINVAL and call(out=None) == EINVAL
    assert call(v=0) == EINVAL and call(v=-1) == EINVAL and call(w=0) == EINVAL and call(h=-5) == EINVAL
    assert call(w=4097, h=4096) == EINVAL and call(out=bufs[0].ptr + 1) == EINVAL and call(tri=bufs[3].ptr + 2) == EINVAL
    bad = _cams(L, sc)
    bad[1].env = sc["body_state"].shape[0]
    assert call(cams_=bad) == EINVAL
    bad[1].env = -1
    assert call(cams_=bad) == EINVAL
    for field, value in (("body_state", None), ("capsules", None), ("num_capsules", 0), ("num_capsules", L.RENDER_MAX_SHAPES + 1),
                         ("num_markers", L.RENDER_MAX_MARKERS + 1), ("num_markers", -1), ("markers", None), ("num_bodies", 0),
                         ("num_bodies", 65), ("num_shape_blocks", 0), ("capsule_stride", 8), ("num_envs", 0)):
        s2, _ = _upload(sc)
        setattr(s2, field, value)
        assert call(scene_=s2) == EINVAL, field
        assert call(scene_=s2, meshes_=None) == EINVAL, field
    # the mesh set's own
    import ctypes as C

    def variant(**kw):
        m = L.RenderMeshes()
        C.memmove(C.byref(m), C.byref(ms.struct), C.sizeof(m))
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    for field in ("vertices", "triangles", "tri_perm", "nodes", "instances_dev"):
        assert call(meshes_=variant(**{field: None})) == EINVAL, field                 # a null array with a non-zero count
    assert call(meshes_=variant(instances=C.POINTER(L.MeshInstance)())) == EINVAL
    for field, value in (("num_instances", -1), ("num_instances", L.RENDER_MAX_INSTANCES + 1), ("num_triangles", 0),
                         ("num_triangles", L.RENDER_MAX_TRIANGLES + 1), ("num_vertices", 0), ("num_nodes", 0),
                         ("num_nodes", 2 * L.RENDER_MAX_TRIANGLES + 1), ("nodes", ms.struct.nodes + 4)):
        assert call(meshes_=variant(**{field: value})) == EINVAL, (field, value)
    for field, value in (("owner", -1), ("owner", sc["body_state"].shape[1]), ("root", -1), ("root", ms.struct.num_nodes)):
        arr = ms.instance_array()
        setattr(arr[0], field, value)
        assert call(meshes_=variant(instances=C.cast(arr, C.POINTER(L.MeshInstance)))) == EINVAL, (field, value)
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)
    assert call() == 0                                        # and the same arguments, corrected, render
    torch.cuda.synchronize()
    assert not bufs[0].untouched() and not bufs[3].untouched()


def test_player_records_with_meshes_and_identical_statistics(tmp_path):
    """phc_amd.run.main(test=True games=8 +render.video=DIR +render.meshes=MJCF) on an untrained H1 agent, with an MJCF and STLs written here
    (one ellipsoid per body, one colour): 8 PNGs, the statistics of the run without the key, and pixels in the instances' colour."""
    from phc_amd import run
    from phc_amd.config import compose
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    import test_render_mesh_cpu as cpu
    over = ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"]
    names = list(HumanoidIm.host_only(compose(["env.num_envs=2", *over]))._body_names)
    rgb = (0.1, 0.9, 0.2)
    mjcf = cpu.write_robot_mjcf(str(tmp_path), names, rgb)
    base = ["test=True", "games=8", "env.num_envs=16", "env.motion_file=synthetic:2:0", f"output_path={tmp_path / 'out'}", *over]
    ref = run.main(list(base))
    d = tmp_path / "video"
    got = run.main(base + ["+render.video=" + str(d), "+render.width=200", "+render.height=150", "+render.meshes=" + str(mjcf)])
    assert got == ref
    pngs = sorted(f for f in os.listdir(d) if f.endswith(".png"))
    assert pngs == [f"frame_{i:06d}.png" for i in range(8)]
    for f in pngs:
        img = _png_rgba(d / f)
        assert img.shape == (150, 200, 4)
        match = cpu.in_colour(img, rgb)
        assert match.sum() > 200, f"{f}: {match.sum()} pixels in the instances' colour"
