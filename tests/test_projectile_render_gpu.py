"""-m gpu: the renderer's per-marker radii and colours (phc_render_scene_t.marker_radii / marker_colors; the recorder draws thrown projectiles with them).
With both arrays NULL a frame is the frame of the scene without the two fields (tests/test_render_gpu.py and tests/test_render_mesh_gpu.py hold those to their
oracles unchanged); here: arrays that repeat marker_radius / marker_color give the NULL frame byte for byte, through phc_render and through phc_render_mesh, and a scene with the
reference markers plus two projectiles of another radius and colour against an fp64 per-marker variant of render_oracle.render_view, under test_render_gpu.py's
rules (hit ids bit-exact, depth within 1 mm, RGB within one level, outside the oracle's exclusions)."""
import numpy as np
import pytest
import torch

import render_oracle as ro
import test_render_gpu as tr

pytestmark = pytest.mark.gpu


def _run(sc, radii=None, colors=None):
    import phc_amd.render as R
    L, lib = tr._lib()
    scene, keep = tr._upload(sc, True)
    if radii is not None:
        keep["radii"] = torch.from_numpy(np.asarray(radii, np.float32)).cuda()
        keep["colors"] = torch.from_numpy(np.ascontiguousarray(colors, np.float32)).cuda()
        scene = R.scene_struct(keep["caps"], sc["body_state"].shape[0], sc["body_state"].shape[1], keep["bs"], env_shape=keep["env_shape"], markers=keep["mk"],
                               marker_radius=R.MARKER_RADIUS, marker_radii=keep["radii"], marker_colors=keep["colors"])
    V, H, W = len(sc["cameras"]), sc["H"], sc["W"]
    rgba, dep, ids = tr.SentBuf((V, H, W, 4), torch.uint8), tr.SentBuf((V, H, W), torch.float32), tr.SentBuf((V, H, W), torch.int32)
    assert lib.phc_render(scene, tr._cams(L, sc), V, W, H, rgba.ptr, dep.ptr, ids.ptr, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for b, n in ((rgba, "rgba"), (dep, "depth"), (ids, "hit_id")):
        b.check(n)
    return rgba.t.cpu().numpy(), dep.t.cpu().numpy(), ids.t.cpu().numpy()


def render_view_per_marker(sc, env, cam, radii, colors):
    """render_oracle.render_view with a radius and a colour per marker, from its own pieces: marker m becomes a capsule with a = b = 0 owned by an extra body
    NB + m that sits at the marker (identity rotation) and is coloured by an extended palette; its hit id S + m is renamed MARKER_ID + m."""
    import phc_amd.render as R
    nb, S, M = sc["body_state"].shape[1], sc["capsules"].shape[1], sc["markers"].shape[1]
    caps = np.concatenate([sc["capsules"][0], np.concatenate([np.zeros((M, 6)), np.asarray(radii, np.float64)[:, None]], axis=1)])
    owner = np.concatenate([sc["owner"][0], nb + np.arange(M)])
    extra = np.zeros((M, 13))
    extra[:, 0:3], extra[:, 6] = sc["markers"][env], 1.0
    bodies = np.concatenate([sc["body_state"][env].astype(np.float64), extra])
    palette = [R.PALETTE[(i % 16) % len(R.PALETTE)] for i in range(nb)] + [tuple(c) for c in np.asarray(colors, np.float64)]
    o = ro.render_view(R.STYLE, palette, caps, owner, bodies, cam, sc["W"], sc["H"], markers=None)
    o["id"] = np.where(o["id"] >= S, o["id"] - S + ro.MARKER_ID, o["id"])
    return o


def _scene():
    sc = ro.make_scene("smpl")
    sc["cameras"] = sc["cameras"][:4]
    root = sc["body_state"][1, 0, 0:3]
    proj = np.stack([root + np.array([0.45, 0.10, 0.25]), root + np.array([-0.30, 0.40, -0.35])]).astype(np.float32)   # one beside the chest, one by the legs
    mk = np.concatenate([sc["markers"], np.broadcast_to(proj, (sc["markers"].shape[0], 2, 3))], axis=1)
    sc["markers"] = np.ascontiguousarray(mk, np.float32)
    return sc


def test_uniform_arrays_give_the_null_frame():
    import phc_amd.render as R
    sc = _scene()
    M = sc["markers"].shape[1]
    null = _run(sc)
    same = _run(sc, [R.MARKER_RADIUS] * M, [R.STYLE["marker_color"]] * M)
    for a, b, name in zip(null, same, ("rgba", "depth", "hit_id")):
        assert a.tobytes() == b.tobytes(), name
    assert (null[2] >= ro.MARKER_ID).any(), "markers in view"
    with pytest.raises(ValueError, match="per marker"):
        _run(sc, [0.1] * (M - 1), [R.STYLE["marker_color"]] * M)


def test_uniform_arrays_give_the_null_frame_through_the_mesh_renderer():
    """phc_render_mesh poses its markers in its own kernel: one mesh scene with markers in view, NULL arrays against arrays that repeat the scene's values,
    and against arrays that do not."""
    import phc_amd.render as R
    import render_mesh_oracle as rmo
    import test_render_mesh_gpu as tm
    L, lib = tr._lib()
    sc = rmo.make_scene("h1_mixed")
    ms = tm._mesh_set(sc)
    M = sc["markers"].shape[1]

    def run(radii, colors):
        scene, keep = tr._upload(sc, True)
        if radii is not None:
            keep["radii"] = torch.tensor(radii, dtype=torch.float32, device="cuda")
            keep["colors"] = torch.tensor(colors, dtype=torch.float32, device="cuda")
            scene.marker_radii, scene.marker_colors = keep["radii"].data_ptr(), keep["colors"].data_ptr()
        V, H, W = len(sc["cameras"]), sc["H"], sc["W"]
        bufs = [tr.SentBuf((V, H, W, 4), torch.uint8), tr.SentBuf((V, H, W), torch.float32), tr.SentBuf((V, H, W), torch.int32)]
        assert lib.phc_render_mesh(scene, ms.struct, tr._cams(L, sc), V, W, H, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        for b in bufs:
            b.check("mesh frame")
        return [b.t.cpu().numpy() for b in bufs]
    null = run(None, None)
    same = run([R.MARKER_RADIUS] * M, [list(R.STYLE["marker_color"])] * M)
    assert (null[2] >= ro.MARKER_ID).any(), "markers in view"
    for a, b, name in zip(null, same, ("rgba", "depth", "hit_id")):
        assert a.tobytes() == b.tobytes(), name
    other = run([2 * R.MARKER_RADIUS] * M, [list(R.PROJECTILE_COLOR)] * M)
    assert (other[2] >= ro.MARKER_ID).sum() > (null[2] >= ro.MARKER_ID).sum() and other[0].tobytes() != null[0].tobytes(), "the arrays are read"


def test_per_marker_radius_and_colour_match_the_fp64_oracle():
    import phc_amd.render as R
    sc = _scene()
    M = sc["markers"].shape[1]
    radii = [R.MARKER_RADIUS] * (M - 2) + [0.1, 0.1]
    colors = [R.STYLE["marker_color"]] * (M - 2) + [R.PROJECTILE_COLOR] * 2
    rgba, dep, ids = _run(sc, radii, colors)
    seen = 0
    for v, (env, cam) in enumerate(sc["cameras"]):
        o = render_view_per_marker(sc, env, cam, radii, colors)
        keep, keep_rgb = ~o["excl"], ~o["excl_rgb"]
        bad_id = (ids[v] != o["id"]) & keep
        fin = np.isfinite(o["depth"])
        both = keep & fin & (ids[v] == o["id"])
        derr = np.zeros(o["depth"].shape)
        derr[both] = np.abs(dep[v][both].astype(np.float64) - o["depth"][both])
        rerr = np.where(keep_rgb[..., None], np.abs(rgba[v, ..., :3].astype(np.int64) - o["rgba"][..., :3].astype(np.int64)), 0)
        proj_px = int((o["id"] >= ro.MARKER_ID + M - 2).sum())
        seen += proj_px
        print(f"view {v}: excluded {keep.size - keep.sum()} px, id mismatches {int(bad_id.sum())}, max |depth err| {derr.max():.3e} m, max rgb err {int(rerr.max())}, "
              f"{proj_px} px of projectiles")
        assert not bad_id.any(), f"view {v}: hit_id differs at {np.argwhere(bad_id)[:5].tolist()}"
        assert (np.isinf(dep[v]) == ~fin)[keep].all()
        assert derr.max() <= 1e-3 and rerr.max() <= 1
    assert seen > 200, "the projectiles must be in view"


def test_recorder_draws_the_projectiles():
    """A task with `+projectile`: the frame's marker list is the reference markers (when asked for) plus one entry per slot, with the sphere's radius."""
    import phc_amd.render as R
    from test_projectile_gpu import PROJ, _task
    task, env = _task(PROJ + ["+projectile.count=2"])
    env.reset()
    for _ in range(8):
        task.step(torch.zeros(task.num_envs, task.num_dof, device=task.device))
    marks, radii, colors = R.projectile_markers(task.ref_body_pos, task._proj.pos, task._proj.opt.radius)
    M0 = task.ref_body_pos.shape[1]
    assert marks.shape == (task.num_envs, M0 + 2, 3) and torch.equal(marks[:, M0:], task._proj.pos.permute(1, 0, 2))
    assert radii.tolist() == pytest.approx([R.MARKER_RADIUS] * M0 + [0.1, 0.1]) and colors[M0:].flatten().tolist() == pytest.approx(list(R.PROJECTILE_COLOR) * 2)
    cam = R.Camera()
    root = task._humanoid_root_states[0, 0:3]
    cam.follow(root.cpu().numpy())
    # slot 0 of env 0 next to the chest, slot 1 parked: the frame shows marker 0 and not marker 1
    task._proj.pos[0, 0] = root + torch.tensor([0.0, 0.0, 0.9], device=task.device)
    task._proj.pos[1, 0] = torch.tensor([0.0, 0.0, -1000.0], device=task.device)
    a, ids = R.render_envs(task, [0], [cam], 160, 120, markers=False, hit_id=True)
    ids = ids.cpu().numpy()
    assert int(task._proj.thrown) > 0 and a.shape == (1, 120, 160, 4)
    assert set(np.unique(ids)) <= set(range(-2, 64)) | {ro.MARKER_ID}, "without reference markers the projectiles are markers 0 and 1; a parked one is out of sight"
    assert (ids == ro.MARKER_ID).sum() > 10, "the projectile above the head is drawn"
    grey = a.cpu().numpy()[0][ids[0] == ro.MARKER_ID][:, :3].astype(int)
    assert (np.abs(grey - grey[:, :1]).max() <= 1), "in a neutral grey"
    assert len(task._proj.marker_cache) == 1
    R.render_envs(task, [0], [cam], 160, 120, markers=False)
    assert len(task._proj.marker_cache) == 1, "radii and colours are uploaded once per task"
