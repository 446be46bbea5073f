"""Kinematic clip viewer: plays a clip library through the offscreen renderer, without simulating (the counterpart of the reference's
scripts/vis/vis_motion_mj.py for headless hosts).

    python -m phc_amd.view_motion env.motion_file=<clips> [robot=... env=... sim=... control=...] +render.video=out \\
           [+replay.keys=[k1,k2] | +replay.clips=4] [+replay.compare=<other clips>] [+replay.fps=30] [+replay.frames=N] \\
           [+render.meshes=<mjcf>] [+render.markers=True] [+render.follow=True] [+render.width=.. +render.height=..] \\
           [+render.format=avi|both +render.quality=90]     # one Motion-JPEG <name>-<date>.avi, coded on the device (phc_amd/video.py)

Tiles: `replay.clips` = the first k clips of the library (default 1), or the clips named by `replay.keys`; one tile each.  Frame i shows the
library's own get_motion_state at t = i / fps; a clip shorter than the longest holds its last frame.  The positions, rotations and velocities
are packed into a [rows, NB, 13] body-state block that the renderer reads in place of rigid_body_state; the robots' extended bodies are drawn
as markers.  Frames are rendered in chunks: F_chunk x tiles rows are the "envs" of one scene, with one lookup, one render call, one copy of
the root track to the host (for the follow cameras) and one copy of the images back per chunk.  No stepper, reset or post-physics launch is
issued: the task is built for its model, capsules and motion-library class only.

`replay.compare=<other clips>` loads a second library, matches clips by key and draws each pair side by side under the same camera (the
first library's root); it reports per clip `compare_mm`, the mean distance of corresponding bodies over the frames both clips have."""
import math
import os
import sys

import numpy as np
import torch

CHUNK_VIEWS = 64   # views of one render call: F_chunk = CHUNK_VIEWS // tiles frames (at least 1)


# ---------------------------------------------------------------------------------------------------------------- pure helpers
def select_keys(all_keys, keys=None, clips=1):
    """The clips to show: `keys` in the order given (ValueError for one the library lacks), else the first `clips` of the library."""
    all_keys = [str(k) for k in all_keys]
    if keys:
        keys = [str(k) for k in keys]
        missing = [k for k in keys if k not in all_keys]
        if missing:
            raise ValueError(f"replay.keys: no clip named {', '.join(missing)} in the library ({len(all_keys)} clips)")
        return keys
    if int(clips) < 1:
        raise ValueError(f"replay.clips={clips}: at least 1")
    return all_keys[:int(clips)]


def match_keys(keys, other_keys):
    """Every shown clip must exist in the compared library."""
    other = {str(k) for k in other_keys}
    missing = [k for k in keys if k not in other]
    if missing:
        raise ValueError(f"replay.compare: the other library has no clip named {', '.join(missing)}")
    return list(keys)


def num_frames(lengths, fps, frames=None):
    """`frames` when given, else every frame time i / fps up to the longest clip's end."""
    return int(frames) if frames else int(math.floor(max(float(l) for l in lengths) * float(fps) + 1e-6)) + 1


def frame_times(lengths, fps, first, count):
    """-> float64 [count, k]: t = i / fps for frames first .. first + count - 1, held at each clip's own length (its last frame)."""
    t = (np.arange(first, first + count, dtype=np.float64) / float(fps))[:, None]
    return np.minimum(t, np.asarray(lengths, np.float64)[None, :])


def common_frames(lengths_a, lengths_b, fps, first, count):
    """-> bool [count, k]: frames whose time lies within both clips (the frames `compare_mm` averages over)."""
    t = (np.arange(first, first + count, dtype=np.float64) / float(fps))[:, None]
    return t <= np.minimum(np.asarray(lengths_a, np.float64), np.asarray(lengths_b, np.float64))[None, :]


def tile_layout(k, compare):
    """-> (tiles, cols, source): `tiles` views per frame in row-major order, `cols` of the grid, source[v] = (library 0 / 1, clip).  With
    compare a pair takes two neighbouring cells of one row."""
    if compare:
        pairs_per_row = max(1, math.ceil(math.sqrt(k) / 2))
        return 2 * k, 2 * pairs_per_row, [(v % 2, v // 2) for v in range(2 * k)]
    return k, math.ceil(math.sqrt(k)), [(0, v) for v in range(k)]


# ---------------------------------------------------------------------------------------------------------------- the viewer
def make_task(argv):
    """The task the viewer reads its model from: `argv` composed as phc_amd.run does in player mode, one env per shown clip."""
    from .config import compose
    from .env.tasks.vec_task import parse_task
    from .utils.flags import flags
    cfg = compose(list(argv) + ["test=True"])
    rp = cfg.get("replay", None) or {}
    keys = list(rp.get("keys", None) or [])
    k = len(keys) if keys else int(rp.get("clips", 1))
    if k < 1:
        raise ValueError(f"replay.clips={k}: at least 1")
    cfg = compose(list(argv) + ["test=True", f"env.num_envs={k}"])
    saved = (flags.test, flags.im_eval)
    flags.test, flags.im_eval = True, False          # player mode: clips in library order, no heading randomisation, no cropping
    try:
        torch.manual_seed(int(cfg.seed))
        task, _ = parse_task(cfg)
    finally:
        flags.test, flags.im_eval = saved
    return task


def _sub_library(task, data, keys):
    """A motion library of the task's class over `keys` of the clip dict `data`, loaded in that order (env i = clip i)."""
    from .config import EasyDict
    from .utils.flags import flags
    cfg = EasyDict(dict(task._motion_train_lib.m_cfg))
    cfg.im_eval = False
    cfg.motion_file = {k: data[k] for k in keys}
    lib = task._motion_lib_cls(cfg)
    if lib._num_unique_motions != len(keys):
        raise ValueError("replay: a selected clip is shorter than env.min_length")
    saved = (flags.test, flags.im_eval)
    flags.test, flags.im_eval = True, False
    try:
        n = len(keys)
        lib.load_motions(skeleton_trees=task.skeleton_trees[:1] * n, gender_betas=task.humanoid_shapes[:1].cpu().repeat(n, 1),
                         limb_weights=task.humanoid_limb_and_weights[:1].cpu().repeat(n, 1), random_sample=False, start_idx=0, max_len=-1)
    finally:
        flags.test, flags.im_eval = saved
    return lib


def _clip_dict(task, source):
    """The clip dict of a motion file, a synthetic spec or a dict, as the task would load it."""
    from .utils.synthetic_motion import motion_from_spec
    from .env.tasks.humanoid_im import BASE_ROT
    mf = motion_from_spec(source, task.model, task._is_robot, task._robot_consts["default_dof_pos"] if task._is_robot else None,
                          num_extend=task.num_extend_bodies, min_frames=max(30, int(task._min_motion_len) if task._min_motion_len > 0 else 30),
                          base_rot=None if task._has_upright_start else BASE_ROT)
    if isinstance(mf, dict):
        return mf
    import joblib
    if not os.path.isfile(mf):
        raise FileNotFoundError(f"motion file {mf!r} not found")
    return joblib.load(mf)


def _body_state(state, nb):
    """get_motion_state's dict -> [rows, NB, 13] (pos, xyzw rotation, linear and angular velocity), and the extended bodies' positions or None."""
    bs = torch.cat([state["rg_pos"], state["rb_rot"], state["body_vel"], state["body_ang_vel"]], dim=-1).contiguous()
    ext = state["rg_pos_t"][:, nb:].contiguous() if "rg_pos_t" in state and state["rg_pos_t"].shape[1] > nb else None
    return bs, ext


def main(argv=None, task=None):
    """-> dict(frames, clips, compare_mm).  `task`: a task from make_task(argv), to look at afterwards (tests); built here otherwise."""
    from . import render as R
    argv = list(sys.argv[1:] if argv is None else argv)
    task = make_task(argv) if task is None else task
    cfg = task.cfg
    rc, rp = cfg.get("render", None) or {}, cfg.get("replay", None) or {}
    if not rc.get("video", None):
        raise ValueError("view_motion writes frames: give +render.video=<directory>")
    fps = float(rp.get("fps", 30))
    data = task._motion_train_lib._motion_data_load
    keys = select_keys(list(data.keys()), list(rp.get("keys", None) or []), rp.get("clips", 1))
    k = len(keys)
    libs = [_sub_library(task, data, keys)]
    if rp.get("compare", None):
        other = _clip_dict(task, rp["compare"])
        libs.append(_sub_library(task, other, match_keys(keys, other.keys())))
    lengths = [lib.get_motion_length().cpu().numpy().astype(np.float64) for lib in libs]
    F = num_frames(lengths[0] if len(libs) == 1 else np.maximum(*lengths), fps, rp.get("frames", None))
    tiles, cols, source = tile_layout(k, len(libs) > 1)
    width, height = int(rc.get("width", 640)), int(rc.get("height", 480))
    markers_on, follow = bool(rc.get("markers", True)), bool(rc.get("follow", True))
    dev, nb = task.device, task.num_bodies
    capsules = R.task_capsules(task)[:1].contiguous()      # (one body shape: the library was run through env 0's skeleton)
    meshes = None
    if rc.get("meshes", None):
        from .render_mesh import task_mesh_set
        meshes = task_mesh_set(task, str(rc["meshes"]), str(rc.get("mesh_color", "asset")))
    fmt, quality = R.video_options(rc)
    if fmt != "png" and torch.device(task.device).type != "cuda":
        raise RuntimeError(f"+render.format={fmt} launches phc_jpeg_encode on a HIP device; the task's tensors are on {task.device} (there is no CPU fallback)")
    recorder = R.VideoRecorder(str(rc["video"]), fps=max(1, int(round(fps))), name=str(cfg.get("exp_name", "motion")), fmt=fmt, quality=quality)
    cameras = [R.Camera() for _ in range(k)]
    placed = False
    err_sum = torch.zeros(k, dtype=torch.float64, device=dev)
    err_cnt = torch.zeros(k, dtype=torch.float64, device=dev)
    chunk = max(1, CHUNK_VIEWS // tiles)
    for f0 in range(0, F, chunk):
        n = min(chunk, F - f0)
        # one lookup per library: rows ordered (frame, clip)
        states = []
        for li, lib in enumerate(libs):
            t = torch.from_numpy(frame_times(lengths[li], fps, f0, n).astype(np.float32)).to(dev).reshape(-1)
            ids = torch.arange(k, device=dev).repeat(n)
            states.append(_body_state(lib.get_motion_state(ids, t), nb))
        if len(libs) > 1:
            both = torch.from_numpy(common_frames(lengths[0], lengths[1], fps, f0, n)).to(dev)
            dist = (states[0][0][..., 0:3] - states[1][0][..., 0:3]).norm(dim=-1).mean(dim=-1).reshape(n, k).to(torch.float64)
            err_sum += (dist * both).sum(0)
            err_cnt += both.sum(0)
            # rows of the scene ordered (frame, tile): tile v shows clip v // 2 of library v % 2
            pick = lambda a, b: torch.stack([a.reshape(n, k, *a.shape[1:]), b.reshape(n, k, *b.shape[1:])], dim=2).reshape(n * tiles, *a.shape[1:])
            bs = pick(states[0][0], states[1][0])
            ext = pick(states[0][1], states[1][1]) if states[0][1] is not None else None
        else:
            bs, ext = states[0]
        roots = states[0][0][:, 0, 0:3].reshape(n, k, 3).cpu().numpy()          # the chunk's root track, for the cameras
        views = []
        for f in range(n):
            if follow or not placed:
                for c in range(k):
                    cameras[c].follow(roots[f, c])
                placed = True
            views += [R.Camera(cam.eye, cam.target, cam.up, cam.fov_y) for cam in (cameras[c] for _, c in source)]
        mk = ext if (markers_on and ext is not None) else None
        scene = R.scene_struct(capsules, n * tiles, nb, bs, env_shape=None, markers=mk)
        rows = list(range(n * tiles))
        if meshes is not None:
            from . import render_mesh
            img = render_mesh.render(scene, meshes, views, rows, width, height, device=dev, lib=task._lib)
        else:
            img = R.render(scene, views, rows, width, height, device=dev, lib=task._lib)
        if fmt == "png":
            img = img.cpu()                                                      # the chunk's images, one copy
            for f in range(n):
                recorder.add(R.tile(img[f * tiles:(f + 1) * tiles], cols))
        else:                                                                    # tiled on the device, the whole chunk coded in one call; only the scans come back
            recorder.add_many(torch.stack([R.tile(img[f * tiles:(f + 1) * tiles], cols) for f in range(n)]))
    recorder.close()
    out = {"frames": F, "clips": keys, "compare_mm": None}
    if "format" in rc:
        out["video"] = recorder.avi_path
    if len(libs) > 1:
        mm = (err_sum / err_cnt.clamp(min=1) * 1000.0).cpu().numpy()
        out["compare_mm"] = {key: float(v) for key, v in zip(keys, mm)}
    print(out)
    return out


if __name__ == "__main__":
    main()
