"""Offscreen recording of headless runs: the HIP ray caster of csrc/phc_render.hip (`phc_render`, include/phc_amd.h) behind a small host API.

Replaces the reference player's camera sensor and video writer (phc/env/tasks/base_task.py:176-195,405-437): the frames come from a kernel of
our own because the GPU hosts have no display and no rasteriser.  What is drawn: every collision capsule of the env's articulation (boxes
appear as their capsule stand-ins; the H1 / G1 visual meshes are drawn only with `+render.meshes=<the robot's MJCF>`: render_mesh.py), the ground z = 0 with a 1 m checker, the shadows of one
directional light and, optionally, the reference bodies of the next frame as 5 cm spheres (humanoid_im.py:597-619 `_update_marker`).

    python -m phc_amd.run test=True ... +render.video=out [+render.envs=4 +render.width=640 +render.height=480 +render.markers=True +render.follow=True]
                                        [+render.format=avi|both +render.quality=90]   (a Motion-JPEG file coded on the device: video.py)

Nothing here runs unless `render.video` is set: the training and benchmark paths never import this module.
"""
import ctypes as C
import datetime
import importlib.util
import math
import os
import struct
import zlib

import numpy as np
import torch

from . import _lib as L

# body colours (linear 0..1, one per body index modulo 16), marker / ground / sky colours and the light (unit vector toward it)
PALETTE = ((0.90, 0.55, 0.30), (0.30, 0.55, 0.85), (0.35, 0.75, 0.45), (0.85, 0.80, 0.35), (0.70, 0.40, 0.75), (0.40, 0.75, 0.80),
           (0.85, 0.45, 0.55), (0.55, 0.60, 0.35), (0.95, 0.70, 0.50), (0.45, 0.45, 0.80), (0.60, 0.85, 0.60), (0.80, 0.60, 0.30),
           (0.60, 0.50, 0.85), (0.35, 0.65, 0.65), (0.90, 0.60, 0.70), (0.70, 0.70, 0.50))
_L = np.array([-0.35, -0.45, 0.82])
STYLE = dict(marker_color=(0.95, 0.20, 0.15), ground_color=((0.80, 0.80, 0.76), (0.58, 0.60, 0.62)), sky_color=(0.62, 0.75, 0.90),
             light_dir=tuple(float(v) for v in _L / np.linalg.norm(_L)), ambient=0.35, diffuse=0.65)
MARKER_RADIUS = 0.05   # urdf/traj_marker.urdf


class Camera:
    """Pinhole look-at camera (vertical field of view in degrees).  `follow(root_pos)` is the reference's viewer / recorder camera
    (humanoid.py:1715-1743): the first call places it at (x, y - 3, 1) looking at (x, y, 1); later calls keep its x / y offset to the root
    and its height and re-target (x, y, 1)."""

    def __init__(self, eye=(0.0, -3.0, 1.0), target=(0.0, 0.0, 1.0), up=(0.0, 0.0, 1.0), fov_y=60.0):
        self.eye = np.asarray(eye, dtype=np.float64).copy()
        self.target = np.asarray(target, dtype=np.float64).copy()
        self.up = np.asarray(up, dtype=np.float64).copy()
        self.fov_y = float(fov_y)
        self._prev_root = None

    def follow(self, root_pos):
        root = np.asarray(root_pos, dtype=np.float64)[:3]
        if self._prev_root is None:                                   # _init_camera
            self.eye = np.array([root[0], root[1] - 3.0, 1.0])
        else:                                                         # _update_camera
            delta = self.eye - self._prev_root
            self.eye = np.array([root[0] + delta[0], root[1] + delta[1], self.eye[2]])
        self.target = np.array([root[0], root[1], 1.0])
        self._prev_root = root.copy()
        return self

    def struct(self, env):
        c = L.Camera()
        c.env = int(env)
        c.eye[:], c.target[:], c.up[:] = [float(v) for v in self.eye], [float(v) for v in self.target], [float(v) for v in self.up]
        c.fov_y = math.radians(self.fov_y)
        return c


def capsule_table(models):
    """-> float32 [K, 8 S]: capsule s of model k = a[3], b[3] in the owner body's frame, radius, owner (ArticulationModel.shape_capsules() /
    shape_owner(): primary capsules then the extra ones).  The K models share one topology (per-env body shapes); a block with fewer
    capsules than the largest is padded with radius-0 entries, which are not drawn."""
    S = max(m.num_shapes_collision for m in models)
    out = np.zeros((len(models), S, 8), dtype=np.float32)
    for k, m in enumerate(models):
        n = m.num_shapes_collision
        out[k, :n, 0:7] = m.shape_capsules()
        out[k, :n, 7] = m.shape_owner()
    return out.reshape(len(models), 8 * S)


def scene_struct(capsules, num_envs, num_bodies, body_state, env_shape=None, markers=None, marker_radius=MARKER_RADIUS, style=None, marker_radii=None,
                 marker_colors=None):
    """phc_render_scene_t over device tensors: capsules float32 [K, 8 S] (capsule_table), body_state [N, NB, 13], env_shape int32 [N] or
    None, markers float32 [N, M, 3] or None; marker_radii float32 [M] / marker_colors float32 [M, 3] or None (marker_radius / the style's colour for all)."""
    st = dict(STYLE, **(style or {}))
    s = L.RenderScene()
    s.num_envs, s.num_bodies = int(num_envs), int(num_bodies)
    s.body_state, s.capsules = body_state.data_ptr(), capsules.data_ptr()
    s.num_shape_blocks = int(capsules.shape[0])
    s.num_capsules = int(capsules.shape[1]) // 8
    s.capsule_stride = int(capsules.stride(0))
    s.env_shape = env_shape.data_ptr() if env_shape is not None else None
    s.markers = markers.data_ptr() if markers is not None else None
    s.num_markers = int(markers.shape[1]) if markers is not None else 0
    s.marker_radius = float(marker_radius)
    for name, t, width in (("marker_radii", marker_radii, 1), ("marker_colors", marker_colors, 3)):
        if t is not None and (markers is None or t.dtype != torch.float32 or t.numel() != width * int(markers.shape[1]) or not t.is_contiguous()):
            raise ValueError(f"{name}: a contiguous float32 tensor of {width} value(s) per marker")
    s.marker_radii = marker_radii.data_ptr() if marker_radii is not None else None
    s.marker_colors = marker_colors.data_ptr() if marker_colors is not None else None
    for i in range(L.RENDER_PALETTE):
        s.palette[i][:] = PALETTE[i % len(PALETTE)]
    s.marker_color[:] = st["marker_color"]
    s.ground_color[0][:], s.ground_color[1][:] = st["ground_color"]
    s.sky_color[:], s.light_dir[:] = st["sky_color"], st["light_dir"]
    s.ambient, s.diffuse = float(st["ambient"]), float(st["diffuse"])
    return s


def render(scene, cameras, env_ids, width, height, depth=False, hit_id=False, device="cuda", lib=None):
    """One phc_render call on the current stream: view v shows env env_ids[v] through cameras[v].  -> rgba uint8 [V, H, W, 4] (+ depth f32
    [V, H, W], hit_id int32 [V, H, W] when asked for), on the device."""
    lib = lib or L.load()
    V = len(env_ids)
    cams = (L.Camera * V)(*[c.struct(e) for c, e in zip(cameras, env_ids)])
    rgba = torch.empty((V, height, width, 4), dtype=torch.uint8, device=device)
    dep = torch.empty((V, height, width), dtype=torch.float32, device=device) if depth else None
    ids = torch.empty((V, height, width), dtype=torch.int32, device=device) if hit_id else None
    L.check(lib.phc_render(C.byref(scene), cams, V, int(width), int(height), rgba.data_ptr(), dep.data_ptr() if depth else None,
                           ids.data_ptr() if hit_id else None, torch.cuda.current_stream().cuda_stream), "phc_render")
    out = (rgba,) + ((dep,) if depth else ()) + ((ids,) if hit_id else ())
    return out if len(out) > 1 else rgba


def task_capsules(task):
    """The capsule table of a task's shape models on its device (upload once per recorder)."""
    return torch.from_numpy(capsule_table(task.shape_models)).to(task.device)


def render_envs(task, env_ids, cameras, width, height, markers=True, depth=False, hit_id=False, capsules=None, meshes=None):
    """Render envs `env_ids` of a HumanoidIm task (its rigid_body_state; markers = the task's ref_body_pos, the next frame's reference
    bodies) on the task's stream.  Reads simulator state only: no RNG draw, no task buffer written.  capsules: task_capsules(task), to
    skip the upload.  meshes: an uploaded render_mesh.MeshSet, drawn through phc_render_mesh in place of the capsules of its bodies."""
    caps = task_capsules(task) if capsules is None else capsules   # (held until the launch: the scene keeps raw pointers only)
    env_shape = task._env_shape if len(task.shape_models) > 1 else None
    marks, radii, colors = (task.ref_body_pos if markers else None), None, None
    proj = getattr(task, "_proj", None)
    if proj is not None:   # `+projectile.*`: the projectiles behind the reference markers, each with its own radius, a neutral grey (parked ones sit far below the ground)
        marks, radii, colors = projectile_markers(marks, proj.pos, proj.opt.radius, cache=proj.marker_cache)   # (held until the launch: the scene keeps raw pointers only)
    scene = scene_struct(caps, task.num_envs, task.num_bodies, task._rigid_body_state_reshaped, env_shape=env_shape, markers=marks, marker_radii=radii,
                         marker_colors=colors)
    if meshes is not None:
        from . import render_mesh
        return render_mesh.render(scene, meshes, cameras, [int(e) for e in env_ids], width, height, depth=depth, hit_id=hit_id, device=task.device,
                                  lib=task._lib)
    return render(scene, cameras, [int(e) for e in env_ids], width, height, depth=depth, hit_id=hit_id, device=task.device, lib=task._lib)


PROJECTILE_COLOR = (0.5, 0.5, 0.5)


def projectile_markers(markers, pos, radius, marker_radius=MARKER_RADIUS, marker_color=None, cache=None):
    """The marker list with the projectiles appended: markers [N, M, 3] or None, pos [P, N, 3] (ProjectileSchedule.pos) -> markers [N, M + P, 3], radii
    [M + P], colours [M + P, 3].  Radii and colours are the same in every frame of a task: `cache` (a dict, ProjectileSchedule.marker_cache) keeps them on
    the device per marker count, so a frame uploads nothing."""
    M = 0 if markers is None else int(markers.shape[1])
    P = int(pos.shape[0])
    p = pos.permute(1, 0, 2)
    marks = (p if markers is None else torch.cat([markers, p], dim=1)).contiguous()
    base = tuple(STYLE["marker_color"] if marker_color is None else marker_color)
    key = (M, P, float(radius), float(marker_radius), base)
    if cache is None or key not in cache:
        radii = torch.tensor([marker_radius] * M + [float(radius)] * P, dtype=torch.float32, device=pos.device)
        colors = torch.tensor([list(base)] * M + [list(PROJECTILE_COLOR)] * P, dtype=torch.float32, device=pos.device)
        if cache is None:
            return marks, radii, colors
        cache[key] = (radii, colors)
    return (marks,) + cache[key]


def tile(frames, cols):
    """[V, H, W, C] -> one [rows * H, cols * W, C] grid image (row-major; empty cells black)."""
    V, H, W, Ch = frames.shape
    cols = max(1, min(int(cols), V))
    rows = (V + cols - 1) // cols
    out = frames.new_zeros((rows * H, cols * W, Ch))
    for v in range(V):
        r, c = divmod(v, cols)
        out[r * H:(r + 1) * H, c * W:(c + 1) * W] = frames[v]
    return out


def write_png(path, rgba, level=1):
    """8-bit RGBA PNG with the standard library (zlib + struct).  rgba: [H, W, 4] uint8 array or tensor."""
    a = rgba.cpu().numpy() if isinstance(rgba, torch.Tensor) else np.asarray(rgba)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 4
    H, W = a.shape[:2]
    raw = np.concatenate([np.zeros((H, 1), dtype=np.uint8), a.reshape(H, W * 4)], axis=1).tobytes()   # filter type 0 per row

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b""))


def _mp4_backend():
    """imageio with its ffmpeg plugin, if this process can import both; never installs anything."""
    if importlib.util.find_spec("imageio") is None or importlib.util.find_spec("imageio_ffmpeg") is None:
        return None
    try:
        import imageio
        return imageio
    except Exception:
        return None


def video_options(rc):
    """`render.format` (png, the default; avi; both) and `render.quality` (1 .. 100, default 90) of the `render.*` keys -> (format, quality)."""
    fmt = str(rc.get("format", "png"))
    if fmt not in ("png", "avi", "both"):
        raise ValueError(f"render.format={fmt}: png, avi or both")
    quality = int(rc.get("quality", 90))
    if not 1 <= quality <= 100:
        raise ValueError(f"render.quality={quality}: 1 .. 100")
    return fmt, quality


class VideoRecorder:
    """Numbered PNG frames `frame_000000.png ...` in `directory`, plus `<name>-<date>.mp4` at `fps` when imageio's ffmpeg backend is importable
    (base_task.py:176-195,428-437: output/renderings/<exp_name>-<date>.mp4 at fps = 1 / dt).  `fmt` = avi writes `<name>-<date>.avi` (Motion-JPEG coded on
    the device: phc_amd/video.py) in place of the PNGs and the mp4, both writes all of them; png is the default and imports nothing more."""

    def __init__(self, directory, fps=30, name="video", fmt="png", quality=90):
        self.fmt, self.quality = video_options({"format": fmt, "quality": quality})
        self.dir = directory
        os.makedirs(directory, exist_ok=True)
        self.fps, self.name, self.count = int(fps), name, 0
        self._imageio, self._writer = (_mp4_backend() if self.fmt != "avi" else None), None
        self.mp4_path = None
        self.avi_path, self._avi, self._jpeg = None, None, None

    def add(self, frame):
        if self.fmt != "png":
            self._add_avi(frame[None])
        if self.fmt != "avi":
            self._add_png(frame)
        self.count += 1

    def add_many(self, frames):
        """frames [n, H, W, 4] on the device: in avi mode one phc_jpeg_encode call for all of them."""
        if self.fmt != "png":
            self._add_avi(frames)
        if self.fmt != "avi":
            for a in frames.cpu():
                self._add_png(a)
                self.count += 1
        else:
            self.count += int(frames.shape[0])

    def _add_avi(self, frames):
        from . import video
        if not isinstance(frames, torch.Tensor) or frames.device.type != "cuda":
            raise RuntimeError("render.format=avi codes the frames with phc_jpeg_encode on a HIP device; these frames are in host memory (there is no CPU fallback)")
        if self._avi is None:
            self._jpeg = video.JpegEncoder()
            self.avi_path = os.path.join(self.dir, f"{self.name}-{datetime.datetime.now().strftime('%Y-%m-%d-%H:%M:%S')}.avi")
            self._avi = video.AviWriter(self.avi_path, int(frames.shape[2]), int(frames.shape[1]), self.fps)
        for jpeg in self._jpeg.encode(frames, self.quality):
            self._avi.add(jpeg)

    def _add_png(self, frame):
        a = frame.cpu().numpy() if isinstance(frame, torch.Tensor) else np.asarray(frame)
        write_png(os.path.join(self.dir, f"frame_{self.count:06d}.png"), a)
        if self._imageio is not None:
            if self._writer is None:
                self.mp4_path = os.path.join(self.dir, f"{self.name}-{datetime.datetime.now().strftime('%Y-%m-%d-%H:%M:%S')}.mp4")
                self._writer = self._imageio.get_writer(self.mp4_path, fps=self.fps, macro_block_size=None)
            self._writer.append_data(a[..., :3])

    def close(self):
        if self._writer is not None:
            self._writer.close()
            self._writer = None
        if self._avi is not None:
            self._avi.close()
            self._avi = None


class TaskRecorder:
    """The `render.*` override keys of a task (read with cfg.get: they are not part of the built-in config tree):
      render.video   directory of the frames (recording is on when set)
      render.envs    k: a grid of envs 0 .. k-1, one camera each (default 1: env 0, as the reference records)
      render.width / render.height   one view's size (default 640 x 480)
      render.markers draw the next frame's reference bodies (default flags.show_traj, as the reference)
      render.follow  cameras follow their env's root (default True; False: the first placement stays)
      render.meshes  path of the robot's MJCF: its visual meshes are drawn (phc_render_mesh) in place of the capsules of the bodies that carry one
      render.mesh_color  asset (default: the MJCF rgba of each geom) or palette (the body palette)
      render.format  png (default: numbered PNG frames), avi (one Motion-JPEG `<name>-<date>.avi`, coded on the device: phc_amd/video.py) or both
      render.quality JPEG quality of the avi, 1 .. 100 (default 90)"""

    def __init__(self, task, rc):
        from .utils.flags import flags
        self.task = task
        fmt, quality = video_options(rc)
        if fmt != "png" and torch.device(task.device).type != "cuda":
            raise RuntimeError(f"+render.format={fmt} launches phc_jpeg_encode on a HIP device; the task's tensors are on {task.device} (there is no CPU fallback)")
        self.k = max(1, min(int(rc.get("envs", 1)), task.num_envs))
        self.width, self.height = int(rc.get("width", 640)), int(rc.get("height", 480))
        self.markers = bool(rc.get("markers", flags.show_traj))
        self.follow = bool(rc.get("follow", True))
        self.cameras = [Camera() for _ in range(self.k)]
        self._placed = False
        self.capsules = task_capsules(task)
        self.meshes = None
        if rc.get("meshes", None):
            from .render_mesh import task_mesh_set
            self.meshes = task_mesh_set(task, str(rc["meshes"]), str(rc.get("mesh_color", "asset")))
        rank = int(os.environ.get("RANK", "0"))        # (torchrun: every rank records its own envs into a directory of its own)
        self.recorder = VideoRecorder(os.path.join(str(rc["video"]), f"rank{rank}") if rank else str(rc["video"]), fps=max(1, int(round(1.0 / task.dt))), name=str(task.cfg.get("exp_name", "video")),
                                      fmt=fmt, quality=quality)

    def record(self):
        t = self.task
        if self.follow or not self._placed:
            roots = t._humanoid_root_states[:self.k, 0:3].cpu().numpy()
            for cam, r in zip(self.cameras, roots):
                cam.follow(r)
            self._placed = True
        frames = render_envs(t, range(self.k), self.cameras, self.width, self.height, markers=self.markers, capsules=self.capsules, meshes=self.meshes)
        self.recorder.add(tile(frames, math.ceil(math.sqrt(self.k))))

    def close(self):
        self.recorder.close()
