"""fp64 numpy ray caster: the oracle of phc_render (include/phc_amd.h), written from the geometric definitions.

  capsule  = the points within r of the segment [a, b] (a marker sphere: a = b);
  ground   = the plane z = 0, colour ground_color[(floor(x) + floor(y)) & 1];
  camera   = unit(f + sx r + sy u) through pixel centres (the header's formula), row 0 at the top;
  shading  = C * (ambient + diffuse * lit), lit = max(n . L, 0), or 0 when the ray from (hit + 1e-3 n) toward L enters a capsule or marker;
  u8       = floor(clip(v, 0, 1) * 255 + 0.5);  sky colour (unshaded) on a miss.

Besides rgba / depth / hit id it returns, per pixel, the EXCLUSION flags of the comparison: a pixel is excluded (from every comparison)
when the primary ray passes within DELTA of a silhouette of any shape (|distance(ray, segment) - r| < DELTA), when its two nearest surface
hits are within DELTA in depth, or when its ground hit lies within DELTA of a checker line; and from the RGB comparison alone when its
shadow ray passes within DELTA of a silhouette or starts within DELTA of a surface.  DELTA = 1e-4 m: fp32 world coordinates of a few metres
carry ~1e-6 m of rounding, and DELTA is 100 times that.

The test scenes are generated here too, on the host: seeded joint rotations, fp64 forward kinematics (motion_lib.robot_fk) to body poses,
uploaded as rigid_body_state.  So the CPU test and the GPU test see exactly the same inputs."""
import math

import numpy as np

DELTA = 1.0e-4
SHADOW_OFFSET = 1.0e-3
MARKER_ID = 1000


# ---------------------------------------------------------------------------------------------------------------- geometry
def camera_rays(eye, target, up, fov_y, W, H):
    """-> unit directions [H, W, 3] (fov_y in radians)."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    th = math.tan(0.5 * fov_y)
    sx = (2.0 * (np.arange(W) + 0.5) / W - 1.0) * th * (W / H)
    sy = (1.0 - 2.0 * (np.arange(H) + 0.5) / H) * th
    d = f[None, None] + sx[None, :, None] * r[None, None] + sy[:, None, None] * u[None, None]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def _sphere_entry(o, d, c, r):
    """Smaller root of |o + t d - c| = r per ray (nan when the ray misses)."""
    q = o - c
    b = np.einsum("...k,...k->...", q, d)
    disc = b * b - (np.einsum("...k,...k->...", q, q) - r * r)
    with np.errstate(invalid="ignore"):
        return np.where(disc >= 0, -b - np.sqrt(np.maximum(disc, 0)), np.nan)


def _cylinder_entry(o, d, a, b, r):
    """Smaller root of dist(o + t d, line ab) = r whose foot lies on the segment (nan otherwise)."""
    u = b - a
    uu = u @ u
    if uu == 0:
        return np.full(o.shape[:-1] if o.ndim > 1 else d.shape[:-1], np.nan)
    w = o - a
    ud = d @ u
    uw = np.einsum("...k,k->...", w, u)
    wd = np.einsum("...k,...k->...", w, d)
    A = uu - ud * ud
    B = uu * wd - uw * ud
    Cc = uu * (np.einsum("...k,...k->...", w, w) - r * r) - uw * uw
    disc = B * B - A * Cc
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (-B - np.sqrt(np.maximum(disc, 0))) / A
        y = uw + t * ud
        ok = (disc >= 0) & (A > 1e-12 * uu) & (y >= 0) & (y <= uu)
    return np.where(ok, t, np.nan)


def capsule_entry(o, d, a, b, r):
    """First entry t > 0 of the ray into the capsule (inf if none), and the smallest |t| of a component entry (for the shadow-origin test).
    The capsule is the union of the lateral cylinder and the two end spheres; its first entry is the smallest first entry of the three."""
    roots = np.stack([_sphere_entry(o, d, a, r), _sphere_entry(o, d, b, r), _cylinder_entry(o, d, a, b, r)])
    pos = np.where(roots > 0, roots, np.inf)
    return np.nanmin(np.where(np.isnan(roots), np.inf, pos), axis=0), np.nanmin(np.where(np.isnan(roots), np.inf, np.abs(roots)), axis=0)


def segment_distance(o, d, a, b):
    """Distance between the half-line o + t d (t >= 0, |d| = 1) and the segment [a, b]."""
    u = b - a
    w = a - o
    wp = w - np.einsum("...k,...k->...", w, d)[..., None] * d
    up = u - np.einsum("...k,k->...", d, u)[..., None] * d
    uu = np.einsum("...k,...k->...", up, up)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.clip(np.where(uu > 0, -np.einsum("...k,...k->...", wp, up) / np.where(uu > 0, uu, 1), 0.0), 0.0, 1.0)
    x = a + s[..., None] * u                                       # closest point of the segment to the line
    t = np.einsum("...k,...k->...", x - o, d)
    line = np.linalg.norm(x - o - t[..., None] * d, axis=-1)
    # behind the origin: the closest point of the half-line is the origin itself
    uu2 = u @ u
    s0 = np.clip(np.einsum("...k,k->...", o - a, u) / uu2, 0, 1) if uu2 > 0 else np.zeros(o.shape[:-1] if o.ndim > 1 else t.shape)
    pt = np.linalg.norm(a + s0[..., None] * u - o, axis=-1)
    return np.where(t >= 0, line, pt)


def world_capsules(capsules, owner, body_state):
    """capsules [S, 7] (a, b in the owner frame, r), owner [S], body_state [NB, 13] -> A [S, 3], B [S, 3], r [S] in world space."""
    bs = np.asarray(body_state, np.float64)
    p, q = bs[owner, 0:3], bs[owner, 3:7]

    def rot(v):   # v + 2 w (q x v) + 2 q x (q x v)   (the xyzw quaternion as stored, not renormalised)
        t = 2.0 * np.cross(q[:, :3], v)
        return v + q[:, 3:4] * t + np.cross(q[:, :3], t)
    cap = np.asarray(capsules, np.float64)
    return p + rot(cap[:, 0:3]), p + rot(cap[:, 3:6]), cap[:, 6]


# ---------------------------------------------------------------------------------------------------------------- the oracle
def render_view(style, palette, capsules, owner, body_state, camera, W, H, markers=None, marker_radius=0.05):
    """One view.  capsules [S, 7] of the env's block, owner [S], body_state [NB, 13] of the env, camera = (eye, target, up, fov_y radians),
    markers [M, 3] or None.  -> dict(rgba u8 [H, W, 4], depth [H, W], id [H, W], excl [H, W] (every comparison), excl_rgb [H, W])."""
    eye = np.asarray(camera[0], np.float64)
    d = camera_rays(*camera, W, H).reshape(-1, 3)
    P = d.shape[0]
    o = np.broadcast_to(eye, d.shape)
    A, B, R = world_capsules(capsules, owner, body_state)
    nb = np.asarray(body_state).shape[0]
    drawn = (R > 0) & (owner >= 0) & (owner < nb)
    cols = [np.asarray(palette[int(ow) % len(palette)], np.float64) for ow in owner]
    ids = list(range(len(R)))
    if markers is not None and marker_radius > 0:
        mk = np.asarray(markers, np.float64)
        A, B = np.concatenate([A, mk]), np.concatenate([B, mk])
        R = np.concatenate([R, np.full(len(mk), float(marker_radius))])
        drawn = np.concatenate([drawn, np.ones(len(mk), bool)])
        cols += [np.asarray(style["marker_color"], np.float64)] * len(mk)
        ids += [MARKER_ID + m for m in range(len(mk))]
    prims = [i for i in range(len(R)) if drawn[i]]

    # primary ray: every surface's entry, the ground, the silhouettes
    T = np.full((len(prims) + 1, P), np.inf)
    sil = np.zeros(P, bool)
    for j, i in enumerate(prims):
        T[j], _ = capsule_entry(o, d, A[i], B[i], R[i])
        sil |= np.abs(segment_distance(o, d, A[i], B[i]) - R[i]) < DELTA
    with np.errstate(divide="ignore"):
        tg = np.where((d[:, 2] < 0) & (eye[2] > 0), -eye[2] / np.where(d[:, 2] < 0, d[:, 2], -1), np.inf)
    T[-1] = tg
    order = np.sort(T, axis=0)
    with np.errstate(invalid="ignore"):
        near2 = (order[1] - order[0] < DELTA) & np.isfinite(order[1])
    k = np.argmin(T, axis=0)
    t = T[k, np.arange(P)]
    hit = np.isfinite(t)
    ground = hit & (k == len(prims))
    x = eye + np.where(hit, t, 0)[:, None] * d
    hit_id = np.full(P, -1, np.int64)
    hit_id[ground] = -2
    n = np.zeros((P, 3))
    n[:, 2] = 1.0
    base = np.broadcast_to(np.asarray(style["sky_color"], np.float64), (P, 3)).copy()
    gx, gy = np.floor(x[:, 0]), np.floor(x[:, 1])
    parity = ((gx + gy) % 2).astype(np.int64)
    g0, g1 = (np.asarray(c, np.float64) for c in style["ground_color"])
    base[ground] = np.where(parity[ground, None] == 1, g1, g0)
    line = ground & ((np.abs(x[:, 0] - np.round(x[:, 0])) < DELTA) | (np.abs(x[:, 1] - np.round(x[:, 1])) < DELTA))
    for j, i in enumerate(prims):
        m = hit & (k == j)
        if not m.any():
            continue
        hit_id[m] = ids[i]
        base[m] = cols[i]
        u = B[i] - A[i]
        uu = u @ u
        s = np.clip((x[m] - A[i]) @ u / uu, 0, 1) if uu > 0 else np.zeros(m.sum())
        nn = x[m] - (A[i] + s[:, None] * u)
        n[m] = nn / np.linalg.norm(nn, axis=-1, keepdims=True)
    x[ground, 2] = 0.0

    # shading and the shadow ray
    L = np.asarray(style["light_dir"], np.float64)
    lit = np.maximum(n @ L, 0.0)
    sh = hit & (lit > 0)
    excl_sh = np.zeros(P, bool)
    if sh.any():
        os_ = x[sh] + SHADOW_OFFSET * n[sh]
        Ls = np.broadcast_to(L, os_.shape)
        occ = np.zeros(len(os_), bool)
        for i in prims:
            te, tabs = capsule_entry(os_, Ls, A[i], B[i], R[i])
            occ |= np.isfinite(te)
            m_ex = (np.abs(segment_distance(os_, Ls, A[i], B[i]) - R[i]) < DELTA) | (tabs < DELTA)
            tmp = np.zeros(P, bool)
            tmp[sh] = m_ex
            excl_sh |= tmp
        lit_sh = lit[sh]
        lit_sh[occ] = 0.0
        lit[sh] = lit_sh
    shade = np.where(hit, style["ambient"] + style["diffuse"] * lit, 1.0)
    rgb = np.floor(np.clip(base * shade[:, None], 0, 1) * 255 + 0.5).astype(np.uint8)
    rgba = np.concatenate([rgb, np.full((P, 1), 255, np.uint8)], axis=1)
    excl = sil | near2 | line
    return dict(rgba=rgba.reshape(H, W, 4), depth=np.where(hit, t, np.inf).reshape(H, W), id=hit_id.reshape(H, W),
                excl=excl.reshape(H, W), excl_rgb=(excl | excl_sh).reshape(H, W))


# ---------------------------------------------------------------------------------------------------------------- test scenes
def posed_bodies(model, rng, root_xy=(0.0, 0.0), yaw=0.0, spread=0.35):
    """Seeded joint rotations -> fp64 FK (motion_lib.robot_fk) -> body_state [NB, 13] (pos, xyzw quaternion, zero velocities), lifted
    so that the lowest capsule surface sits 1 cm above the ground."""
    from phc_amd.motion_lib import _mat_to_quat_xyzw, robot_fk
    nb = model.num_bodies
    pose = np.zeros((1, nb, 3))
    pose[0, 0] = [0.0, 0.0, yaw]
    for i in range(1, nb):
        c = int(model.dof_count[i])
        if c == 3:
            pose[0, i] = rng.normal(0.0, spread, 3)
        elif c == 1:
            pose[0, i] = model.dof_axis[model.dof_start[i]] * rng.normal(0.0, spread)
    wpos, wmat, _, _ = robot_fk(model.parent, model.local_translation, model.local_rotation, [], np.zeros((0, 3)), np.zeros((0, 4)), pose,
                                np.array([[root_xy[0], root_xy[1], 0.0]]))
    bs = np.zeros((nb, 13))
    bs[:, 0:3] = wpos[0]
    bs[:, 3:7] = _mat_to_quat_xyzw(wmat[0])
    caps, own = model.shape_capsules(), model.shape_owner()
    A, B, R = world_capsules(caps, own, bs)
    ok = R > 0
    bs[:, 2] += 0.01 - np.min(np.minimum(A[ok, 2], B[ok, 2]) - R[ok])
    return bs


def look(eye, target, up=(0.0, 0.0, 1.0), fov_deg=60.0):
    """A camera as the kernel receives it: every value rounded to fp32 (phc_camera_t)."""
    f32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    return (f32(eye), f32(target), f32(up), float(np.float32(math.radians(fov_deg))))


FOV = 40.0   # degrees, vertical


def standard_cameras(root, n=8):
    """Views of a humanoid standing at root (x, y), 40 degree vertical field of view: obliques from 6 azimuths pitched 30 degrees down (every
    ground ray descends at >= 10 degrees), the top-down view and the low view from 0.25 m whose lowest ray climbs at 5 degrees (sky behind)."""
    x, y = root
    cams = []
    for k in range(n - 2):
        az = 2 * math.pi * k / (n - 2) + 0.3
        dist = 2.6 + 0.4 * (k % 3)
        cams.append(look((x - dist * math.sin(az), y - dist * math.cos(az), 0.9 + dist * math.tan(math.radians(30.0))), (x, y, 0.9), fov_deg=FOV))
    cams.append(look((x + 0.01, y, 4.5), (x, y, 0.0), up=(0.0, 1.0, 0.0), fov_deg=FOV))                      # top-down
    pitch = math.radians(26.0)                                                                                # lowest ray: >= 5 degrees up (corners included)
    cams.append(look((x, y - 2.5, 0.25), (x, y, 0.25 + 2.5 * math.tan(pitch)), fov_deg=FOV))                  # low view
    return cams[:n]


def ground_ray_angles(camera, W, H):
    """min |d.z| over the rays that meet the ground, and over those that do not (degrees): the 5 degree rule of the test scenes."""
    d = camera_rays(*camera, W, H).reshape(-1, 3)
    down = d[:, 2] < 0
    el = np.degrees(np.arcsin(np.abs(d[:, 2])))
    return (el[down].min() if down.any() else 90.0), (el[~down].min() if (~down).any() else 90.0)


SCENES = ("smpl", "h1", "g1", "smpl_shape")


def make_scene(name, W=160, H=120, seed=0):
    """-> dict(models, capsules [K, S, 7], owner [S], env_shape [N] | None, body_state [N, NB, 13] float32, markers [N, M, 3] float32,
    cameras [(env, camera)], W, H).  Scene `smpl`: 2 envs, 8 views of env 1; `h1` / `g1`: 2 envs, 4 views; `smpl_shape`: the three
    gender bodies of smpl_humanoid_shape on envs 0 / 1 / 2 (env_shape = env % 3), 2 views of each."""
    from phc_amd.model import load_model
    from phc_amd import robots
    rng = np.random.default_rng(seed + 1000 * SCENES.index(name))
    if name == "smpl_shape":
        models = [load_model(f"smpl_{g}_humanoid") for g in (0, 1, 2)]
        N = 3
        env_shape = np.arange(N, dtype=np.int32) % 3
    else:
        models = [load_model(f"{'smpl' if name == 'smpl' else name}_humanoid")]
        N = 2
        env_shape = None
    for m in models:
        robots.apply_collision_filter(m, "smpl" if name.startswith("smpl") else name)
    nb = models[0].num_bodies
    bs = np.zeros((N, nb, 13))
    mk = np.zeros((N, nb, 3))
    roots = []
    for e in range(N):
        root = (rng.uniform(-3, 3), rng.uniform(-3, 3))
        roots.append(root)
        m = models[env_shape[e] if env_shape is not None else 0]
        bs[e] = posed_bodies(m, rng, root, yaw=rng.uniform(-math.pi, math.pi))
        ref = posed_bodies(m, rng, (root[0] + 0.35, root[1] + 0.2), yaw=rng.uniform(-math.pi, math.pi))   # a nearby "reference" pose
        mk[e] = ref[:, 0:3]
    if name == "smpl":
        cams = [(1, c) for c in standard_cameras(roots[1], 8)]
    elif name in ("h1", "g1"):
        cams = [(e, c) for e in range(N) for c in standard_cameras(roots[e], 8)[::3][:2]]
    else:
        cams = [(e, c) for e in range(N) for c in (standard_cameras(roots[e], 8)[1], standard_cameras(roots[e], 8)[4])]
    from phc_amd.render import capsule_table
    tab = capsule_table(models).reshape(len(models), -1, 8)           # [K, S, 8]: blocks padded with radius-0 capsules
    return dict(models=models, capsules=tab[..., :7], owner=tab[..., 7].astype(np.int64), env_shape=env_shape, body_state=bs.astype(np.float32),
                markers=mk.astype(np.float32), cameras=cams, W=W, H=H)


def render_scene(sc, markers=True, marker_radius=0.05):
    """The oracle's views of a make_scene() scene (the colours and the light of phc_amd.render.STYLE / PALETTE): list of render_view() dicts,
    one per camera."""
    from phc_amd import render as R
    style, palette = R.STYLE, R.PALETTE
    out = []
    for env, cam in sc["cameras"]:
        blk = int(sc["env_shape"][env]) if sc["env_shape"] is not None else 0
        out.append(render_view(style, palette, sc["capsules"][blk], sc["owner"][blk], sc["body_state"][env], cam, sc["W"], sc["H"],
                               markers=sc["markers"][env] if markers else None, marker_radius=marker_radius))
    return out
