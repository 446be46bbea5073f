"""fp64 numpy oracle of phc_render_mesh (include/phc_amd.h): render_oracle's scene plus triangle meshes, written from the definitions.

  instance  = mesh vertices v taken to the world by x = p_body + rot(q_body, pos) + rot(unit(q_body (x) quat), v);
  triangle  = brute-force Moller-Trumbore over ALL triangles of every instance whose bounding sphere the ray meets (the sphere test is exact
              in fp64 and padded by 1 mm: it drops no hit), two-sided, u >= 0, v >= 0, u + v <= 1, t > 0; |e1 x e2| <= 1e-12 never hit;
  normal    = unit(e1 x e2) flipped to oppose the ray, flat; base colour = the instance's rgb;
  capsules  = render_oracle's, without those whose owner body carries an instance; ground, markers, sky, shading: render_oracle's;
  shadow    = the ray from (hit + 1e-3 n) toward the light is occluded by every drawn capsule, marker and instance.

EXCLUSIONS, besides render_oracle's (capsule silhouettes, depth ties of the two nearest surfaces, checker lines, shadow boundaries):
  * excl (every comparison): the primary ray passes within DELTA = 1e-4 m of a triangle edge (segment) at a ray parameter 0 < t <= first hit
    + DELTA (an edge of a mesh it hits or just misses; edges hidden behind the first hit do not count), or its first hit is a triangle with
    |d . n| < GRAZE;
  * excl_rgb: the shadow ray meets a triangle at |t| < DELTA, or passes within DELTA of a triangle edge at t > 0 while no triangle occludes
    it for certain (a hit at t > 0 whose three edges are all at least DELTA from the ray: then the light is blocked whatever happens at
    the edge).

GRAZE = 0.02 comes from the depth bound (tests/test_render_mesh_gpu.py): a sideways error eps of the ray moves the hit on a plane by
eps / |d . n| along the ray, and eps <= 8e-6 m there.

The test scenes (make_scene) are generated here, on the host; the meshes are tetrahedron, triangle, cube, quad and icospheres scaled to
ellipsoids.  Nothing is read from a file."""
import functools
import math

import numpy as np

import render_oracle as ro

DELTA = ro.DELTA
GRAZE = 0.02
MESH_ID = 2000
MIN_CROSS = 1.0e-12
SPHERE_PAD = 1.0e-3


# ---------------------------------------------------------------------------------------------------------------- meshes
def icosphere(subdiv):
    """Unit icosphere: 20 * 4^subdiv triangles, vertices on the unit sphere, outward winding.  -> vertices f64 [NV, 3], faces int [NT, 3]"""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / math.sqrt(1 + p * p) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v), np.asarray(f, np.int64)


def ellipsoid(subdiv, semi_axes):
    v, f = icosphere(subdiv)
    return (v * np.asarray(semi_axes)).astype(np.float32), f


def tetrahedron(size):
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float64) * (size / (2 * math.sqrt(2)))
    return v.astype(np.float32), np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int64)


def cube(size):
    h = 0.5 * size
    v = np.array([(x, y, z) for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float32)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v, np.asarray(f, np.int64)


def quad_grid(size, n):
    """A flat n x n grid of squares (2 n^2 triangles) in the plane z = 0 of the mesh frame: every box of its tree has zero thickness."""
    g = np.linspace(-0.5 * size, 0.5 * size, n + 1)
    v = np.array([(x, y, 0.0) for y in g for x in g], np.float32)
    f = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            f += [(a, a + 1, a + n + 2), (a, a + n + 2, a + n + 1)]
    return v, np.asarray(f, np.int64)


# ---------------------------------------------------------------------------------------------------------------- geometry
def _rot(q, v):
    """v rotated by the xyzw quaternion q (as given): v + 2 w (q x v) + 2 q x (q x v)"""
    t = 2.0 * np.cross(q[:3], v)
    return v + q[3] * t + np.cross(q[:3], t)


def _qmul(a, b):
    return np.concatenate([a[3] * b[:3] + b[3] * a[:3] + np.cross(a[:3], b[:3]), [a[3] * b[3] - a[:3] @ b[:3]]])


def world_vertices(inst, vertices, body_state):
    """The mesh-frame vertices [n, 3] of an instance in the world (the header's composition, fp64)."""
    bs = np.asarray(body_state, np.float64)[inst["owner"]]
    qb = bs[3:7]
    q = _qmul(qb, np.asarray(inst["quat"], np.float32).astype(np.float64))
    q /= np.linalg.norm(q)
    org = bs[0:3] + _rot(qb, np.asarray(inst["pos"], np.float32).astype(np.float64))
    return org + _rot(q, np.asarray(vertices, np.float64))


def _seg_line(o, d, a, b):
    """Paired arrays [n, 3]: distance between the line o + t d (|d| = 1) and the segment [a, b], and t of the line's closest point."""
    e, w = b - a, a - o
    wp = w - np.einsum("nk,nk->n", w, d)[:, None] * d
    ep = e - np.einsum("nk,nk->n", e, d)[:, None] * d
    ee = np.einsum("nk,nk->n", ep, ep)
    s = np.clip(np.where(ee > 0, -np.einsum("nk,nk->n", wp, ep) / np.where(ee > 0, ee, 1.0), 0.0), 0.0, 1.0)
    x = a + s[:, None] * e - o
    t = np.einsum("nk,nk->n", x, d)
    return np.linalg.norm(x - t[:, None] * d, axis=1), t


def trace(o, d, tri, chunk=1 << 20):
    """Rays o + t d ([K, 3] each, |d| = 1) against the triangles tri [T, 3, 3], brute force.  -> per ray: t1 (first hit at t > 0, inf), k1 (its
    triangle, -1), cos1 (|d . n| there), t2 (second hit, inf), tmin_abs (smallest |t| of a plane hit inside a triangle, any sign), edge_t
    [K]: the smallest ray parameter t > 0 at which the ray is within DELTA of a triangle edge (inf if none), sure [K]: some triangle is hit
    at t > 0 with all three of its edges at least DELTA away from the ray."""
    K, T = len(o), len(tri)
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    g = np.cross(e1, e2)
    gn = np.linalg.norm(g, axis=1)
    ok = gn > MIN_CROSS
    e2xv0, v0xe1, v0g = np.cross(e2, v0), np.cross(v0, e1), np.einsum("tk,tk->t", v0, g)
    elen = np.stack([np.linalg.norm(tri[:, 2] - tri[:, 1], axis=1), np.linalg.norm(e2, axis=1), np.linalg.norm(e1, axis=1)], 1)   # the edges on which w, u, v vanish
    t1, k1, cos1 = np.full(K, np.inf), np.full(K, -1, np.int64), np.ones(K)
    t2, tabs, edge_t = np.full(K, np.inf), np.full(K, np.inf), np.full(K, np.inf)
    sure = np.zeros(K, bool)
    step = max(1, chunk // max(T, 1))
    for s in range(0, K, step):
        oo, dd = o[s:s + step], d[s:s + step]
        m = np.cross(oo, dd)
        dg = dd @ g.T                                                    # d . g   [k, T]
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where((dg != 0) & ok[None], 1.0 / np.where(dg != 0, dg, 1.0), np.nan)
            t = (v0g[None] - oo @ g.T) * inv
            # u, v of the header: u = tv . (d x e2) / det, v = d . (tv x e1) / det, det = e1 . (d x e2) = -d . g, tv = o - v0
            u = (m @ e2.T - dd @ e2xv0.T) * -inv
            v = (-(m @ e1.T) - dd @ v0xe1.T) * -inv
            w = 1.0 - u - v
            inside = (u >= 0) & (v >= 0) & (w >= 0)
            tt = np.where(inside & (t > 0), t, np.inf)
            ta = np.where(inside, np.abs(t), np.inf)
        idx = np.argmin(tt, axis=1)
        r = np.arange(len(oo))
        t1[s:s + step] = tt[r, idx]
        k1[s:s + step] = np.where(np.isfinite(tt[r, idx]), idx, -1)
        cos1[s:s + step] = np.abs(dg[r, idx]) / np.where(ok[idx], gn[idx], 1.0)
        if T > 1:
            t2[s:s + step] = np.partition(tt, 1, axis=1)[:, 1]
        tabs[s:s + step] = ta.min(axis=1)
        # edge candidates: the ray's line within DELTA of an edge's LINE needs (in-plane distance) * |d . n| < DELTA, i.e.
        # |barycentric| * |d . g| / |edge| < DELTA (the 3D distance is that over sin(angle(ray, edge)) <= 1); the exact segment test decides.
        with np.errstate(invalid="ignore"):
            adg = np.abs(dg)
            # (in-plane distance to an edge's line) * |d . n| >= DELTA for all three edges: the ray is >= DELTA from every edge of the triangle
            clear = (w * adg >= DELTA * elen[None, :, 0]) & (u * adg >= DELTA * elen[None, :, 1]) & (v * adg >= DELTA * elen[None, :, 2])
            sure[s:s + step] = (clear & (t > 0)).any(axis=1)
            for bary, j, (pa, pb) in ((w, 0, (1, 2)), (u, 1, (2, 0)), (v, 2, (0, 1))):
                cand = np.abs(bary) * adg < DELTA * elen[None, :, j]
                ri, ti = np.nonzero(cand & ok[None])
                if len(ri) == 0:
                    continue
                dist, tc = _seg_line(oo[ri], dd[ri], tri[ti, pa], tri[ti, pb])
                near = (dist < DELTA) & (tc > 0)
                if near.any():
                    cur = edge_t[s:s + step]
                    np.minimum.at(cur, ri[near], tc[near])
                    edge_t[s:s + step] = cur
        # (rays parallel to a triangle's plane, dg == 0, can only be near its edges at grazing incidence: the neighbours' candidates cover them)
    return t1, k1, cos1, t2, tabs, edge_t, sure


# ---------------------------------------------------------------------------------------------------------------- the oracle
def render_view(style, palette, capsules, owner, body_state, camera, W, H, meshes, instances, markers=None, marker_radius=0.05):
    """One view.  As render_oracle.render_view, plus meshes = [(vertices f32 [n, 3], faces [m, 3])] and instances = [dict(mesh, owner, pos,
    quat (xyzw), rgb)].  -> dict(rgba, depth, id, tri (the hit triangle's index in the concatenation of the meshes' faces, -1), excl, excl_rgb)."""
    eye = np.asarray(camera[0], np.float64)
    d = ro.camera_rays(*camera, W, H).reshape(-1, 3)
    P = d.shape[0]
    o = np.broadcast_to(eye, d.shape)
    owner = np.asarray(owner)
    A, B, R = ro.world_capsules(capsules, owner, body_state)
    nb = np.asarray(body_state).shape[0]
    meshed = {int(i["owner"]) for i in instances}
    drawn = (R > 0) & (owner >= 0) & (owner < nb) & ~np.isin(owner, list(meshed))
    cols = [np.asarray(palette[int(ow) % len(palette)], np.float64) for ow in owner]
    ids = list(range(len(R)))
    if markers is not None and marker_radius > 0:
        mk = np.asarray(markers, np.float64)
        A, B = np.concatenate([A, mk]), np.concatenate([B, mk])
        R = np.concatenate([R, np.full(len(mk), float(marker_radius))])
        drawn = np.concatenate([drawn, np.ones(len(mk), bool)])
        cols += [np.asarray(style["marker_color"], np.float64)] * len(mk)
        ids += [ro.MARKER_ID + m for m in range(len(mk))]
    prims = [i for i in range(len(R)) if drawn[i]]
    tri_base = np.concatenate([[0], np.cumsum([len(f) for _, f in meshes])])
    world = []                                   # per instance: triangles [T, 3, 3] in the world, sphere centre, radius
    for ins in instances:
        v, f = meshes[ins["mesh"]]
        vw = world_vertices(ins, v, body_state)
        c = 0.5 * (vw.min(0) + vw.max(0))
        world.append((vw[np.asarray(f)], c, np.linalg.norm(vw - c, axis=1).max() + SPHERE_PAD))

    def in_sphere(oo, dd, c, rad):
        w = c - oo
        tc = np.einsum("nk,nk->n", w, dd)
        return np.linalg.norm(w - tc[:, None] * dd, axis=1) <= rad

    # primary ray
    NPr, NI = len(prims), len(instances)
    T = np.full((NPr + 1 + 2 * NI, P), np.inf)    # prims, ground, first and second hit of every instance
    sil = np.zeros(P, bool)
    for j, i in enumerate(prims):
        T[j], _ = ro.capsule_entry(o, d, A[i], B[i], R[i])
        sil |= np.abs(ro.segment_distance(o, d, A[i], B[i]) - R[i]) < DELTA
    with np.errstate(divide="ignore"):
        T[NPr] = np.where((d[:, 2] < 0) & (eye[2] > 0), -eye[2] / np.where(d[:, 2] < 0, d[:, 2], -1), np.inf)
    ktri = np.full((NI, P), -1, np.int64)
    kcos = np.ones((NI, P))
    edge_t = np.full(P, np.inf)
    for j, (tw, c, rad) in enumerate(world):
        sel = np.nonzero(in_sphere(o, d, c, rad))[0]
        if len(sel) == 0:
            continue
        t1, k1, c1, t2, _, et, _ = trace(o[sel], d[sel], tw)
        T[NPr + 1 + j, sel], T[NPr + 1 + NI + j, sel] = t1, t2
        ktri[j, sel], kcos[j, sel] = k1, c1
        edge_t[sel] = np.minimum(edge_t[sel], et)
    order = np.sort(T, axis=0)
    with np.errstate(invalid="ignore"):
        near2 = (order[1] - order[0] < DELTA) & np.isfinite(order[1])
    k = np.argmin(T, axis=0)
    t = T[k, np.arange(P)]
    hit = np.isfinite(t)
    ground = hit & (k == NPr)
    x = eye + np.where(hit, t, 0)[:, None] * d
    hit_id = np.full(P, -1, np.int64)
    tri_id = np.full(P, -1, np.int64)
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
    graze = np.zeros(P, bool)
    mesh_hit = np.zeros(P, bool)
    for j, ins in enumerate(instances):
        m = hit & (k == NPr + 1 + j)
        if not m.any():
            continue
        mesh_hit |= m
        hit_id[m] = MESH_ID + j
        tri_id[m] = tri_base[ins["mesh"]] + ktri[j, m]
        base[m] = np.asarray(ins["rgb"], np.float32).astype(np.float64)
        tw = world[j][0][ktri[j, m]]
        nn = np.cross(tw[:, 1] - tw[:, 0], tw[:, 2] - tw[:, 0])
        nn /= np.linalg.norm(nn, axis=1, keepdims=True)
        n[m] = np.where(np.einsum("nk,nk->n", nn, d[m])[:, None] > 0, -nn, nn)
        graze[m] = kcos[j, m] < GRAZE
    x[ground, 2] = 0.0
    with np.errstate(invalid="ignore"):
        edge = edge_t <= np.where(hit, t, np.inf) + DELTA

    # shading and the shadow ray
    L = np.asarray(style["light_dir"], np.float64)
    lit = np.maximum(n @ L, 0.0)
    sh = hit & (lit > 0)
    excl_sh = np.zeros(P, bool)
    if sh.any():
        os_ = x[sh] + ro.SHADOW_OFFSET * n[sh]
        Ls = np.broadcast_to(L, os_.shape)
        occ = np.zeros(len(os_), bool)
        ex = np.zeros(len(os_), bool)
        near_edge, sure = np.zeros(len(os_), bool), np.zeros(len(os_), bool)
        for i in prims:
            te, tabs = ro.capsule_entry(os_, Ls, A[i], B[i], R[i])
            occ |= np.isfinite(te)
            ex |= (np.abs(ro.segment_distance(os_, Ls, A[i], B[i]) - R[i]) < DELTA) | (tabs < DELTA)
        for tw, c, rad in world:
            sel = np.nonzero(in_sphere(os_, Ls, c, rad))[0]
            if len(sel) == 0:
                continue
            t1, _, _, _, tabs, et, su = trace(os_[sel], Ls[sel], tw)
            occ[sel] |= np.isfinite(t1)
            ex[sel] |= tabs < DELTA
            near_edge[sel] |= np.isfinite(et)
            sure[sel] |= su
        ex |= near_edge & ~sure
        excl_sh[sh] = ex
        lit_sh = lit[sh]
        lit_sh[occ] = 0.0
        lit[sh] = lit_sh
    shade = np.where(hit, style["ambient"] + style["diffuse"] * lit, 1.0)
    rgb = np.floor(np.clip(base * shade[:, None], 0, 1) * 255 + 0.5).astype(np.uint8)
    rgba = np.concatenate([rgb, np.full((P, 1), 255, np.uint8)], axis=1)
    excl = sil | near2 | line | edge | graze
    return dict(rgba=rgba.reshape(H, W, 4), depth=np.where(hit, t, np.inf).reshape(H, W), id=hit_id.reshape(H, W), tri=tri_id.reshape(H, W),
                excl=excl.reshape(H, W), excl_rgb=(excl | excl_sh).reshape(H, W))


# ---------------------------------------------------------------------------------------------------------------- test scenes
def orbit(center, dist, az_deg, el_deg=30.0, fov_deg=ro.FOV):
    """A camera `dist` from `center`, el_deg above it (every ground ray of a 40 degree view then descends at >= 10 degrees)."""
    az, el = math.radians(az_deg), math.radians(el_deg)
    c = np.asarray(center, np.float64)
    return ro.look(c + dist * np.array([math.sin(az) * math.cos(el), -math.cos(az) * math.cos(el), math.sin(el)]), c, fov_deg=fov_deg)


def _quat_z_to(axis):
    """xyzw quaternion that turns +z into the unit vector axis."""
    z = np.array([0.0, 0.0, 1.0])
    c = float(z @ axis)
    if c < -1 + 1e-9:
        return np.array([1.0, 0.0, 0.0, 0.0])
    q = np.concatenate([np.cross(z, axis), [1.0 + c]])
    return q / np.linalg.norm(q)


def _body_ellipsoids(sc, subdiv, skip=(), rng=None):
    """One ellipsoid per body of the scene's model, around the body's first capsule (semi-axes r, r, half length + r with r = the capsule's
    radius but at least 9 cm: smaller ones have so small triangles that 1e-4 m around their edges is over a tenth of their area; geom frame
    = the capsule's midpoint and axis: not the identity), except the bodies in `skip`.  Colours from a seeded draw."""
    caps, own = sc["capsules"][0], sc["owner"][0]
    meshes, instances = [], []
    nb = sc["body_state"].shape[1]
    for b in range(nb):
        if b in skip:
            continue
        s = [i for i in range(len(own)) if own[i] == b and caps[i, 6] > 0]
        if s:
            a, e, r = caps[s[0], 0:3].astype(np.float64), caps[s[0], 3:6].astype(np.float64), float(caps[s[0], 6])
        else:
            a = e = np.zeros(3)
            r = 0.05
        half = 0.5 * np.linalg.norm(e - a)
        r = max(r, 0.09)
        axis = (e - a) / (2 * half) if half > 1e-9 else np.array([0.0, 0.0, 1.0])
        meshes.append(ellipsoid(subdiv, (r, r, half + r)))
        instances.append(dict(mesh=len(meshes) - 1, owner=b, pos=(0.5 * (a + e)).astype(np.float32), quat=_quat_z_to(axis).astype(np.float32),
                              rgb=rng.uniform(0.2, 0.95, 3).astype(np.float32)))
    return meshes, instances


SCENES = ("tetra", "triangle", "cube", "quad", "axis", "frames_far", "h1_mixed", "g1_all", "ico5")
_Q = np.array([0.18, -0.32, 0.41, 0.0])
_Q[3] = math.sqrt(1.0 - _Q[:3] @ _Q[:3])


@functools.lru_cache(maxsize=None)
def make_scene(name):
    """render_oracle's `h1` scene (`g1` for g1_all) with meshes: -> its dict plus meshes, instances, and the cameras / W / H of this scene.
      tetra / triangle / cube / quad: one instance beside env 0's robot, carried by body 0 (whose capsules vanish); quad is seen from above
      and from below its plane; axis: the cube under a 161 x 121 view whose centre ray is exactly -z; frames_far: env 1's root moved 8 m
      out, rotated geom frames, one ellipsoid mesh instanced three times; h1_mixed: a subdivision-3 ellipsoid on every body but one;
      g1_all: a subdivision-2 ellipsoid on each of the 38 bodies and a second instance on body 0; ico5: one subdivision-5 sphere, 64 x 48."""
    rng = np.random.default_rng(50 + SCENES.index(name))
    sc = dict(ro.make_scene("g1" if name == "g1_all" else "h1"))
    sc["body_state"] = sc["body_state"].copy()
    W, H = 160, 120
    root = sc["body_state"][0, 0, 0:3].astype(np.float64)
    q0 = sc["body_state"][0, 0, 3:7].astype(np.float64)
    off = np.array([0.9, 0.2, -root[2] + 0.45])                        # instance centre: beside the robot, 0.45 m above the ground
    inv_q0 = np.concatenate([-q0[:3], q0[3:]])
    pos = _rot(inv_q0, off).astype(np.float32)                          # (in body 0's frame)
    center = root + _rot(q0, pos.astype(np.float64))
    one = lambda mesh, quat=_Q, rgb=(0.2, 0.7, 0.9): ([mesh], [dict(mesh=0, owner=0, pos=pos, quat=np.asarray(quat, np.float32), rgb=np.asarray(rgb, np.float32))])
    if name == "tetra":
        meshes, instances = one(tetrahedron(0.5))
        cams = [(0, orbit(center, 1.2, 20.0)), (0, orbit(center, 1.3, 200.0, 45.0))]
    elif name == "triangle":
        meshes, instances = one((np.array([(-0.3, -0.25, 0.0), (0.35, -0.2, 0.05), (0.0, 0.4, -0.05)], np.float32), np.array([(0, 1, 2)])))
        cams = [(0, orbit(center, 1.0, 75.0, 50.0)), (0, orbit(center, 1.0, 250.0, 35.0))]
    elif name == "cube":
        meshes, instances = one(cube(0.35))
        cams = [(0, orbit(center, 1.2, 130.0)), (0, orbit(center, 1.2, -40.0, 55.0))]
    elif name == "quad":
        # the mesh plane stands steeply (its normal 70 degrees off the vertical), so that one camera above the ground sees each face
        nrm = np.array([math.sin(math.radians(70.0)), 0.0, math.cos(math.radians(70.0))])
        meshes, instances = one(quad_grid(0.5, 6), quat=_qmul(inv_q0, _quat_z_to(nrm)))
        cams = [(0, orbit(center, 1.1, 90.0, 35.0)), (0, orbit(center, 1.1, 270.0, 35.0))]
    elif name == "axis":
        meshes, instances = one(cube(0.35), quat=(0.0, 0.0, 0.0, 1.0))
        sc["body_state"][0, 0, 3:7] = (0.0, 0.0, 0.0, 1.0)             # body 0 axis-aligned: the cube's faces are too
        pos = off.astype(np.float32)
        instances[0]["pos"] = pos
        center = root + pos.astype(np.float64)
        W, H = 161, 121
        cams = [(0, ro.look((center[0], center[1], center[2] + 1.2), (center[0], center[1], 0.0), up=(0.0, 1.0, 0.0), fov_deg=ro.FOV))]
    elif name == "frames_far":
        shift = np.array([8.0, -8.0, 0.0]) - np.concatenate([sc["body_state"][1, 0, 0:2], [0.0]])
        sc["body_state"][1, :, 0:3] += shift.astype(np.float32)
        sc["markers"] = sc["markers"].copy()
        sc["markers"][1] += shift.astype(np.float32)
        meshes = [ellipsoid(3, (0.10, 0.14, 0.20))]
        instances = []
        for b, p in ((0, (0.0, 0.0, 0.05)), (2, (0.02, 0.0, -0.2)), (7, (0.0, 0.03, -0.15))):
            q = rng.normal(size=4)
            instances.append(dict(mesh=0, owner=b, pos=np.asarray(p, np.float32), quat=(q / np.linalg.norm(q)).astype(np.float32),
                                  rgb=rng.uniform(0.2, 0.95, 3).astype(np.float32)))
        r1 = sc["body_state"][1, 0, 0:3].astype(np.float64)
        cams = [(1, orbit((r1[0], r1[1], 0.8), 1.5, 30.0)), (1, orbit((r1[0], r1[1], 0.8), 1.5, 190.0, 40.0))]
    elif name == "h1_mixed":
        meshes, instances = _body_ellipsoids(sc, 3, skip=(4,), rng=rng)
        cams = [(0, orbit((root[0], root[1], 0.9), 2.4, 25.0)), (1, orbit(tuple(sc["body_state"][1, 0, 0:2].astype(np.float64)) + (0.9,), 2.4, 160.0, 35.0))]
    elif name == "g1_all":
        meshes, instances = _body_ellipsoids(sc, 2, rng=rng)
        assert len(instances) == 38
        meshes.append(ellipsoid(2, (0.05, 0.08, 0.05)))
        instances.append(dict(mesh=len(meshes) - 1, owner=0, pos=np.array([0.0, 0.0, 0.22], np.float32), quat=_Q.astype(np.float32),
                              rgb=np.array([0.9, 0.9, 0.2], np.float32)))
        cams = [(0, orbit((root[0], root[1], 0.7), 1.9, 60.0)), (1, orbit(tuple(sc["body_state"][1, 0, 0:2].astype(np.float64)) + (0.7,), 1.9, 230.0, 35.0))]
    else:
        v, f = icosphere(5)
        meshes, instances = one(((0.3 * v).astype(np.float32), f))
        W, H = 64, 48
        cams = [(0, orbit(center, 1.3, 100.0))]
    sc.update(meshes=meshes, instances=instances, cameras=cams, W=W, H=H)
    return sc


@functools.lru_cache(maxsize=None)
def render_scene(name, markers=True):
    """The oracle's views of make_scene(name), computed once per process."""
    from phc_amd import render as R
    sc = make_scene(name)
    return [render_view(R.STYLE, R.PALETTE, sc["capsules"][0], sc["owner"][0], sc["body_state"][env], cam, sc["W"], sc["H"], sc["meshes"],
                        sc["instances"], markers=sc["markers"][env] if markers else None) for env, cam in sc["cameras"]]
