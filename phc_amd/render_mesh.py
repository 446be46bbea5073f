"""Triangle meshes for the offscreen renderer: the host side of `phc_render_mesh` (csrc/phc_render_mesh.hip, include/phc_amd.h).

  load_stl            binary or ASCII STL -> vertices, faces
  build_bvh           numpy bounding-volume hierarchy: median split on the longest axis of the centroid bounds, depth-first layout with a
                      skip link per node, the permutation back to the caller's triangle order kept
  read_mjcf_visuals   the visual mesh geoms of a robot's MJCF, per body
  MeshSet             several meshes + their posed instances as the device arrays of phc_render_meshes_t
  task_mesh_set       the MeshSet of a task from `+render.meshes=<mjcf>` (body names matched to the task's)
  render              one phc_render_mesh call

The package ships no meshes: the user points at their own copy of the robot's files.  Nothing here runs unless `render.meshes` is set."""
import ctypes as C
import os
import xml.etree.ElementTree as ET

import numpy as np

from . import _lib as L

LEAF_SIZE = 2   # triangles per leaf of build_bvh: the fastest of 2 / 4 / 8 on the MI355X (profiles/render_mesh/README.md)


# ---------------------------------------------------------------------------------------------------------------- STL
def load_stl(path):
    """-> vertices float32 [NV, 3] (duplicates merged), faces int32 [NT, 3] in file order.  Binary STL (80-byte header, uint32 count, 50-byte
    records) is recognised by its size; anything else is read as ASCII (`vertex x y z` lines, three per facet)."""
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw, dtype="<u4", count=1, offset=80)[0]) if len(raw) >= 84 else -1
    if n >= 0 and len(raw) == 84 + 50 * n:
        rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), count=n, offset=84)
        tri = rec["v"].reshape(-1, 3).astype(np.float32)
    else:
        vals = [ln.split()[1:4] for ln in raw.decode("ascii", "replace").splitlines() if ln.strip().startswith("vertex")]
        tri = np.asarray(vals, dtype=np.float64).astype(np.float32).reshape(-1, 3)
    if len(tri) == 0 or len(tri) % 3:
        raise ValueError(f"{path}: not an STL with whole triangles")
    verts, inv = np.unique(tri, axis=0, return_inverse=True)
    return np.ascontiguousarray(verts, np.float32), np.ascontiguousarray(inv.reshape(-1, 3), np.int32)


# ---------------------------------------------------------------------------------------------------------------- BVH
def build_bvh(vertices, faces, leaf_size=LEAF_SIZE):
    """-> dict(nodes: structured [NN] (lo f32[3], skip i32, hi f32[3], leaf i32: phc_bvh_node_t), order int32 [NT]: order[k] = the caller's
    index of the triangle at leaf position k (tri_perm), radius / center of the bounding sphere).  Depth-first layout: the first child of an
    interior node n is n + 1, skip = the node after n's subtree (-1 after the last).  Boxes are the exact fp32 bounds of their triangles."""
    assert 1 <= leaf_size <= 15
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64)
    corners = v[f]                                   # [NT, 3, 3]
    tlo, thi = corners.min(1), corners.max(1)
    cen = corners.astype(np.float64).mean(1)
    lo, hi, skip, leaf, order = [], [], [], [], []

    def build(idx):
        n = len(lo)
        lo.append(tlo[idx].min(0))
        hi.append(thi[idx].max(0))
        skip.append(-1)
        if len(idx) <= leaf_size:
            leaf.append(16 * len(order) + len(idx))
            order.extend(idx.tolist())
        else:
            leaf.append(-1)
            c = cen[idx]
            axis = int(np.argmax(c.max(0) - c.min(0)))
            half = len(idx) // 2
            part = np.argpartition(c[:, axis], half - 1) if c[:, axis].max() > c[:, axis].min() else np.arange(len(idx))
            build(idx[np.sort(part[:half])])
            build(idx[np.sort(part[half:])])
        skip[n] = len(lo)

    build(np.arange(len(f)))
    nodes = np.zeros(len(lo), dtype=np.dtype([("lo", "<f4", 3), ("skip", "<i4"), ("hi", "<f4", 3), ("leaf", "<i4")]))
    nodes["lo"], nodes["hi"], nodes["leaf"] = np.asarray(lo), np.asarray(hi), leaf
    sk = np.asarray(skip)
    nodes["skip"] = np.where(sk >= len(lo), -1, sk)
    center = 0.5 * (nodes["lo"][0].astype(np.float64) + nodes["hi"][0].astype(np.float64))
    used = v[np.unique(f)].astype(np.float64)
    radius = float(np.linalg.norm(used - center, axis=1).max())
    return dict(nodes=nodes, order=np.asarray(order, np.int32), center=center.astype(np.float32), radius=radius)


# ---------------------------------------------------------------------------------------------------------------- MJCF
def _floats(s, default):
    return np.asarray([float(x) for x in s.split()], np.float64) if s else np.asarray(default, np.float64)


def read_mjcf_visuals(path):
    """The visual mesh geoms of an MJCF: -> list of dict(body, file (absolute path of the STL), scale [3], pos [3], quat xyzw [4], rgba [4]) in
    document order.  A geom is visual when contype = 0 and conaffinity = 0 after its defaults (the top-level <default>, a named class given by
    the geom's `class` or an enclosing body's `childclass`, nested classes inheriting) are applied.  ValueError when the file has no such geom
    or an STL it names is missing."""
    root = ET.parse(path).getroot()
    comp = root.find("compiler")
    meshdir = os.path.join(os.path.dirname(os.path.abspath(path)), comp.attrib.get("meshdir", "") if comp is not None else "")
    files = {}
    for a in root.findall("asset"):
        for me in a.findall("mesh"):
            files[me.attrib.get("name", os.path.splitext(os.path.basename(me.attrib["file"]))[0])] = (
                os.path.join(meshdir, me.attrib["file"]), _floats(me.attrib.get("scale"), [1, 1, 1]))
    top, classes = {}, {}

    def walk_defaults(node, inherited):
        for d in node.findall("default"):
            attrs = dict(inherited)
            if d.find("geom") is not None:
                attrs.update(d.find("geom").attrib)
            if "class" in d.attrib:
                classes[d.attrib["class"]] = attrs
            walk_defaults(d, attrs)

    dflt = root.find("default")
    if dflt is not None:
        if dflt.find("geom") is not None:
            top = dict(dflt.find("geom").attrib)
        walk_defaults(dflt, top)
    out = []

    def walk(body, childclass):
        childclass = body.attrib.get("childclass", childclass)
        for g in body.findall("geom"):
            cls = g.attrib.get("class", childclass)
            if cls is not None and cls not in classes:
                raise ValueError(f"{path}: geom of body {body.attrib.get('name')} uses the unknown default class {cls}")
            at = dict(classes[cls] if cls is not None else top, **g.attrib)
            if at.get("type") != "mesh" or int(at.get("contype", 1)) != 0 or int(at.get("conaffinity", 1)) != 0:
                continue
            if at.get("mesh") not in files:
                raise ValueError(f"{path}: geom of body {body.attrib.get('name')} names the mesh {at.get('mesh')}, which <asset> does not list")
            f, scale = files[at["mesh"]]
            if not os.path.exists(f):
                raise ValueError(f"{path}: the mesh file {f} of body {body.attrib.get('name')} is missing")
            w, x, y, z = _floats(at.get("quat"), [1, 0, 0, 0])
            out.append(dict(body=body.attrib.get("name"), file=f, scale=scale, pos=_floats(at.get("pos"), [0, 0, 0]),
                            quat=np.array([x, y, z, w]), rgba=_floats(at.get("rgba"), [0.5, 0.5, 0.5, 1.0])))
        for b in body.findall("body"):
            walk(b, childclass)

    for b in root.find("worldbody").findall("body"):
        walk(b, None)
    if not out:
        raise ValueError(f"{path}: no visual mesh geoms (type=mesh with contype=0 conaffinity=0, directly or through a default class)")
    return out


# ---------------------------------------------------------------------------------------------------------------- mesh sets
class MeshSet:
    """Meshes and their instances, concatenated into the arrays of phc_render_meshes_t.
      add_mesh(vertices, faces) -> mesh index;  add_instance(mesh, owner, pos, quat_xyzw, rgb);  upload(device) -> self
    After upload(), `struct` is the phc_render_meshes_t (it points into tensors held here: keep the MeshSet alive while it is in use)."""

    def __init__(self, leaf_size=LEAF_SIZE):
        self.leaf_size = leaf_size
        self.vertices, self.triangles, self.tri_perm, self.nodes = [], [], [], []
        self.meshes = []        # (root node, center, radius, first triangle, triangle count)
        self.instances = []     # (mesh, owner, pos, quat, rgb)
        self._nv = self._nt = self._nn = 0
        self.struct = None

    def add_mesh(self, vertices, faces):
        v, f = np.asarray(vertices, np.float32), np.asarray(faces, np.int32)
        if f.ndim != 2 or f.shape[1] != 3 or len(f) == 0 or f.min() < 0 or f.max() >= len(v):
            raise ValueError("faces must be [NT >= 1, 3] indices into vertices")
        b = build_bvh(v, f, self.leaf_size)
        nodes = b["nodes"].copy()
        nodes["skip"] = np.where(nodes["skip"] < 0, -1, nodes["skip"] + self._nn)
        nodes["leaf"] = np.where(nodes["leaf"] < 0, -1, nodes["leaf"] + 16 * self._nt)
        self.vertices.append(v)
        self.triangles.append(f[b["order"]] + self._nv)
        self.tri_perm.append(b["order"] + self._nt)           # (the caller's order: the meshes' faces one after the other)
        self.nodes.append(nodes)
        self.meshes.append((self._nn, b["center"], float(np.nextafter(np.float32(b["radius"]), np.float32(np.inf))), self._nt, len(f)))
        self._nv, self._nt, self._nn = self._nv + len(v), self._nt + len(f), self._nn + len(nodes)
        return len(self.meshes) - 1

    def add_instance(self, mesh, owner, pos=(0.0, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0), rgb=(0.5, 0.5, 0.5)):
        self.instances.append((int(mesh), int(owner), np.asarray(pos, np.float32), np.asarray(quat, np.float32), np.asarray(rgb, np.float32)))
        return len(self.instances) - 1

    def instance_array(self):
        arr = (L.MeshInstance * max(1, len(self.instances)))()
        for i, (m, owner, pos, quat, rgb) in enumerate(self.instances):
            root, center, radius = self.meshes[m][:3]
            arr[i].owner, arr[i].root, arr[i].radius = owner, root, radius
            arr[i].pos[:], arr[i].quat[:], arr[i].center[:], arr[i].rgb[:] = pos.tolist(), quat.tolist(), center.tolist(), rgb.tolist()
        return arr

    def arrays(self):
        """-> vertices f32 [NV, 3], triangles i32 [NT, 3], tri_perm i32 [NT], nodes (structured) [NN]"""
        return (np.concatenate(self.vertices), np.concatenate(self.triangles).astype(np.int32), np.concatenate(self.tri_perm).astype(np.int32),
                np.concatenate(self.nodes))

    def upload(self, device="cuda"):
        import torch
        if self._nt > L.RENDER_MAX_TRIANGLES or len(self.instances) > L.RENDER_MAX_INSTANCES:
            raise ValueError(f"{self._nt} triangles / {len(self.instances)} instances: above the renderer's maxima "
                             f"({L.RENDER_MAX_TRIANGLES} / {L.RENDER_MAX_INSTANCES})")
        v, t, p, n = self.arrays()
        self._host = self.instance_array()
        inst = np.frombuffer(self._host, dtype=np.uint8)[:C.sizeof(L.MeshInstance) * len(self.instances)]
        self._dev = dict(v=torch.from_numpy(v).to(device), t=torch.from_numpy(t).to(device), p=torch.from_numpy(p).to(device),
                         n=torch.from_numpy(n.view(np.uint8).reshape(-1).copy()).to(device),
                         i=torch.from_numpy(inst.copy() if len(inst) else np.zeros(16, np.uint8)).to(device))
        s = L.RenderMeshes()
        s.num_vertices, s.num_triangles, s.num_nodes, s.num_instances = len(v), len(t), len(n), len(self.instances)
        s.vertices, s.triangles, s.tri_perm, s.nodes = (self._dev[k].data_ptr() for k in "vtpn")
        s.instances = C.cast(self._host, C.POINTER(L.MeshInstance))
        s.instances_dev = self._dev["i"].data_ptr()
        self.struct = s
        return self


def task_mesh_set(task, mjcf, color="asset"):
    """The MeshSet of `+render.meshes=<mjcf>` on a task's device: every visual mesh geom of the file on the task body of the same name.
    color: "asset" = the geom's MJCF rgba, "palette" = the body palette of the capsule renderer."""
    from .render import PALETTE
    if color not in ("asset", "palette"):
        raise ValueError(f"render.mesh_color={color}: asset or palette")
    if getattr(task, "has_shape_variation", False):
        raise ValueError("render.meshes with robot.has_shape_variation: one mesh set serves all envs, per-env body shapes cannot be drawn")
    if not os.path.exists(mjcf):
        raise ValueError(f"render.meshes: {mjcf} does not exist")
    names = list(task._body_names)
    ms, loaded = MeshSet(), {}
    for g in read_mjcf_visuals(mjcf):
        if g["body"] not in names:
            raise ValueError(f"{mjcf}: body {g['body']} carries a visual mesh but is not a body of the task ({', '.join(names)})")
        key = (g["file"], tuple(g["scale"]))
        if key not in loaded:
            v, f = load_stl(g["file"])
            loaded[key] = ms.add_mesh(v * g["scale"].astype(np.float32), f)
        owner = names.index(g["body"])
        ms.add_instance(loaded[key], owner, g["pos"], g["quat"], g["rgba"][:3] if color == "asset" else PALETTE[owner % len(PALETTE)])
    return ms.upload(task.device)


def render(scene, meshes, cameras, env_ids, width, height, depth=False, hit_id=False, tri_id=False, device="cuda", lib=None):
    """One phc_render_mesh call on the current stream (meshes: an uploaded MeshSet or None): phc_amd.render.render with meshes.  -> rgba uint8
    [V, H, W, 4] (+ depth f32, hit_id i32, tri_id i32 [V, H, W] when asked for), on the device."""
    import torch
    lib = lib or L.load()
    V = len(env_ids)
    cams = (L.Camera * V)(*[c.struct(e) for c, e in zip(cameras, env_ids)])
    rgba = torch.empty((V, height, width, 4), dtype=torch.uint8, device=device)
    dep = torch.empty((V, height, width), dtype=torch.float32, device=device) if depth else None
    ids = torch.empty((V, height, width), dtype=torch.int32, device=device) if hit_id else None
    tri = torch.empty((V, height, width), dtype=torch.int32, device=device) if tri_id else None
    L.check(lib.phc_render_mesh(C.byref(scene), C.byref(meshes.struct) if meshes is not None else None, cams, V, int(width), int(height),
                                rgba.data_ptr(), dep.data_ptr() if depth else None, ids.data_ptr() if hit_id else None,
                                tri.data_ptr() if tri_id else None, torch.cuda.current_stream().cuda_stream), "phc_render_mesh")
    out = (rgba,) + tuple(x for x in (dep, ids, tri) if x is not None)
    return out if len(out) > 1 else rgba
