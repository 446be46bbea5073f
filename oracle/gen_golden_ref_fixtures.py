"""Fixtures that let the reference-checking CPU tests run without a reference checkout (tests/golden/).

    python oracle/gen_golden_ref_fixtures.py            (needs the reference checkout, see ref_shim.REFERENCE_ROOT)

What it records, all of it data the reference's programs read or produce:
  ref_cfg/                    the reference's yaml config tree (phc/data/cfg), copied as is
  ref_mjcf/                   the SMPL MJCF files (phc/data/assets/mjcf) and poselib's ant.xml skeleton fixture, copied as is
  ref_robot/<robot>/          the H1 / G1 MJCF files (phc/data/assets/robot), copied as is
  ref_robot_meshes_<robot>    per STL mesh of that robot: the vertices on the boundary of the mesh's convex hull, in order of first
                              appearance (every vertex that any direction's support point can be, so the compiler's hull contact points
                              come out the same as from the full STL files; interior vertices and the triangles are dropped)
  ref_running_mean_std        the reference's RunningMeanStd on a seeded input sequence: outputs and final moments
  ref_replay_buffer           the reference's ReplayBuffer on a seeded store / sample sequence: storage, samples, count, head
  ref_bypass_mlp              the reference's MLP (units 2048-1024-512, SiLU): state-dict keys and shapes, and its actions on seeded
                              inputs with seeded weights loaded
"""
import os
import shutil
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
from phc_amd.model import _stl_vertices  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
SMPL_MJCF = ["smpl_0_humanoid.xml", "smpl_1_humanoid.xml", "smpl_2_humanoid.xml", "smpl_humanoid.xml"]
ROBOTS = {"h1": "unitree_h1/h1.xml", "g1": "unitree_g1/g1.xml"}


def hull_boundary_vertices(v):
    """Distinct vertices of `v` (in order of first appearance) that lie on the boundary of its convex hull."""
    from scipy.spatial import ConvexHull
    _, first = np.unique(v, axis=0, return_index=True)
    u = v[np.sort(first)]
    h = ConvexHull(u.astype(np.float64))
    scale = float(np.abs(u).max())
    dist = np.full(len(u), -np.inf)
    for i in range(0, len(u), 4096):
        dist[i:i + 4096] = (u[i:i + 4096].astype(np.float64) @ h.equations[:, :3].T + h.equations[:, 3]).max(1)
    return u[dist >= -1e-5 * scale]


def seeded_state_dict(keys, shapes, seed):
    """Weights for the MLP fixture: N(0, 1 / fan_in) matrices and N(0, 0.01^2) biases from one seeded generator, key by key."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in zip(keys, shapes):
        s = tuple(int(x) for x in s if x)    # (out, in) of a matrix, (out, 0) of a bias
        sd[k] = torch.randn(s, generator=g) * (s[1] ** -0.5 if len(s) == 2 else 0.01)
    return sd


def main():
    ref = ref_shim.REFERENCE_ROOT
    assert os.path.isdir(os.path.join(ref, "phc")), "needs the reference checkout (not the archive)"
    dst = os.path.join(OUT, "ref_cfg")
    shutil.rmtree(dst, ignore_errors=True)
    shutil.copytree(os.path.join(ref, "phc", "data", "cfg"), dst)
    os.makedirs(os.path.join(OUT, "ref_mjcf"), exist_ok=True)
    for x in SMPL_MJCF:
        shutil.copyfile(os.path.join(ref, "phc", "data", "assets", "mjcf", x), os.path.join(OUT, "ref_mjcf", x))
    shutil.copyfile(os.path.join(ref, "poselib", "poselib", "skeleton", "tests", "ant.xml"), os.path.join(OUT, "ref_mjcf", "ant.xml"))
    for rb, xml in ROBOTS.items():
        src = os.path.join(ref, "phc", "data", "assets", "robot", xml)
        os.makedirs(os.path.join(OUT, "ref_robot", rb), exist_ok=True)
        shutil.copyfile(src, os.path.join(OUT, "ref_robot", rb, os.path.basename(xml)))
        mdir = os.path.join(os.path.dirname(src), "meshes")
        meshes = {f: hull_boundary_vertices(_stl_vertices(os.path.join(mdir, f)).astype(np.float32)) for f in sorted(os.listdir(mdir))}
        np.savez_compressed(os.path.join(OUT, f"ref_robot_meshes_{rb}.npz"), **meshes)

    ref_shim.install()
    torch.manual_seed(0)
    rms = ref_shim.ref_module("phc.utils.running_mean_std").RunningMeanStd((7,))
    rms.train()
    xs = [torch.randn(50, 7) * (i + 1) + i for i in range(4)]
    ys = [rms(x) for x in xs]
    np.savez_compressed(os.path.join(OUT, "ref_running_mean_std.npz"), xs=torch.stack(xs).numpy(), ys=torch.stack(ys).detach().numpy(),
                        running_mean=rms.running_mean.numpy(), running_var=rms.running_var.numpy(), count=rms.count.numpy())

    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_replay_buffer", os.path.join(ref, "phc", "learning", "replay_buffer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(42)
    rb = mod.ReplayBuffer(37, "cpu")
    g = torch.Generator().manual_seed(1)
    out = {}
    for i, (n_store, n_sample) in enumerate(((10, 5), (20, 16), (15, 30), (37, 8), (3, 50), (9, 37))):
        rb.store({"amp_obs": torch.randn(n_store, 4, generator=g)})
        out[f"sample_{i}"] = rb.sample(n_sample)["amp_obs"].numpy()
    np.savez_compressed(os.path.join(OUT, "ref_replay_buffer.npz"), data=rb._data_buf["amp_obs"].numpy(), total_count=np.int64(rb.get_total_count()),
                        head=np.int64(rb._head), **out)

    MLP = ref_shim.ref_module("phc.learning.mlp").MLP
    mlp = MLP(input_dim=934, output_dim=69, units=[2048, 1024, 512], activation="silu")
    keys = list(mlp.state_dict())
    shapes = [list(v.shape) + [0] * (2 - v.dim()) for v in mlp.state_dict().values()]
    mlp.load_state_dict(seeded_state_dict(keys, shapes, 4))
    x = torch.randn(5, 934, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want = mlp(x)
    np.savez_compressed(os.path.join(OUT, "ref_bypass_mlp.npz"), keys=np.array(keys), shapes=np.array(shapes, dtype=np.int64), seed=np.int64(4),
                        x=x.numpy(), actions=want.numpy())
    print("wrote the reference fixtures under", OUT)


if __name__ == "__main__":
    main()
