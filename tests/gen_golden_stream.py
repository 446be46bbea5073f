"""TEST INFRASTRUCTURE -- golden for phc_stream_track: the keypoint-stream path of HumanoidImMCPDemo from the reference's OWN code.

Run where the reference checkout is (oracle/ref_shim.py finds it):  python tests/gen_golden_stream.py   -> tests/golden/stream_track.npz

The reference's module imports the simulator, aiohttp, cv2 and a websocket client the shim cannot supply, so nothing of it is imported: the `obs_v == 7`
branch of `HumanoidImMCPDemo._compute_task_obs_demo` (humanoid_im_mcp_demo.py:252-310), the module's `smpl_2_mujoco` table and the assignments of `__init__`
that the branch reads (`to_isaac_mat`, `mean_limb_lengths`, the three deques, `prev_ref_body_pos`, `close_distance`) are cut out of the file's AST and executed
on a stand-in `self`, the way tests/gen_golden_teleop.py cuts the reward methods out.  `requests.get` is a stub that returns the frame, `Tensor.cuda` is the
identity; `compute_imitation_observations_v7` and `SkeletonMotion._compute_velocity` are the reference's, through the shim.

16 envs and 35 consecutive frames (the deque of 30 fills and wraps), full-body tracking, frames in the SMPL joint order and y-up as the reference expects them.
Envs 0-5 stay within close_distance (0.5) of their target root, 6-10 between the two distances, 11-15 beyond far_distance (3); no env's distance lies within
1e-3 (relative) of either threshold in any step -- asserted below -- so that no gate can flip on rounding.  The body state is one per env (the same in every
step: the file stays below its size limit).  The reference's start is kept: prev_ref_body_pos = 0, so the first velocity is position / dt; the launch
reproduces it with has_prev preset.  The file holds arrays and names only."""
import ast
import collections
import os
import sys
import types

import numpy as np
import scipy.ndimage
import torch
from scipy.spatial.transform import Rotation as sRot

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

ref_shim.install()
import stream_util as su  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "stream_track.npz")
F = np.float32
N, STEPS, NB, MARGIN, FAR = 16, 35, 24, 1e-3, 3.0
INIT_FIELDS = ("to_isaac_mat", "mean_limb_lengths", "root_pos_acc", "body_rot_acc", "body_pos_acc", "prev_ref_body_pos", "close_distance")


def reference_code():
    path = ref_shim.data_path(os.path.join("phc", "env", "tasks", "humanoid_im_mcp_demo.py"))
    tree = ast.parse(open(path).read())
    table = next(n for n in tree.body if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "smpl_2_mujoco")
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "HumanoidImMCPDemo")
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    init = [n for n in fns["__init__"].body if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) in tuple("self." + f for f in INIT_FIELDS)]
    assert len(init) == len(INIT_FIELDS)
    v6 = next(n for n in fns["_compute_task_obs_demo"].body if isinstance(n, ast.If) and ast.unparse(n.test) == "self.obs_v == 6")
    v7 = v6.orelse[0]
    assert isinstance(v7, ast.If) and ast.unparse(v7.test) == "self.obs_v == 7"
    comp = lambda body, what: compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), f"<humanoid_im_mcp_demo.py: {what}>", "exec")
    return comp([table], "smpl_2_mujoco"), comp(init, "__init__ assignments"), comp(v7.body, "obs_v 7 branch")


def inputs():
    """Frames [STEPS, N, 24, 3] in the SMPL joint order, y-up; one body state per env [N, 24, 13] (z-up, the simulator's frame)."""
    rng = np.random.default_rng(317)
    # the simulator-frame offset of each env's target root from the origin: 0 | 1 - 2 m | 4 - 5 m
    r = np.concatenate([np.zeros(6), rng.uniform(1.0, 2.0, 5), rng.uniform(4.0, 5.0, 5)])
    ang = rng.uniform(0, 2 * np.pi, N)
    sim_off = np.stack([r * np.cos(ang), r * np.sin(ang), np.zeros(N)], axis=-1)
    src_off = np.stack([sim_off[:, 0], -sim_off[:, 2], sim_off[:, 1]], axis=-1)    # to_isaac_mat maps (x, y, z) to (x, z, -y)
    frames = su.keypoint_stream(STEPS, N, NB, seed=318, offset=src_off, drift=0.1)
    rbs = su.body_states(1, N, NB, seed=319)[0]
    rbs[:, 0, :3] = rng.uniform(-0.1, 0.1, (N, 3)).astype(F)
    return frames, rbs


def main():
    table, init, branch = reference_code()
    him = ref_shim.ref_module("phc.env.tasks.humanoid_im")
    skel = ref_shim.ref_module("poselib.poselib.skeleton.skeleton3d")
    frame_box = [None]
    requests = types.SimpleNamespace(get=lambda url: types.SimpleNamespace(json=lambda: {"j3d": frame_box[0]}))
    space = {"torch": torch, "np": np, "sRot": sRot, "deque": collections.deque, "filters": scipy.ndimage, "requests": requests, "SERVER": "0.0.0.0",
             "SkeletonMotion": skel.SkeletonMotion, "humanoid_im": him}
    exec(table, space)
    names, parents = su.smpl_model()
    me = types.SimpleNamespace(num_envs=N, device="cpu", obs_v=7, zero_out_far=True, far_distance=FAR, _has_upright_start=True,
                               skeleton_trees=[types.SimpleNamespace(parent_indices=list(parents))], _track_bodies_id=torch.arange(NB))
    exec(init, space, {"self": me})
    frames, rbs = inputs()
    body = torch.from_numpy(rbs)
    rec = {k: [] for k in ("ref_body_pos", "ref_body_vel", "task_obs", "distance")}
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for s in range(STEPS):
            frame_box[0] = frames[s].astype(np.float64)
            loc = {"self": me, "root_pos": body[:, 0, :3], "root_rot": body[:, 0, 3:7], "body_pos_subset": body[:, :, :3][:, me._track_bodies_id],
                   "body_vel_subset": body[:, :, 7:10][:, me._track_bodies_id]}
            exec(branch, space, loc)
            rec["ref_body_pos"].append(loc["ref_rb_pos"].numpy().copy())
            rec["ref_body_vel"].append(loc["ref_body_vel"].numpy().copy())
            rec["task_obs"].append(loc["obs"].numpy().copy())
            rec["distance"].append(loc["distance"].numpy().copy())
    finally:
        torch.Tensor.cuda = cuda
    dist = np.stack(rec["distance"]).astype(np.float64)
    for thr in (float(me.close_distance), FAR):
        assert not (np.abs(dist - thr) <= MARGIN * np.maximum(dist, thr)).any(), f"a distance lies within {MARGIN} of the threshold {thr}"
    cls = (dist > me.close_distance).astype(int) + (dist > FAR)
    assert all((cls == c).all(axis=0).any() for c in (0, 1, 2)), "an env must sit in each distance class for the whole run"
    out = {k: np.stack(v).astype(F) for k, v in rec.items()}
    out.update(frames=frames, rigid_body_state=rbs, smpl_2_mujoco=np.array(space["smpl_2_mujoco"], np.int32), to_isaac_mat=me.to_isaac_mat.numpy().astype(np.float64),
               mean_limb_lengths=np.asarray(me.mean_limb_lengths, np.float64).reshape(-1), close_distance=np.array(me.close_distance, np.float64),
               far_distance=np.array(FAR, np.float64), dt=np.array(1 / 30, np.float64), window=np.array(me.root_pos_acc.maxlen, np.int32),
               body_names=np.array(names))
    np.savez_compressed(OUT, **out)
    print("classes per env (last step):", cls[-1], "\nwrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
