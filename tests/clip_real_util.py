"""Shared by tests/test_clip_real_cpu.py and tests/test_clip_real_gpu.py: the host build of phc_amd/csrc/phc_clip_real.h (tests/clip_real_shim.cpp, g++), the
three trees, the constructed robot clips, the oracle (the robot branch of `_run_clip_job`: the existing host path, never the code under test) with the
conditions on its own intermediate values, and the field-by-field comparison at the tolerances that follow from "both sides compute in fp64 and round once"."""
import ctypes as C
import functools
import types

import numpy as np

from clip_util import ANG_FLOOR, EPS32, GUARD
import host_build
LENGTHS = (3, 4, 8, 9, 16, 17, 18, 40)      # the filter radius (8) exceeds, meets and undershoots the clip; 3 frames: the dvs quirk at its edge
FPS = (30, 60, 30, 60, 60, 30, 60, 30)
TREES = ("h1", "g1", "chain")
SEED = {"h1": 3, "g1": 3, "chain": 3}
EINVAL, EUNSUPPORTED = -1, -2
POINTERS = ("parents", "offsets", "rest_mat", "pose_aa", "trans", "clip_start", "clip_dt", "contact_body", "contact_pos", "contact_radius", "scratch", "frames")
# (field, value, code) phc_clip_process_real must refuse, for the chain (115 frames, 8 clips, 3 + 1 bodies, stride 52)
BAD_ARGS = (("num_clips", 0, EINVAL), ("num_clips", -1, EINVAL), ("num_bodies", 0, EINVAL), ("num_bodies", -1, EINVAL), ("num_ext", -1, EINVAL),
            ("num_contacts", 0, EINVAL), ("num_contacts", -1, EINVAL), ("num_ext", 62, EUNSUPPORTED), ("frame_stride", 48, EINVAL), ("frame_stride", 56, EINVAL),
            ("frame_stride", 0, EINVAL), ("scratch_bytes", 0, EINVAL), ("num_frames", 23, EINVAL), ("num_frames", 1 << 40, EUNSUPPORTED))


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("clip_real_shim.cpp", "phc_clip_real.hip")
    lib.clip_real_args_check_of.argtypes = [C.POINTER(L.ClipRealArgs)]
    lib.clip_real_args_check_of.restype = C.c_int
    lib.clip_real_scratch_bytes_of.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.clip_real_scratch_bytes_of.restype = C.c_longlong
    lib.clip_real_frames_per_block_of.argtypes = [C.c_int, C.c_int]
    lib.clip_real_frames_per_block_of.restype = C.c_int
    lib.clip_real_stride_of.argtypes = [C.c_int, C.c_int]
    lib.clip_real_stride_of.restype = C.c_int
    lib.clip_real_process_host.argtypes = [C.POINTER(L.ClipRealArgs)]
    lib.clip_real_process_host.restype = C.c_int
    return lib


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def robot(name):
    """-> (robot config with `extend_config`, model).  `chain`: a constructed revolute chain of 3 bodies with 1 extended body hanging off the middle one,
    rest rotations that are not identity, five contact points."""
    if name == "chain":
        rng = np.random.RandomState(17)
        rest = _unit(rng.normal(size=(3, 4)))          # wxyz
        model = types.SimpleNamespace(
            body_names=["base", "mid", "tip"], num_bodies=3, num_dof=2, parent=np.array([-1, 0, 1], dtype=np.int32),
            local_translation=rng.uniform(-0.4, 0.4, (3, 3)), local_rotation=rest, dof_axis=_unit(rng.normal(size=(2, 3))),
            contact_body=np.array([0, 1, 2, 2, 1], dtype=np.int32), contact_pos=rng.uniform(-0.1, 0.1, (5, 3)), contact_radius=rng.uniform(0.0, 0.05, 5))
        rc = {"extend_config": [{"joint_name": "probe", "parent_name": "mid", "pos": [0.1, -0.2, 0.3], "rot": list(_unit(rng.normal(size=4)))}]}
        return rc, model
    from phc_amd import robots
    from phc_amd.cfg_defaults import GROUPS
    from phc_amd.model import load_model
    rc = GROUPS["robot"][f"unitree_{name}"]
    model = load_model(f"{rc['humanoid_type']}_humanoid")
    robots.apply_robot_gains(model, robots.ROBOTS[rc["humanoid_type"]])
    return rc, model


def _rotvec(q):
    """xyzw unit quaternions -> rotation vectors."""
    q = np.where(q[..., 3:] < 0, -q, q)
    n = np.linalg.norm(q[..., :3], axis=-1, keepdims=True)
    return q[..., :3] / np.maximum(n, 1e-300) * (2.0 * np.arctan2(n, q[..., 3:]))


@functools.lru_cache(maxsize=None)
def make_clips(name):
    """Eight clips (LENGTHS, FPS) on tree `name`, `make_robot_clip` (the chain: the same construction on its own two axes) with these changes: the roots move
    at very different speeds (a filter that leaks across a clip boundary shows far above tolerance); in the odd clips the root starts near a half turn about
    x / y / z or near identity and then turns 0.35 .. 0.6 rad per frame about a fixed random axis (all four `_mat_to_quat_xyzw` candidates are taken,
    and the quaternion changes sign between consecutive frames where the candidate switches); some joints are held bit-identical over a clip.
    -> dict name -> {pose_aa [T, NB+E, 3] float32, root_trans_offset [T, 3], fps} in the schema of MotionLibReal."""
    from phc_amd.motion_lib import _q_mul
    from phc_amd.utils.synthetic_motion import make_robot_clip
    rc, model = robot(name)
    ne, nb = len(rc["extend_config"]), model.num_bodies
    rng = np.random.default_rng(SEED[name])
    out = {}
    for u, (T, fps) in enumerate(zip(LENGTHS, FPS)):
        if name == "chain":
            pose = np.zeros((T, nb + ne, 3))
            ang = 0.4 * rng.normal(size=(1, nb - 1)) + np.cumsum(rng.normal(0.0, 0.08, size=(T, nb - 1)), axis=0)
            pose[:, 1:nb] = model.dof_axis[None] * ang[..., None]
            pose[:, 0] = rng.normal(0.0, 0.2, size=3) + np.cumsum(rng.normal(0.0, 0.03, size=(T, 3)), axis=0)
        else:
            pose = make_robot_clip(rng, model, T, num_extend=ne, fps=fps)["pose_aa"].astype(np.float64)
        if u % 2:
            start = np.roll(np.array([1.0, 0.0, 0.0, 0.0]), u // 2)[[1, 2, 3, 0]] + rng.normal(0.0, 0.15, size=4)   # w, x, y, z dominant in turn (xyzw)
            axis, step = _unit(rng.normal(size=3)), rng.uniform(0.35, 0.6)
            turn = np.concatenate([axis[None] * np.sin(0.5 * step * np.arange(T))[:, None], np.cos(0.5 * step * np.arange(T))[:, None]], axis=-1)
            pose[:, 0] = _rotvec(_unit(_q_mul(turn, np.broadcast_to(_unit(start), (T, 4)))))
        held = [j for j in range(1, nb) if rng.uniform() < 0.25] or [1]
        pose[:, held] = pose[0, held]
        v = (-1.0) ** u * (3.0 + 2.0 * u) * np.array([np.cos(u), np.sin(u), 0.05])
        trans = np.array([0.3 * u, -0.2 * u, 1.0]) + v * (np.arange(T)[:, None] / fps) + rng.normal(scale=0.01, size=(T, 3))
        out[f"clip{u}"] = {"pose_aa": pose.astype(np.float32), "root_trans_offset": trans, "fps": fps, "held": held}
    return out


def library(name, fix=True, device="cpu", **over):
    """A MotionLibReal over the constructed clips (on the CPU unless told otherwise), as tests/test_fit_robot_motion.py builds one."""
    from phc_amd.config import EasyDict
    from phc_amd.motion_lib import FixHeightMode, MotionLibReal
    rc, model = robot(name)
    cfg = {"motion_file": {k: {f: v for f, v in c.items() if f != "held"} for k, c in make_clips(name).items()}, "device": device,
           "fix_height": FixHeightMode.full_fix if fix else FixHeightMode.no_fix, "min_length": -1, "max_length": -1, "im_eval": False, "multi_thread": False,
           "smpl_type": name, "randomrize_heading": False, "step_dt": 1 / 50, "robot": rc, "robot_model": model}
    cfg.update(over)
    lib = MotionLibReal(EasyDict(cfg))
    lib.num_joints = model.num_bodies     # (what load_motions sets from the skeleton trees)
    return lib


@functools.lru_cache(maxsize=None)
def case(name, fix=True):
    """-> (consts of `MotionLibReal._clip_consts`, pose_aa list f64, trans list, fps list): the arguments of `process_robot_clips_device`."""
    lib = library(name, fix)
    jobs = [lib._clip_payload(c, 0, -1, None) for c in lib._motion_data_list]
    return lib._clip_consts(None), [j[1] for j in jobs], [j[2] for j in jobs], [j[3] for j in jobs]


def fields(nb, ne):
    J, o, out = nb + ne, 0, {}
    stride = (7 * J + 6 * nb + 2 * (nb - 1) + 3) // 4 * 4
    for k, w in (("gts", 3 * J), ("grs", 4 * J), ("gvs", 3 * nb), ("gavs", 3 * nb), ("dof_pos", nb - 1), ("dvs", nb - 1)):
        out[k] = slice(o, o + w)
        o += w
    out["pad"] = slice(o, stride)
    return out, stride


@functools.lru_cache(maxsize=None)
def oracle(name, fix=True):
    """-> (records [F, stride] float32 of the existing host path, fps per frame [F], clip_dz [U] of `fix_trans_height`).  Asserts the conditions on the
    oracle's own intermediate values (thresholds of the arithmetic, not tolerances: nothing is excluded from the comparison):
      * the largest and second-largest q_abs of `_mat_to_quat_xyzw` are at least 1e-9 apart for every frame and body, and all four candidates are taken;
      * no axis-angle has a length in [1e-7, 1e-5] (the series branch of `_aa_to_quat_xyzw` sits at 1e-6); exact zeros exist;
      * some consecutive frames have rotation quaternions with a negative dot product (a candidate switch: `pos_unit` in the angular velocity);
      * some joints are bit-identical over a clip."""
    from phc_amd.motion_lib import _mat_to_quat_xyzw, _run_clip_job, robot_fk
    consts, poses, trans, fps = case(name, fix)
    lib = library(name, fix)
    recs, dz, taken, neg, zeros, held = [], [], set(), 0, 0, 0
    for u, (p, t, f) in enumerate(zip(poses, trans, fps)):
        rec, fps_out, T = _run_clip_job((0, p, t, f), consts)
        assert (fps_out, T) == (int(f), LENGTHS[u]) and rec.dtype == np.float32
        recs.append(rec)
        dz.append(lib.fix_trans_height(p, t)[1])
        _, wmat, _, pose = robot_fk(consts["parent"], consts["local_translation"], consts["local_rotation"], consts["ext_parent"], consts["ext_pos"],
                                    consts["ext_rot"], p, t)
        m = [wmat[..., i, i] for i in range(3)]
        q_abs = np.sqrt(np.maximum(np.stack([1 + m[0] + m[1] + m[2], 1 + m[0] - m[1] - m[2], 1 - m[0] + m[1] - m[2], 1 - m[0] - m[1] + m[2]], -1), 0.0))
        top = np.sort(q_abs, axis=-1)
        assert (top[..., 3] - top[..., 2]).min() >= 1e-9, "inputs too close to a tie of the matrix -> quaternion candidates"
        taken |= set(np.unique(q_abs.argmax(-1)).tolist())
        ang = np.linalg.norm(pose, axis=-1)
        assert not ((ang >= 1e-7) & (ang <= 1e-5)).any(), "inputs too close to the small-angle threshold"
        zeros += int((ang == 0).sum())
        q = _mat_to_quat_xyzw(wmat)
        neg += int(((q[1:] * q[:-1]).sum(-1) < 0).sum())
        h = make_clips(name)[f"clip{u}"]["held"]
        assert (p[:, h] == p[:1, h]).all()
        held += len(h)
    assert taken == {0, 1, 2, 3}, taken
    assert neg > 0 and zeros > 0 and held > 0
    return np.concatenate(recs), np.repeat(np.asarray(fps, dtype=np.float64), LENGTHS), np.asarray(dz)


def compare(got, want, fps_frame, nb, ne, scale=1.0, what=""):
    """Field by field: gts / grs / gvs / dof_pos / dvs within `scale` fp32 rounding flips, gavs the same plus the acos floor; the pad floats exactly 0."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    fl, stride = fields(nb, ne)
    assert want.shape[1] == stride
    worst = {}
    for k, s in fl.items():
        a, b = got[:, s].astype(np.float64), want[:, s].astype(np.float64)
        if k == "pad":
            worst[k] = float(np.abs(a).max()) if a.size else 0.0
            ok = not a.size or ((got[:, s] == 0).all() and (want[:, s] == 0).all())
        else:
            tol = EPS32 * np.maximum(np.abs(b), 1.0)
            if k == "gavs":
                tol = tol + ANG_FLOOR * (fps_frame / 30.0)[:, None]
            worst[k] = float((np.abs(a - b) / (scale * tol)).max()) if a.size else 0.0
            ok = worst[k] <= 1.0
        print(f"{what} {k}: worst {'|value|' if k == 'pad' else '|diff| / tolerance'} = {worst[k]:.3e}")
        assert ok, (what, k, worst[k])
    return worst


def arrays(name, fix=True):
    """The validated host arrays of a case (what `process_robot_clips_device` uploads) -> (dict of numpy arrays, sizes)."""
    from phc_amd.motion_lib import validate_robot_clip_inputs
    consts, poses, trans, fps = case(name, fix)
    v = validate_robot_clip_inputs(consts, poses, trans, fps)
    J = v["num_bodies"] + v["num_ext"]
    arrs = dict(parents=v["parents"], offsets=v["offsets"], rest_mat=v["rest_mat"], contact_body=v["contact_body"], contact_pos=v["contact_pos"],
                contact_radius=v["contact_radius"], clip_dt=np.ascontiguousarray(v["dt"]), clip_start=np.concatenate([[0], np.cumsum(v["nf"])]).astype(np.int64),
                pose_aa=np.ascontiguousarray(np.concatenate([p[:, :J] for p in poses]), dtype=np.float64),
                trans=np.ascontiguousarray(np.concatenate(trans), dtype=np.float64))
    return arrs, dict(U=len(poses), F=int(v["nf"].sum()), NB=v["num_bodies"], E=v["num_ext"], C=v["contact_body"].shape[0], fix=v["fix_height"])


def host_args(name, fix, frames, scratch, keep):
    """phc_clip_real_args_t over numpy arrays (host memory: for the host build only).  `keep` collects the arrays the struct points into."""
    from phc_amd import abi
    arrs, n = arrays(name, fix)
    keep.append(arrs)
    return abi.clip_real_args_struct(n["U"], n["F"], n["NB"], n["E"], n["C"], n["fix"], scratch, scratch.nbytes, frames, **arrs), n


def host_process(name, fix=True):
    """The three launches' per-lane functions looped over by the host build -> (records [F, stride] float32, clip_dz [U]); guard words behind frames and scratch
    checked, every float of every record written over a 7.0 fill."""
    _, n = arrays(name, fix)
    stride = int(shim().clip_real_stride_of(n["NB"], n["E"]))
    sb = int(shim().clip_real_scratch_bytes_of(n["F"], n["NB"], n["U"]))
    frames = np.full(n["F"] * stride + 4, np.float32(7.0), dtype=np.float32)
    frames[-4:].view(np.int32)[:] = GUARD
    scratch = np.zeros(sb // 8 + 2, dtype=np.float64)
    scratch[-2:].view(np.int64)[:] = GUARD
    keep = []
    a, _ = host_args(name, fix, frames[:-4].reshape(n["F"], stride), scratch[:-2], keep)
    assert shim().clip_real_process_host(a) == 0
    assert (frames[-4:].view(np.int32) == GUARD).all() and (scratch[-2:].view(np.int64) == GUARD).all()
    got = frames[:-4].reshape(n["F"], stride).copy()
    assert not (got == 7.0).any(), "every float of every record is written"
    dz0 = n["F"] * 6 * n["NB"]
    return got, scratch[dz0:dz0 + n["U"]].copy()
