"""Shared by tests/test_fit_device_cpu.py and tests/test_fit_device_gpu.py: the host build of phc_amd/csrc/phc_fit.h (tests/fit_shim.cpp, g++), the constructed
batches, the runner over host or device memory with guard words behind every array, and the torch-fp64 single-iteration oracle (autograd +
torch.optim.Adam + clamp + `gaussian_filter_time`: never the code under test) with the fp32 rounding bound it derives from the magnitudes it sums."""
import ctypes as C
import functools

import numpy as np
import torch

import host_build

GUARD = 0x5A5A5A5A
GUARD_WORDS = 4
EPS32 = 2.0 ** -24                              # half an fp32 ulp, relative: one rounding
EINVAL, EUNSUPPORTED = -1, -2
LENGTHS = (1, 2, 3, 4, 5, 6, 48)                # one batch; TF = 8 (4 for G1): below, at and above a tile, and the 5-tap filter wider than the clip
STEPS = (0, 3, 0, 7, 1, 0, 12)                  # Adam steps each clip has behind it: one counter per clip
STATE = ("dof", "dof_m", "dof_v", "root_rot", "root_rot_m", "root_rot_v", "root_off", "root_off_m", "root_off_v", "step", "loss")
MODEL = ("parents", "offsets", "rest", "axis", "range", "match_body", "match_slot", "subtree")
LR = 0.02


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("fit_shim.cpp", "phc_fit.hip")
    lib.fit_args_check_of.argtypes = [C.POINTER(L.FitArgs), C.c_int]
    lib.fit_args_check_of.restype = C.c_int
    lib.fit_scratch_bytes_of.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.fit_scratch_bytes_of.restype = C.c_longlong
    lib.fit_tile_frames_of.argtypes = [C.c_int]
    lib.fit_tile_frames_of.restype = C.c_int
    lib.fit_taps_of.argtypes = [C.c_void_p]
    lib.fit_taps_of.restype = None
    lib.fit_iterate_host.argtypes = [C.POINTER(L.FitArgs), C.c_int]
    lib.fit_iterate_host.restype = C.c_int
    return lib


@functools.lru_cache(maxsize=None)
def robot(name):
    from phc_amd import robots
    from phc_amd.cfg_defaults import GROUPS
    from phc_amd.model import load_model
    rc = GROUPS["robot"][name]
    model = load_model(f"{rc['humanoid_type']}_humanoid")
    robots.apply_robot_gains(model, robots.ROBOTS[rc["humanoid_type"]])
    return rc, model


@functools.lru_cache(maxsize=None)
def model_arrays(name):
    """unitree_h1 / unitree_g1: `fit_model_arrays`; chain3: bodies 0 - 1 - 2 and one extended body on body 1, matched: the root and the extended body, so the
    joint of body 2 has no matched body below it (its gradient is the regulariser's alone)."""
    if name != "chain3":
        from phc_amd.utils.fit_robot_motion import fit_model_arrays
        return fit_model_arrays(robot(name)[1], robot(name)[0])
    rng = np.random.RandomState(3)
    q = rng.normal(size=(4, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    rest = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
    axis = rng.normal(size=(2, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    return dict(parents=np.array([-1, 0, 1, 1], dtype=np.int32), offsets=rng.uniform(-0.4, 0.4, (4, 3)).astype(np.float32), rest=rest.astype(np.float32),
                axis=axis.astype(np.float32), range=np.array([[-1.0, 1.5], [-0.5, 2.0]], dtype=np.float32), match_body=np.array([0, 3], dtype=np.int32),
                match_slot=np.array([1, 0], dtype=np.int32), subtree=np.array([3, 2, 0], dtype=np.uint32))


def dims(marr):
    nbe, nd = len(marr["parents"]), len(marr["axis"])
    return nd + 1, nbe - nd - 1, nd, len(marr["match_body"])     # NB, E, ND, M


def fk64(marr, root_rot, dof, root_pos):
    """torch fp64 FK of the arrays (the statement of `RobotFK`): root_rot [T, 3], dof [T, ND], root_pos [T, 3] -> positions [T, NB + E, 3]."""
    from phc_amd.utils.fit_robot_motion import _aa_to_mat
    nb, ne, nd, _ = dims(marr)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    offsets, rest, axis = t(marr["offsets"]), t(marr["rest"]).reshape(-1, 3, 3), t(marr["axis"])
    pos, rot = [None] * (nb + ne), [None] * (nb + ne)
    Rj = _aa_to_mat(axis[None] * dof[..., None])
    for i, p in enumerate(marr["parents"]):
        if p < 0:
            pos[i], rot[i] = root_pos, _aa_to_mat(root_rot)
        else:
            pos[i] = rot[p] @ offsets[i] + pos[p]
            rot[i] = rot[p] @ (rest[i] @ Rj[:, i - 1]) if i < nb else rot[p] @ rest[i]
    return torch.stack(pos, dim=1)


@functools.lru_cache(maxsize=None)
def make_batch(name, seed=0):
    """The constructed batch (LENGTHS): per clip a state in mid-fit -- joint angles inside their ranges, a root rotation, a root offset, moments of a few steps --
    and targets a few centimetres off the FK of a neighbouring state.  The regimes:
      clip 0 (1 frame)    a clip of one frame;
      clip 1 (2 frames)   every joint AT its lower or upper limit with its target pose beyond that limit (`outward` counts the joints whose gradient pushes outward);
      clip 2 (3 frames)   root_off = 0 and the matched root's target = root_trans_offset: that residual is exactly zero;
      clip 3 (4 frames)   root rotation vector exactly 0, |r|^2 just below and just above 1e-8, |r| = 3.1;
      clips 4-6           generic; the last one is long enough for whole tiles and the filter's interior.
    Values are fp32 numbers held in numpy arrays.  Moments are zero (the gradient is then 10 x the first moment after one trip)."""
    marr = model_arrays(name)
    nb, ne, nd, M = dims(marr)
    rng = np.random.RandomState(100 + seed)
    F_ = sum(LENGTHS)
    start = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    lo, hi = marr["range"][:, 0].astype(np.float64), marr["range"][:, 1].astype(np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    dof = mid + half * rng.uniform(-0.8, 0.8, (F_, nd))
    root_rot = rng.normal(scale=0.5, size=(F_, 3))
    root_off = rng.normal(scale=0.05, size=(len(LENGTHS), 3))
    root_off[2] = 0.0
    f3 = int(start[3])
    d = np.array([0.6, -0.64, 0.48])
    root_rot[f3 + 0] = 0.0
    root_rot[f3 + 1] = d * 0.99e-4
    root_rot[f3 + 2] = d * 1.01e-4
    root_rot[f3 + 3] = d * 3.1
    rto = np.array([0.3, -0.2, 0.95]) + rng.normal(scale=0.3, size=(F_, 3))
    clip = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    dof, root_rot, root_off, rto = f32(dof), f32(root_rot), f32(root_off), f32(rto)
    # clip 1: every joint at a limit; its target pose lies 0.4 rad BEYOND that limit, so the gradient pushes outward and the clamp holds the joint
    side = rng.uniform(size=(LENGTHS[1], nd)) < 0.5
    dof[start[1]:start[2]] = f32(np.where(side, lo, hi))
    # targets: the FK of a state 0.1 rad and a few centimetres away
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    dof_t = dof.astype(np.float64) + 0.1 * rng.normal(size=(F_, nd))
    dof_t[start[1]:start[2]] = np.where(side, lo - 0.4, hi + 0.4)
    pos = fk64(marr, t(root_rot) + 0.1 * t(rng.normal(size=(F_, 3))), t(dof_t), t(rto) + t(root_off)[clip]).numpy()
    target = np.zeros((F_, M, 3))
    target[:, marr["match_slot"]] = pos[:, marr["match_body"]] + rng.normal(scale=0.03, size=(F_, M, 3))
    target = f32(target)
    root_entries = [m for m in range(M) if marr["match_body"][m] == 0]
    for m in root_entries:
        target[start[2]:start[3], marr["match_slot"][m]] = rto[start[2]:start[3]]
    case = dict(name=name, marr=marr, start=start, target=target, rto=rto, dof=dof, root_rot=root_rot, root_off=root_off,
                step=np.asarray(STEPS, dtype=np.int32), zero_entries=root_entries)
    g = oracle_step(case, zero_state(case))["grad"]["dof"][start[1]:start[2]]
    case["outward"] = int(((g > 0) == side).sum())
    return case


def zero_state(case):
    """The state a test hands to an iteration: the case's parameters, zero moments, the case's step counters."""
    F_, nd, C_ = case["dof"].shape[0], case["dof"].shape[1], len(case["start"]) - 1
    z = lambda *s: np.zeros(s, dtype=np.float32)
    return dict(dof=case["dof"].copy(), dof_m=z(F_, nd), dof_v=z(F_, nd), root_rot=case["root_rot"].copy(), root_rot_m=z(F_, 3), root_rot_v=z(F_, 3),
                root_off=case["root_off"].copy(), root_off_m=z(C_, 3), root_off_v=z(C_, 3), step=case["step"].copy(), loss=z(C_))


def sub_case(case, clips):
    """The batch made of `clips` (indices into the case's clips, any order, repeats allowed) and the state rows that go with it."""
    s = case["start"]
    rows = np.concatenate([np.arange(s[c], s[c + 1]) for c in clips])
    out = dict(case, start=np.concatenate([[0], np.cumsum([s[c + 1] - s[c] for c in clips])]).astype(np.int64))
    for k in ("target", "rto", "dof", "root_rot"):
        out[k] = np.ascontiguousarray(case[k][rows])
    out["root_off"] = np.ascontiguousarray(case["root_off"][list(clips)])
    out["step"] = np.ascontiguousarray(case["step"][list(clips)])
    return out


def _guarded(a):
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = np.empty(flat.size + GUARD_WORDS, dtype=flat.dtype)
    buf[:flat.size] = flat
    buf[flat.size:].view(np.int32)[:] = GUARD
    return buf


def place(case, state, device=None, scratch_fill=None):
    """The arrays of one call in host (device None) or device memory, every state array and the scratch with guard words behind it -> (phc_fit_args_t, mem);
    `mem` keeps the arrays alive and is what `collect` reads."""
    from phc_amd import abi
    marr = case["marr"]
    nb, ne, nd, M = dims(marr)
    F_, C_ = case["dof"].shape[0], len(case["start"]) - 1
    sb = int(shim().fit_scratch_bytes_of(F_, C_, nb + ne))
    bufs = {k: _guarded(state[k]) for k in STATE}
    bufs["scratch"] = _guarded(np.zeros(sb // 4, dtype=np.int32) if scratch_fill is None else np.full(sb // 4, scratch_fill, dtype=np.int32))
    const = {k: np.ascontiguousarray(marr[k]) for k in MODEL}
    const.update(clip_start=np.ascontiguousarray(case["start"]), target=case["target"], root_trans_offset=case["rto"])
    if device is None:
        mem = dict(bufs, **const)
    else:
        up = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)
        mem = {k: up(v) for k, v in dict(bufs, **const).items()}
    sized = {k: mem[k][:mem[k].shape[0] - GUARD_WORDS] for k in STATE}
    mem["_host_start"] = np.ascontiguousarray(case["start"])
    mem["_shapes"] = {k: state[k].shape for k in STATE}
    args = abi.fit_args_struct(nb, ne, M, C_, F_, LR, mem["scratch"], sb, clip_start_host=mem["_host_start"], **sized, **{k: mem[k] for k in const})
    return args, mem


def collect(mem):
    """The state arrays of `place` back as numpy, after checking the guard words behind each of them and behind the scratch."""
    out = {}
    for k in list(STATE) + ["scratch"]:
        b = mem[k].cpu().numpy() if isinstance(mem[k], torch.Tensor) else mem[k]
        assert (b[-GUARD_WORDS:].view(np.int32) == GUARD).all(), f"guard words behind {k} overwritten"
        if k != "scratch":
            out[k] = b[:-GUARD_WORDS].reshape(mem["_shapes"][k]).copy()
    return out


def run(case, state, iterations, device=None, segments=None, scratch_fill=None):
    """`iterations` trips (or one call per entry of `segments`) from `state` on the host build (device None) or through phc_fit_iterate on `device`.
    -> the new state (numpy)."""
    from phc_amd import _lib as L
    args, mem = place(case, state, device, scratch_fill)
    for n in (segments or [iterations]):
        if device is None:
            rc = shim().fit_iterate_host(args, int(n))
        else:
            rc = L.load().phc_fit_iterate(args, int(n), torch.cuda.current_stream(device).cuda_stream)
        assert rc == 0, rc
    return collect(mem)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the oracle

def _depth_and_reach(marr):
    """Per body: the number of bodies on its chain and the sum of |offset| along it (what, with the root position, its world position is summed from)."""
    par, off = marr["parents"], np.abs(marr["offsets"].astype(np.float64)).sum(1)
    depth, reach = np.zeros(len(par)), np.zeros(len(par))
    for i, p in enumerate(par):
        if p >= 0:
            depth[i], reach[i] = depth[p] + 1, reach[p] + off[i]
    return depth, reach


def oracle_step(case, state):
    """One trip in torch fp64 from `state` (any float dtype; read as exact numbers): autograd for the gradient, torch.optim.Adam with the state's moments and
    step counters, clamp, `gaussian_filter_time` per clip.  -> dict(grad, E, next, loss):
      grad[k]  d loss_c / d parameter for k in dof / root_rot / root_off;
      E[k]     the fp32 rounding bound of that gradient: with eps = 2^-24, a world position summed from the root position and the offsets along a chain of
               n bodies is taken to carry dp = 2 (n + 2) eps (|root position|_1 + sum |offset|_1) (a 3x3 product chain: a couple of roundings per level on a term of
               that size); a residual r = p - g then carries dr = dp + eps |g|, its direction u = r / |r| du = 2 dr / |r| + 2 eps (0 for an exactly zero
               residual, where both sides give u = 0); a term a . ((p_m - p_j) x u_m) carries |p_m - p_j| du + (dp_m + dp_j) |u| + 2 (n + 2) eps |p_m - p_j|
               (the last: the axis in the world, the cross and the dot product); E is the sum of that over the terms the gradient sums, over T_c M, plus
               4 eps |gradient| (the division, the regulariser, and reading the gradient back from the first moment).  For the root rotation vector the
               terms are multiplied by |J_l^T|_1 <= 1 + |r| / 2 + |r|^2 / 6 and 8 eps (|r| + |r|^2) |tau| is added for the Jacobian's own coefficients;
      next[k]  the parameters after Adam, clamp and smoothing; next moments under dof_m ...; loss [C]."""
    from phc_amd.utils.fit_robot_motion import gaussian_filter_time
    marr, start = case["marr"], case["start"]
    nb, ne, nd, M = dims(marr)
    C_ = len(start) - 1
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    lo, hi = t(marr["range"][:, 0]), t(marr["range"][:, 1])
    mb, ms = marr["match_body"], marr["match_slot"]
    depth, reach = _depth_and_reach(marr)
    out = dict(grad={k: np.zeros(state[k].shape) for k in ("dof", "root_rot", "root_off")}, E={k: np.zeros(state[k].shape) for k in ("dof", "root_rot", "root_off")},
               next={k: np.zeros(state[k].shape) for k in STATE[:9]}, loss=np.zeros(C_))
    for c in range(C_):
        sl = slice(int(start[c]), int(start[c + 1]))
        T = sl.stop - sl.start
        p = {"dof": t(state["dof"][sl]).requires_grad_(True), "root_rot": t(state["root_rot"][sl]).requires_grad_(True),
             "root_off": t(state["root_off"][c:c + 1]).requires_grad_(True)}
        rto, g = t(case["rto"][sl]), t(case["target"][sl])
        pos = fk64(marr, p["root_rot"], p["dof"], rto + p["root_off"])
        res = pos[:, mb] - g[:, ms]
        loss = res.norm(dim=-1).mean() + (0.01 * torch.mean(torch.square(p["dof"])) if nd else 0.0)
        opt = torch.optim.Adam(list(p.values()), lr=LR)
        loss.backward()
        for k, v in p.items():
            ks = slice(c, c + 1) if k == "root_off" else sl
            opt.state[v] = {"step": torch.tensor(float(state["step"][c])), "exp_avg": t(state[k + "_m"][ks]).clone(), "exp_avg_sq": t(state[k + "_v"][ks]).clone()}
            out["grad"][k][ks] = v.grad.numpy()
        opt.step()
        with torch.no_grad():
            p["dof"].clamp_(lo, hi)
            if nd:
                p["dof"].copy_(gaussian_filter_time(p["dof"]))
        for k, v in p.items():
            ks = slice(c, c + 1) if k == "root_off" else sl
            out["next"][k][ks] = v.detach().numpy()
            out["next"][k + "_m"][ks] = opt.state[v]["exp_avg"].numpy()
            out["next"][k + "_v"][ks] = opt.state[v]["exp_avg_sq"].numpy()
        out["loss"][c] = float(loss.detach())
        # the rounding bound
        P = pos.detach().numpy()
        R = res.detach().numpy()
        rn = np.linalg.norm(R, axis=-1)                                                   # [T, M]
        base = np.abs(case["rto"][sl].astype(np.float64) + state["root_off"][c].astype(np.float64)).sum(-1)     # [T]
        dp = 2 * (depth[None] + 2) * EPS32 * (base[:, None] + reach[None])               # [T, NBE]
        dr = dp[:, mb] + EPS32 * np.abs(g.numpy()[:, ms]).sum(-1)
        zero = rn == 0
        du = np.where(zero, 0.0, 2 * dr / np.where(zero, 1.0, rn) + 2 * EPS32)
        un = np.where(zero, 0.0, 1.0)
        anc = np.zeros((nb, M), dtype=bool)                                              # entry m below or at body j
        for m in range(M):
            k = int(mb[m])
            while k >= 0:
                if k < nb:
                    anc[k, m] = True
                k = int(marr["parents"][k])
        for j in range(nb):
            ms_j = np.flatnonzero(anc[j]) if j else np.arange(M)
            d = np.linalg.norm(P[:, mb[ms_j]] - P[:, j:j + 1], axis=-1)                   # [T, |ms_j|]
            term = d * du[:, ms_j] + (dp[:, mb[ms_j]] + dp[:, j:j + 1]) * un[:, ms_j] + 2 * (depth[mb[ms_j]] + 2)[None] * EPS32 * d
            e = term.sum(-1) / (T * M)
            if j == 0:
                r = np.linalg.norm(state["root_rot"][sl].astype(np.float64), axis=-1)
                tau = (d * un[:, ms_j]).sum(-1) / (T * M)
                e = e * (1 + r / 2 + r * r / 6) + 8 * EPS32 * (r + r * r) * tau
                out["E"]["root_rot"][sl] = e[:, None] + 4 * EPS32 * np.abs(out["grad"]["root_rot"][sl])
            else:
                out["E"]["dof"][sl, j - 1] = e + 4 * EPS32 * np.abs(out["grad"]["dof"][sl, j - 1])
        out["E"]["root_off"][c] = du.sum() / (T * M) + 4 * EPS32 * np.abs(out["grad"]["root_off"][c])
    return out


def torch32_grad(case, state):
    """The gradient torch's fp32 autograd gives for the parent's loss statement on the same state (how the floor of the gradient bound was measured)."""
    from phc_amd.utils.fit_robot_motion import _aa_to_mat
    marr, start = case["marr"], case["start"]
    nb, ne, nd, M = dims(marr)
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    offsets, rest, axis = t(marr["offsets"]), t(marr["rest"]).reshape(-1, 3, 3), t(marr["axis"])
    out = {k: np.zeros(state[k].shape) for k in ("dof", "root_rot", "root_off")}
    for c in range(len(start) - 1):
        sl = slice(int(start[c]), int(start[c + 1]))
        dof, rr, ro = t(state["dof"][sl]).requires_grad_(True), t(state["root_rot"][sl]).requires_grad_(True), t(state["root_off"][c:c + 1]).requires_grad_(True)
        pose = torch.cat([rr[:, None], axis * dof[..., None], torch.zeros((sl.stop - sl.start, ne, 3))], dim=1)
        R = _aa_to_mat(pose)
        pos, rot = [None] * (nb + ne), [None] * (nb + ne)
        for i, p in enumerate(marr["parents"]):
            if p < 0:
                pos[i], rot[i] = t(case["rto"][sl]) + ro, R[:, 0]
            else:
                pos[i] = (rot[p] @ offsets[i]) + pos[p]
                rot[i] = rot[p] @ (rest[i] @ R[:, i])
        pos = torch.stack(pos, dim=1)
        loss = (pos[:, marr["match_body"]] - t(case["target"][sl])[:, marr["match_slot"]]).norm(dim=-1).mean() + (0.01 * torch.mean(torch.square(dof)) if nd else 0.0)
        loss.backward()
        out["dof"][sl], out["root_rot"][sl], out["root_off"][c] = dof.grad.numpy(), rr.grad.numpy(), ro.grad.numpy()[0]
    return out


def robot_clip_inputs(name, seed=5, T=48):
    """The case of tests/test_fit_robot_motion.py (`make_robot_clip`, seed 5, T = 48) for robot `name`: (smpl_joints, root_trans, root_aa)."""
    from scipy.spatial.transform import Rotation as sRot
    from phc_amd.utils.fit_robot_motion import SMPL_BONE_ORDER_NAMES, RobotFK
    from phc_amd.utils.synthetic_motion import make_robot_clip
    rc, model = robot(name)
    ext = list(rc["extend_config"])
    gt = make_robot_clip(np.random.default_rng(seed), model, T, num_extend=len(ext))
    fk = RobotFK(model, ext, dtype=torch.float64)
    pos, _ = fk(torch.from_numpy(gt["pose_aa"]), torch.from_numpy(gt["root_trans_offset"]))
    joints = np.zeros((T, 24, 3))
    for rname, sname in rc["joint_matches"]:
        joints[:, SMPL_BONE_ORDER_NAMES.index(sname)] = pos[:, fk.names.index(rname)].numpy()
    root_aa = (sRot.from_rotvec(gt["pose_aa"][:, 0]) * sRot.from_quat([0.5, 0.5, 0.5, 0.5])).as_rotvec()
    return joints, joints[:, 0].copy(), root_aa


def clip_case(name, seed=5, T=48):
    """`robot_clip_inputs` as a one-clip batch at the fit's zero start (what `fit_clips(backend="device")` uploads)."""
    from phc_amd.utils.fit_robot_motion import _FitProblem, fit_model_arrays
    rc, model = robot(name)
    pb = _FitProblem(model, rc, *robot_clip_inputs(name, seed, T))
    nd = model.num_bodies - 1
    return dict(name=name, marr=fit_model_arrays(model, rc), start=np.array([0, T], dtype=np.int64), target=np.ascontiguousarray(pb.target.numpy()),
                rto=np.ascontiguousarray(pb.root_trans_offset.numpy()), dof=np.zeros((T, nd), dtype=np.float32),
                root_rot=np.ascontiguousarray(pb.gt_root.numpy()), root_off=np.zeros((1, 3), dtype=np.float32), step=np.zeros(1, dtype=np.int32), zero_entries=[])
