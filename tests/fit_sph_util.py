"""Shared by tests/test_fit_keypoints_cpu.py and tests/test_fit_keypoints_gpu.py: the host build of phc_amd/csrc/phc_fit_sph.h (tests/fit_sph_shim.cpp, g++), the
constructed batches, the runner over host or device memory with guard words behind every array, and the torch-fp64 single-iteration oracle (autograd +
torch.optim.Adam + clamp + `gaussian_filter_time` on the statement of phc_amd/utils/fit_keypoints.py's docstring, written out here: never the code under test)
with the fp32 rounding bound of tests/fit_util.py extended to rotation-vector joints."""
import ctypes as C
import functools

import numpy as np
import torch

import fit_util as U
from fit_util import EINVAL, EPS32, EUNSUPPORTED, GUARD_WORDS, LENGTHS, LR, STATE, STEPS, collect, sub_case, zero_state   # noqa: F401
import host_build

MODEL = ("parents", "offsets", "rest", "range", "match_body", "match_slot", "subtree")      # no `axis`: phc_fit_sph_iterate does not read it
NAMES = ["chain4s", "smpl24", "smpl22"]
DIR = np.array([0.6, -0.64, 0.48])              # a unit vector: the direction of the constructed small / large rotation vectors


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("fit_sph_shim.cpp", "phc_fit_sph.hip")
    lib.fit_sph_args_check_of.argtypes = [C.POINTER(L.FitArgs), C.c_int]
    lib.fit_sph_args_check_of.restype = C.c_int
    lib.fit_sph_scratch_bytes_of.argtypes = [C.c_longlong, C.c_int, C.c_int]
    lib.fit_sph_scratch_bytes_of.restype = C.c_longlong
    lib.fit_sph_iterate_host.argtypes = [C.POINTER(L.FitArgs), C.c_int]
    lib.fit_sph_iterate_host.restype = C.c_int
    return lib


@functools.lru_cache(maxsize=None)
def smpl_model():
    from phc_amd.model import load_model
    return load_model("smpl_humanoid")


def _ranges(rng, n):
    """Constructed ranges [n, 2] (the shipped limits are +-pi and wider: no clamp would ever act): asymmetric, inside +-1.5, with 0 inside."""
    return np.stack([-rng.uniform(0.3, 1.5, n), rng.uniform(0.3, 1.5, n)], axis=-1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def model_arrays(name):
    """chain4s: bodies 0 - 1 - 2 and body 3 on body 1, random rest rotations; matched: the root and body 3 with the target columns permuted, so the joint of
    body 2 has no matched body below it.  smpl24: the shipped model, every body matched.  smpl22: the hands unmatched."""
    from phc_amd.utils.fit_keypoints import subtree_words
    if name == "chain4s":
        rng = np.random.RandomState(3)
        q = rng.normal(size=(4, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        w, x, y, z = q.T
        rest = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)
        parents, mb = np.array([-1, 0, 1, 1], dtype=np.int32), np.array([0, 3], dtype=np.int32)
        return dict(parents=parents, offsets=rng.uniform(-0.4, 0.4, (4, 3)).astype(np.float32), rest=rest.astype(np.float32), range=_ranges(rng, 9), match_body=mb,
                    match_slot=np.array([1, 0], dtype=np.int32), subtree=subtree_words(parents, mb))
    m = smpl_model()
    names = list(m.body_names)
    mb = np.array([i for i, n in enumerate(names) if name == "smpl24" or n not in ("L_Hand", "R_Hand")], dtype=np.int32)
    parents = np.asarray(m.parent, dtype=np.int32)
    rest = np.tile(np.eye(3).reshape(1, 9), (len(names), 1))
    assert np.array_equal(np.asarray(m.local_rotation)[:, 0], np.ones(len(names)))      # the SMPL family's rest rotations are the identity
    return dict(parents=parents, offsets=np.asarray(m.local_translation, dtype=np.float32), rest=rest.astype(np.float32),
                range=_ranges(np.random.RandomState(11), 3 * (len(names) - 1)), match_body=mb, match_slot=np.arange(len(mb), dtype=np.int32),
                subtree=subtree_words(parents, mb))


def dims(marr):
    nb = len(marr["parents"])
    return nb, 3 * (nb - 1), len(marr["match_body"])     # NB, ND, M


def aa_to_mat(aa):
    """exp of rotation vectors [..., 3] -> [..., 3, 3] (the statement's own: sin t / t and (1 - cos t) / t^2 with their series below t^2 = 1e-8)."""
    t2 = (aa * aa).sum(-1, keepdim=True)
    small = t2 < 1e-8
    t2s = torch.where(small, torch.ones_like(t2), t2)
    t = torch.sqrt(t2s)
    A = torch.where(small, 1.0 - t2 / 6.0, torch.sin(t) / t)
    B = torch.where(small, 0.5 - t2 / 24.0, (1.0 - torch.cos(t)) / t2s)
    x, y, z = aa[..., 0], aa[..., 1], aa[..., 2]
    zero = torch.zeros_like(x)
    K = torch.stack([zero, -z, y, z, zero, -x, -y, x, zero], dim=-1).reshape(aa.shape[:-1] + (3, 3))
    return torch.eye(3, dtype=aa.dtype).expand(K.shape) + A[..., None] * K + B[..., None] * (K @ K)


def fk(marr, root_rot, dof, root_pos, dtype=torch.float64):
    """The statement's FK in torch: root_rot [T, 3], dof [T, 3 (NB - 1)], root_pos [T, 3] -> positions [T, NB, 3]."""
    nb = len(marr["parents"])
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), dtype=dtype)
    offsets, rest = t(marr["offsets"]), t(marr["rest"]).reshape(-1, 3, 3)
    Rj = aa_to_mat(dof.reshape(dof.shape[0], nb - 1, 3))
    pos, rot = [None] * nb, [None] * nb
    for i, p in enumerate(marr["parents"]):
        if p < 0:
            pos[i], rot[i] = root_pos, aa_to_mat(root_rot)
        else:
            pos[i] = rot[p] @ offsets[i] + pos[p]
            rot[i] = rot[p] @ (rest[i] @ Rj[:, i - 1])
    return torch.stack(pos, dim=1)


def loss_of(marr, root_rot, dof, root_off, rto, g):
    pos = fk(marr, root_rot, dof, rto + root_off, dtype=dof.dtype)
    res = pos[:, list(marr["match_body"])] - g[:, list(marr["match_slot"])]
    return res.norm(dim=-1).mean() + 0.01 * torch.mean(torch.square(dof)), pos, res


@functools.lru_cache(maxsize=None)
def make_batch(name, seed=0):
    """The constructed batch (LENGTHS): per clip a state in mid-fit and targets a few centimetres off the FK of a neighbouring state.  The regimes:
      clip 0 (1 frame)    a clip of one frame;
      clip 1 (2 frames)   every joint component AT its lower or upper limit with its target pose beyond that limit (`outward` counts the components whose
                          gradient pushes outward);
      clip 2 (3 frames)   root_off = 0 and the matched root's target = root_trans_offset: that residual is exactly zero;
      clip 3 (4 frames)   rotation vector exactly 0, |r|^2 just below and just above 1e-8, |r| = 3.1: the root's AND the joint of body 1's;
      clips 4-6           generic; the last one is long enough for whole tiles and the filter's interior.
    Values are fp32 numbers held in numpy arrays.  Moments are zero (the gradient is then 10 x the first moment after one trip)."""
    marr = model_arrays(name)
    nb, nd, M = dims(marr)
    rng = np.random.RandomState(200 + seed)
    F_ = sum(LENGTHS)
    start = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    lo, hi = marr["range"][:, 0].astype(np.float64), marr["range"][:, 1].astype(np.float64)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    dof = mid + half * rng.uniform(-0.8, 0.8, (F_, nd))
    root_rot = rng.normal(scale=0.5, size=(F_, 3))
    root_off = rng.normal(scale=0.05, size=(len(LENGTHS), 3))
    root_off[2] = 0.0
    f3 = int(start[3])
    for k, scale in enumerate((0.0, 0.99e-4, 1.01e-4, 3.1)):
        root_rot[f3 + k] = DIR * scale
        dof[f3 + k, 0:3] = DIR[[1, 2, 0]] * scale
    rto = np.array([0.3, -0.2, 0.95]) + rng.normal(scale=0.3, size=(F_, 3))
    clip = np.repeat(np.arange(len(LENGTHS)), LENGTHS)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    dof, root_rot, root_off, rto = f32(dof), f32(root_rot), f32(root_off), f32(rto)
    side = rng.uniform(size=(LENGTHS[1], nd)) < 0.5
    dof[start[1]:start[2]] = f32(np.where(side, lo, hi))
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    dof_t = dof.astype(np.float64) + 0.1 * rng.normal(size=(F_, nd))
    dof_t[start[1]:start[2]] = np.where(side, lo - 0.4, hi + 0.4)
    pos = fk(marr, t(root_rot) + 0.1 * t(rng.normal(size=(F_, 3))), t(dof_t), t(rto) + t(root_off)[clip]).numpy()
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


def place(case, state, device=None, scratch_fill=None):
    """The arrays of one call in host (device None) or device memory, every state array and the scratch with guard words behind it -> (phc_fit_args_t, mem)."""
    from phc_amd import abi
    marr = case["marr"]
    nb, nd, M = dims(marr)
    F_, C_ = case["dof"].shape[0], len(case["start"]) - 1
    sb = int(shim().fit_sph_scratch_bytes_of(F_, C_, nb))
    bufs = {k: U._guarded(state[k]) for k in STATE}
    bufs["scratch"] = U._guarded(np.zeros(sb // 4, dtype=np.int32) if scratch_fill is None else np.full(sb // 4, scratch_fill, dtype=np.int32))
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
    args = abi.fit_args_struct(nb, 0, M, C_, F_, LR, mem["scratch"], sb, clip_start_host=mem["_host_start"], axis=None, **sized, **{k: mem[k] for k in const})
    return args, mem


def run(case, state, iterations, device=None, segments=None, scratch_fill=None):
    """`iterations` trips (or one call per entry of `segments`) from `state` on the host build (device None) or through phc_fit_sph_iterate on `device`."""
    from phc_amd import _lib as L
    args, mem = place(case, state, device, scratch_fill)
    for n in (segments or [iterations]):
        if device is None:
            rc = shim().fit_sph_iterate_host(args, int(n))
        else:
            rc = L.load().phc_fit_sph_iterate(args, int(n), torch.cuda.current_stream(device).cuda_stream)
        assert rc == 0, rc
    return collect(mem)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the oracle

def oracle_step(case, state):
    """One trip in torch fp64 from `state`: autograd for the gradient, torch.optim.Adam with the state's moments and step counters, clamp,
    `gaussian_filter_time` per clip.  -> dict(grad, E, next, loss) as `fit_util.oracle_step`, whose rounding-bound construction E is kept term by term (world
    positions, residual directions, one torque term per matched entry below the joint); a joint's three components share the bound of its torque, multiplied
    by the Jacobian factor 1 + |r| / 2 + |r|^2 / 6 and with 8 eps (|r| + |r|^2) |tau| added for the Jacobian's own coefficients, as the root's."""
    from phc_amd.utils.fit_robot_motion import gaussian_filter_time
    marr, start = case["marr"], case["start"]
    nb, nd, M = dims(marr)
    C_ = len(start) - 1
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))
    lo, hi = t(marr["range"][:, 0]), t(marr["range"][:, 1])
    mb, ms = marr["match_body"], marr["match_slot"]
    depth, reach = U._depth_and_reach(marr)
    keys = ("dof", "root_rot", "root_off")
    out = dict(grad={k: np.zeros(state[k].shape) for k in keys}, E={k: np.zeros(state[k].shape) for k in keys},
               next={k: np.zeros(state[k].shape) for k in STATE[:9]}, loss=np.zeros(C_))
    for c in range(C_):
        sl = slice(int(start[c]), int(start[c + 1]))
        T = sl.stop - sl.start
        p = {"dof": t(state["dof"][sl]).requires_grad_(True), "root_rot": t(state["root_rot"][sl]).requires_grad_(True),
             "root_off": t(state["root_off"][c:c + 1]).requires_grad_(True)}
        g = t(case["target"][sl])
        loss, pos, res = loss_of(marr, p["root_rot"], p["dof"], p["root_off"], t(case["rto"][sl]), g)
        opt = torch.optim.Adam(list(p.values()), lr=LR)
        loss.backward()
        for k, v in p.items():
            ks = slice(c, c + 1) if k == "root_off" else sl
            opt.state[v] = {"step": torch.tensor(float(state["step"][c])), "exp_avg": t(state[k + "_m"][ks]).clone(), "exp_avg_sq": t(state[k + "_v"][ks]).clone()}
            out["grad"][k][ks] = v.grad.numpy()
        opt.step()
        with torch.no_grad():
            p["dof"].clamp_(lo, hi)
            p["dof"].copy_(gaussian_filter_time(p["dof"]))
        for k, v in p.items():
            ks = slice(c, c + 1) if k == "root_off" else sl
            out["next"][k][ks] = v.detach().numpy()
            out["next"][k + "_m"][ks] = opt.state[v]["exp_avg"].numpy()
            out["next"][k + "_v"][ks] = opt.state[v]["exp_avg_sq"].numpy()
        out["loss"][c] = float(loss.detach())
        # the rounding bound
        P, R = pos.detach().numpy(), res.detach().numpy()
        rn = np.linalg.norm(R, axis=-1)                                                   # [T, M]
        base = np.abs(case["rto"][sl].astype(np.float64) + state["root_off"][c].astype(np.float64)).sum(-1)     # [T]
        dp = 2 * (depth[None] + 2) * EPS32 * (base[:, None] + reach[None])               # [T, NB]
        dr = dp[:, mb] + EPS32 * np.abs(g.numpy()[:, ms]).sum(-1)
        zero = rn == 0
        du = np.where(zero, 0.0, 2 * dr / np.where(zero, 1.0, rn) + 2 * EPS32)
        un = np.where(zero, 0.0, 1.0)
        for j in range(nb):
            ms_j = np.flatnonzero((marr["subtree"][j] >> np.arange(M)) & 1) if j else np.arange(M)
            d = np.linalg.norm(P[:, mb[ms_j]] - P[:, j:j + 1], axis=-1)                   # [T, |ms_j|]
            term = d * du[:, ms_j] + (dp[:, mb[ms_j]] + dp[:, j:j + 1]) * un[:, ms_j] + 2 * (depth[mb[ms_j]] + 2)[None] * EPS32 * d
            e = term.sum(-1) / (T * M)
            tau = (d * un[:, ms_j]).sum(-1) / (T * M)
            cols = slice(0, 3) if j == 0 else slice(3 * (j - 1), 3 * j)
            k = "root_rot" if j == 0 else "dof"
            r = np.linalg.norm(state[k][sl, cols].astype(np.float64), axis=-1)
            e = e * (1 + r / 2 + r * r / 6) + 8 * EPS32 * (r + r * r) * tau
            out["E"][k][sl, cols] = e[:, None] + 4 * EPS32 * np.abs(out["grad"][k][sl, cols])
        out["E"]["root_off"][c] = du.sum() / (T * M) + 4 * EPS32 * np.abs(out["grad"]["root_off"][c])
    return out


def torch32_grad(case, state):
    """The gradient torch's fp32 autograd gives for the same statement on the same state (how the floor of the gradient bound is measured)."""
    marr, start = case["marr"], case["start"]
    t = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32))
    out = {k: np.zeros(state[k].shape) for k in ("dof", "root_rot", "root_off")}
    for c in range(len(start) - 1):
        sl = slice(int(start[c]), int(start[c + 1]))
        dof, rr, ro = t(state["dof"][sl]).requires_grad_(True), t(state["root_rot"][sl]).requires_grad_(True), t(state["root_off"][c:c + 1]).requires_grad_(True)
        loss, _, _ = loss_of(marr, rr, dof, ro, t(case["rto"][sl]), t(case["target"][sl]))
        loss.backward()
        out["dof"][sl], out["root_rot"][sl], out["root_off"][c] = dof.grad.numpy(), rr.grad.numpy(), ro.grad.numpy()[0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# whole clips

@functools.lru_cache(maxsize=None)
def walk_keypoints(seconds):
    """The body positions [T, 24, 3] of `make_gait_clip(model, "walk", seconds, heading=2.0)`, from a forward kinematics written out here."""
    from scipy.spatial.transform import Rotation as sRot
    from phc_amd.utils.synthetic_motion import make_gait_clip
    m = smpl_model()
    clip = make_gait_clip(m, "walk", seconds=seconds, heading=2.0)
    q = np.asarray(clip["pose_quat_global"], dtype=np.float64)
    T, nb = q.shape[:2]
    R = sRot.from_quat(q.reshape(-1, 4)).as_matrix().reshape(T, nb, 3, 3)
    pos = np.zeros((T, nb, 3))
    pos[:, 0] = np.asarray(clip["root_trans_offset"], dtype=np.float64)
    for b in range(1, nb):
        pos[:, b] = pos[:, m.parent[b]] + R[:, m.parent[b]] @ np.asarray(m.local_translation[b], dtype=np.float64)
    return pos


def noisy_walk(seconds, noise):
    """`walk_keypoints` with seeded gaussian noise of `noise` metres on every keypoint (0: the clean keypoints, some of whose residuals start at exactly 0)."""
    kp = walk_keypoints(seconds)
    return kp if noise == 0 else kp + np.random.RandomState(17).normal(scale=noise, size=kp.shape)


def clip_case(seconds=1.0, noise=0.0):
    """`noisy_walk` as a one-clip batch at the fit's real start (Kabsch root, zeros): what `fit_keypoint_clips(backend="device")` uploads."""
    from phc_amd.utils.fit_keypoints import kabsch_root, sph_model_arrays
    m = smpl_model()
    kp = noisy_walk(seconds, noise)
    T = len(kp)
    idx = list(range(m.num_bodies))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(name="walk", marr=sph_model_arrays(m, idx), start=np.array([0, T], dtype=np.int64), target=f32(kp), rto=f32(kp[:, 0]),
                dof=np.zeros((T, 3 * (m.num_bodies - 1)), dtype=np.float32), root_rot=f32(kabsch_root(m, kp, idx)), root_off=np.zeros((1, 3), dtype=np.float32),
                step=np.zeros(1, dtype=np.int32), zero_entries=[])
