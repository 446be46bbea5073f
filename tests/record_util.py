"""Shared by tests/test_motion_record_cpu.py and tests/test_motion_record_gpu.py: the host build of phc_amd/csrc/phc_record.h (tests/record_shim.cpp, g++), the
caller-side state of a phc_motion_record launch in host memory with guard elements behind every array, constructed simulator states for the three model
families, and two oracles: a numpy statement of the row rule (which row goes where, the header, the four counters -- exact) and an fp64 statement of a row's
computed columns (the root's exp map, the robots' axis x angle rows) on the same fp32 data."""
import ctypes as C
import functools

import numpy as np

import host_build

GUARD = 16            # guard elements of the array's own type behind every array
F = np.float32
DT = F(1 / 30)
REF, SEED, ONE = 1, 2, 4     # PHC_RECORD_*
FLAG_SETS = ("none", "all", "first", "last", "alternate")
# quat_to_exp_map against an fp64 statement: the bound tests/test_oracle_golden.py::test_quat_kat holds this function to on tests/golden/quat_kat.npz
EXP_MAP_ATOL = 1e-4
# a revolute row is ONE fp32 product axis_k * angle per component; against the fp64 product of the same fp32 factors that is half an ulp of the result,
# |axis| <= 1 and |angle| <= 4 here: 2^-24 * 4 = 2.4e-7
AXIS_ANGLE_ATOL = 2.4e-7
OVER = {"smpl": (), "h1": ("robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"),
        "g1": ("robot=unitree_g1", "env=env_im_g1_phc", "sim=robot_sim", "control=robot_control")}


@functools.lru_cache(maxsize=None)
def shim():
    from phc_amd import _lib as L
    lib = host_build.shim("record_shim.cpp", "phc_record.hip")
    pm, pa = C.POINTER(L.Model), C.POINTER(L.MotionRecordArgs)
    for name, args, res in (("record_sizeof_args", [], C.c_int), ("record_block", [], C.c_int), ("record_width_of", [C.c_int] * 4, C.c_int),
                            ("record_group_of", [C.c_int] * 2, C.c_int), ("motion_record_check_of", [pm, pa], C.c_int), ("motion_record_host_of", [pm, pa], None)):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, res
    return lib


@functools.lru_cache(maxsize=None)
def family(name):
    """-> dict(model, NB, E, D, ints, floats, jt, ds, axis) of "smpl" (24 bodies, 69 DoFs), "h1" or "g1" (all-revolute, with their extended bodies)."""
    from phc_amd.config import compose
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    t = HumanoidIm.host_only(compose(["env.num_envs=2", *OVER[name]]))
    m = t.model
    ints, floats = m.pack()
    NB = int(m.num_bodies)
    axis = np.zeros((NB, 3), F)
    for j in range(NB):
        if int(m.joint_type[j]) == 2:
            axis[j] = floats.reshape(-1)[j * m.BODY_FLOATS + 25:j * m.BODY_FLOATS + 28]
    return dict(name=name, model=m, NB=NB, E=int(t.num_extend_bodies), D=int(m.num_dof), ints=np.ascontiguousarray(ints, np.int32),
                floats=np.ascontiguousarray(floats, F), jt=np.asarray(m.joint_type[:NB]), ds=np.asarray(m.dof_start[:NB]), axis=axis)


def width(fam, flags=0):
    return 3 + 4 * fam["NB"] + 3 * (fam["NB"] + fam["E"]) + fam["D"] + 7 + (3 * fam["NB"] if flags & REF else 0)


def host_model(fam):
    """phc_model_t over the family's host tables (filled by hand: abi.model_struct would ask the library about them)."""
    from phc_amd import _lib as L
    m = L.Model()
    mod = fam["model"]
    m.num_bodies, m.num_dof, m.max_level, m.num_contact_pts, m.num_shapes = fam["NB"], fam["D"], int(mod.max_level), len(mod.contact_body), 1
    m.ints, m.floats = fam["ints"].ctypes.data, fam["floats"].ctypes.data
    return m


def guarded(shape, dtype, fill):
    """An array of `shape` in front of GUARD sentinel elements -> (view, whole allocation)."""
    n = int(np.prod(shape))
    whole = np.empty(n + GUARD, dtype=dtype)
    whole[:n] = fill
    whole[n:] = sentinel(dtype)
    return whole[:n].reshape(shape), whole


def sentinel(dtype):
    return np.array(-12345.5 if np.dtype(dtype).kind == "f" else 0x5A5A5A5A, dtype=dtype)


def guards_intact(wholes):
    return all((w[-GUARD:] == sentinel(w.dtype)).all() for w in wholes)


def roots(rng, n):
    """n fp32 root rotations from tests/rotation_cases.py's members: angles over [0, 2 pi), near 0 and near pi, w < 0, |w| = 1 to rounding."""
    import rotation_cases as rc
    q, _, _ = rc.exp_map_members(rng, n)
    return q


def make_sources(fam, N, seed, flag_set="alternate"):
    """A constructed simulator state of N envs (numpy, guarded) by the field names of phc_motion_record_args_t."""
    rng = np.random.default_rng(seed)
    NB, D = fam["NB"], fam["D"]
    wholes, src = [], {}

    def put(name, a):
        v, w = guarded(a.shape, a.dtype, 0)
        v[...] = a
        src[name] = v
        wholes.append(w)
    root = rng.standard_normal((N, 13)).astype(F)
    root[:, 3:7] = roots(rng, N)
    rbs = rng.standard_normal((N, NB, 13)).astype(F)
    q = rng.standard_normal((N, NB, 4))
    rbs[:, :, 3:7] = (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(F)
    rbs[:, 0, 3:7] = root[:, 3:7]
    rbs[:, ::3, 3:7] *= -1       # both hemispheres: the copy must not flip any
    put("root_states", root)
    put("dof_state", rng.uniform(-4, 4, (N, D, 2)).astype(F))
    put("rigid_body_state", rbs)
    put("progress_buf", rng.integers(0, 300, N).astype(np.int64))
    flag = np.zeros(N, np.int64)
    if flag_set == "all":
        flag[:] = 1
    elif flag_set == "first":
        flag[0] = 1
    elif flag_set == "last":
        flag[-1] = 1
    elif flag_set == "alternate":
        flag[::2] = 7          # (non-zero = set)
    put("flag", flag)
    put("motion_ids", rng.integers(0, 1000, N).astype(np.int64))
    put("motion_start_times", rng.uniform(0, 5, N).astype(F))
    put("motion_start_times_offset", rng.uniform(0, 1, N).astype(F))
    put("ref_body_pos", rng.standard_normal((N, NB, 3)).astype(F))
    return src, wholes


def make_block(N, cap, W, offset=0):
    """The caller-owned block and the four counters (guarded).  `offset`: the frames start that many floats into their allocation."""
    wholes, st = [], {}
    n = N * cap * W
    whole = np.empty(offset + n + GUARD, F)
    whole[:] = sentinel(F)
    st["frames"] = whole[offset:offset + n].reshape(N, cap, W)
    wholes.append(whole)
    for name, shape in (("header", (N, cap, 4)), ("len", (N,)), ("seg", (N,)), ("closed", (N,)), ("dropped", (N,))):
        v, w = guarded(shape, np.int32, -7 if name == "header" else 0)
        st[name] = v
        wholes.append(w)
    return st, wholes


def args_of(fam, src, st, cap, flags=0, limit=None, dt=DT):
    from phc_amd import abi
    arrays = dict(src)
    if not flags & REF:
        arrays.pop("ref_body_pos")
    a = abi.motion_record_args_struct(src["root_states"].shape[0], fam["NB"], fam["E"], fam["D"], cap, dt, ref=bool(flags & REF), seed=bool(flags & SEED),
                                      one_segment=bool(flags & ONE), **arrays, **st)
    a._keep = (arrays, st, limit)
    if limit is not None:
        a.limit = limit.ctypes.data
    return a


# ---- oracles -------------------------------------------------------------------------------------------------------------------------------------------
def rows_f64(fam, src, flags=0, dt=DT):
    """-> (rows fp64 [N, W], computed bool [W], tol fp64 [W]): the frame rows on the fp32 data; `computed` marks the columns that are not copies (the root's
    exp map, the revolute bodies' rows, the time) and `tol` their absolute bound (0 for the copies and the time, which is three fp32 operations restated)."""
    import phc_oracle as po
    NB, E, D = fam["NB"], fam["E"], fam["D"]
    N = src["root_states"].shape[0]
    root, dof = src["root_states"].astype(np.float64), src["dof_state"][..., 0]
    aa = np.zeros((N, NB + E, 3))
    aa[:, 0] = po.quat_to_exp_map(root[:, 3:7])
    comp, tol = np.zeros((NB + E, 3), bool), np.zeros((NB + E, 3))
    comp[0], tol[0] = True, EXP_MAP_ATOL
    for j in range(1, NB):
        s = int(fam["ds"][j])
        if fam["jt"][j] == 1:
            aa[:, j] = dof[:, s:s + 3]
        elif fam["jt"][j] == 2:
            aa[:, j] = fam["axis"][j].astype(np.float64)[None] * dof[:, s].astype(np.float64)[:, None]
            comp[j], tol[j] = True, AXIS_ANGLE_ATOL
    t = ((src["progress_buf"].astype(F) * F(dt)).astype(F) + src["motion_start_times"]).astype(F) + src["motion_start_times_offset"]
    parts = [root[:, 0:3], src["rigid_body_state"][:, :, 3:7].reshape(N, -1), aa.reshape(N, -1), dof, root[:, 7:13], t[:, None].astype(np.float64)]
    cparts = [np.zeros(3, bool), np.zeros(4 * NB, bool), comp.reshape(-1), np.zeros(D, bool), np.zeros(6, bool), np.zeros(1, bool)]
    tparts = [np.zeros(3), np.zeros(4 * NB), tol.reshape(-1), np.zeros(D), np.zeros(6), np.zeros(1)]
    if flags & REF:
        parts.append(src["ref_body_pos"].reshape(N, -1))
        cparts.append(np.zeros(3 * NB, bool))
        tparts.append(np.zeros(3 * NB))
    return np.concatenate([p.astype(np.float64) for p in parts], axis=1), np.concatenate(cparts), np.concatenate(tparts)


def columns(fam, flags=0):
    """-> (computed bool [W], tol fp64 [W]) of rows_f64, without a state."""
    z = {"root_states": np.zeros((1, 13), F), "dof_state": np.zeros((1, fam["D"], 2), F), "rigid_body_state": np.zeros((1, fam["NB"], 13), F),
         "progress_buf": np.zeros(1, np.int64), "motion_start_times": np.zeros(1, F), "motion_start_times_offset": np.zeros(1, F),
         "ref_body_pos": np.zeros((1, fam["NB"], 3), F)}
    z["root_states"][0, 6] = 1
    _, comp, tol = rows_f64(fam, z, flags)
    return comp, tol


def rule(st, src, cap, flags=0, limit=None):
    """The row rule on copies of the counters -> (written row index per env, or -1; the new header rows; the new counters)."""
    ln, seg, closed, dropped = (st[k].copy() for k in ("len", "seg", "closed", "dropped"))
    N = len(ln)
    at, head = np.full(N, -1), {}
    for i in range(N):
        if closed[i]:
            continue
        room = cap if limit is None else min(cap, int(limit[i]))
        flag = 0 if flags & SEED else int(src["flag"][i] != 0)
        if ln[i] >= room:
            dropped[i] += 1
        else:
            at[i] = ln[i]
            head[i] = (int(seg[i]), int(src["progress_buf"][i]), int(src["motion_ids"][i]), flag)
            ln[i] += 1
        if flag:
            if flags & ONE:
                closed[i] = 1
            else:
                seg[i] += 1
    return at, head, dict(len=ln, seg=seg, closed=closed, dropped=dropped)


def check_call(fam, src, st_before, st_after, cap, flags=0, limit=None, exact_rows=None):
    """One call's effect against the oracles: counters and headers exact, written rows' copied columns bit-equal and computed ones within their bound (or, with
    `exact_rows` [N, W] fp32 -- the host build's rows --, copied columns bit-equal to it and computed ones within the bound of the fp64 statement), every other
    row and header untouched."""
    at, head, cnt = rule(st_before, src, cap, flags, limit)
    for k, v in cnt.items():
        assert np.array_equal(st_after[k], v), k
    want, comp, tol = rows_f64(fam, src, flags)
    for i in range(len(at)):
        keep = np.ones(cap, bool)
        if at[i] >= 0:
            f = int(at[i])
            keep[f] = False
            got = st_after["frames"][i, f]
            assert tuple(st_after["header"][i, f]) == head[i], (i, f)
            assert got[~comp].tobytes() == want[i, ~comp].astype(F).tobytes(), (i, f)
            err = np.abs(got[comp].astype(np.float64) - want[i, comp])
            assert (err <= tol[comp]).all(), (i, f, float(err.max()))
            if exact_rows is not None:
                assert got[~comp].tobytes() == exact_rows[i, ~comp].tobytes(), (i, f)
        assert st_after["frames"][i, keep].tobytes() == st_before["frames"][i, keep].tobytes(), i
        assert st_after["header"][i, keep].tobytes() == st_before["header"][i, keep].tobytes(), i


def snapshot(st):
    return {k: v.copy() for k, v in st.items()}
