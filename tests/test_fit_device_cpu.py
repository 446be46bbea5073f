"""The device retargeting fit (phc_fit_iterate, phc_amd/csrc/phc_fit.h) without a GPU: its ABI, every refusal of `check_fit` and of `fit_clips`, and the host
build of its per-lane code (tests/fit_shim.cpp) on constructed states against the torch-fp64 oracle of tests/fit_util.py -- the gradient, the update, a short
trajectory against `fit_clip(dtype=float64)`, and the bits under segmenting and placement."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fit_util as U
import host_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["chain3", "unitree_h1", "unitree_g1"]
GRAD_FLOOR = 0.0     # see test_gradient_on_constructed_states
POINTERS = ("parents", "offsets", "rest", "axis", "range", "match_body", "match_slot", "subtree", "clip_start", "clip_start_host", "target", "root_trans_offset",
            "dof", "dof_m", "dof_v", "root_rot", "root_rot_m", "root_rot_v", "root_off", "root_off_m", "root_off_v", "step", "loss", "scratch")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. ABI

def test_abi_names_struct_size_and_version():
    from phc_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "phc_amd.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(phc_\w+)\s*\(", header, flags=re.M))
    for name in ("phc_fit_scratch_bytes", "phc_fit_iterate"):
        assert name in L.EXPORTED_SYMBOLS and name in declared
    # (phc_fit_args_t and PHC_FIT_MAX_MATCHED against their mirrors: tests/test_abi_and_host.py)
    assert [f[0] for f in L.FitArgs._fields_ if f[1] is C.c_void_p] == list(POINTERS)
    lib = L.load()
    assert lib.phc_abi_version() == 37
    assert lib.phc_fit_scratch_bytes(100, 3, 23) == U.shim().fit_scratch_bytes_of(100, 3, 23) > 0
    for bad in ((-1, 3, 23), (100, 0, 23), (100, 3, 0), (100, 3, 65)):
        assert lib.phc_fit_scratch_bytes(*bad) == U.EINVAL


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. refusals

def _host_args(case, keep, **override):
    """phc_fit_args_t over numpy arrays for the checks alone (nothing is launched): `override` replaces fields after the valid struct is built."""
    from phc_amd import abi
    marr = case["marr"]
    nb, ne, nd, M = U.dims(marr)
    F_, C_ = case["dof"].shape[0], len(case["start"]) - 1
    st = U.zero_state(case)
    sb = int(U.shim().fit_scratch_bytes_of(F_, C_, nb + ne))
    scratch = np.zeros(sb // 4, dtype=np.int32)
    arrays = dict({k: np.ascontiguousarray(marr[k]) for k in U.MODEL}, clip_start=case["start"], clip_start_host=case["start"].copy(), target=case["target"],
                  root_trans_offset=case["rto"], **st)
    keep.append((arrays, scratch))
    a = abi.fit_args_struct(nb, ne, M, C_, F_, U.LR, scratch, sb, **arrays)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def _starts(case, edit):
    s = case["start"].copy()
    edit(s)
    return s


REFUSALS = ([(f"null {p}", {p: None}, 1, U.EINVAL) for p in POINTERS]
            + [("iterations < 0", {}, -1, U.EINVAL), ("num_bodies + num_ext > 64", {"num_ext": 62}, 1, U.EUNSUPPORTED),
               ("more than 32 matched", {"num_matched": 33}, 1, U.EUNSUPPORTED), ("scratch one byte short", {"scratch_bytes": -1}, 1, U.EINVAL),
               ("no clips", {"num_clips": 0}, 1, U.EINVAL), ("no matched body", {"num_matched": 0}, 1, U.EINVAL), ("num_ext < 0", {"num_ext": -1}, 1, U.EINVAL),
               ("clip_start: an empty clip", {"clip_start_host": lambda s: s.__setitem__(3, s[2])}, 1, U.EINVAL),
               ("clip_start: descending", {"clip_start_host": lambda s: s.__setitem__(3, s[2] - 1)}, 1, U.EINVAL),
               ("clip_start: does not start at 0", {"clip_start_host": lambda s: s.__setitem__(0, 1)}, 1, U.EINVAL),
               ("clip_start: does not end at num_frames", {"clip_start_host": lambda s: s.__setitem__(len(s) - 1, s[-1] + 1)}, 1, U.EINVAL),
               ("clip_start: runs past num_frames in between", {"clip_start_host": lambda s: s.__setitem__(len(s) - 2, s[-1] + 5)}, 1, U.EINVAL),
               ("misaligned dof", {"dof_offset": 2}, 1, U.EINVAL)])


@pytest.mark.parametrize("what,override,iterations,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_fit_refuses(what, override, iterations, code):
    case = U.make_batch("chain3")
    keep = []
    assert U.shim().fit_args_check_of(_host_args(case, keep), 1) == 0 and U.shim().fit_args_check_of(_host_args(case, keep), 0) == 0
    a = _host_args(case, keep)
    arrays = keep[-1][0]
    for k, v in override.items():
        if callable(v):
            s = _starts(case, v)
            keep.append(s)
            setattr(a, k, s.ctypes.data)
        elif k == "scratch_bytes":
            a.scratch_bytes = a.scratch_bytes + v
        elif k == "dof_offset":
            a.dof = a.dof + v
        else:
            setattr(a, k, v)
    assert U.shim().fit_args_check_of(a, iterations) == code
    assert U.shim().fit_args_check_of(None, 1) == U.EINVAL
    # the host build's iterate runs the same check first and touches nothing
    before = [x.copy() for x in arrays.values()]
    assert U.shim().fit_iterate_host(a, iterations) == code
    after = list(arrays.values())
    assert all(np.array_equal(x, y) for x, y in zip(before, after))


def test_fit_clips_python_side_errors():
    from phc_amd.utils.fit_robot_motion import fit_clips
    rc, model = U.robot("unitree_h1")
    clip = U.robot_clip_inputs("unitree_h1", T=6)
    with pytest.raises(ValueError, match="backend"):
        fit_clips(model, rc, {"a": clip}, iterations=1, backend="gpu")
    with pytest.raises(ValueError, match="empty_one"):
        fit_clips(model, rc, {"a": clip, "empty_one": (np.zeros((0, 24, 3)), np.zeros((0, 3)), None)}, iterations=1)
    with pytest.raises(ValueError, match="empty_one"):
        fit_clips(model, rc, {"empty_one": (np.zeros((0, 24, 3)), np.zeros((0, 3)), None)}, iterations=1, backend="device", device="cuda:0")
    with pytest.raises(RuntimeError, match="backend=host"):
        fit_clips(model, rc, {"a": clip}, iterations=1, backend="device", device="cpu")   # never a fallback


def test_fit_clips_host_backend_is_fit_clip_and_dtype_default_is_unchanged():
    """`backend="host"` loops over `fit_clip`; `fit_clip`'s new keyword at its default and `fit_clip_state` run the same statements: equal bits."""
    from phc_amd.utils.fit_robot_motion import fit_clip, fit_clip_state, fit_clips
    rc, model = U.robot("unitree_h1")
    clip = U.robot_clip_inputs("unitree_h1", T=6)
    a = fit_clips(model, rc, {"k": clip}, iterations=3)["k"]
    b = fit_clip(model, rc, *clip, iterations=3)
    c = fit_clip(model, rc, *clip, iterations=3, dtype=torch.float32)
    dof, rot, _, loss = fit_clip_state(model, rc, *clip, iterations=3)
    for k in ("root_trans_offset", "pose_aa", "dof", "root_rot", "smpl_joints"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(b[k], c[k]) and b[k].dtype == a[k].dtype
    assert b["dof"].dtype == np.float32 and np.array_equal(b["pose_aa"][:, 0], rot) and b["fit_loss"] == loss
    assert fit_clip(model, rc, *clip, iterations=3, dtype=torch.float64)["dof"].dtype == np.float64


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. gradient

def check_gradient(case, got, oracle, what):
    """`got`: the state after ONE trip from zero moments, so that the first moment is (1 - 0.9) x the gradient.  Bound: 4 E + GRAD_FLOOR."""
    worst = {}
    for k in ("dof", "root_rot", "root_off"):
        g = got[k + "_m"].astype(np.float64) * 10.0
        assert np.isfinite(g).all()
        err, tol = np.abs(g - oracle["grad"][k]), 4 * oracle["E"][k] + GRAD_FLOOR
        worst[k] = float((err - tol).max())
        print(f"{what} {k}: max |gradient| {np.abs(oracle['grad'][k]).max():.3e}, max error {err.max():.3e}, max (error - bound) {worst[k]:.3e}")
        assert worst[k] <= 0.0, (what, k, worst[k])
    return worst


def check_regimes(case, got, oracle):
    s = case["start"]
    nb, ne, nd, M = U.dims(case["marr"])
    # joints with no matched body below them: the regulariser alone, 0.02 dof / (T ND)
    free = [j for j in range(1, nb) if case["marr"]["subtree"][j] == 0]
    assert free or case["name"] == "unitree_h1", "chain3 and G1 have joints without a matched body below them (H1 has none)"
    T = np.repeat(np.diff(s), np.diff(s))[:, None]
    reg = 0.02 * case["dof"].astype(np.float64) / (T * nd)
    for j in free:
        np.testing.assert_allclose(oracle["grad"]["dof"][:, j - 1], reg[:, j - 1], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(got["dof_m"][:, j - 1].astype(np.float64) * 10, reg[:, j - 1], rtol=4 * U.EPS32 * 2, atol=1e-30)
    # the exactly zero residual: finite, and root_off's gradient is the other entries' alone (checked against the oracle by the caller)
    assert case["zero_entries"] and np.isfinite(got["root_off_m"]).all() and np.isfinite(got["root_rot_m"]).all()
    # at the limits
    # at the limits: the regime is there when at least a quarter of clip 1's (frame, joint) pairs are pushed outward (a joint with no matched body below it
    # is pulled towards 0 by the regulariser alone, outward only where 0 lies beyond the limit)
    assert case["outward"] >= 2 * nd // 4, (case["outward"], nd)


@pytest.mark.parametrize("name", NAMES)
def test_gradient_on_constructed_states(name):
    """The analytic gradient of the host build against autograd in fp64, clips of 1, 2, 3, 4, 5, 6 and 48 frames in one batch (regimes: `fit_util.make_batch`).
    Bound 4 E + floor with E the oracle's rounding bound (`fit_util.oracle_step`).  The floor is the smallest value at which torch's fp32 autograd gradient of
    the parent's loss statement passes too; measured on these cases (3 models, this test's second half): its largest error - 4 E is negative everywhere
    (closest: 4.7e-1 of the bound, the root rotation vector of chain3; the host build's closest is 1.3e-1), so the floor is 0."""
    case = U.make_batch(name)
    st = U.zero_state(case)
    oracle = U.oracle_step(case, st)
    got = U.run(case, st, 1)
    check_gradient(case, got, oracle, f"{name} host build")
    check_regimes(case, got, oracle)
    assert np.array_equal(got["step"], case["step"] + 1)
    np.testing.assert_allclose(got["loss"], oracle["loss"], rtol=1e-5)
    g32 = U.torch32_grad(case, st)
    for k in ("dof", "root_rot", "root_off"):
        over = float((np.abs(g32[k] - oracle["grad"][k]) - 4 * oracle["E"][k]).max())
        print(f"{name} torch fp32 autograd {k}: max (error - 4 E) {over:.3e}")
        assert over <= GRAD_FLOOR


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. update

def expected_update(case, st, got):
    """Adam + clamp + smoothing in fp64 applied to the build's OWN new moments (so the gradient's error stays out) -> (next parameters, their bounds).
    Bound: the Adam statement rounds sqrt, the division by bc2_sqrt, + eps, m / denom, the product with step_size and the sum (6 roundings, all but the last on
    the step D, the last on the parameter), and the two scalars are fp32 roundings of fp64 numbers (2 more on D): eps (|p| + 8 |D|) + eps |p|.  The clamp is
    exact.  The filter multiplies by fp32 taps (1 rounding each on the tap, 1 on the product) and adds five terms (4): its error is at most 7 eps times the
    weighted sum of |x|, on top of the weighted sum of the inputs' own bounds."""
    from phc_amd.utils.fit_robot_motion import gaussian_filter_time
    s = case["start"]
    nxt, bound = {}, {}
    for k in ("dof", "root_rot", "root_off"):
        step = st["step"].astype(np.float64) + 1
        per = step if k == "root_off" else np.repeat(step, np.diff(s))
        size = (U.LR / (1 - 0.9 ** per))[:, None]
        bc2s = np.sqrt(1 - 0.999 ** per)[:, None]
        m, v, p = (got[k + "_m"].astype(np.float64), got[k + "_v"].astype(np.float64), st[k].astype(np.float64))
        D = size * m / (np.sqrt(v) / bc2s + 1e-8)
        nxt[k], bound[k] = p - D, U.EPS32 * (2 * np.abs(p) + 8 * np.abs(D))
    lo, hi = case["marr"]["range"][:, 0].astype(np.float64), case["marr"]["range"][:, 1].astype(np.float64)
    x = np.clip(nxt["dof"], lo, hi)
    for c in range(len(s) - 1):
        sl = slice(int(s[c]), int(s[c + 1]))
        f = lambda a: gaussian_filter_time(torch.from_numpy(np.ascontiguousarray(a))).numpy()
        nxt["dof"][sl], bound["dof"][sl] = f(x[sl]), f(bound["dof"][sl]) + 7 * U.EPS32 * f(np.abs(x[sl]))
    return nxt, bound, x


def check_update(case, st, got, what):
    nxt, bound, clamped = expected_update(case, st, got)
    for k in ("dof", "root_rot", "root_off"):
        err = np.abs(got[k].astype(np.float64) - nxt[k])
        print(f"{what} next {k}: max error {err.max():.3e}, max error / bound {(err / bound[k]).max():.3f}")
        assert (err <= bound[k]).all(), (what, k, float((err / bound[k]).max()))
    return clamped


@pytest.mark.parametrize("name", NAMES)
def test_update_on_constructed_states(name):
    case = U.make_batch(name)
    st = U.zero_state(case)
    rng = np.random.RandomState(7)
    for k in ("dof", "root_rot", "root_off"):      # moments of a fit in progress
        st[k + "_m"] = rng.normal(scale=0.01, size=st[k].shape).astype(np.float32)
        st[k + "_v"] = (rng.uniform(0.2, 2.0, size=st[k].shape) * 1e-4).astype(np.float32)
    got = U.run(case, st, 1)
    clamped = check_update(case, st, got, f"{name} host build")
    s = case["start"]
    lo, hi = case["marr"]["range"][:, 0], case["marr"]["range"][:, 1]
    # clip 1 started at the limits: the clamp held what Adam pushed outward
    held = (clamped[s[1]:s[2]] == lo) | (clamped[s[1]:s[2]] == hi)
    assert held.sum() >= held.size // 4, held.sum()
    assert (got["dof"] >= lo - 1e-6).all() and (got["dof"] <= hi + 1e-6).all()
    # a clip's neighbours never leak into it: other targets, angles and moments next door, the same bits here
    for c in (0, 3, 6):
        other = dict(case, target=case["target"].copy(), rto=case["rto"].copy())
        st2 = {k: v.copy() for k, v in st.items()}
        mine = np.zeros(case["dof"].shape[0], dtype=bool)
        mine[s[c]:s[c + 1]] = True
        other["target"][~mine] += 0.7
        other["rto"][~mine] -= 0.3
        for k in ("dof", "dof_m", "root_rot", "root_rot_v"):
            st2[k][~mine] *= np.float32(0.5)
        got2 = U.run(other, st2, 1)
        for k in U.STATE:
            rows = slice(c, c + 1) if got[k].shape[0] == len(s) - 1 else slice(s[c], s[c + 1])
            assert np.array_equal(got[k][rows], got2[k][rows]), (name, c, k)
        assert not np.array_equal(got["dof"][~mine], got2["dof"][~mine])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. trajectory

def check_trajectory(name, got, what, iterations=10):
    """dof, root rotation vector and root_off after `iterations` trips from the zero start against `fit_clip(dtype=float64)`: max(4 d32, 2e-6), d32 the
    deviation of the unchanged fp32 host fit from the fp64 run on the same case, computed here."""
    from phc_amd.utils.fit_robot_motion import fit_clip_state
    rc, model = U.robot(name)
    clip = U.robot_clip_inputs(name)
    torch.manual_seed(0)
    want = fit_clip_state(model, rc, *clip, iterations=iterations, dtype=torch.float64)
    host32 = fit_clip_state(model, rc, *clip, iterations=iterations)
    for k, w, h, g in zip(("dof", "root_rot", "root_off"), want, host32, (got["dof"], got["root_rot"], got["root_off"][0])):
        d32, err = float(np.abs(h - w).max()), float(np.abs(g.astype(np.float64) - w).max())
        print(f"{what} {k} after {iterations} iterations: error {err:.3e}, d32 {d32:.3e}, bound {max(4 * d32, 2e-6):.3e}")
        assert err <= max(4 * d32, 2e-6), (what, k, err, d32)


@pytest.mark.parametrize("name", ["unitree_h1", "unitree_g1"])
def test_trajectory_of_ten_iterations(name):
    case = U.clip_case(name)
    got = U.run(case, U.zero_state(case), 10)
    assert got["step"].tolist() == [10]
    check_trajectory(name, got, f"{name} host build")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. segmenting and placement

PLACEMENTS = {"alone": lambda c: [c], "first": lambda c: [c, 1, 4, 6], "last": lambda c: [6, 2, 5, c], "middle": lambda c: [4, 6, c, 0, 2]}


def check_segmenting_and_placement(name, device=None):
    case = U.make_batch(name)
    st = U.zero_state(case)
    whole = U.run(case, st, 10, device=device)
    parts = U.run(case, st, 10, device=device, segments=[3, 7], scratch_fill=0x7FC00000)    # (what a call finds in the scratch does not matter either)
    for k in U.STATE:
        assert np.array_equal(whole[k], parts[k], equal_nan=True), (name, "3 + 7 != 10", k)
    assert whole["step"].tolist() == (case["step"] + 10).tolist()
    s = case["start"]
    for c in (0, 3, 6):
        for how, order in PLACEMENTS.items():
            clips = order(c)
            sub = U.sub_case(case, clips)
            got = U.run(sub, U.zero_state(sub), 10, device=device)
            at = clips.index(c)
            for k in U.STATE:
                per_clip = whole[k].shape[0] == len(s) - 1
                a = whole[k][c:c + 1] if per_clip else whole[k][s[c]:s[c + 1]]
                b = got[k][at:at + 1] if per_clip else got[k][sub["start"][at]:sub["start"][at + 1]]
                assert np.array_equal(a, b), (name, c, how, k)


@pytest.mark.parametrize("name", ["chain3", "unitree_g1"])
def test_segmenting_and_placement_keep_the_bits(name):
    check_segmenting_and_placement(name)


def test_butterfly_order_and_taps():
    """The host statement of the group sum follows phc_group.h's butterfly (partners ^1, ^2, ^7, ^15, ^16, ^32), and the taps are the normalised gaussian."""
    from phc_amd.utils.fit_robot_motion import gaussian_filter_time
    lib = U.shim()
    lib.fit_group_sum_of.argtypes = [C.c_void_p, C.c_int]
    lib.fit_group_sum_of.restype = C.c_float
    rng = np.random.RandomState(0)
    for G in (32, 64):
        v = (rng.normal(size=G) * 10.0 ** rng.uniform(-3, 3, G)).astype(np.float32)
        w = v.copy()
        for mask in (1, 2, 7, 15, 16, 32):
            if mask < G:
                w = (w + w[np.arange(G) ^ mask]).astype(np.float32)
        assert (w == w[0]).all() and lib.fit_group_sum_of(v.ctypes.data, G) == w[0]
    taps = np.zeros(5, dtype=np.float32)
    lib.fit_taps_of(taps.ctypes.data)
    x = torch.zeros(9, 1, dtype=torch.float64)
    x[4] = 1.0
    np.testing.assert_allclose(taps, gaussian_filter_time(x)[2:7, 0].numpy(), rtol=2 ** -23)
    assert lib.fit_tile_frames_of(23) == 8 and lib.fit_tile_frames_of(32) == 8 and lib.fit_tile_frames_of(33) == 4


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# the sanitizer program

def test_host_build_runs_clean_under_the_address_and_undefined_sanitizers():
    """tests/fit_asan_main.cpp (its own main; nothing is loaded into Python): a 3-body chain with an extended body and a 34-body chain, clips of 1, 2 and 9
    frames, on heap arrays of exact size."""
    returncode, stdout, stderr = host_build.run_sanitized("fit_asan_main.cpp")
    print(stdout[-2000:], stderr)
    assert returncode == 0 and stdout.strip().endswith("ok"), stdout + stderr
