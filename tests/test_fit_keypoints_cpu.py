"""The spherical-joint keypoint fit (phc_fit_sph_iterate, phc_amd/csrc/phc_fit_sph.h; phc_amd/utils/fit_keypoints.py) without a GPU: its ABI, every refusal of
`check_fit_sph` and of `fit_keypoint_clips`, the host build of its per-lane code (tests/fit_sph_shim.cpp) on constructed states against the torch-fp64 oracle of
tests/fit_sph_util.py -- the gradient, the exact regimes, the update, a short trajectory against the fp64 host fit, the bits under segmenting and placement --
and the host backend end to end."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import fit_sph_util as S
import host_build
import test_fit_device_cpu as T0      # the update's expected value and bound, the placements: shared with the revolute fit's tests

ROOT = host_build.ROOT
GRAD_FLOOR = 0.0     # see test_gradient_on_constructed_states
POINTERS = tuple(p for p in T0.POINTERS if p != "axis")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. ABI

def test_abi_names_prototypes_and_version():
    from phc_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "phc_amd.h")).read()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(phc_\w+)\s*\(", header, flags=re.M))
    for name in ("phc_fit_sph_scratch_bytes", "phc_fit_sph_iterate"):
        assert name in L.EXPORTED_SYMBOLS and name in declared
    lib = L.load()
    assert lib.phc_fit_sph_scratch_bytes.argtypes == [C.c_int64, C.c_int32, C.c_int32] and lib.phc_fit_sph_scratch_bytes.restype is C.c_int64
    assert lib.phc_fit_sph_iterate.argtypes == [C.POINTER(L.FitArgs), C.c_int32, C.c_void_p] and lib.phc_fit_sph_iterate.restype is C.c_int32
    assert re.search(r"int64_t phc_fit_sph_scratch_bytes\(int64_t num_frames, int32_t num_clips, int32_t num_bodies\);", header)
    assert re.search(r"int32_t phc_fit_sph_iterate\(const phc_fit_args_t\* args[^)]*, int32_t iterations, void\* stream\);", header)
    assert lib.phc_abi_version() == 37
    assert lib.phc_fit_sph_scratch_bytes(100, 3, 24) == S.shim().fit_sph_scratch_bytes_of(100, 3, 24) > 0
    # tile_start [C + 1] i32 | coef [C, 2] f32 | partial [F / 8 + C, 5] f32 | rows [F, 3 (NB - 1)] f32, each part rounded up to 16 bytes
    assert lib.phc_fit_sph_scratch_bytes(100, 3, 24) == 16 + 32 + (15 * 5 * 4 + 15) // 16 * 16 + 100 * 69 * 4
    for bad in ((-1, 3, 24), (100, 0, 24), (100, 3, 0), (100, 3, 33)):
        assert lib.phc_fit_sph_scratch_bytes(*bad) == S.EINVAL


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. refusals

REFUSALS = ([(f"null {p}", {p: None}, 1, S.EINVAL) for p in POINTERS]
            + [("iterations < 0", {}, -1, S.EINVAL), ("33 bodies", {"num_bodies": 33}, 1, S.EUNSUPPORTED), ("an extended body", {"num_ext": 1}, 1, S.EUNSUPPORTED),
               ("33 matched", {"num_matched": 33}, 1, S.EUNSUPPORTED), ("scratch one byte short", {"scratch_bytes": -1}, 1, S.EINVAL),
               ("no clips", {"num_clips": 0}, 1, S.EINVAL), ("num_ext < 0", {"num_ext": -1}, 1, S.EINVAL), ("NaN lr", {"lr": float("nan")}, 1, S.EINVAL),
               ("clip_start: an empty clip", {"clip_start_host": lambda s: s.__setitem__(3, s[2])}, 1, S.EINVAL),
               ("clip_start: does not end at num_frames", {"clip_start_host": lambda s: s.__setitem__(len(s) - 1, s[-1] + 1)}, 1, S.EINVAL),
               ("misaligned dof", {"dof_offset": 2}, 1, S.EINVAL)])


def apply_override(case, args, override, keep):
    for k, v in override.items():
        if callable(v):
            keep.append(T0._starts(case, v))
            setattr(args, k, keep[-1].ctypes.data)
        elif k == "scratch_bytes":
            args.scratch_bytes += v
        elif k == "dof_offset":
            args.dof += v
        else:
            setattr(args, k, v)


@pytest.mark.parametrize("what,override,iterations,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_fit_sph_refuses_and_leaves_the_state(what, override, iterations, code):
    case = S.make_batch("chain4s")
    st = {k: np.full_like(v, 7) for k, v in S.zero_state(case).items()}
    args, mem = S.place(case, st)
    assert args.axis is None                                  # `axis` is not read: null is fine
    assert S.shim().fit_sph_args_check_of(args, 1) == 0 and S.shim().fit_sph_args_check_of(args, 0) == 0
    assert S.shim().fit_sph_iterate_host(args, 0) == 0        # a no-op
    keep = []
    apply_override(case, args, override, keep)
    assert S.shim().fit_sph_args_check_of(args, iterations) == code
    assert S.shim().fit_sph_args_check_of(None, 1) == S.EINVAL
    assert S.shim().fit_sph_iterate_host(args, iterations) == code
    got = S.collect(mem)
    for k in S.STATE:
        assert (got[k] == 7).all(), k


def test_python_side_errors():
    from phc_amd.model import load_model
    from phc_amd.utils.fit_keypoints import fit_keypoint_clips
    model = S.smpl_model()
    kp = S.walk_keypoints(1.0)[:6]
    names = list(model.body_names)
    with pytest.raises(ValueError, match="backend"):
        fit_keypoint_clips(model, {"a": kp}, iterations=1, backend="gpu")
    with pytest.raises(ValueError, match="empty_one"):
        fit_keypoint_clips(model, {"a": kp, "empty_one": np.zeros((0, 24, 3))}, iterations=1)
    with pytest.raises(ValueError, match="empty_one"):
        fit_keypoint_clips(model, {"empty_one": np.zeros((0, 24, 3))}, iterations=1, backend="device", device="cuda:0")
    with pytest.raises(ValueError, match="24 columns"):
        fit_keypoint_clips(model, {"a": kp}, iterations=1, bodies=names[:23])
    with pytest.raises(ValueError, match="Tail"):
        fit_keypoint_clips(model, {"a": kp}, iterations=1, bodies=names[:23] + ["Tail"])
    with pytest.raises(ValueError, match="bodies"):
        fit_keypoint_clips(model, {"a": kp[:, :20]}, iterations=1)                        # neither 24 nor 22 columns and no names
    with pytest.raises(RuntimeError, match="backend=host"):
        fit_keypoint_clips(model, {"a": kp}, iterations=1, backend="device", device="cpu")   # never a fallback
    with pytest.raises(ValueError, match="fit_robot_motion"):
        fit_keypoint_clips(load_model("h1_humanoid"), {"a": kp}, iterations=1)
    with pytest.raises(ValueError, match="two keypoints"):
        fit_keypoint_clips(model, {"a": kp[:, :2]}, iterations=1, bodies=names[:2])       # one child of the root: no start rotation
    keep = [n for n in names if n != "L_Knee"]
    with pytest.raises(ValueError, match="L_Ankle"):
        fit_keypoint_clips(model, {"a": kp[:, [names.index(n) for n in keep]]}, iterations=1, bodies=keep, bone_lengths="model")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. gradient and the exact regimes

def check_gradient(case, got, oracle, what):
    """`got`: the state after ONE trip from zero moments, so that the first moment is (1 - 0.9) x the gradient.  Bound: 4 E + GRAD_FLOOR."""
    worst = {}
    for k in ("dof", "root_rot", "root_off"):
        g = got[k + "_m"].astype(np.float64) * 10.0
        assert np.isfinite(g).all()
        err, tol = np.abs(g - oracle["grad"][k]), 4 * oracle["E"][k] + GRAD_FLOOR
        worst[k] = float((err - tol).max())
        print(f"{what} {k}: max |gradient| {np.abs(oracle['grad'][k]).max():.3e}, max error {err.max():.3e}, max (error - bound) {worst[k]:.3e}, "
              f"max error / bound {(err / np.maximum(tol, 1e-300)).max():.3f}")
        assert worst[k] <= 0.0, (what, k, worst[k])
    return worst


def free_joints(marr):
    """Joints with no matched body strictly below their own body: their own keypoint, if any, has lever arm exactly 0."""
    nb, nd, M = S.dims(marr)
    mb = marr["match_body"]
    return [j for j in range(1, nb) if all(int(mb[m]) == j for m in range(M) if (int(marr["subtree"][j]) >> m) & 1)]


def check_regimes(case, got, oracle):
    s, marr = case["start"], case["marr"]
    nb, nd, M = S.dims(marr)
    free = free_joints(marr)
    if case["name"] == "chain4s":
        assert free == [2, 3]
    else:
        names = list(S.smpl_model().body_names)
        assert {names[j] for j in free} >= {"L_Toe", "R_Toe", "Head", "L_Hand", "R_Hand"}
    T = np.repeat(np.diff(s), np.diff(s))[:, None]
    reg = 0.02 * case["dof"].astype(np.float64) / (T * nd)
    for j in free:
        cols = slice(3 * (j - 1), 3 * j)
        np.testing.assert_allclose(oracle["grad"]["dof"][:, cols], reg[:, cols], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(got["dof_m"][:, cols].astype(np.float64) * 10, reg[:, cols], rtol=4 * S.EPS32 * 2, atol=1e-30)
    assert case["zero_entries"] and np.isfinite(got["root_off_m"]).all() and np.isfinite(got["root_rot_m"]).all()
    # at the limits: the regime is there when at least a quarter of clip 1's (frame, component) pairs are pushed outward
    assert case["outward"] >= 2 * nd // 4, (case["outward"], nd)
    # the constructed rotation vectors of clip 3, the root's and the joint of body 1's: 0, either side of the series' threshold, 3.1
    for k in ("root_rot", "dof"):
        r2 = (case[k][s[3]:s[4], 0:3].astype(np.float64) ** 2).sum(-1)
        assert r2[0] == 0.0 and 0 < r2[1] < 1e-8 < r2[2] < 1.1e-8 and abs(np.sqrt(r2[3]) - 3.1) < 1e-6


@pytest.mark.parametrize("name", S.NAMES)
def test_gradient_on_constructed_states(name):
    """The analytic gradient of the host build against autograd in fp64, clips of 1, 2, 3, 4, 5, 6 and 48 frames in one batch (regimes: `fit_sph_util.make_batch`).
    Bound 4 E + floor with E the oracle's rounding bound (`fit_sph_util.oracle_step`).  The floor is the smallest value at which torch's fp32 autograd gradient
    of the same statement passes too; measured on these cases (3 models, this test's second half): its largest error - 4 E is negative everywhere (closest:
    1.4e-1 of the bound, the root rotation vector of chain4s; the host build's closest is 1.5e-1, a joint of smpl22), so the floor is 0."""
    case = S.make_batch(name)
    st = S.zero_state(case)
    oracle = S.oracle_step(case, st)
    got = S.run(case, st, 1)
    check_gradient(case, got, oracle, f"{name} host build")
    check_regimes(case, got, oracle)
    assert np.array_equal(got["step"], case["step"] + 1)
    np.testing.assert_allclose(got["loss"], oracle["loss"], rtol=1e-5)
    g32 = S.torch32_grad(case, st)
    for k in ("dof", "root_rot", "root_off"):
        over = float((np.abs(g32[k] - oracle["grad"][k]) - 4 * oracle["E"][k]).max())
        print(f"{name} torch fp32 autograd {k}: max (error - 4 E) {over:.3e}")
        assert over <= GRAD_FLOOR


def hands_case():
    """smpl22 from the zero start: a few frames of the walk's keypoints without the hands."""
    from phc_amd.utils.fit_keypoints import sph_model_arrays
    case = S.clip_case(1.0)
    m = S.smpl_model()
    idx = [i for i, n in enumerate(m.body_names) if n not in ("L_Hand", "R_Hand")]
    return dict(case, marr=sph_model_arrays(m, idx), target=np.ascontiguousarray(case["target"][:, idx])), [3 * (i - 1) + c for i in range(24) if i not in idx for c in range(3)]


def check_hands_stay_zero(device=None):
    case, cols = hands_case()
    got = S.run(case, S.zero_state(case), 10, device=device)
    assert len(cols) == 6 and (got["dof"][:, cols] == 0.0).all() and (got["dof_m"][:, cols] == 0.0).all()
    assert np.abs(got["dof"]).max() > 1e-3          # (the other joints did move)


def test_unmatched_hands_stay_exactly_zero():
    check_hands_stay_zero()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. update

def fit_moments(st, seed=7):
    rng = np.random.RandomState(seed)
    for k in ("dof", "root_rot", "root_off"):      # moments of a fit in progress
        st[k + "_m"] = rng.normal(scale=0.01, size=st[k].shape).astype(np.float32)
        st[k + "_v"] = (rng.uniform(0.2, 2.0, size=st[k].shape) * 1e-4).astype(np.float32)
    return st


def check_update_and_clamp(case, st, got, what):
    """Adam + clamp + filter in fp64 on the build's own new moments at `expected_update`'s rounding bound; the clamp holds; everything lies in the ranges."""
    clamped = T0.check_update(case, st, got, what)
    s = case["start"]
    lo, hi = case["marr"]["range"][:, 0], case["marr"]["range"][:, 1]
    held = (clamped[s[1]:s[2]] == lo) | (clamped[s[1]:s[2]] == hi)
    assert held.sum() >= held.size // 4, held.sum()
    assert (got["dof"] >= lo - 1e-6).all() and (got["dof"] <= hi + 1e-6).all()


@pytest.mark.parametrize("name", S.NAMES)
def test_update_on_constructed_states(name):
    case = S.make_batch(name)
    st = fit_moments(S.zero_state(case))
    got = S.run(case, st, 1)
    check_update_and_clamp(case, st, got, f"{name} host build")
    s = case["start"]
    # a clip's neighbours never leak into it: other targets, vectors and moments next door, the same bits here
    for c in (0, 3, 6):
        other = dict(case, target=case["target"].copy(), rto=case["rto"].copy())
        st2 = {k: v.copy() for k, v in st.items()}
        mine = np.zeros(case["dof"].shape[0], dtype=bool)
        mine[s[c]:s[c + 1]] = True
        other["target"][~mine] += 0.7
        other["rto"][~mine] -= 0.3
        for k in ("dof", "dof_m", "root_rot", "root_rot_v"):
            st2[k][~mine] *= np.float32(0.5)
        got2 = S.run(other, st2, 1)
        for k in S.STATE:
            rows = slice(c, c + 1) if got[k].shape[0] == len(s) - 1 else slice(s[c], s[c + 1])
            assert np.array_equal(got[k][rows], got2[k][rows]), (name, c, k)
        assert not np.array_equal(got["dof"][~mine], got2["dof"][~mine])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. trajectory

NOISES = (0.0, 0.01)    # the clean walk (the rest-pose frames' residuals start at exactly 0: the L1 direction there is rounding) and 1 cm of keypoint noise


@functools.lru_cache(maxsize=None)
def host_states(iterations=10, noise=0.0):
    from phc_amd.utils.fit_keypoints import fit_keypoint_state
    kp = S.noisy_walk(1.0, noise)
    return tuple(fit_keypoint_state(S.smpl_model(), kp, iterations=iterations, dtype=dt) for dt in (torch.float64, torch.float32))


def check_trajectory(got, what, iterations=10, noise=0.0):
    """Joint vectors, root rotation vector and root_off after `iterations` trips from the real start (Kabsch root, zeros) on the 31-frame walk against the fp64
    host fit: max(4 d32, 2e-6), d32 the deviation of the fp32 host fit from the fp64 run on the same case, computed here.  On the clean walk the rule says
    little: the clip ramps out of the rest pose, so residuals of the first frames start at exactly 0, their L1 directions are rounding, and Adam's normalised
    step turns that into d32 ~ 5e-2 rad after ten iterations (measured).  With 1 cm of keypoint noise no residual is near 0: d32 ~ 2e-6, bound ~ 1e-5 (host
    build: 8.5e-7 measured), which is the case that holds the kernels to the statement."""
    want, host32 = host_states(iterations, noise)
    for k, w, h, g in zip(("dof", "root_rot", "root_off"), want, host32, (got["dof"], got["root_rot"], got["root_off"][0])):
        d32, err = float(np.abs(h - w).max()), float(np.abs(g.astype(np.float64) - w).max())
        print(f"{what} {k} after {iterations} iterations: error {err:.3e}, d32 {d32:.3e}, bound {max(4 * d32, 2e-6):.3e}")
        assert err <= max(4 * d32, 2e-6), (what, k, err, d32)


@pytest.mark.parametrize("noise", NOISES)
def test_trajectory_of_ten_iterations(noise):
    case = S.clip_case(1.0, noise)
    assert case["dof"].shape == (31, 69)
    got = S.run(case, S.zero_state(case), 10)
    assert got["step"].tolist() == [10]
    check_trajectory(got, f"host build, noise {noise}", noise=noise)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. segmenting and placement

def check_segmenting_and_placement(name, device=None):
    case = S.make_batch(name)
    st = S.zero_state(case)
    whole = S.run(case, st, 10, device=device)
    parts = S.run(case, st, 10, device=device, segments=[3, 7], scratch_fill=0x7FC00000)    # (what a call finds in the scratch does not matter either)
    for k in S.STATE:
        assert np.array_equal(whole[k], parts[k], equal_nan=True), (name, "3 + 7 != 10", k)
    assert whole["step"].tolist() == (case["step"] + 10).tolist()
    s = case["start"]
    for c in (0, 3, 6):
        for how, order in T0.PLACEMENTS.items():
            clips = order(c)
            sub = S.sub_case(case, clips)
            got = S.run(sub, S.zero_state(sub), 10, device=device)
            at = clips.index(c)
            for k in S.STATE:
                per_clip = whole[k].shape[0] == len(s) - 1
                a = whole[k][c:c + 1] if per_clip else whole[k][s[c]:s[c + 1]]
                b = got[k][at:at + 1] if per_clip else got[k][sub["start"][at]:sub["start"][at + 1]]
                assert np.array_equal(a, b), (name, c, how, k)


@pytest.mark.parametrize("name", ["chain4s", "smpl24"])
def test_segmenting_and_placement_keep_the_bits(name):
    check_segmenting_and_placement(name)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# 7. end to end

@functools.lru_cache(maxsize=None)
def host_fits(iterations):
    """The host backend on the 61-frame walk in fp32 and fp64 (computed once; the GPU file's yardstick too)."""
    from phc_amd.utils.fit_keypoints import fit_keypoint_clips
    kp = S.walk_keypoints(2.0)
    return tuple(fit_keypoint_clips(S.smpl_model(), {"walk": kp}, iterations=iterations, dtype=dt)["walk"] for dt in (torch.float32, torch.float64))


def check_clip(out, kp, iterations, what):
    """The gates of the end-to-end run: the error against both host precisions, the layout, and the way back through `MotionLibSMPL`'s own clip reader."""
    from phc_amd.config import EasyDict
    from phc_amd.env.tasks.humanoid_im import SkeletonTree
    from phc_amd.motion_lib import MotionLibSMPL
    m = S.smpl_model()
    h32, h64 = host_fits(iterations)
    e, e32, e64 = out["fit_keypoint_error"], h32["fit_keypoint_error"], h64["fit_keypoint_error"]
    print(f"{what}: fit_keypoint_error after {iterations} iterations {e * 1000:.3f} mm; host fp32 {e32 * 1000:.3f} mm, host fp64 {e64 * 1000:.3f} mm")
    assert e <= 2 * max(e32, e64), (e, e32, e64)
    T = len(kp)
    assert set(out) == {"pose_quat_global", "root_trans_offset", "pose_aa", "fps", "keypoints", "fit_loss", "fit_keypoint_error"}
    assert out["pose_quat_global"].shape == (T, 24, 4) and out["root_trans_offset"].shape == (T, 3) and out["pose_aa"].shape == (T, 72) and out["fps"] == 30
    np.testing.assert_allclose(out["keypoints"], kp, atol=1e-6)
    lib = MotionLibSMPL(EasyDict(dict(motion_file={"walk": out}, device="cpu", step_dt=1 / 30)))
    proc, fps, frames = lib._process_unique_clip(lib._motion_data_list[0], SkeletonTree(m.body_names, m.parent, m.local_translation), -1, None)
    assert frames == T and fps == 30
    back = float(np.linalg.norm(np.asarray(proc["gts"], dtype=np.float64) - kp, axis=-1).mean())      # catches quaternion order and body order
    print(f"{what}: keypoints through MotionLibSMPL's clip FK: {back * 1000:.3f} mm")
    assert abs(back - e) <= 1e-5, (back, e)
    return lib


def test_host_backend_end_to_end():
    kp = S.walk_keypoints(2.0)
    assert kp.shape == (61, 24, 3)
    check_clip(host_fits(100)[0], kp, 100, "host backend")


def test_order_up_and_bone_lengths():
    from phc_amd import stream
    from phc_amd.utils.fit_keypoints import fit_keypoint_clips
    m = S.smpl_model()
    kp = S.walk_keypoints(1.0)[:12]
    M = np.asarray(stream.TO_ISAAC_MAT, dtype=np.float64)
    raw = np.zeros_like(kp)
    raw[:, list(stream.SMPL_2_MUJOCO)] = kp @ np.linalg.inv(M.T)       # SMPL order, y up: what order="smpl", up="y" undo
    assert not np.allclose(raw, kp)
    a = fit_keypoint_clips(m, {"k": kp}, iterations=10)["k"]
    b = fit_keypoint_clips(m, {"k": raw}, iterations=10, order="smpl", up="y")["k"]
    np.testing.assert_allclose(b["keypoints"], a["keypoints"], atol=1e-6)
    for k in ("pose_quat_global", "root_trans_offset", "pose_aa"):
        np.testing.assert_allclose(b[k], a[k], atol=2e-5)               # fp32 fits of inputs one rounding apart, 10 iterations
    c = fit_keypoint_clips(m, {"k": 1.1 * kp}, iterations=2, bone_lengths="model")["k"]
    par = np.asarray(m.parent)
    bones = np.linalg.norm(c["keypoints"][:, 1:] - c["keypoints"][:, par[1:]], axis=-1)
    np.testing.assert_allclose(bones, np.broadcast_to(np.linalg.norm(m.local_translation[1:], axis=-1), bones.shape), atol=1e-6)
    np.testing.assert_allclose(c["keypoints"][:, 0], 1.1 * kp[:, 0], atol=1e-6)
    d = fit_keypoint_clips(m, {"k": kp[:, [i for i, n in enumerate(m.body_names) if n not in ("L_Hand", "R_Hand")]]}, iterations=10)["k"]
    hands = [i for i, n in enumerate(m.body_names) if n in ("L_Hand", "R_Hand")]
    assert (d["pose_aa"].reshape(-1, 24, 3)[:, hands] == 0.0).all() and d["keypoints"].shape[1] == 22


def test_cli_writes_a_library(tmp_path):
    import joblib
    from phc_amd.utils import fit_keypoints
    kp = S.walk_keypoints(1.0)
    np.savez(tmp_path / "kp.npz", **{"a/joints": kp[:5], "b/joints": kp[5:12], "b/fps": np.float64(60)})
    fit_keypoints.main(["--joints", str(tmp_path / "kp.npz"), "--out", str(tmp_path / "clips.pkl"), "--iterations", "2"])
    out = joblib.load(tmp_path / "clips.pkl")
    assert list(out) == ["a", "b"] and out["a"]["fps"] == 30 and out["b"]["fps"] == 60 and out["b"]["pose_quat_global"].shape == (7, 24, 4)


def test_host_build_runs_clean_under_the_address_and_undefined_sanitizers():
    """tests/fit_sph_asan_main.cpp (its own main; nothing is loaded into Python): a 4-body tree, a 1-body model and a 32-body chain, clips of 1, 2 and 9
    frames, on heap arrays of exact size with a null `axis`."""
    returncode, stdout, stderr = host_build.run_sanitized("fit_sph_asan_main.cpp")
    print(stdout[-2000:], stderr)
    assert returncode == 0 and stdout.strip().endswith("ok"), stdout + stderr
