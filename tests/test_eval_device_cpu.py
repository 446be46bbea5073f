"""CPU checks of the evaluation sweep's device metric path: the 3x3 similarity solve of phc_amd/csrc/phc_eval.h (`eval_similarity`, the uniform
part of `phc_eval_accumulate`'s Procrustes term), built for the host with g++ and compared against `im_eval._procrustes` (numpy SVD, fp64)."""
import ctypes as C

import numpy as np
import pytest

import host_build

F = np.float32
CLOUDS, POINTS = 200, 24


@pytest.fixture(scope="module")
def shim():
    lib = host_build.shim("eval_similarity_shim.cpp", "phc_eval.hip")
    lib.eval_similarity_batch.argtypes = [C.c_int] + [C.c_void_p] * 4
    lib.eval_similarity_batch.restype = None
    return lib


def _clouds(noise, seed):
    """CLOUDS (pred, gt) pairs of POINTS points, float64.  gt: humanoid-shaped (std 0.15 / 0.06 / 0.5 m); pred: a rotated, scaled, shifted and
    noised copy.  Every 5th pred is mirrored in y (det < 0), every 7th is an exact rotation + scale (no noise), every 11th is planar (pred and gt)."""
    rng = np.random.default_rng(seed)
    gt = rng.normal(size=(CLOUDS, POINTS, 3)) * np.array([0.15, 0.06, 0.5])
    gt[::11, :, 0] = 0.0
    pred = np.empty_like(gt)
    for i in range(CLOUDS):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        g = gt[i].copy()
        if i % 11 != 0 and i % 7 != 0:
            g = g + rng.normal(size=g.shape) * noise
        elif i % 7 != 0:   # planar: the noise stays in the plane
            g[:, [1, 2]] += rng.normal(size=(POINTS, 2)) * noise
        if i % 5 == 0:
            g[:, 1] = -g[:, 1]
        pred[i] = rng.uniform(0.7, 1.4) * g @ R.T + rng.normal(size=3) * 0.3
    return pred, gt


def _device_form(lib, pred, gt):
    """The kernel's evaluation: fp32 lane values (centred clouds, H, sum of squares), `eval_similarity`, fp32 residual norms."""
    p = (pred - pred.mean(1, keepdims=True)).astype(F)
    g = (gt - gt.mean(1, keepdims=True)).astype(F)
    H = np.ascontiguousarray(np.einsum("tji,tjk->tik", p, g).astype(F).reshape(len(p), 9))
    ss = np.ascontiguousarray((p * p).sum((1, 2)).astype(F))
    R = np.zeros((len(p), 9), dtype=F)
    sc = np.zeros(len(p), dtype=F)
    lib.eval_similarity_batch(len(p), H.ctypes.data, ss.ctypes.data, R.ctypes.data, sc.ctypes.data)
    aligned = sc[:, None, None] * np.einsum("tij,tkj->tki", R.reshape(-1, 3, 3), p)
    return np.linalg.norm((aligned - g).astype(np.float64), axis=-1).mean(-1) * 1000, R.reshape(-1, 3, 3)


@pytest.mark.parametrize("noise", [1e-3, 2e-2, 2e-1])
def test_similarity_solve_matches_numpy_procrustes(shim, noise):
    from phc_amd.learning.im_eval import _procrustes
    pred, gt = _clouds(noise, seed=int(noise * 1e4))
    want = np.linalg.norm(_procrustes(pred, gt) - gt, axis=-1).mean(-1) * 1000   # mm
    got, R = _device_form(shim, pred, gt)
    np.testing.assert_allclose(np.linalg.det(R.astype(np.float64)), 1.0, atol=1e-5)      # proper rotations, also for the mirrored clouds
    idx = np.arange(CLOUDS)
    assert (want[(idx % 7 == 0) & (idx % 5 != 0)] < 1e-3).all()         # pure rotation + scale: nothing left after the alignment
    assert (want[(idx % 5 == 0) & (idx % 11 != 0)] > 1e-3).all()        # a mirrored 3-D cloud cannot be aligned by a proper rotation
    err = np.abs(got - want)
    print(f"noise {noise}: max |device form - numpy| = {err.max():.3e} mm (residuals up to {want.max():.1f} mm)")
    assert (err <= 1e-3 + 1e-5 * np.abs(want)).all(), f"worst {err.max():.3e} mm at cloud {err.argmax()}"


def test_metrics_from_sums_is_compute_metrics_per_clip():
    """The device path's last step on the host: totals over frames and bodies -> the five metrics, NaN for clips that are too short."""
    from phc_amd.learning import im_eval as E
    rng = np.random.default_rng(0)
    T, NB, frames = 7, 24, [0, 1, 2, 3, 7]
    P = rng.normal(size=(T, len(frames), NB, 3))
    G = P + rng.normal(size=P.shape) * 0.02
    want = E.compute_metrics_per_clip([P[:n, i] for i, n in enumerate(frames)], [G[:n, i] for i, n in enumerate(frames)])
    sums = np.zeros((len(frames), 5))
    for i, n in enumerate(frames):
        p, g = P[:n, i], G[:n, i]
        if n == 0:
            continue
        pl, gl = p - p[:, :1], g - g[:, :1]
        norms = lambda x: np.linalg.norm(x, axis=-1).sum()
        sums[i] = [norms(p - g), norms(pl - gl), norms(E._procrustes(pl, gl) - gl), norms(np.diff(p, 2, axis=0) - np.diff(g, 2, axis=0)) if n > 2 else 0.0,
                   norms(np.diff(p, axis=0) - np.diff(g, axis=0)) if n > 1 else 0.0]
    got = E.metrics_from_sums(sums, np.array(frames, dtype=np.int32), NB)
    for k in E.METRICS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, equal_nan=True, err_msg=k)
    assert np.isnan(got["vel_dist"][:3]).all() and not np.isnan(got["vel_dist"][3:]).any() and np.isnan(got["mpjpe_g"]).tolist() == [True] + [False] * 4


def test_switch_and_binding():
    """`eval_metrics` accepts host / device only (checked where `evaluate` starts, before the task is touched); the entry point is bound."""
    from types import SimpleNamespace
    from phc_amd import _lib as L
    from phc_amd.learning.im_eval import evaluate
    with pytest.raises(ValueError, match="eval_metrics must be host or device"):
        evaluate(SimpleNamespace(task=None, vec_env=None, config={"eval_metrics": "gpu"}))
    assert "phc_eval_accumulate" in L.EXPORTED_SYMBOLS and hasattr(L.load(), "phc_eval_accumulate")
    assert C.sizeof(L.EvalArgs) == 24 + 15 * C.sizeof(C.c_void_p)
