"""The reference-motion lookup on constructed rotations in every regime of its quaternion math, through the shipped entry points only
(phc_motion_state, phc_amp_obs_demo, phc_amp_ref_table) and on both backends (tests/backends.py).

The golden motion library is 30 fps mocap: consecutive frames a small angle apart, moderate joint angles, an upright root.  It never takes slerp's
`c < 0` flip at a large angle, half_theta in (0.5, pi / 2), cos_half_theta rounding to 1; quat_to_exp_map / exp_map_round_trip with w < 0, |w| at or
beyond 1, not-quite-unit quaternions, either 1e-5 mask; the heading functions with a yaw beyond +-pi / 2 or a tilted root; or phc_motion_state at the
32 / 64-lane switch.  On the device these functions run t_rcp / t_div / t_sqrt / t_sincos / t_normalize_angle and ocml's acosf / atan2f, which the
host emulation (libm) does not.  tests/rotation_cases.py constructs the libraries and states the tolerance rule: per regime bin,
E_bin = |fp32 oracle - fp64 oracle| (the reference formula's own fp32 error); a backend passes at <= 4 E_bin + 2e-6 from the fp64 oracle, and the
well-conditioned cases additionally at 2e-5 from the fp32 oracle.

Measured 2026-10-18 on the tree of 9df2844 plus this file, hostemu on the CPU and hip on an MI355X (`pytest -s` prints these lines).  Columns: the
bin (pair regime, decade of s = sin(half_theta); for dof_pos also the sign of w and the decade of sin_theta of the slerped rotation; `nan`: c > 1 resp.
|w| > 1 on not-quite-unit data), cases, E_bin, largest distance to the fp64 oracle of hostemu and of hip.  The bound of a bin is 4 E_bin + 2e-6.
No hip bin needed more than the bound; the largest distance / bound over all bins is 0.37 (hip, AMP root block, identical pairs: 1.4e-6 of 3.9e-6).
The lerped outputs are bit-equal to the fp32 oracle on both backends.  Well-conditioned cases against the fp32 oracle (bound 2e-5): rb_rot 1.8e-7
hostemu / 2.4e-7 hip, dof_pos 8.3e-7 / 6.0e-7.

rb_rot: 8952 cases, 0 excluded (0.00 %)
  bin                                          n     E_bin   hostemu       hip
  identical s~1e-4                           748  0.00e+00  0.00e+00  0.00e+00
  identical s~1e-5                            49  0.00e+00  0.00e+00  0.00e+00
  identical s~nan                            667  0.00e+00  0.00e+00  0.00e+00
  large s~1e-1                              1224  2.14e-07  1.79e-07  1.82e-07
  mid s~1e-1                                1776  1.09e-06  1.03e-06  1.03e-06
  near_antipodal s~1e-1                     1434  1.73e-07  1.57e-07  1.94e-07
  small s~1e-2                               714  3.78e-05  3.79e-05  3.79e-05
  small s~1e-3                               744  1.07e-05  1.07e-05  1.07e-05
  tiny s~1e-4                                810  1.24e-04  1.24e-04  1.24e-04
  tiny s~1e-5                                 78  7.84e-05  7.84e-05  7.84e-05
  tiny s~nan                                 708  1.04e-04  1.04e-04  1.04e-04
dof_pos: 8579 cases, 7 excluded (0.08 %)
  bin                                          n     E_bin   hostemu       hip
  identical s~1e-2 w+ sin~1e-1                42  9.79e-07  1.39e-06  1.15e-06
  identical s~1e-3 w+ sin~1e-4               108  1.58e-10  9.96e-11  1.58e-10
  identical s~1e-3 w- sin~1e-4               108  7.43e-08  5.52e-08  7.43e-08
  identical s~1e-4 w+ sin~1e-1               208  3.77e-07  2.37e-07  3.77e-07
  identical s~1e-4 w+ sin~1e-2                18  9.86e-07  9.86e-07  9.86e-07
  identical s~1e-4 w+ sin~1e-4               180  4.74e-12  4.77e-12  4.77e-12
  identical s~1e-4 w- sin~1e-1               230  4.89e-07  4.86e-07  4.13e-07
  identical s~1e-4 w- sin~1e-2                12  5.44e-07  5.41e-07  5.37e-07
  identical s~1e-5 w+ sin~1e-1                42  1.81e-07  1.81e-07  1.68e-07
  identical s~1e-5 w+ sin~1e-5                72  0.00e+00  0.00e+00  0.00e+00
  identical s~1e-5 w- sin~1e-1                54  2.92e-07  3.52e-07  4.48e-07
  identical s~nan w+ sin~1e-1                248  3.26e-07  2.39e-07  2.48e-07
  identical s~nan w+ sin~1e-5                252  0.00e+00  0.00e+00  0.00e+00
  identical s~nan w+ sin~nan                  72  0.00e+00  0.00e+00  0.00e+00
  identical s~nan w- sin~1e-1                273  4.35e-07  4.35e-07  4.59e-07
  identical s~nan w- sin~1e-2                 18  2.31e-07  6.22e-07  2.27e-07
  identical s~nan w- sin~1e-4                108  1.76e-07  1.76e-07  1.76e-07
  identical s~nan w- sin~1e-5                108  0.00e+00  0.00e+00  0.00e+00
  identical s~nan w- sin~nan                  72  0.00e+00  0.00e+00  0.00e+00
  large s~1e-1 w+ sin~1e-1                   573  7.44e-07  4.91e-07  7.02e-07
  large s~1e-1 w+ sin~1e-2                     8  3.95e-07  3.95e-07  3.95e-07
  large s~1e-1 w- sin~1e-1                   592  6.14e-07  5.56e-07  5.58e-07
  large s~1e-1 w- sin~1e-2                     8  4.05e-07  4.05e-07  3.82e-07
  mid s~1e-1 w+ sin~1e-1                     792  2.53e-06  2.79e-06  2.99e-06
  mid s~1e-1 w+ sin~1e-2                      12  2.98e-07  2.67e-07  2.67e-07
  mid s~1e-1 w+ sin~1e-3                       2  4.36e-08  4.36e-08  4.55e-08
  mid s~1e-1 w- sin~1e-1                     615  2.09e-06  2.09e-06  2.09e-06
  mid s~1e-1 w- sin~1e-2                      16  9.12e-07  8.78e-07  8.78e-07
  mid s~1e-1 w- sin~1e-3                       3  2.63e-07  2.63e-07  2.63e-07
  near_antipodal s~1e-1 w+ sin~1e-1          538  6.74e-07  5.54e-07  6.48e-07
  near_antipodal s~1e-1 w+ sin~1e-2            8  6.05e-07  6.05e-07  6.05e-07
  near_antipodal s~1e-1 w+ sin~1e-3            2  1.67e-07  1.67e-07  1.67e-07
  near_antipodal s~1e-1 w- sin~1e-1          671  5.59e-07  6.53e-07  5.23e-07
  near_antipodal s~1e-1 w- sin~1e-2            9  9.39e-07  1.24e-06  7.75e-07
  near_antipodal s~1e-1 w- sin~1e-3            2  4.32e-07  2.90e-08  4.33e-07
  small s~1e-1 w+ sin~1e-1                     6  7.90e-07  6.02e-07  7.99e-07
  small s~1e-2 w+ sin~1e-1                   324  6.58e-05  6.58e-05  6.57e-05
  small s~1e-2 w+ sin~1e-2                    16  1.50e-06  1.51e-06  1.49e-06
  small s~1e-2 w- sin~1e-1                   358  8.50e-05  8.48e-05  8.52e-05
  small s~1e-2 w- sin~1e-2                    20  2.84e-06  2.70e-06  2.86e-06
  small s~1e-2 w- sin~1e-3                     2  2.23e-07  1.28e-07  1.28e-07
  small s~1e-3 w+ sin~1e-1                   210  3.01e-05  3.03e-05  3.01e-05
  small s~1e-3 w+ sin~1e-2                    18  5.60e-07  5.45e-07  5.67e-07
  small s~1e-3 w- sin~1e-1                   270  2.54e-05  2.55e-05  2.56e-05
  small s~1e-3 w- sin~1e-2                     6  4.99e-07  4.25e-07  6.22e-07
  small s~nan w+ sin~1e-1                      6  6.65e-08  6.65e-08  6.65e-08
  small s~nan w- sin~1e-1                      6  9.01e-08  6.08e-08  1.78e-07
  tiny s~1e-2 w+ sin~1e-1                     24  5.85e-07  6.59e-07  6.59e-07
  tiny s~1e-2 w- sin~1e-1                     24  6.03e-07  6.24e-07  6.95e-07
  tiny s~1e-4 w+ sin~1e-1                    276  2.61e-04  2.61e-04  2.61e-04
  tiny s~1e-4 w+ sin~1e-3                      6  3.54e-05  3.54e-05  3.54e-05
  tiny s~1e-4 w- sin~1e-1                    252  2.17e-04  2.17e-04  2.17e-04
  tiny s~1e-4 w- sin~1e-2                     24  1.46e-05  1.46e-05  1.46e-05
  tiny s~1e-5 w+ sin~1e-1                     30  1.74e-05  1.74e-05  1.74e-05
  tiny s~1e-5 w+ sin~1e-2                      6  2.13e-07  1.98e-07  1.98e-07
  tiny s~1e-5 w- sin~1e-1                     30  2.61e-04  2.61e-04  2.61e-04
  tiny s~nan w+ sin~1e-1                     270  3.53e-07  2.81e-07  2.88e-07
  tiny s~nan w+ sin~1e-2                       6  6.72e-07  6.65e-07  6.72e-07
  tiny s~nan w- sin~1e-1                     288  3.94e-07  2.65e-07  3.94e-07
  tiny s~nan w- sin~1e-2                      18  6.07e-07  6.07e-07  5.99e-07
AMP rows (per run: bins, cases, excluded, largest E_bin, largest distance hostemu / hip, largest distance / bound hostemu / hip)
  amp grid full root                   9   1250   0  3.23e-04  3.23e-04  3.23e-04  0.34  0.37
  amp grid full joint                 65  23750   0  2.03e-04  2.03e-04  2.03e-04  0.25  0.25
  amp grid full dof_vel                1   1250   0  1.19e-07  1.19e-07  1.19e-07  0.05  0.05
  amp grid table root                  9   1250   0  3.23e-04  3.23e-04  3.23e-04  0.34  0.37
  amp grid table joint                65  23750   0  2.03e-04  2.03e-04  2.03e-04  0.25  0.25
  amp grid table dof_vel               1   1250   0  1.19e-07  1.19e-07  1.19e-07  0.05  0.05
  amp off-grid full root               9   1300   0  5.05e-04  5.06e-04  5.05e-04  0.27  0.37
  amp off-grid full joint             57  24700   0  2.03e-04  2.03e-04  2.03e-04  0.25  0.25
  amp off-grid full dof_vel            1   1300   0  2.38e-07  2.38e-07  2.38e-07  0.08  0.08
  amp off-grid table root              9   1300   0  5.05e-04  5.06e-04  5.05e-04  0.27  0.37
  amp off-grid table joint            57  24700   0  2.03e-04  2.03e-04  2.03e-04  0.25  0.25
  amp off-grid table dof_vel           1   1300   0  2.38e-07  2.38e-07  2.38e-07  0.08  0.08
  amp base_rot grid full root          9   1250   0  2.09e-04  2.09e-04  2.09e-04  0.33  0.25
  amp base_rot grid full joint        60  23750   0  2.18e-04  2.18e-04  2.18e-04  0.25  0.25
  amp base_rot grid full dof_vel       1   1250   0  2.38e-07  2.38e-07  2.38e-07  0.08  0.08
  amp base_rot grid table root         9   1250   0  2.09e-04  2.09e-04  2.09e-04  0.33  0.25
  amp base_rot grid table joint       60  23750   0  2.18e-04  2.18e-04  2.18e-04  0.25  0.25
  amp base_rot grid table dof_vel      1   1250   0  2.38e-07  2.38e-07  2.38e-07  0.08  0.08
  amp base_rot off-grid full root      8   1300   0  2.09e-04  2.09e-04  2.09e-04  0.30  0.25
  amp base_rot off-grid full joint    56  24700   0  2.18e-04  2.18e-04  2.18e-04  0.25  0.25
  amp base_rot off-grid full dof_vel   1   1300   0  2.38e-07  2.38e-07  2.38e-07  0.08  0.08
  amp base_rot off-grid table root     8   1300   0  2.09e-04  2.09e-04  2.09e-04  0.30  0.25
  amp base_rot off-grid table joint   56  24700   0  2.18e-04  2.18e-04  2.18e-04  0.25  0.25
  amp base_rot off-grid table dof_vel   1   1300   0  2.38e-07  2.38e-07  2.38e-07  0.08  0.08
"""
import functools

import numpy as np
import pytest

import phc_oracle as po
import rotation_cases as rc
from backends import BACKENDS, get_backend, model_on, motion_lib_on
from test_task_parity import make_im_params

F = np.float32
EINVAL = -1                      # PHC_EINVAL
BLENDS = (0.0, 1 / 64, 1 / 4, 1 / 2, 3 / 4, 63 / 64)
CLIPS = 60                       # 2-frame clips of the SMPL library: 60 x 24 pairs per rotation field, ~240 per (global regime, local regime)
NB = 24


@functools.lru_cache(maxsize=None)
def smpl_library(base_rot=False):
    rng = np.random.default_rng(20 + int(base_rot))
    lib = rc.make_library(NB, 0, 3, rc.make_pairs(rng, CLIPS, NB, amp_roots=True, base_rot=base_rot), rng)
    for v in lib.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lib


@functools.lru_cache(maxsize=None)
def regime_lookups():
    """(ids, times, reference) of test a: every 2-frame clip at every blend, time = blend / 30, and the 5-frame clip at 13 times up to its length."""
    lib = smpl_library()
    pid = lib["pair_motion_ids"]
    ids = np.concatenate([np.repeat(pid, len(BLENDS)), np.full(13, lib["long_motion_id"])]).astype(np.int64)
    times = np.concatenate([np.tile(np.array(BLENDS, F) / F(30), len(pid)), np.linspace(0, 4 / 30, 13).astype(F)]).astype(F)
    times[-1] = lib["motion_lengths"][lib["long_motion_id"]]      # time == motion_length: frame nf - 1 with blend 0
    return ids, times, rc.reference(lib, ids, times)


@pytest.mark.parametrize("backend", BACKENDS)
def test_slerp_and_exp_map_regimes(backend):
    """phc_motion_state over every slerp regime x blend, the joints' exp-map over [0, 2 pi) and its edge members.
    Frame indices and the blend factor are bit-exact, and so are the lerped outputs (rg_pos, body_vel, body_ang_vel, dof_vel) against the fp32 oracle, on
    the device too: measured 0 ulp, the task kernels are compiled without FMA contraction and only the t_* functions use explicit fmas.  rb_rot and
    dof_pos follow the per-bin rule of rotation_cases.check_bins; the structural assertions below need no tolerance."""
    be = get_backend(backend)
    lib_np = smpl_library()
    lib, keep = motion_lib_on(be, lib_np)
    ids, times, (r32, r64, cases) = regime_lookups()
    n = len(ids)
    out = {k: be.zeros(s) for k, s in dict(rg_pos=(n, NB, 3), rb_rot=(n, NB, 4), body_vel=(n, NB, 3), body_ang_vel=(n, NB, 3),
                                           dof_pos=(n, 69), dof_vel=(n, 69), blend=(n,)).items()}
    i0, i1 = be.zeros(n, np.int64), be.zeros(n, np.int64)
    assert be.motion_state(lib, n, be.arr(ids), be.arr(times), None, *[out[k] for k in ("rg_pos", "rb_rot", "body_vel", "body_ang_vel", "dof_pos", "dof_vel")],
                           i0, i1, out["blend"]) == 0
    be.sync()
    got = {k: be.np(v) for k, v in out.items()}
    assert all(np.isfinite(v).all() for v in got.values())                    # (the |w| > 1 members included)

    # frame pair and blend: taken from the oracle, never assumed (time == motion_length is frame nf - 1 at blend 0; a last frame blends with itself)
    w0, w1, wb = po.calc_frame_blend(times, lib_np["motion_lengths"][ids], lib_np["motion_num_frames"][ids], lib_np["motion_dt"][ids])
    np.testing.assert_array_equal(be.np(i0), w0)
    np.testing.assert_array_equal(be.np(i1), w1)
    np.testing.assert_array_equal(got["blend"], wb)
    assert set(np.round(wb * 64).astype(int)) >= {0, 1, 16, 32, 48, 63}
    f0, f1 = r32["f0l"], r32["f1l"]

    # lerps: two products and a sum, no contraction on either backend (phc_kernels.hip is built with -ffp-contract=off)
    for k in ("rg_pos", "body_vel", "body_ang_vel", "dof_vel"):
        np.testing.assert_array_equal(got[k].reshape(r32[k].shape), r32[k], err_msg=k)

    # rb_rot and dof_pos, per regime bin
    rot = got["rb_rot"]
    rc.check_bins(f"{backend} rb_rot", rot.reshape(-1, 4), r32["rb_rot"].reshape(-1, 4), r64["rb_rot"].reshape(-1, 4),
                  rc.bin_keys(cases, "rb_rot").reshape(-1), rc.excluded(cases, "rb_rot").reshape(-1), rc.well_conditioned(cases, "rb_rot").reshape(-1))
    j = slice(1, None)
    rc.check_bins(f"{backend} dof_pos", got["dof_pos"].reshape(-1, 3), r32["dof_pos"].reshape(-1, 3), r64["dof_pos"].reshape(-1, 3),
                  rc.bin_keys(cases, "dof_pos")[:, j].reshape(-1), rc.excluded(cases, "dof_pos")[:, j].reshape(-1),
                  rc.well_conditioned(cases, "dof_pos")[:, j].reshape(-1))
    assert {rc.REGIMES[r] for r in np.unique(cases["g_regime"])} == set(rc.REGIMES) == {rc.REGIMES[r] for r in np.unique(cases["l_regime"])}

    # structure
    q0, q1 = lib_np["grs"][f0].astype(np.float64), lib_np["grs"][f1].astype(np.float64)
    q1 = np.where(((q0 * q1).sum(-1) < 0)[..., None], -q1, q1)                 # sign-aligned with q0
    reg = cases["g_regime"]
    same = reg == rc.IDENTICAL
    assert same.sum() > 1000 and (rot[same] == lib_np["grs"][f0][same]).all()   # identical pairs return q0 bit for bit
    tiny = reg == rc.REGIMES.index("tiny")
    mid = 0.5 * (q0 + q1)
    assert tiny.sum() > 1000 and (np.abs(rot - mid) <= 0.5 * np.abs(q1 - q0) + 1e-6)[tiny].all()     # the midpoint or q0, nothing else
    with np.errstate(invalid="ignore"):
        unit = ~tiny & (cases["g_s"] >= 0.05)
    assert unit.sum() > 3000 and np.abs(np.linalg.norm(rot.astype(np.float64), axis=-1) - 1.0)[unit].max() <= 4e-6
    masked = ((cases["sin_theta"] < 0.5e-5) | np.isnan(cases["sin_theta"]))[:, 1:]     # (NaN: |w| > 1, the default axis)
    assert masked.sum() > 100 and (got["dof_pos"].reshape(n, NB - 1, 3)[masked] == 0).all()


@functools.lru_cache(maxsize=None)
def amp_lookups(base_rot, on_grid):
    """(ids, t0, times [n, 10], reference of the n x 10 lookups): every clip started on its frames (the per-frame table serves those) or between them."""
    lib = smpl_library(base_rot)
    pid, lid = lib["pair_motion_ids"], lib["long_motion_id"]
    if on_grid:
        ids = np.concatenate([pid, pid, np.full(5, lid)])
        t0 = np.concatenate([np.zeros(len(pid), F), np.full(len(pid), rc.DT), np.arange(5).astype(F) * rc.DT]).astype(F)
    else:
        rng = np.random.default_rng(31)
        ids = np.concatenate([pid, pid, np.full(10, lid)])
        t0 = (rng.uniform(0.05, 0.95, len(ids)).astype(F) * lib["motion_lengths"][ids]).astype(F)
    ids = ids.astype(np.int64)
    dt = F(2 * (1 / 60))
    times = (t0[:, None] + (-dt) * np.arange(10, dtype=F)[None]).astype(F)       # humanoid_amp.py:258-260
    return ids, t0, times, rc.reference(lib, np.repeat(ids, 10), times.reshape(-1))


def _amp_rows(ms, key_ids, dof_subset, upright):
    return po.build_amp_observations_smpl(ms["root_pos"], ms["root_rot"], ms["root_vel"], ms["root_ang_vel"], ms["dof_pos"], ms["dof_vel"],
                                          ms["rg_pos"][:, key_ids], dof_subset, upright=upright)


def _check_amp_rows(label, rows, want32, want64, cases, amp_slot):
    """The per-bin rule on the three kinds of columns of [m, 196] AMP rows: the root block (height, rotation, heading-local velocities and key body
    positions: the root pair's slerp and the heading), each joint's 6 rotation columns (the local pair's slerp and the exp-map round trip), and the
    joint velocities (a lerp)."""
    nj = int((amp_slot >= 0).sum())
    root_cols = np.r_[0:13, 13 + 9 * nj:196]
    rc.check_bins(f"{label} root", rows[:, root_cols], want32[:, root_cols], want64[:, root_cols], rc.bin_keys(cases, "rb_rot")[:, 0],
                  rc.excluded(cases, "rb_rot")[:, 0], rc.well_conditioned(cases, "rb_rot")[:, 0])
    bodies = np.array([j for j in range(1, NB) if amp_slot[j] >= 0])
    cols = (13 + 6 * amp_slot[bodies])[:, None] + np.arange(6)[None]             # [nj, 6]
    pick = lambda a: a[:, cols].reshape(-1, 6)
    rc.check_bins(f"{label} joint", pick(rows), pick(want32), pick(want64), rc.bin_keys(cases, "dof_pos")[:, bodies].reshape(-1),
                  rc.excluded(cases, "amp_joint")[:, bodies].reshape(-1), rc.well_conditioned(cases, "dof_pos")[:, bodies].reshape(-1))
    vel = slice(13 + 6 * nj, 13 + 9 * nj)
    m = len(rows)
    rc.check_bins(f"{label} dof_vel", rows[:, vel], want32[:, vel], want64[:, vel], np.full(m, "dof_vel", dtype=object), np.zeros(m, bool), np.ones(m, bool))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("remove_base_rot", [False, True])
def test_amp_rows_over_rotation_regimes(backend, remove_base_rot):
    """phc_amp_obs_demo, built in full and from the phc_amp_ref_table rows, over root yaws in all four quadrants with tilts up to 60 deg and joint
    rotations over [0, 2 pi) with the edge members (the exp-map round trip and the heading functions), against po.get_motion_state +
    po.build_amp_observations_smpl in fp32 and fp64 under the per-bin rule.  With remove_base_rot the library's root rotations carry the factor the
    kernel strips, so the heading stays as well conditioned."""
    be = get_backend(backend)
    lib_np = smpl_library(remove_base_rot)
    model, mstruct, keepm = model_on(be)
    lib, keep = motion_lib_on(be, lib_np)
    N = 6
    extra = dict(remove_base_rot=True) if remove_base_rot else {}
    prm, keepp = make_im_params(be, model, N, **extra)
    track_slot, reset_mask, key_ids, amp_slot, td = keepp
    dof_subset = np.concatenate([np.arange(3 * (j - 1), 3 * j) for j in range(1, NB) if amp_slot[j] >= 0])
    nf, starts = lib_np["motion_num_frames"], lib_np["length_starts"]
    Ftot = int(starts[-1] + nf[-1])
    nxt = np.arange(1, Ftot + 1, dtype=np.int64)
    nxt[starts + nf - 1] = starts + nf - 1
    table = be.zeros((Ftot, 196))
    assert be.amp_ref_table(mstruct, lib, prm, Ftot, be.arr(nxt), table) == 0
    be.sync()
    assert np.isfinite(be.np(table)).all()
    prm_t, keept = make_im_params(be, model, N, amp_ref_table=table, **extra)

    for on_grid in (True, False):
        ids, t0, times, (r32, r64, cases) = amp_lookups(remove_base_rot, on_grid)
        n = len(ids)
        o_full, o_tab = be.zeros((n, 10, 196)), be.zeros((n, 10, 196))
        ids_d, t0_d = be.arr(ids), be.arr(t0)
        assert be.amp_obs_demo(mstruct, lib, prm, n, ids_d, t0_d, o_full) == 0 and be.amp_obs_demo(mstruct, lib, prm_t, n, ids_d, t0_d, o_tab) == 0
        be.sync()
        full, tab = be.np(o_full).reshape(n * 10, 196), be.np(o_tab).reshape(n * 10, 196)
        want32, want64 = (_amp_rows(r, key_ids, dof_subset, not remove_base_rot) for r in (r32, r64))
        tag = f"{backend} amp{' base_rot' if remove_base_rot else ''} {'grid' if on_grid else 'off-grid'}"
        _check_amp_rows(tag + " full", full, want32, want64, cases, amp_slot)
        _check_amp_rows(tag + " table", tab, want32, want64, cases, amp_slot)
        # table rows are the full build bit for bit where the blend factor is 0, and lookups between frames are built in full
        b = r32["blend"]
        exact = (b == 0) | (b > 1e-4)
        assert (exact.mean() > 0.95) if on_grid else ((b > 1e-4).sum() >= n)
        np.testing.assert_array_equal(tab[exact], full[exact])
        yaw = po.calc_heading(po.remove_base_rot(r64["root_rot"]) if remove_base_rot else r64["root_rot"])
        assert (np.abs(yaw) > np.pi / 2 + 0.1).sum() > 100 and (np.abs(yaw) < np.pi / 2 - 0.1).sum() > 100      # t_sincos with k = +-1 and k = 0


# ---- phc_motion_state at the 32 / 64-lane switch ------------------------------------------------------------------------------------------------
PAD = 64
SENT = {np.dtype(np.float32): F(1.2345e30), np.dtype(np.int64): np.int64(-0x5A5A5A5A5A5A5A5B)}


class Sent:
    """An output array inside a sentinel-filled allocation of the backend: `t` is the view the kernel writes; `check()` asserts that the padding came back
    unchanged, `untouched()` that nothing at all was written."""

    def __init__(self, be, shape, dtype=np.float32):
        self.be, self.n, self.s = be, int(np.prod(shape)), SENT[np.dtype(dtype)]
        assert self.n > 0
        self.base = be.arr(np.full(PAD + self.n + PAD, self.s, dtype=dtype))
        self.t = self.base[PAD:PAD + self.n].reshape(shape)

    def np(self):
        return self.be.np(self.t)

    def check(self, what):
        a = self.be.np(self.base)
        assert (a[:PAD] == self.s).all() and (a[PAD + self.n:] == self.s).all(), f"{what}: write outside the buffer"

    def untouched(self):
        return bool((self.be.np(self.base) == self.s).all())


@functools.lru_cache(maxsize=None)
def edge_library(nb, ne, dpj):
    rng = np.random.default_rng(1000 * nb + 10 * ne + dpj)
    lib = rc.make_library(nb, ne, dpj, rc.make_pairs(rng, 6, nb, ne, spherical=dpj != 1, regimes=("mid",)), rng)
    for v in lib.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return lib


LANE_SHAPES = [(32, 0, 3), (33, 0, 3), (20, 3, 1), (29, 3, 1), (30, 3, 1), (38, 0, 1), (64, 0, 1), (61, 3, 1)]
OUTPUTS = ("rg_pos", "rb_rot", "body_vel", "body_ang_vel", "dof_pos", "dof_vel", "idx0", "idx1", "blend", "rg_pos_ext", "rb_rot_ext")


def _edge_buffers(be, n, nb, ne, dpj):
    nd = (nb - 1) * (1 if dpj == 1 else 3)
    shapes = dict(rg_pos=(n, nb, 3), rb_rot=(n, nb, 4), body_vel=(n, nb, 3), body_ang_vel=(n, nb, 3), dof_pos=(n, nd), dof_vel=(n, nd), idx0=(n,), idx1=(n,),
                  blend=(n,))
    if ne:
        shapes.update(rg_pos_ext=(n, ne, 3), rb_rot_ext=(n, ne, 4))
    return {k: Sent(be, s, np.int64 if k in ("idx0", "idx1") else np.float32) for k, s in shapes.items()}


def _launch(be, lib, n, ids, times, off, bufs, present):
    return be.motion_state(lib, n, ids, times, off, *[bufs[k].t if k in present and k in bufs else None for k in OUTPUTS])


def _lane_group_case(be, nb, ne, dpj):
    lib_np = edge_library(nb, ne, dpj)
    lib, keep = motion_lib_on(be, lib_np)
    assert lib.num_bodies + lib.num_ext_bodies == nb + ne and lib.dofs_per_joint == dpj
    per_block = 256 // (64 if nb + ne > 32 else 32)
    rng = np.random.default_rng(7)
    for n in (1, per_block - 1, per_block, per_block + 1):
        ids = rng.integers(0, len(lib_np["motion_lengths"]), n).astype(np.int64)
        times = (rng.random(n).astype(F) * lib_np["motion_lengths"][ids]).astype(F)
        times[0] = lib_np["motion_lengths"][ids[0]]
        off = rng.standard_normal((n, 3)).astype(F)
        r32 = rc.reference(lib_np, ids, times, off)[0]
        want = dict(r32, idx0=r32["f0l"] - lib_np["length_starts"][ids], idx1=r32["f1l"] - lib_np["length_starts"][ids])
        if ne:
            want.update(rg_pos_ext=r32["rg_pos_t"][:, nb:], rb_rot_ext=r32["rg_rot_t"][:, nb:])
        ids_d, times_d, off_d = be.arr(ids), be.arr(times), be.arr(off)
        for present in (OUTPUTS, ("rb_rot", "rg_pos_ext")):
            bufs = _edge_buffers(be, n, nb, ne, dpj)
            assert _launch(be, lib, n, ids_d, times_d, off_d, bufs, present) == 0
            be.sync()
            for k, b in bufs.items():
                what = f"({nb}, {ne}, {dpj}) n={n} {k}"
                if k not in present:
                    assert b.untouched(), what + ": written although absent"
                    continue
                b.check(what)
                if k in ("idx0", "idx1", "blend"):
                    np.testing.assert_array_equal(b.np(), want[k], err_msg=what)
                else:
                    np.testing.assert_allclose(b.np().reshape(want[k].shape), want[k], rtol=0, atol=2e-5, err_msg=what)
    # n = 0: returns 0 and writes nothing
    bufs = _edge_buffers(be, 1, nb, ne, dpj)
    assert _launch(be, lib, 0, ids_d, times_d, off_d, bufs, OUTPUTS) == 0
    be.sync()
    assert all(b.untouched() for b in bufs.values()), f"({nb}, {ne}, {dpj}) n=0"


@pytest.mark.parametrize("backend", BACKENDS)
def test_motion_state_lane_group_edges(backend):
    """phc_motion_state with 32 and 33 slots (bodies + extended bodies), the two sides of the 32 -> 64 lanes-per-lookup switch, with and without extended
    bodies, and at the 64-slot limit; n one lookup below, at and above a 256-thread block.  Every output sits in a sentinel-padded allocation (the
    padding comes back unchanged); once with every optional output, once with only rb_rot and rg_pos_ext, the stand-ins of the absent ones untouched.
    2e-5 against the fp32 oracle (`mid` rotations only), the golden test's figure.  65 slots are refused with PHC_EINVAL before any launch."""
    be = get_backend(backend)
    for nb, ne, dpj in LANE_SHAPES:
        _lane_group_case(be, nb, ne, dpj)
    nb, ne, dpj = 62, 3, 1
    lib, keep = motion_lib_on(be, edge_library(nb, ne, dpj))
    n = 3
    bufs = _edge_buffers(be, n, nb, ne, dpj)
    assert _launch(be, lib, n, be.zeros(n, np.int64), be.zeros(n), None, bufs, OUTPUTS) == EINVAL
    be.sync()
    assert all(b.untouched() for b in bufs.values())
