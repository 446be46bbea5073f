"""The task kernels (k_im_post_physics, k_im_reset) on CONSTRUCTED states in every decision regime, against the whole-step oracle with a branch trace
(oracle/task_oracle.py, pinned to the reference's outputs by test_task_oracle_cpu.py).  The cases and their margins: tests/task_regimes.py.

  decisions, counters, clocks, progress, list membership     equal to the oracle's, exactly (no case is excluded)
  floating outputs                                            per regime bin (case class x output block) E_bin = |fp32 oracle - fp64 oracle|; a backend
                                                              passes at <= 4 E_bin + 2e-6 from the fp64 oracle; bins with E_bin <= 2e-6 (well conditioned)
                                                              additionally at 1e-5 from the fp32 oracle, the bar phc_math.h pins the device functions at
  exclusions                                                  observation columns of envs whose root's rotated x axis is within 0.1 of vertical (the heading
                                                              atan2); at most 2 % per test, printed
  placement                                                   a case gives the same bits in the batch, alone (N = 1) and at env 0 / 7 / 8 / last of a benign batch
  instantiations (hip)                                        plain-eligible groups: shipped == phc_task_force_generic(1), bit for bit; the others are not plain

Run with -s for the per-bin table.  Both backends of tests/backends.py (`hip` under the gpu marker).

Measured 2026-10-20 on the tree of 0e0b144 plus this change, hostemu on the CPU and hip on an MI355X.  `pytest -s` prints one line per bin (case class x
output block: 1550 bins per backend); below they are merged once per output block and once per group of cases (tests/task_regimes.py GROUPS, and the
reset tests): bins, cases, excluded cases, the largest E_bin, the largest distance to the fp64 oracle of hostemu and of hip, and the worst
distance / bound of a single bin (bound = 4 E_bin + 2e-6).  No bin of either backend needed more than the bound, and no case was excluded (the
tilts stop at 85 degrees about x, which does not lift the x axis, and 80 about y: horizontal length >= 0.17).  Where E_bin is large it is the REFERENCE's fp32
error -- slerp of two mocap frames divides sin(t acos c) by sqrt(1 - c^2) at c ~ 1 - 1e-4 (not-quite-unit reference rotations: 1.7e-4 in the rotation
columns, 1e-3 in exp(-k_rot mean(angle^2)), because 2 acos(w) of such a rotation against itself is not 0) -- and both backends sit ON the fp32 oracle
there (distance = E_bin, ratio 0.25).  The largest ratios are absolute: a body 4 m from its reference (occlusion group) gives position differences of
magnitude 4, where 4 ulp are 1.9e-6 of the 2e-6 floor.  Per-frame AMP table against the full build: 2.4e-7 hostemu, 4.8e-7 hip, 98 % of the rows bit-equal on both.

bins 1550
  output block               bins  cases  excl  max E_bin   hostemu       hip  worst dist/bound (hostemu, hip)
  reward                       52   1089     0  4.77e-04  4.77e-04  4.77e-04  0.25  0.25
  reward_raw.pos               52   1089     0  1.16e-06  1.16e-06  1.16e-06  0.17  0.17
  reward_raw.rot               52   1089     0  1.59e-03  1.59e-03  1.59e-03  0.25  0.25
  reward_raw.vel               52   1089     0  1.01e-07  3.01e-08  3.13e-08  0.01  0.01
  reward_raw.angvel            52   1089     0  1.01e-07  3.08e-08  3.32e-08  0.01  0.01
  reward_raw.power             52   1089     0  3.95e-08  4.84e-08  2.48e-08  0.02  0.01
  self_obs.height              71   1093     0  0.00e+00  0.00e+00  0.00e+00  0.00  0.00
  self_obs.pos                 74   1229     0  8.30e-06  8.43e-06  8.40e-06  0.33  0.33
  self_obs.rot                 74   1229     0  1.70e-04  1.70e-04  1.70e-04  0.25  0.25
  self_obs.vel                 74   1229     0  6.10e-05  5.59e-05  6.10e-05  0.25  0.25
  self_obs.angvel              74   1229     0  1.53e-05  1.53e-05  1.53e-05  0.28  0.26
  task_obs.dpos                62    685     0  2.70e-05  2.75e-05  2.77e-05  0.94  0.94
  task_obs.drot                62    685     0  7.85e-04  7.85e-04  7.84e-04  0.25  0.25
  task_obs.dvel                62    685     0  1.06e-04  6.28e-05  1.06e-04  0.21  0.25
  task_obs.dangvel             62    685     0  4.41e-06  4.44e-06  4.47e-06  0.24  0.24
  task_obs.ref_pos             62    685     0  2.70e-05  2.75e-05  2.77e-05  0.25  0.25
  task_obs.ref_rot             62    685     0  7.83e-04  7.83e-04  7.83e-04  0.25  0.25
  amp_obs                      74   1229     0  6.55e-04  6.55e-04  6.55e-04  0.41  0.41
  ref1_pos                     74   1229     0  6.26e-07  6.26e-07  6.26e-07  0.14  0.14
  ref1_rot                     52   1089     0  3.88e-05  3.88e-05  3.88e-05  0.25  0.25
  ref1_vel                     52   1089     0  9.36e-08  9.36e-08  9.36e-08  0.04  0.04
  ref1_dof_pos                 52   1089     0  2.08e-05  2.09e-05  2.10e-05  0.25  0.25
  goff                         68   1137     0  5.07e-07  5.07e-07  5.07e-07  0.13  0.13
  point_goal                   19     45     0  3.94e-07  3.94e-07  3.94e-07  0.11  0.11
  task_obs                     12    544     0  1.72e-04  1.73e-04  1.72e-04  0.25  0.25
  body_pos                     16     48     0  0.00e+00  0.00e+00  0.00e+00  0.00  0.00
  body_rot                     16     48     0  3.80e-05  3.81e-05  3.81e-05  0.25  0.25
  body_vel                     16     48     0  0.00e+00  0.00e+00  0.00e+00  0.00  0.00
  body_ang_vel                 16     48     0  0.00e+00  0.00e+00  0.00e+00  0.00  0.00
  dof_pos                      16     48     0  7.86e-04  7.86e-04  7.86e-04  0.25  0.25
  dof_vel                      16     48     0  0.00e+00  0.00e+00  0.00e+00  0.00  0.00
  group                      bins  cases  excl  max E_bin   hostemu       hip  worst dist/bound (hostemu, hip)
  termination                 115   1150     0  1.11e-03  1.11e-03  1.11e-03  0.27  0.27
  termination_equal            23     46     0  1.28e-03  1.28e-03  1.28e-03  0.25  0.25
  mean_root_below              46     46     0  1.45e-03  1.45e-03  1.45e-03  0.25  0.25
  mean_root_above              46     46     0  1.45e-03  1.45e-03  1.45e-03  0.25  0.25
  no_collision_check           23     46     0  1.11e-03  1.10e-03  1.11e-03  0.25  0.25
  no_early_termination         23     46     0  1.11e-03  1.10e-03  1.11e-03  0.25  0.25
  occlusion                    69     69     0  1.11e-03  1.10e-03  1.11e-03  0.94  0.94
  track_reward                 23     69     0  8.44e-04  8.43e-04  8.43e-04  0.25  0.25
  cycle_zero_out_far          168    504     0  5.30e-04  5.30e-04  5.30e-04  0.25  0.25
  recovery                     23     92     0  1.11e-03  1.10e-03  1.11e-03  0.25  0.25
  reward                       69    575     0  1.11e-03  1.10e-03  1.11e-03  0.41  0.41
  obs_v6                       69   3128     0  6.30e-04  6.30e-04  6.30e-04  0.25  0.25
  obs_v6_base_rot              69   3128     0  6.79e-04  6.79e-04  6.80e-04  0.28  0.26
  obs_v6_global_root           66   2992     0  6.30e-04  6.30e-04  6.30e-04  0.25  0.25
  obs_v2                       54   2448     0  6.30e-04  6.30e-04  6.30e-04  0.25  0.25
  obs_v7_base_rot              54   2448     0  6.79e-04  6.79e-04  6.80e-04  0.28  0.26
  obs_v8                       54   2448     0  6.30e-04  6.30e-04  6.30e-04  0.25  0.25
  obs_v9_global_root           54   2448     0  6.30e-04  6.30e-04  6.30e-04  0.25  0.25
  g1_upper_lanes               46    322     0  1.39e-03  1.39e-03  1.39e-03  0.25  0.25
  h1_extended                  23     92     0  1.56e-03  1.56e-03  1.56e-03  0.25  0.25
  h1_cycled                    23     69     0  1.59e-03  1.59e-03  1.59e-03  0.25  0.25
  reset                        80    480     0  7.86e-04  7.86e-04  7.86e-04  0.25  0.25
  reset_far                   252    504     0  7.86e-04  7.86e-04  7.86e-04  0.25  0.25
  reset_from_state0            39    598     0  1.73e-04  1.72e-04  1.72e-04  0.26  0.25
  reset_from_state1            39    598     0  1.73e-04  1.72e-04  1.72e-04  0.26  0.25
  largest hip dist / bound:
    occlusion / occluded_other task_obs.dpos: E_bin 7.45e-09, hip 1.91e-06, bound 2.03e-06
    reward / pos_error amp_obs: E_bin 9.54e-07, hip 2.38e-06, bound 5.81e-06
    occlusion / occluded_other self_obs.pos: E_bin 9.54e-07, hip 1.91e-06, bound 5.81e-06
    termination / unmasked_far amp_obs: E_bin 2.84e-07, hip 8.34e-07, bound 3.14e-06
    occlusion / occluded_other self_obs.angvel: E_bin 1.79e-07, hip 7.15e-07, bound 2.72e-06
    obs_v6_base_rot / root_tilt_x self_obs.angvel: E_bin 7.16e-07, hip 1.25e-06, bound 4.87e-06"""
import numpy as np
import pytest

import task_oracle as to
import task_regimes as tr
from backends import BACKENDS, get_backend
from phc_amd import abi

F = np.float32
FACTOR, FLOOR, STRICT, WELL, MAX_EXCLUDED = 4.0, 2e-6, 1e-5, 2e-6, 0.02
HEADING_FIELDS = ("self_obs", "task_obs", "amp_obs")


def blocks(cfg, field, width):
    """Column blocks of an output, so that an ill-conditioned block (reference rotations) does not lend its E_bin to a well-conditioned one."""
    J, nb = len(cfg["track_ids"]), cfg["num_bodies"]
    h = 1 if cfg["root_height_obs"] else 0
    if field == "task_obs" and cfg["obs_v"] in (4, 6):
        cuts = [("dpos", 3 * J), ("drot", 6 * J), ("dvel", 3 * J), ("dangvel", 3 * J), ("ref_pos", 3 * J), ("ref_rot", 6 * J)]
    elif field == "self_obs":
        cuts = [("height", h), ("pos", 3 * (nb - 1)), ("rot", 6 * nb), ("vel", 3 * nb), ("angvel", 3 * nb)]
    elif field == "reward_raw":
        cuts = [("pos", 1), ("rot", 1), ("vel", 1), ("angvel", 1)] + ([("power", 1)] if cfg["power_reward"] else [])
    else:
        return [("", slice(0, width))]
    out, a = [], 0
    for name, w in cuts:
        if w:
            out.append((name, slice(a, a + w)))
        a += w
    assert a == width, (field, a, width)
    return out


def compare(label, g, got, o32, o64, t64, table, exact=tr.POST_EXACT, floats=tr.POST_FLOAT):
    """The rules of the module docstring for one launch's outputs `got` (env-aligned with the oracle's); `g`: anything with `names` and `cfg`."""
    for k in exact:
        if got.get(k) is not None and o64.get(k) is not None:
            np.testing.assert_array_equal(got[k], o64[k], err_msg=f"{label}: {k}")
    classes = np.array([n.split("/")[0] for n in g.names])
    band = t64["heading_horizontal"] < tr.HEADING_BAND if "heading_horizontal" in t64 else np.zeros(len(classes), bool)
    bad = []
    for field in floats:
        if got.get(field) is None or o64.get(field) is None:
            continue
        N = len(classes)
        a, r32, r64 = (np.asarray(x, np.float64).reshape(N, -1) for x in (got[field], o32[field], o64[field]))
        assert np.isfinite(a).all() and np.isfinite(r32).all() and np.isfinite(r64).all(), f"{label}: {field} not finite"
        excl = band if field in HEADING_FIELDS else np.zeros(N, bool)
        assert excl.mean() <= MAX_EXCLUDED, f"{label}: {field}: {100 * excl.mean():.1f} % excluded"
        for bname, sl in blocks(g.cfg, field, a.shape[1]):
            for c in sorted(set(classes)):
                m = (classes == c) & ~excl
                if not m.any():
                    continue
                E, D, D32 = np.abs(r32[m, sl] - r64[m, sl]).max(), np.abs(a[m, sl] - r64[m, sl]).max(), np.abs(a[m, sl] - r32[m, sl]).max()
                table.append((label, f"{c} {field}.{bname}".rstrip("."), int(m.sum()), int(((classes == c) & excl).sum()), E, D))
                if not D <= FACTOR * E + FLOOR or (E <= WELL and not D32 <= STRICT):
                    bad.append((c, field, bname, f"E_bin={E:.2e} dist={D:.2e} to_fp32={D32:.2e}"))
    assert not bad, f"{label}: bins beyond 4 E_bin + 2e-6 (or, well conditioned, beyond 1e-5 of the fp32 oracle): {bad}"


def print_table(table):
    for label, key, n, ex, E, D in table:
        print(f"[{label}] {key:<44s} n={n:<4d} excl={ex:<3d} E_bin={E:.2e} dist={D:.2e} bound={FACTOR * E + FLOOR:.2e}")


def amp_history(g, seed=0):
    N = len(g.names)
    return np.random.default_rng(seed).standard_normal((N, g.cfg["num_amp_obs_steps"], tr.obs_sizes(g.cfg)[2])).astype(F)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(tr.GROUPS))
def test_post_physics_regimes(backend, name):
    be = get_backend(backend)
    g, o32, o64, t64 = tr.group(name)
    hist = amp_history(g)
    got = tr.run_post(be, g.su, g.cfg, g.st, hist, want_plain=g.plain)
    table = []
    compare(f"{name}/{backend}", g, got, o32, o64, t64, table)
    print_table(table)
    np.testing.assert_array_equal(got["amp_hist"], hist[:, :-1])                                # the history shift
    listed = tr.listed_envs(got)
    np.testing.assert_array_equal(np.sort(listed), np.nonzero(o64["reset"])[0])                 # list membership: each finished env once
    rl, rc = got["reset_lists"], got["reset_counts"]
    assert (rc[0] == 0).all() and (rc[2] == 0).all()
    assert all(((rl[s, :rc[1, s]] >> 3) % abi.RESET_SUBLISTS == s).all() for s in range(abi.RESET_SUBLISTS))


def rows(st, idx):
    return {k: (None if v is None else np.asarray(v)[idx]) for k, v in st.items()}


def benign(g, n):
    """n envs of the group's option set that sit on the reference, mid clip, nothing pending."""
    st = tr.base_state(g.kind, g.cfg, np.arange(n) % 6, np.full(n, 5), np.full(n, 0.2, F), seed=99)
    fill = dict(cycle_counter=(np.int32, 0), recovery_counter=(np.int32, 0), point_goal=(F, 0.05), cycle_phase=(F, 0.5))
    for k, v in g.st.items():
        if k not in st:
            st[k] = np.full(n, fill[k][1], fill[k][0]) if k in fill else np.zeros((n,) + np.asarray(v).shape[1:], np.asarray(v).dtype)
    return st


PLACED = tr.POST_EXACT + tr.POST_FLOAT + ("amp_hist",)


def _bits(a):
    return a.view(np.int32) if a.dtype == F else a


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(tr.GROUPS))
def test_placement(backend, name):
    """Every case of the group (12 spread over it where it has more than 60): in the batch, alone (N = 1), and at env 0 / 7 / 8 / last of 20 benign envs
    (env 8 opens the second 256-thread block at 32 lanes per env) -- the per-env outputs are the same bits."""
    be = get_backend(backend)
    g, o32, o64, t64 = tr.group(name)
    N = len(g.names)
    pick = np.arange(N) if N <= 60 else np.unique(np.linspace(0, N - 1, 12).astype(int))
    hist = amp_history(g)
    batch = tr.run_post(be, g.su, g.cfg, g.st, hist)
    slots = np.array([0, 7, 8, 19])
    for i in range(0, len(pick), 4):
        chunk = pick[i:i + 4]
        st, h = benign(g, 20), amp_history(g, 1)[:1].repeat(20, 0)
        for p, c in zip(slots, chunk):
            for k in st:
                if st[k] is not None:
                    st[k][p] = np.asarray(g.st[k])[c]
            h[p] = hist[c]
        emb = tr.run_post(be, g.su, g.cfg, st, h)
        for p, c in zip(slots, chunk):
            one = tr.run_post(be, g.su, g.cfg, rows(g.st, [c]), hist[[c]])
            for k in PLACED:
                if batch.get(k) is not None:
                    np.testing.assert_array_equal(_bits(one[k][0]), _bits(batch[k][c]), err_msg=f"{name}: {g.names[c]}: {k} alone")
                    np.testing.assert_array_equal(_bits(emb[k][p]), _bits(batch[k][c]), err_msg=f"{name}: {g.names[c]}: {k} at env {p}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(tr.GROUPS))
def test_instantiations(name):
    """Plain-eligible groups run the plain instantiation as shipped and the generic one under phc_task_force_generic(1): every written tensor has the
    same bits.  Every other group must report is_plain false (run_post asserts it) and must not change under the switch."""
    be = get_backend("hip")
    g, o32, o64, t64 = tr.group(name)
    hist = amp_history(g)
    shipped = tr.run_post(be, g.su, g.cfg, g.st, hist, want_plain=g.plain)
    old = be.lib.phc_task_force_generic(1)
    try:
        generic = tr.run_post(be, g.su, g.cfg, g.st, hist, want_plain=g.plain)
    finally:
        be.lib.phc_task_force_generic(old)
    np.testing.assert_array_equal(np.sort(tr.listed_envs(shipped)), np.sort(tr.listed_envs(generic)))
    for k, v in shipped.items():
        if v is not None and k != "reset_lists":      # (the order inside a sub-list is the order of the atomics)
            np.testing.assert_array_equal(v.view(np.int32) if v.dtype == F else v, generic[k].view(np.int32) if v.dtype == F else generic[k], err_msg=f"{name}: {k}")


# ---- resets ----------------------------------------------------------------------------------------------------------------------------------------
class Cases:
    def __init__(self, names, cfg):
        self.names, self.cfg = names, cfg


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("far_start", [False, True])
def test_reset_at_the_clip_edges(backend, far_start):
    """phc_im_reset with a phase array: start time 0 (history times negative: frame 0), start in the last frame (t + dt past the end: clamped index, blend
    1); with zero_out_far_train the far start -- reference moved to a point of the 5 m disk, cycle_counter = zero_out_far_steps, observations gated."""
    be = get_backend(backend)
    su = tr.setup("smpl")
    cfg, mids, env_ids, phase, t, uv = tr.reset_edge_case(far_start)
    opt = dict(offset_rand=uv, cycle_counter=np.full(len(mids), 5, np.int32), point_goal=np.full(len(mids), 9, F)) if far_start else {}
    got = tr.run_reset(be, su, cfg, mids, env_ids, phase, **opt)
    trace = {}
    o32 = to.reset_step(su.lib, cfg, mids[env_ids], t, F, None if uv is None else uv[env_ids])
    o64 = to.reset_step(su.lib, cfg, mids[env_ids], t, np.float64, None if uv is None else uv[env_ids], trace=trace)
    sub = {k: (None if v is None else v[env_ids]) for k, v in got.items()}
    names = [f"phase_{phase[i]:g}/{i}" for i in range(len(env_ids))]
    if far_start:
        t32 = {}
        to.reset_step(su.lib, cfg, mids[env_ids], t, F, uv[env_ids], trace=t32)
        d = trace["zof_dist"]
        for T in (0.3, 3.0):
            assert tr.margin_ok(d, t32["zof_dist"], np.float64(F(T))).all()
        assert (d < 0.3).sum() >= 3 and ((d > 0.3) & (d < 3.0)).sum() >= 3 and (d > 3.0).sum() >= 3
        assert (sub["cycle_counter"] == 37).all()
        names = [("near" if x < 0.3 else "mid" if x < 3.0 else "far") + "_" + n for x, n in zip(d, names)]
    else:
        assert (t[phase == 0] == 0).all() and (to.motion_time(np.ones(len(t), np.int64), cfg["dt"], t, 0 * t)[phase == 1] >= su.lib["motion_lengths"][mids[env_ids]][phase == 1]).all()
    table = []
    compare(f"reset{'_far' if far_start else ''}/{backend}", Cases(names, cfg), sub, o32, o64, {}, table, exact=tr.RESET_EXACT if far_start else tr.RESET_EXACT[:3],
            floats=tr.RESET_FLOAT)
    print_table(table)
    assert (sub["reset"] == 0).all() and (sub["terminate"] == 0).all() and (sub["contact"] == 0).all() and (sub["dof_force"] == 0).all()
    np.testing.assert_array_equal(sub["pd_target"], sub["dof_pos"])
    np.testing.assert_array_equal(sub["root"], np.concatenate([sub[k][:, 0] for k in ("body_pos", "body_rot", "body_vel", "body_ang_vel")], -1))
    rest = np.setdiff1d(np.arange(len(mids)), env_ids)
    assert (got["progress"][rest] == 7).all() and (got["start"][rest] == -1).all() and (got["body_pos"][rest] == 1).all() and (got["self_obs"][rest] == 0).all()
    assert (got["amp_obs"][rest] == 0).all() and (got["reset"][rest] == 1).all() and (got["contact"][rest] == 1).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_reset_amp_history_from_the_per_frame_table(backend):
    """With amp_ref_table set the history frames come from the per-frame table: against the full build of the same backend (5e-6, the bound
    test_task_parity.py holds the same rows to on the same library) and, by the bins of the full build, against the oracle."""
    be = get_backend(backend)
    su = tr.setup("smpl")
    cfg, mids, env_ids, phase, t, _ = tr.reset_edge_case()
    full = tr.run_reset(be, su, cfg, mids, env_ids, phase)
    tab = tr.run_reset(be, su, cfg, mids, env_ids, phase, table=True)
    d = np.abs(full["amp_obs"] - tab["amp_obs"])
    print(f"[reset_table/{backend}] table vs full build: max {d.max():.2e}, rows bit-equal {100 * (d.max(-1) == 0).mean():.0f} %")
    assert d.max() <= 5e-6 and (d.max(-1) == 0).mean() > 0.5
    for k, v in full.items():
        if k != "amp_obs" and v is not None:
            np.testing.assert_array_equal(v, tab[k], err_msg=k)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("fill", [0, 1])
def test_reset_from_a_tilted_yawed_fallen_state(backend, fill):
    """phc_im_reset_from_state on the tilted / yawed states of the observation group (every body off the reference): observations at progress 0 against
    the env's unchanged clock, AMP frame 0 (fill_history 0) or every frame (1) from the state, everything else kept."""
    be = get_backend(backend)
    g, _, _, t64 = tr.group("obs_v6")
    N = len(g.names)
    env_ids = np.arange(N)[::3].copy()
    st = dict(g.st, progress=np.full(N, 9, np.int64))
    hist = amp_history(g, 3)
    got = tr.run_reset_from_state(be, g.su, g.cfg, st, env_ids, fill, hist)
    sub_st = rows(st, env_ids)
    tr64 = {}
    o32, o64 = to.reset_from_state(g.su.lib, g.cfg, sub_st, F, fill), to.reset_from_state(g.su.lib, g.cfg, sub_st, np.float64, fill, trace=tr64)
    sub = {k: (None if v is None else v[env_ids]) for k, v in got.items()}
    sub["amp_obs"] = sub["amp_obs"][:, 0]
    table = []
    compare(f"reset_from_state{fill}/{backend}", Cases([g.names[i] for i in env_ids], g.cfg), sub, o32, o64, tr64, table, exact=("progress",),
            floats=("self_obs", "task_obs", "amp_obs", "ref1_pos"))
    print_table(table)
    A = got["amp_obs"]
    if fill:
        for k in range(1, A.shape[1]):
            np.testing.assert_array_equal(A[env_ids, k], A[env_ids, 0])
    else:
        np.testing.assert_array_equal(A[env_ids, 1:], hist[env_ids, 1:])
    rest = np.setdiff1d(np.arange(N), env_ids)
    np.testing.assert_array_equal(A[rest], hist[rest])
    np.testing.assert_array_equal(got["pd_target"][env_ids], st["dof_pos"][env_ids])
    np.testing.assert_array_equal(got["body_rot"], st["body_rot"])
    assert (got["progress"][rest] == 9).all() and (got["contact"][env_ids] == 0).all() and (got["contact"][rest] == 1).all()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("N", [300, 384])
def test_reset_lists_when_every_env_finishes(backend, N):
    """Every env's clip ends in the same launch: each env is listed exactly once, in the sub-list of its workgroup, and the counts sum to N.  At N = 300
    (38 workgroups of 8 envs over 16 sub-lists of capacity 24) the five sub-lists that own three full workgroups are filled to their capacity, the others
    hold 20 or 16; at N = 384 every sub-list count equals its capacity."""
    be = get_backend(backend)
    su = tr.setup("smpl")
    cfg = tr.oracle_cfg("smpl")
    mids = np.arange(N) % 6
    st = tr.base_state("smpl", cfg, mids, np.full(N, 5), su.lib["motion_lengths"][mids].astype(F), seed=30)
    o64 = to.post_step(su.lib, cfg, st, np.float64)
    assert (o64["reset"] == 1).all() and (o64["terminate"] == 0).all()
    got = tr.run_post(be, su, cfg, st, want_plain=True)
    np.testing.assert_array_equal(got["reset"], o64["reset"])
    np.testing.assert_array_equal(got["terminate"], o64["terminate"])
    rl, rc = got["reset_lists"], got["reset_counts"]
    cap = abi.reset_sublist_cap(N)
    want = np.bincount((np.arange(N) >> 3) % abi.RESET_SUBLISTS, minlength=abi.RESET_SUBLISTS)
    np.testing.assert_array_equal(rc[1], want)
    assert rc[1].sum() == N and rc[1].max() == cap and (rc[1] == cap).sum() == {300: 5, 384: 16}[N] and (rc[0] == 0).all() and (rc[2] == 0).all()
    np.testing.assert_array_equal(np.sort(tr.listed_envs(got)), np.arange(N))
    assert all(((rl[s, :rc[1, s]] >> 3) % abi.RESET_SUBLISTS == s).all() for s in range(abi.RESET_SUBLISTS))


@pytest.mark.gpu
@pytest.mark.parametrize("far_start", [False, True])
def test_reset_instantiations(far_start):
    """The reset launch of the plain-eligible edge cases through the plain and the generic k_im_reset: every written tensor has the same bits; the far
    start (zero_out_far) is not plain and must not change under the switch."""
    be = get_backend("hip")
    su = tr.setup("smpl")
    cfg, mids, env_ids, phase, t, uv = tr.reset_edge_case(far_start)
    opt = dict(offset_rand=uv, cycle_counter=np.full(len(mids), 5, np.int32), point_goal=np.full(len(mids), 9, F)) if far_start else {}
    shipped = tr.run_reset(be, su, cfg, mids, env_ids, phase, want_plain=not far_start, **opt)
    old = be.lib.phc_task_force_generic(1)
    try:
        generic = tr.run_reset(be, su, cfg, mids, env_ids, phase, want_plain=not far_start, **opt)
    finally:
        be.lib.phc_task_force_generic(old)
    for k, v in shipped.items():
        if v is not None:
            np.testing.assert_array_equal(_bits(v), _bits(generic[k]), err_msg=k)
