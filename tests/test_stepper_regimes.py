"""The stepper on constructed states in every solver branch regime: rate cap, exp-map edges, effort clamp, pd_ref clamp, rigid contact (bounce, depenetration cap,
speculative, out of range), body gate, friction cone, capsule closest-point regimes.  Cases, constructors, margins, references: tests/stepper_regimes.py (its docstring
holds the margin table and the branch left out); both backends of tests/backends.py.

Per case:
  1. test_regime_is_reached_with_its_margin              the witness of the fp64 oracle (dyn_oracle.sim_step(trace=...)): the branch was taken, with its margin.  CPU.
  2. test_double_precision_recursion_is_the_dense_scheme  the fp64 build of the recursion == the dense oracle on the case at scale 1e-5: the reference implements the regime.  CPU.
  3. test_backend_equals_the_double_precision_recursion   fp32 host emulation / HIP kernel == the fp64 recursion at check_step_against's tolerances (stepper_regimes.WIDER:
                                                          the rows measured wider); on the device the rows phc_sim_is_plain accepts run through the plain kernel and,
                                                          under phc_sim_force_generic(1), the generic one.
  4. test_regime_state_beside_benign_states               the regime state in env 0, 1 and 2 of N = 3 beside benign states: every row bit-equal to its single-env launch.
  5. test_wrench_instantiation / test_dr_instantiation    rows through phc_sim_step_wrench (all-zero wrench) and phc_sim_step_dr (per-env friction = the global value).
  6. test_point_outside_the_contact_offset_carries_no_force   sub-step 0 of the speculative cases alone: the foot 3 cm above the plane gets exactly no force."""
import numpy as np
import pytest

import stepper_edge_cases as ec
import stepper_regimes as sr
from backends import get_backend
from test_dynamics import check_step_against, run_step

F = np.float32
KEYS = ("root", "dof", "rbs", "df", "cf")


def _rows(rows, cpu=True):
    """(backend, id, lag) for both backends; pd_ref rows on the device only (the host emulation has no res_action path)."""
    out = []
    for rid, lag in rows:
        if cpu and not sr.REGIMES[rid].hip_only:
            out.append(("hostemu", rid, lag))
        out.append(pytest.param("hip", rid, lag, marks=pytest.mark.gpu))
    return out


@pytest.mark.parametrize("rid", list(sr.REGIMES))
def test_regime_is_reached_with_its_margin(rid):
    """A condition on the inputs, decided by the fp64 oracle alone (no backend runs here): the case's states reach the regime the table names, by the table's margin."""
    reg = sr.REGIMES[rid]
    print(f"{rid}: {reg.what}")
    assert sr.witness(reg), "a witness states what it found"


@pytest.mark.parametrize("rid", list(sr.REGIMES))
def test_double_precision_recursion_is_the_dense_scheme(rid):
    """oracle/hostemu/hostemu64.cpp against oracle/dyn_oracle.py on the case's states (inertia_lag 0: the lagged scheme has no dense form), as
    test_dynamics.test_double_precision_build_of_the_recursion_is_the_dense_scheme: check_step_against at scale 1e-5.  The reference of every other test here
    implements the regime."""
    reg = sr.REGIMES[rid]
    m, s = sr.model_of(reg), sr.states(reg)
    outs, _ = sr.dense(reg)
    ref = sr.reference(reg, 0)
    for e, (r, d, rbs, tau, fc) in enumerate(outs):
        got = {k: ref[k][e] for k in KEYS}
        worst = max(sr.error_ratios(m, got, dict(root=r, dof=d, rbs=rbs, df=tau, cf=fc)).values())
        print(f"{rid} state {e}: fp64 recursion vs dense oracle, worst error / check_step_against's tolerance {worst:.2e} (bound 1e-5)")
        check_step_against(m, got, r, d, rbs, tau, fc, f"{rid} state {e}", scale=1e-5)
    assert s["root"].shape[0] == len(outs) <= 3


def _compare(reg, lag, out, ref, tag):
    m = sr.model_of(reg)
    for e in range(out["root"].shape[0]):
        sr.assert_close(m, out, ref, e, tag, sr.wider(reg.id, lag))
    if reg.make == "expmap":   # the stored exp-map is the shortest arc
        for name, x in (("backend", out["dof"]), ("fp64 recursion", ref["dof"])):
            ang = np.linalg.norm(np.asarray(x, np.float64)[:, :, 0].reshape(x.shape[0], -1, 3), axis=-1)
            print(f"{tag}: largest stored |e| ({name}) pi - {np.pi - ang.max():.3e}")
            assert ang.max() <= np.pi + 1e-5
        # The rotation comparison of check_step_against cannot see a joint this close to the identity (1 - |<qa, qb>| of two rotations 1e-5 rad apart is 1e-11), so a
        # wrong small-angle branch would pass it: the stored exp-maps of the tiny joints are compared themselves.  Bound 1 % of |e|: a wrong series coefficient is off
        # by tens of per cent; the series' truncation is 1e-11 of |e|, fp32 rounding of a quaternion component 1e-7, and the rounding of the rates (1e-7 rad/s over 33 ms
        # against |e| >= 1e-5) 1e-3.
        for key in ("series_lo", "series_hi", "near_identity"):
            d = sr.dofs_of(m, sr.EXPMAP[key][0])
            got, want = np.asarray(out["dof"], np.float64)[0, d, 0], np.asarray(ref["dof"], np.float64)[0, d, 0]
            rel = np.linalg.norm(got - want) / np.linalg.norm(want)
            print(f"{tag}: {sr.EXPMAP[key][0]} stored |e| {np.linalg.norm(want):.3e}, relative difference {rel:.2e}")
            assert rel <= 1e-2


@pytest.mark.parametrize("backend,rid,lag", _rows(sr.ROWS))
def test_backend_equals_the_double_precision_recursion(backend, rid, lag):
    reg, be = sr.REGIMES[rid], get_backend(backend)
    s = sr.states(reg)
    rows = list(range(s["root"].shape[0]))
    plain = backend == "hip" and reg.actions == "" and sr.is_plain(be, reg, lag)
    if backend == "hip" and reg.model == "smpl_humanoid" and lag == 1 and reg.actions == "" and not dict(reg.opts).get("lane_mapping"):
        assert plain, "a default SMPL launch with actions and a freeze mask must satisfy phc_sim_is_plain"
    if plain:
        d = sr.launch_states(reg, s, through_actions=True)
        target = sr.action_target(d)
        ref = sr.reference(reg, lag, target=target)
        for generic in (0, 1):
            old = be.lib.phc_sim_force_generic(generic)
            try:
                out = sr.launch(be, reg, lag, s, rows, through_actions=True)
            finally:
                be.lib.phc_sim_force_generic(old)
            assert np.array_equal(out["pd"].view(np.uint32), target.view(np.uint32)), "pd_target is not float32(offset + float32(scale * action))"
            _compare(reg, lag, out, ref, f"{rid} lag {lag} on hip, {'generic' if generic else 'plain'} kernel")
        return
    out = sr.launch(be, reg, lag, s, rows)
    assert np.array_equal(out["pd"].view(np.uint32), sr.formed_target(reg, s).view(np.uint32)), "pd_target is not what the formula gives"
    _compare(reg, lag, out, sr.reference(reg, lag), f"{rid} lag {lag} on {backend}")


@pytest.mark.parametrize("backend,rid,lag", _rows(sr.ROWS))
def test_regime_state_beside_benign_states(backend, rid, lag):
    """Each regime state in env 0, env 1 and the last env of N = 3 beside two benign states of stepper_edge_cases.states_of, under the case's parameters: the benign rows
    are bit for bit their single-env launches and the regime row its own -- a saturating or capped lane leaks nothing into the env that shares its wavefront."""
    reg, be = sr.REGIMES[rid], get_backend(backend)
    keys = ec.outputs_of(sr.case_of(reg, lag))
    lines = []
    for e in range(sr.states(reg)["root"].shape[0]):
        s = sr.beside_benign(reg, e)
        alone = [sr.launch(be, reg, lag, s, [i]) for i in range(3)]
        for i, a in enumerate(alone):
            for t in keys:
                assert np.isfinite(a[t]).all(), f"{rid} state {e}: {t} of row {i} alone is not finite"
        for rows in ([0, 1, 2], [1, 0, 2], [1, 2, 0]):
            out = sr.launch(be, reg, lag, s, rows)
            lines += ec.mismatches(out, ec.stack_refs(alone, rows), keys, f"state {e} in env {rows.index(0)}:")
    assert not lines, f"{rid} lag {lag} on {backend}: {len(lines)} problems\n" + "\n".join(lines[:40])


WRENCH_ROWS = [("effort-smpl", 1), ("cap8-smpl", 1), ("effort-h1-m1", 1)]


@pytest.mark.parametrize("backend,rid,lag", _rows(WRENCH_ROWS))
def test_wrench_instantiation(backend, rid, lag):
    """phc_sim_step_wrench with non-null all-zero force and torque tensors -- the WRENCH twin of the kernel header -- against the fp64 build of the same entry point."""
    reg, be = sr.REGIMES[rid], get_backend(backend)
    s = sr.states(reg)
    out = sr.launch(be, reg, lag, s, list(range(s["root"].shape[0])), wrench=True)
    _compare(reg, lag, out, sr.reference(reg, lag, wrench=True), f"{rid} lag {lag} wrench on {backend}")


@pytest.mark.gpu
@pytest.mark.parametrize("rid,lag", [("pen-friction-h1", 1)])
def test_dr_instantiation(rid, lag):
    """phc_sim_step_dr with per-env friction equal to the global value -- the DR twin of the kernel header -- against the fp64 recursion."""
    import dr_util as du
    reg = sr.REGIMES[rid]
    s, prm = sr.states(reg), sr.params_of(reg, lag)
    n = s["root"].shape[0]
    out = du.hip_step_dr([sr.model_of(reg)], None, prm, s["root"], s["dof"], s["target"], 2, friction=np.full(n, float(prm.friction), F))
    _compare(reg, lag, out, sr.reference(reg, lag), f"{rid} lag {lag} dr on hip")


@pytest.mark.parametrize("backend,rid,lag", _rows([("rigid-spec-smpl", 0), ("rigid-spec-h1", 0)]))
def test_point_outside_the_contact_offset_carries_no_force(backend, rid, lag):
    """Sub-step 0 of the speculative case alone (one simulate call of one sub-step of the same length): the foot 1 cm above the plane is pushed, the foot 3 cm above it --
    outside contact_offset by the witness -- gets exactly no force, on the backend and in the fp64 recursion."""
    import hostemu_util as hu
    reg, be = sr.REGIMES[rid], get_backend(backend)
    m, s = sr.model_of(reg), sr.states(reg)
    full = sr.params_of(reg, lag)
    prm = sr.params_of(reg, lag, substeps=1, sim_dt=float(full.sim_dt) / int(full.substeps))
    out = run_step(be, m, sr.models_on(be, reg)[1], s["root"], s["dof"], s["target"], prm, 1)
    ref = hu.host_sim_step(m, prm, s["root"], s["dof"], s["target"], 1, f64=True)
    names = list(m.body_names)
    left, right = ([names.index(b) for b in sr.FEET[sr.smpl(m)][side]] for side in ("L", "R"))
    for name, cf in (("backend", out["cf"]), ("fp64 recursion", ref["cf"])):
        print(f"{rid} on {backend}, {name}: left foot F_z {cf[0, left, 2]}, right foot F {cf[0, right]}")
        assert (cf[0, right] == 0).all() and cf[0, left, 2].sum() > 10.0
    sr.assert_close(m, out, ref, 0, f"{rid} sub-step 0 on {backend}")
