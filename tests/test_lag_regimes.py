"""The stepper on constructed states in the regimes only the LAGGED scheme (`inertia_lag` 1, the default) has: a ground point that arrives, leaves or changes its
friction regime between two fresh sub-steps, a joint limit held, engaging late or released there, three lagged sub-steps in a row.  Cases, constructors, margins and
witnesses: tests/lag_regimes.py.  The reference is oracle/aba_oracle.py -- the recursion in plain numpy, which shares no expression with csrc/phc_aba.h.

Per case:
  1. test_lag_regime_is_reached_with_its_margin         the witness of the oracle's trace: the regime was reached, with its margin.  CPU, no backend.
  2. test_double_precision_build_is_the_oracle          the fp64 build of the lane code == the oracle at the fresh pair's bound (check_step_against at scale 1e-5, body
                                                        states within 1e-9).  CPU.
  3. test_backend_is_the_oracle                         fp32 host emulation / HIP kernel == the oracle at check_step_against's tolerances (lag_regimes.WIDER: no row needs more).
  4. test_lag_regime_state_beside_benign_states         the regime state in env 0, 1 and 2 of N = 3 beside benign states: every row bit-equal to its single-env launch.
  5. test_arriving_foot_carries_no_force                "arrive" through ONE simulate() call (fresh, lagged): the foot that arrived in the lagged sub-step has contact_force
                                                        exactly zero, on the backend, in the fp64 build and in the oracle.

  6. test_released_limit_keeps_its_implicit_share       the limit cases through ONE simulate() call, so that dof_force publishes the lagged sub-step: a limit that has
                                                        released keeps its implicit share in the kept D^-1, and S5 says so (the departure of phc_aba.h these cases found).

Observed, fp64 build against the oracle (worst body-state difference; dof_force agrees to 2e-12 N m, contact_force to 5e-11 N):
  arrive-smpl 2.4e-14, arrive-h1 1.6e-13, leave-smpl 2.8e-15, leave-h1 4.9e-14, slip-smpl 1.1e-14, slip-h1 1.7e-13, limits-h1 3.6e-15, limits-g1 1.6e-15,
  deep-smpl 2.6e-14, deep-h1 1.0e-13; limits through one simulate() call: h1 8.0e-15, g1 2.2e-15
Observed, fp32 host emulation against the oracle: every quantity of every row below 0.05 of check_step_against's tolerance; no row takes a wider bound (lag_regimes.WIDER
is empty).  The HIP kernel meets the same tolerance on every row."""
import numpy as np
import pytest

import hostemu_util as hu
import lag_regimes as lr
import stepper_edge_cases as ec
import stepper_regimes as sr
from backends import get_backend
from test_aba_oracle import KEYS, assert_equal_fp64
from test_dynamics import run_step

F = np.float32


def _rows(rows):
    return [("hostemu", rid, lag) for rid, lag in rows] + [pytest.param("hip", rid, lag, marks=pytest.mark.gpu) for rid, lag in rows]


@pytest.mark.parametrize("rid", list(lr.REGIMES))
def test_lag_regime_is_reached_with_its_margin(rid):
    """A condition on the inputs, decided by the oracle's trace alone: the case's states reach the regime the table names, by the table's margin."""
    reg = lr.REGIMES[rid]
    print(f"{rid}: {reg.what}")
    assert lr.witness(reg), "a witness states what it found"


@pytest.mark.parametrize("rid", list(lr.REGIMES))
def test_double_precision_build_is_the_oracle(rid):
    reg = lr.REGIMES[rid]
    m, s = sr.model_of(reg), sr.states(reg)
    got = hu.host_sim_step(m, sr.params_of(reg, 1), s["root"], s["dof"], s["target"], 2, f64=True)
    ref, _ = lr.oracle(reg)
    print(f"{rid}: worst dof_force difference {np.abs(got['df'] - ref['df']).max():.2e}, contact_force {np.abs(got['cf'] - ref['cf']).max():.2e}")
    assert_equal_fp64(m, got, ref, f"{rid} lag 1: fp64 build vs oracle")


@pytest.mark.parametrize("backend,rid,lag", _rows(lr.ROWS))
def test_backend_is_the_oracle(backend, rid, lag):
    reg, be = lr.REGIMES[rid], get_backend(backend)
    s = sr.states(reg)
    out = sr.launch(be, reg, lag, s, list(range(s["root"].shape[0])))
    ref, _ = lr.oracle(reg)
    m = sr.model_of(reg)
    w = lr.WIDER.get((rid, lag))
    for e in range(s["root"].shape[0]):
        sr.assert_close(m, out, ref, e, f"{rid} lag {lag} on {backend} vs oracle", None if w is None else {k: (v, max(1.0, 4.0 * v)) for k, v in w.items()})


@pytest.mark.parametrize("backend,rid,lag", _rows(lr.ROWS))
def test_lag_regime_state_beside_benign_states(backend, rid, lag):
    """As test_stepper_regimes.test_regime_state_beside_benign_states: the regime state in env 0, env 1 and the last env of N = 3 beside two benign states, under the
    case's parameters -- every row bit for bit its single-env launch."""
    reg, be = lr.REGIMES[rid], get_backend(backend)
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


@pytest.mark.parametrize("backend,rid,lag", _rows([("arrive-smpl", 1), ("arrive-h1", 1)]))
def test_arriving_foot_carries_no_force(backend, rid, lag):
    """One simulate() call of the arrive case: sub-step 0 fresh (the left foot above the plane), sub-step 1 lagged (it penetrates by the witness's margin and would push).
    contact_force publishes the last sub-step: exactly zero on the bodies of the silent foot, the other foot carries the body."""
    reg, be = lr.REGIMES[rid], get_backend(backend)
    m, s = sr.model_of(reg), sr.states(reg)
    prm = sr.params_of(reg, lag)
    _, traces = lr.oracle(reg)
    sub = traces[0][1]
    assert sub["lagged"] and any(c["depth"] >= 0.001 and c["fn0"] > 0 and not c["pushed"] for c in lr._points(reg, sub, "L"))
    out = run_step(be, m, sr.models_on(be, reg)[1], s["root"], s["dof"], s["target"], prm, 1)
    f64 = hu.host_sim_step(m, prm, s["root"], s["dof"], s["target"], 1, f64=True)
    ref, _ = lr.oracle(reg, num_sim_calls=1)
    names = list(m.body_names)
    left, right = ([names.index(b) for b in sr.FEET[sr.smpl(m)][side]] for side in ("L", "R"))
    for name, cf in ((backend, out["cf"]), ("fp64 build", f64["cf"]), ("oracle", ref["cf"])):
        print(f"{rid}, {name}: left foot F {cf[0, left].tolist()}, right foot F_z {cf[0, right, 2]}")
        assert (cf[0, left] == 0).all() and cf[0, right, 2].sum() > 10.0
    sr.assert_close(m, out, ref, 0, f"{rid} one simulate() call on {backend} vs oracle")


@pytest.mark.parametrize("backend,rid,lag", _rows([("limits-h1", 1), ("limits-g1", 1)]))
def test_released_limit_keeps_its_implicit_share(backend, rid, lag):
    """ONE simulate() call of the limit cases, so that dof_force (S5) publishes the LAGGED sub-step the witness looked at.  A limit that was engaged in the fresh sub-step
    and has released keeps its implicit share dt c + dt^2 k in the kept D^-1: the joint feels tau - (that share) qdd, and S5 has to say so (state 2: -62.7 N m on H1's
    shoulder against -2.0 N m, 0.096 against 0.7 N m on G1's 14-gram link, when the share is left out; the states themselves agree either way).  Backend, fp64 build and
    oracle; held and late states ride along."""
    reg, be = lr.REGIMES[rid], get_backend(backend)
    m, s = sr.model_of(reg), sr.states(reg)
    prm = sr.params_of(reg, lag)
    ref, traces = lr.oracle(reg, num_sim_calls=1)
    body, end = lr.LIMIT_JOINTS[sr.model_kind(m)][2]
    d = sr.dofs_of(m, body)[0]
    last = next(x for x in traces[2][-1]["limits"] if x["dof"] == d)
    assert traces[2][-1]["lagged"] and last["kept"] and last["e"] == 0 and max(last["below"], last["above"]) <= -1e-3, "released in the published sub-step"
    f64 = hu.host_sim_step(m, prm, s["root"], s["dof"], s["target"], 1, f64=True)
    print(f"{rid}: dof_force of {body}: oracle {ref['df'][2, d]:.4f}, fp64 build {f64['df'][2, d]:.4f}")
    assert_equal_fp64(m, f64, ref, f"{rid} one simulate() call: fp64 build vs oracle")
    out = run_step(be, m, sr.models_on(be, reg)[1], s["root"], s["dof"], s["target"], prm, 1)
    for e in range(3):
        sr.assert_close(m, out, ref, e, f"{rid} one simulate() call on {backend} vs oracle")
