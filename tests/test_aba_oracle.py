"""The LAGGED stepping scheme (`inertia_lag` 1, the default) against an independent fp64 oracle, oracle/aba_oracle.py: the articulated-body recursion in plain numpy with
6 x 6 world-axes matrices, which states a lagged sub-step as the fresh code path with the kept I^A and D^-1 substituted and forms p^a by the FRESH expression -- not by the
bias-only rearrangement of csrc/phc_aba.h.  Until this file the only numeric reference of the lagged path was that header compiled with float as double.

  1. test_oracle_is_the_dense_scheme                 aba_oracle (inertia_lag 0) == dyn_oracle (dense M^-1 solve) on every row of
                                                     test_dynamics.test_double_precision_build_of_the_recursion_is_the_dense_scheme, with and without body-body contact:
                                                     the oracle is checked before anything is checked against it.  CPU, no backend.
  2. test_lagged_result_against_elimination_order    re-rooted and pelvis-rooted SMPL at inertia_lag 1, printed side by side (see FINDING below).
  3. test_double_precision_build_is_the_oracle_*     the fp64 build of the lane code (hostemu_util.host_sim_step(f64=True)) at inertia_lag 1 == the oracle: the options
                                                     rows, substeps 2 / 3 / 4 x 1 / 2 simulate() calls (two and three lagged sub-steps in a row), body-body contact, a
                                                     non-zero external wrench over 1 and 2 simulate() calls, every lagged row of stepper_regimes.  CPU.
  4. test_hip_*                                      the HIP kernel against the oracle DIRECTLY, at check_step_against's tolerances: the options rows, the plain and the
                                                     generic kernel, phc_sim_step_wrench with a non-zero wrench (SMPL and the H1 WRENCH_TIGHT twin), phc_sim_step_dr, the
                                                     per-env-shapes instantiation, substeps 3 and 4 on SMPL and G1.  gpu.
The constructed states for the decisions only a lagged sub-step takes are in tests/test_lag_regimes.py.

BOUND of 1 and 3: the fresh pair's -- check_step_against(scale=1e-5) and a worst body-state difference below 1e-9.  No row needed more.  Observed worst body-state
difference, fp64 build against the oracle at inertia_lag 1:
  options rows         smpl 0.95 2.0e-14, smpl 0.80 1.8e-13, smpl aniso 7.9e-14, smpl 3.0 1.9e-14, h1 `pd` 5.3e-12, g1 3.9e-13, smpl pelvis-rooted 1.3e-13
  substeps x calls     smpl 2.0e-14 .. 1.5e-13, h1 4.0e-13 .. 4.8e-12, g1 6.4e-14 .. 1.7e-13
  body-body contact    smpl 1.2e-13, h1 4.0e-12, g1 1.1e-13
  external wrench      smpl 1.1e-13 / 9.9e-14, h1 3.9e-12 / 4.0e-12 (over 1 / 2 simulate() calls)
  stepper_regimes      7.8e-16 .. 3.1e-13 over the seventeen lagged rows (the largest: cap100-smpl)
  the oracle against the dense oracle (inertia_lag 0): 3.6e-15 .. 5.9e-12 (the largest: h1 `pd` at 0.80)
Every row is at the yardstick of the same states through both at inertia_lag 0 (1e-14 .. 7e-12): rounding of fp64.

MUTATIONS of csrc/phc_aba.h (scratch copy, CPU): `t` -> 0.9 t and 0.5 t in the bias-only level-step fail every one of the 49 rows of 3 and every row of
test_lag_regimes.test_double_precision_build_is_the_oracle; `touching &= L.c_touch` disabled fails the arrive and deep rows there and test_arriving_foot_carries_no_force;
a late limit that always gets its damper fails the limits rows there.

FINDING (2): DESIGN 4.1 says the lagged result "depends on the elimination order".  It does: re-rooted at Spine and rooted at the pelvis the oracle's results agree to
1e-13 at inertia_lag 0 and differ by 3e-2 m/s in the body velocities at inertia_lag 1, where lagged and fresh differ by 1.4 m/s -- at the order of the lag error, as DESIGN
says.  (The kept I^A of a body holds its solver children's I^a shifted by the old levers; which bodies are children depends on the base.)  DESIGN stands; the oracle walks
the stepper's own solver tree."""
import numpy as np
import pytest

import aba_oracle as ao
import dyn_oracle as do
import hostemu_util as hu
import stepper_edge_cases as ec
import stepper_regimes as sr
from backends import get_backend, model_on
from phc_amd import abi
from test_dynamics import check_step_against, dense_scheme_row, run_step
from test_stepper_options import OPTIONS_ROWS, options_row

F = np.float32
KEYS = ("root", "dof", "rbs", "df", "cf")
DENSE_ROWS = [("smpl_humanoid", 0, h, a, r) for h, a, r in [(0.95, False, True), (0.80, False, True), (0.80, True, True), (0.80, False, False), (3.0, False, True)]] + \
             [(robot, mode, h, False, True) for robot, mode in (("h1_humanoid", 0), ("h1_humanoid", 1), ("g1_humanoid", 2)) for h in (0.95, 0.80, 3.0)]


def oracle_params(prm):
    """What the oracle computes with: exactly the numbers the C struct holds, body-body forces in the stepper's fixed point (stepper_regimes.dense)."""
    dp, sim_dt, substeps = sr.dense_params(prm)
    dp["self_force_fixed_point"] = sr.FIXED_POINT
    return dp, sim_dt, substeps


def oracle_step(model, prm, root, dof, target, num_sim_calls=2, lag=None, **kw):
    """aba_oracle.sim_step on every env -> {tensor: [n, ...]}."""
    dp, sim_dt, substeps = oracle_params(prm)
    lag = int(prm.inertia_lag) if lag is None else lag
    per = lambda x, e: None if x is None else x[e]
    outs = [ao.sim_step(model, root[e], dof[e], target[e], dp, sim_dt, substeps, num_sim_calls, inertia_lag=lag, force=per(kw.get("force"), e), torque=per(kw.get("torque"), e),
                        wrench_sim_calls=kw.get("wrench_sim_calls")) for e in range(root.shape[0])]
    return {k: np.stack([o[i] for o in outs]) for i, k in enumerate(KEYS)}


def assert_equal_fp64(model, got, ref, tag):
    """The fresh pair's bound: check_step_against at scale 1e-5 and body states within 1e-9.  Prints the worst body-state difference."""
    worst = float(np.abs(np.asarray(got["rbs"]) - ref["rbs"]).max())
    print(f"{tag}: worst body-state difference {worst:.2e}")
    for e in range(ref["root"].shape[0]):
        check_step_against(model, {k: got[k][e] for k in KEYS}, ref["root"][e], ref["dof"][e], ref["rbs"][e], ref["df"][e], ref["cf"][e], f"{tag} env {e}", scale=1e-5)
    assert worst < 1e-9, (tag, worst)
    return worst


def assert_close_fp32(model, out, ref, tag):
    for e in range(ref["root"].shape[0]):
        ratios = sr.error_ratios(model, {k: out[k][e] for k in KEYS}, {k: ref[k][e] for k in KEYS})
        print(f"{tag} env {e}: error / tolerance " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
        check_step_against(model, {k: out[k][e] for k in KEYS}, ref["root"][e], ref["dof"][e], ref["rbs"][e], ref["df"][e], ref["cf"][e], f"{tag} env {e}")


# ---- 1, 2: the oracle itself ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_collision", [0, 1])
@pytest.mark.parametrize("robot,control_mode,height,anisotropic,reroot", DENSE_ROWS)
def test_oracle_is_the_dense_scheme(robot, control_mode, height, anisotropic, reroot, self_collision):
    model, root, dof, target, prm = dense_scheme_row(robot, control_mode, height, anisotropic, reroot, self_collision=self_collision)
    dp, sim_dt, substeps = oracle_params(prm)
    got = oracle_step(model, prm, root, dof, target, 2, lag=0)
    outs = [do.sim_step(model, root[e], dof[e], target[e], params=dp, sim_dt=sim_dt, substeps=substeps, num_sim_calls=2) for e in range(root.shape[0])]
    ref = {k: np.stack([o[i] for o in outs]) for i, k in enumerate(KEYS)}
    assert_equal_fp64(model, got, ref, f"{robot} mode {control_mode} height {height} aniso {anisotropic} reroot {reroot} self_collision {self_collision}: recursion oracle vs dense oracle")
    if height < 0.9:
        assert np.abs(ref["cf"]).sum() > 0, "the low rows must exercise contact"


def test_trace_changes_no_number():
    model, root, dof, target, prm = dense_scheme_row("h1_humanoid", 1, 0.80, False, True, limit_stiffness=2000.0, limit_damping=20.0)
    dp, sim_dt, substeps = oracle_params(prm)
    tr = {}
    a = ao.sim_step(model, root[0], dof[0], target[0], dp, sim_dt, substeps, 2, inertia_lag=1)
    b = ao.sim_step(model, root[0], dof[0], target[0], dp, sim_dt, substeps, 2, inertia_lag=1, trace=tr)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert [s["lagged"] for s in tr["substeps"]] == [False, True, False, True] and tr["substeps"][0]["contacts"] and tr["substeps"][0]["limits"]


@pytest.mark.parametrize("self_collision", [0, 1])
def test_lagged_result_against_elimination_order(self_collision):
    """DESIGN 4.1 says that the lagged result depends on the elimination order.  Re-rooted (base Spine) and pelvis-rooted SMPL through the oracle, side by side: equal to
    rounding at inertia_lag 0, and at inertia_lag 1 apart by far more than rounding (FINDING in the module docstring) -- DESIGN's statement holds, and a reference of the
    lagged scheme has to walk the stepper's own solver tree, as aba_oracle does (model.solver_tree())."""
    lagged, fresh = [], []
    for reroot in (True, False):
        model, root, dof, target, prm = dense_scheme_row("smpl_humanoid", 0, 0.80, False, reroot, self_collision=self_collision, inertia_lag=1)
        lagged.append(oracle_step(model, prm, root, dof, target, 2))
        fresh.append(oracle_step(model, prm, root, dof, target, 2, lag=0))
        print(f"reroot {reroot}: base {int(model.solver_tree()['base'])}, lagged root velocities of env 0 {lagged[-1]['root'][0, 7:13]}, lagged vs fresh body velocities "
              f"{np.abs(lagged[-1]['rbs'][:, :, 7:13] - fresh[-1]['rbs'][:, :, 7:13]).max():.2e}")
    vel = lambda o: o["rbs"][:, :, 7:13]
    d_fresh, d_lag = np.abs(vel(fresh[0]) - vel(fresh[1])).max(), np.abs(vel(lagged[0]) - vel(lagged[1])).max()
    print(f"self_collision {self_collision}: body velocities, re-rooted vs pelvis-rooted: fresh {d_fresh:.2e}, lagged {d_lag:.2e}")
    assert np.abs(lagged[0]["cf"]).sum() > 0
    assert d_fresh < 1e-9
    assert d_lag > 1e-6, "the lagged results of the two elimination orders agree: DESIGN 4.1 says they do not"


# ---- 3: the fp64 build of the lane code against the oracle -----------------------------------------------------------------------------------------------------------
def _options_model(robot, anisotropic, reroot=True):
    return model_on(get_backend("hostemu"), name=robot, anisotropic=anisotropic, reroot=reroot)[0]


@pytest.mark.parametrize("robot,control_mode,height,anisotropic,reroot", [r + (True,) for r in OPTIONS_ROWS] + [("smpl_humanoid", 0, 0.80, False, False)])
def test_double_precision_build_is_the_oracle_on_the_options_rows(robot, control_mode, height, anisotropic, reroot):
    model = _options_model(robot, anisotropic, reroot)
    root, dof, target, prm = options_row(model, 1, control_mode, height)
    got = hu.host_sim_step(model, prm, root, dof, target, 2, f64=True)
    assert_equal_fp64(model, got, oracle_step(model, prm, root, dof, target, 2), f"{robot} mode {control_mode} height {height} aniso {anisotropic} reroot {reroot} lag 1: fp64 build vs oracle")


THREE = [("smpl_humanoid", 0, 0.80), ("h1_humanoid", 1, 0.85), ("g1_humanoid", 2, 0.70)]


@pytest.mark.parametrize("num_sim_calls", [1, 2])
@pytest.mark.parametrize("substeps", [2, 3, 4])
@pytest.mark.parametrize("robot,control_mode,height", THREE)
def test_double_precision_build_is_the_oracle_over_lagged_sub_steps_in_a_row(robot, control_mode, height, substeps, num_sim_calls):
    model = _options_model(robot, False)
    root, dof, target, prm = options_row(model, 1, control_mode, height, n=3, substeps=substeps)
    got = hu.host_sim_step(model, prm, root, dof, target, num_sim_calls, f64=True)
    assert_equal_fp64(model, got, oracle_step(model, prm, root, dof, target, num_sim_calls), f"{robot} substeps {substeps} x {num_sim_calls} calls lag 1: fp64 build vs oracle")


@pytest.mark.parametrize("robot,control_mode,height", THREE)
def test_double_precision_build_is_the_oracle_with_body_body_contact(robot, control_mode, height):
    model = _options_model(robot, False)
    root, dof, target, prm = options_row(model, 1, control_mode, height, n=3, self_collision=1)
    got = hu.host_sim_step(model, prm, root, dof, target, 2, f64=True)
    assert_equal_fp64(model, got, oracle_step(model, prm, root, dof, target, 2), f"{robot} self_collision 1 lag 1: fp64 build vs oracle")


def wrench_of(model, n):
    """A non-zero wrench per env: a force on every body (a fifth of its weight, sideways and up), a push on the root body, a torque on the torso."""
    names = list(model.body_names)
    torso = names.index("Torso" if "Torso" in names else "torso_link")
    force = np.zeros((n, model.num_bodies, 3))
    torque = np.zeros((n, model.num_bodies, 3))
    for e in range(n):
        force[e] = model.mass[:, None] * np.array([1.0 + 0.3 * e, -0.7, 2.0])
        force[e, 0] += (60.0 + 10.0 * e, -40.0, 15.0)
        torque[e, torso] = (8.0, -6.0 + 2.0 * e, 12.0)
    return force.astype(F), torque.astype(F)


@pytest.mark.parametrize("wrench_sim_calls", [1, 2])
@pytest.mark.parametrize("robot,control_mode,height", THREE[:2])
def test_double_precision_build_is_the_oracle_under_an_external_wrench(robot, control_mode, height, wrench_sim_calls):
    model = _options_model(robot, False)
    root, dof, target, prm = options_row(model, 1, control_mode, height, n=3)
    force, torque = wrench_of(model, 3)
    got = hu.host_sim_step(model, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=wrench_sim_calls)
    ref = oracle_step(model, prm, root, dof, target, 2, force=force.astype(np.float64), torque=torque.astype(np.float64), wrench_sim_calls=wrench_sim_calls)
    assert_equal_fp64(model, got, ref, f"{robot} wrench over {wrench_sim_calls} of 2 calls lag 1: fp64 build vs oracle")
    none = oracle_step(model, prm, root, dof, target, 2)
    assert np.abs(ref["rbs"][:, :, 7:13] - none["rbs"][:, :, 7:13]).max() > 1e-2, "the wrench must move the bodies"


@pytest.mark.parametrize("rid", [rid for rid, lag in sr.ROWS if lag == 1])
def test_double_precision_build_is_the_oracle_on_the_regime_rows(rid):
    """Every lagged row of stepper_regimes: its reference sr.reference(reg, 1) -- what the backends of test_stepper_regimes are compared with -- against the oracle."""
    reg = sr.REGIMES[rid]
    m, s = sr.model_of(reg), sr.states(reg)
    ref = oracle_step(m, sr.params_of(reg, 1), s["root"], s["dof"], sr.formed_target(reg, s), 2)
    assert_equal_fp64(m, sr.reference(reg, 1), ref, f"{rid} lag 1: fp64 build vs oracle")


# ---- 4: the HIP kernel against the oracle directly ---------------------------------------------------------------------------------------------------------------------
def _hip():
    return get_backend("hip")


@pytest.mark.gpu
@pytest.mark.parametrize("robot,control_mode,height,anisotropic", OPTIONS_ROWS)
def test_hip_kernel_is_the_oracle_on_the_options_rows(robot, control_mode, height, anisotropic):
    be = _hip()
    model, mstruct, keep = model_on(be, name=robot, anisotropic=anisotropic)
    root, dof, target, prm = options_row(model, 1, control_mode, height)
    out = run_step(be, model, mstruct, root, dof, target, prm, 2)
    assert_close_fp32(model, out, oracle_step(model, prm, root, dof, target, 2), f"{robot} height {height} aniso {anisotropic} lag 1 on hip vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("height", [0.95, 0.80, 3.0])
def test_hip_plain_and_generic_kernels_are_the_oracle(height):
    """The plain-eligible SMPL rows (scalar gains, with body-body contact on as phc_sim_is_plain asks) launched through actions and a freeze mask: the plain kernel (its unrolled sub-step pair) and, under
    phc_sim_force_generic(1), the generic one, each against the oracle with the target the launch forms."""
    be = _hip()
    model, mstruct, keep = model_on(be)
    root, dof, target, prm = options_row(model, 1, 0, height, self_collision=1)   # (the plain launch is the default task's: body-body contact on)
    n, nb, nd = root.shape[0], model.num_bodies, model.num_dof
    rng = np.random.default_rng(23)
    scale, off = rng.uniform(0.5, 1.5, nd).astype(F), rng.normal(0, 0.1, nd).astype(F)
    act = ((target - off[None]) / scale[None]).astype(F)
    formed = (off[None] + (scale[None] * act).astype(F)).astype(F)
    ref = oracle_step(model, prm, root, dof, formed, 2)
    for generic in (0, 1):
        a = dict(root=be.arr(root), dof=be.arr(dof), rbs=be.zeros((n, nb, 13)), cf=be.zeros((n, nb, 3)), df=be.zeros((n, nd)), pd=be.zeros((n, nd)))
        sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"])
        args = (be.arr(act), be.arr(off), be.arr(scale), be.arr(np.zeros(nd, np.int32)))
        assert be.lib.phc_sim_is_plain(mstruct, prm, sim, abi.ptr(args[0]), abi.ptr(args[3]), 2), "a default SMPL launch with actions and a freeze mask must be plain"
        old = be.lib.phc_sim_force_generic(generic)
        try:
            assert be.sim_step(mstruct, prm, sim, *args, 2) == 0
            be.sync()
        finally:
            be.lib.phc_sim_force_generic(old)
        out = {k: be.np(v) for k, v in a.items()}
        assert np.array_equal(out["pd"].view(np.uint32), formed.view(np.uint32))
        assert_close_fp32(model, out, ref, f"smpl height {height} lag 1, {'generic' if generic else 'plain'} kernel vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("robot,control_mode,height", THREE[:2])
def test_hip_wrench_kernel_is_the_oracle(robot, control_mode, height):
    be = _hip()
    model, mstruct, keep = model_on(be, name=robot)
    root, dof, target, prm = options_row(model, 1, control_mode, height)
    n, nb, nd = root.shape[0], model.num_bodies, model.num_dof
    force, torque = wrench_of(model, n)
    a = dict(root=be.arr(root), dof=be.arr(dof), rbs=be.zeros((n, nb, 13)), cf=be.zeros((n, nb, 3)), df=be.zeros((n, nd)), pd=be.arr(target))
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"])
    fo, to = be.arr(force), be.arr(torque)
    assert be.sim_step(mstruct, prm, sim, None, None, None, None, 2, force=fo, torque=to, wrench_sim_calls=1) == 0
    be.sync()
    ref = oracle_step(model, prm, root, dof, target, 2, force=force.astype(np.float64), torque=torque.astype(np.float64), wrench_sim_calls=1)
    assert_close_fp32(model, {k: be.np(v) for k, v in a.items()}, ref, f"{robot} lag 1 wrench on hip vs oracle")


@pytest.mark.gpu
def test_hip_dr_kernel_is_the_oracle():
    import dr_util as du
    model = _options_model("h1_humanoid", False)
    root, dof, target, prm = options_row(model, 1, 1, 0.85)
    out = du.hip_step_dr([model], None, prm, root, dof, target, 2, friction=np.full(root.shape[0], float(prm.friction), F))
    assert_close_fp32(model, out, oracle_step(model, prm, root, dof, target, 2), "h1 lag 1 dr (per-env friction = the global value) on hip vs oracle")


@pytest.mark.gpu
def test_hip_per_env_shapes_kernel_is_the_oracle():
    be = _hip()
    case = ec.CASES["smpl-shapes-lag"]
    models = ec.models_on(be, case)[0]
    s = ec.states_of(case)
    rows = list(range(ec.NUM_STATES))
    rc, out, wrong = ec.launch(be, case, rows)
    assert rc == 0 and not wrong, (rc, wrong)
    prm = ec.params_of(case, models)
    for e in rows:
        m = models[int(s["env_shape"][e])]
        ref = oracle_step(m, prm, s["root"][e:e + 1], s["dof"][e:e + 1], s["target"][e:e + 1], 2)
        assert_close_fp32(m, {k: out[k][e:e + 1] for k in KEYS}, ref, f"smpl shape {int(s['env_shape'][e])} env {e} lag 1 on hip vs oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("substeps", [3, 4])
@pytest.mark.parametrize("robot,control_mode,height", [THREE[0], THREE[2]])
def test_hip_kernel_is_the_oracle_over_lagged_sub_steps_in_a_row(robot, control_mode, height, substeps):
    be = _hip()
    model, mstruct, keep = model_on(be, name=robot)
    root, dof, target, prm = options_row(model, 1, control_mode, height, substeps=substeps)
    out = run_step(be, model, mstruct, root, dof, target, prm, 2)
    assert_close_fp32(model, out, oracle_step(model, prm, root, dof, target, 2), f"{robot} substeps {substeps} lag 1 on hip vs oracle")
