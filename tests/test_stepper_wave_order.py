"""GPU: the stepper with wave-scope ordering at its hand-over points (phc_group.h wave_sync; profiles/stepper_wave_order/README.md).

What could go wrong is a hand-over that a lane reads before another lane of the wavefront wrote it: capsule records, the fixed-point ds_add accumulators of body-body
contact, drive terms, the 27- and 6-float level hand-overs, accelerations, kinematics slots, the staged epilogue.  So:

  1. one env step against the double-precision build of the recursion (oracle/hostemu/hostemu64.cpp) at exactly `check_step_against`'s tolerances, at N = 1 (half a
     wavefront idle), N = 2 (two envs in different regimes in ONE wavefront: env 0 with a leg swung into the other one and a foot on the ground, env 1 in the air) and
     N = 3 (a tail wavefront): the plain launch, the same launch through the generic kernel, inertia_lag = 0, H1 (`pd`) and G1 (64 lanes, one env per wavefront; lagged).
     The constructed contacts are asserted to occur (body-body above 50 N, ground above 1 N), so the atomics-then-collect path is not skipped silently;
  2. the same launch twice from the same state: every output tensor bit-equal (plain SMPL at N = 3, G1 at N = 2);
  3. num_sim_calls 1 and 2 at N = 3 (lagged sub-steps behind a fresh one), against the double-precision recursion; the PD targets bit-equal to the formula."""
import numpy as np
import pytest

from backends import get_backend, model_on
from phc_amd import abi
from test_dynamics import check_step_against, random_states

pytestmark = pytest.mark.gpu
F = np.float32
N_MAX = 3


def _smpl_states(model):
    """root [3, 13], dof [3, D, 2], PD-target wishes [3, D]: env 0 low, nearly at rest, the left leg swung into the right one (in the double-precision recursion: ~1 kN
    between the thighs, ~100 N under the right ankle); env 1 in the air; env 2 a low random state at speed."""
    rng = np.random.default_rng(17)
    low = random_states(model, 6, rng, height=0.80)
    air = random_states(model, 1, rng, height=3.0)
    root, dof, target = (np.stack([low[k][1], air[k][0], low[k][2]]) for k in range(3))
    hip = 3 * (model.body_names.index("L_Hip") - 1)
    root[0, 7:13] *= 0.05
    dof[0, :, 1] *= 0.05
    dof[0, :, 0] *= 0.2
    dof[0, hip, 0] = -0.9
    target[0] = dof[0, :, 0]
    return root.astype(F), dof.astype(F), target.astype(F)


@pytest.fixture(scope="module")
def smpl():
    """The default task's launch (actions and a freeze mask given, self-collision on) and its double-precision references, computed once for all sizes: envs are
    independent and every size runs a prefix."""
    import hostemu_util as hu
    be = get_backend("hip")
    model, mstruct, keep = model_on(be)
    root, dof, target = _smpl_states(model)
    nd = model.num_dof
    rng = np.random.default_rng(5)
    off, scale = rng.normal(0, 0.1, nd).astype(F), rng.uniform(0.5, 1.5, nd).astype(F)
    actions = ((target - off) / scale).astype(F)
    freeze = np.zeros(nd, np.int32)
    for nme in ("L_Hand", "R_Hand"):
        i = 3 * (model.body_names.index(nme) - 1)
        freeze[i:i + 3] = 1
    tgt = (off + (scale * actions).astype(F)).astype(F)   # A2: the product rounded on its own, then the sum
    tgt[:, freeze != 0] = 0.0
    prm = {lag: abi.sim_params_struct(inertia_lag=lag, self_collision=1) for lag in (0, 1)}
    ref = {(lag, calls): hu.sim_step_f64(model, prm[lag], root, dof, tgt, calls) for lag, calls in ((1, 2), (0, 2), (1, 1))}
    return dict(be=be, model=model, mstruct=mstruct, keep=keep, root=root, dof=dof, off=off, scale=scale, actions=actions, freeze=freeze, tgt=tgt, prm=prm, ref=ref)


def _launch(sc, n, generic=False, lag=1, calls=2):
    """-> (does the predicate call the launch plain, {tensor: numpy}) of one launch on the first n envs"""
    be, model, prm = sc["be"], sc["model"], sc["prm"][lag]
    nb, nd = model.num_bodies, model.num_dof
    a = dict(root=be.arr(sc["root"][:n]), dof=be.arr(sc["dof"][:n]), rbs=be.zeros((n, nb, 13)), cf=be.zeros((n, nb, 3)), df=be.zeros((n, nd)), pd=be.zeros((n, nd)))
    act, off, scale, frz = be.arr(sc["actions"][:n]), be.arr(sc["off"]), be.arr(sc["scale"]), be.arr(sc["freeze"])
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"])
    plain = be.lib.phc_sim_is_plain(sc["mstruct"], prm, sim, abi.ptr(act), abi.ptr(frz), calls)
    old = be.lib.phc_sim_force_generic(int(generic))
    try:
        assert be.sim_step(sc["mstruct"], prm, sim, act, off, scale, frz, calls) == 0
        be.sync()
    finally:
        be.lib.phc_sim_force_generic(old)
    return bool(plain), {k: be.np(v) for k, v in a.items()}


def _check(model, out, ref, n, tag):
    worst = {k: float(np.abs(out[k].astype(np.float64) - ref[k][:n]).max()) for k in ("root", "rbs", "df", "cf")}
    print(f"{tag}: largest |device - fp64| " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for e in range(n):
        check_step_against(model, {k: v[e] for k, v in out.items()}, ref["root"][e], ref["dof"][e], ref["rbs"][e], ref["df"][e], ref["cf"][e], f"{tag} env {e}")


def _assert_constructed_contacts(model, cf, tag):
    """env 0: the thighs press on each other (no thigh is near the ground) and a foot carries load; env 1, if there: no force at all"""
    names = model.body_names
    thighs = [names.index("L_Hip"), names.index("R_Hip")]
    feet = [names.index(b) for b in ("L_Ankle", "L_Toe", "R_Ankle", "R_Toe")]
    body_body = float(np.linalg.norm(cf[0, thighs], axis=-1).min())
    ground = float(np.abs(cf[0, feet, 2]).max())
    print(f"{tag}: env 0 body-body {body_body:.1f} N, ground {ground:.1f} N")
    assert body_body > 50.0, f"{tag}: the swung leg does not press on the other one"
    assert ground > 1.0, f"{tag}: no foot of env 0 is on the ground"
    if cf.shape[0] > 1:
        assert np.abs(cf[1]).max() == 0.0, f"{tag}: env 1 is in the air"


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("path", ["plain", "generic", "lag0"])
def test_smpl_step_equals_the_double_precision_recursion(smpl, path, n):
    sc = smpl
    lag = 0 if path == "lag0" else 1
    plain, out = _launch(sc, n, generic=path == "generic", lag=lag)
    assert plain == (lag == 1), "the default task's lagged launch satisfies phc_sim_is_plain, the fresh one does not"
    assert np.array_equal(out["pd"], sc["tgt"][:n]), "PD targets are not the formula's"
    _check(sc["model"], out, sc["ref"][(lag, 2)], n, f"{path} N {n}")
    _assert_constructed_contacts(sc["model"], out["cf"], f"{path} N {n}")


@pytest.mark.parametrize("calls", [1, 2])
def test_lagged_sub_steps_behind_a_fresh_one(smpl, calls):
    """num_sim_calls 1: fresh, lagged; 2: that twice (the plain kernel: its list pins num_sim_calls = 2; one call runs the generic lagged kernel)."""
    sc = smpl
    plain, out = _launch(sc, N_MAX, calls=calls)
    assert plain == (calls == 2)
    assert np.array_equal(out["pd"].view(np.int32), sc["tgt"].view(np.int32)), "PD targets are not bit-equal to the formula"
    _check(sc["model"], out, sc["ref"][(1, calls)], N_MAX, f"num_sim_calls {calls}")


# ---------------------------------------------------------------------------------------------------------------
# robots: revolute joints; H1 in 32-lane groups, G1 in 64-lane groups
# ---------------------------------------------------------------------------------------------------------------
def _robot_launch(rb, n):
    be, model, mstruct, root, dof, target, prm = (rb[k] for k in ("be", "model", "mstruct", "root", "dof", "target", "prm"))
    nb, nd = model.num_bodies, model.num_dof
    a = dict(root=be.arr(root[:n]), dof=be.arr(dof[:n]), rbs=be.zeros((n, nb, 13)), cf=be.zeros((n, nb, 3)), df=be.zeros((n, nd)), pd=be.arr(target[:n]))
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"])
    assert be.sim_step(mstruct, prm, sim, None, None, None, None, 2) == 0
    be.sync()
    return {k: be.np(v) for k, v in a.items()}


_ROBOTS = {}   # per robot: the scene and its reference, computed once


def _robot(name):
    """Three states drawn the way test_stepper_equals_the_double_precision_recursion draws them for the robot, low enough for ground contact; lagged inertias."""
    if name not in _ROBOTS:
        _ROBOTS[name] = _make_robot(name)
    return _ROBOTS[name]


def _make_robot(name):
    import hostemu_util as hu
    be = get_backend("hip")
    model, mstruct, keep = model_on(be, name)
    rng = np.random.default_rng(17)
    root, dof, target = random_states(model, N_MAX, rng, height=0.85 if name == "h1_humanoid" else 0.70, vel=0.5, pose=0.15)
    lo, hi = model.dof_limits()
    dof[:, :, 0] = np.clip(dof[:, :, 0], lo + 0.05, hi - 0.05)
    root, dof, target = root.astype(F), dof.astype(F), np.clip(target, lo, hi).astype(F)
    prm = abi.sim_params_struct(inertia_lag=1, self_collision=1, control_mode=1 if name == "h1_humanoid" else 2, sim_dt=1.0 / 200.0)
    ref = hu.sim_step_f64(model, prm, root, dof, target, 2)
    return dict(name=name, be=be, model=model, mstruct=mstruct, keep=keep, root=root, dof=dof, target=target, prm=prm, ref=ref)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("name", ["h1_humanoid", "g1_humanoid"])
def test_robot_step_equals_the_double_precision_recursion(name, n):
    robot = _robot(name)
    out = _robot_launch(robot, n)
    _check(robot["model"], out, robot["ref"], n, f"{robot['name']} N {n}")
    ground = float(np.abs(out["cf"][:, :, 2]).max())
    print(f"{robot['name']} N {n}: largest ground force {ground:.1f} N")
    assert ground > 1.0, "no body is on the ground"


# ---------------------------------------------------------------------------------------------------------------
# no race: the same launch twice from the same state
# ---------------------------------------------------------------------------------------------------------------
def test_plain_launch_twice_gives_the_same_bits(smpl):
    _, a = _launch(smpl, 3)
    _, b = _launch(smpl, 3)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k} differs between two launches from the same state"


def test_g1_launch_twice_gives_the_same_bits():
    robot = _robot("g1_humanoid")
    a, b = _robot_launch(robot, 2), _robot_launch(robot, 2)
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{k} differs between two launches from the same state"
