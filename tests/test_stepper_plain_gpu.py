"""GPU: the plain launch of the stepper (phc_amd/csrc/phc_sim_plain.h) against the double-precision recursion and against the generic kernel.

One env step (2 x simulate x 2 sub-steps) of the default task's launch -- self-collision on, lagged inertias, actions and a freeze mask given -- at N = 2 (one
wavefront), 3 and 65 (a tail wavefront with one env) and 130.  The states are the ones `test_stepper_equals_the_double_precision_recursion` draws for SMPL
(`random_states` in the air, touching down, in contact; a third of the envs each) plus, in every fourth env, a quiet pose whose left leg is swung into the right one
(body-body contact of over 1 kN in the emulation).  Actions are non-zero: they are chosen so that the PD targets land where `random_states` puts them.

  * the shipped path (the predicate holds: the plain kernel) and the path under `phc_sim_force_generic(1)` are each held to oracle/hostemu/hostemu64.cpp at exactly
    `check_step_against`'s tolerances -- the ones that test holds the stepper to;
  * every tensor the launch writes is compared between the two paths with the same tolerances (the unit is compiled with fast-math: bit equality is not demanded)
    and the largest differences are printed; the PD targets are bit-equal to the formula in both;
  * launches the predicate rejects (no freeze mask, `pd_ref`, the tgs contact model) run the generic kernel whatever the switch says: bit-equal results with the
    switch on and off -- and the generic kernel's device code is, instruction for instruction, the parent's (profiles/stepper_plain_instantiation);
  * `force_average` is NOT in the list: it changes what S4 / S5 publish and never the states, and tests/test_env_gpu.py asks for bit-identical trajectories with
    the switch on and off -- so both values run the plain kernel.  Checked here: same state bits, other forces, and the generic kernel's means within tolerance."""
import numpy as np
import pytest

from backends import get_backend, model_on
from phc_amd import abi
from test_dynamics import check_step_against, random_states

pytestmark = pytest.mark.gpu
F = np.float32
N_MAX = 130
SIZES = [2, 3, 65, 130]


def _states(model):
    """root [N, 13], dof [N, D, 2], pd offset / scale [D], actions [N, D], freeze [D], the PD targets the formula gives [N, D]."""
    rng = np.random.default_rng(17)
    parts = [random_states(model, N_MAX, rng, height=h) for h in (3.0, 0.95, 0.80)]
    pick = np.arange(N_MAX) % 3
    root, dof, target = (np.stack([parts[pick[e]][k][e] for e in range(N_MAX)]) for k in range(3))
    names = model.body_names
    hip = 3 * (names.index("L_Hip") - 1)
    for e in range(1, N_MAX, 4):   # body-body contact: the left leg swung into the right one, in the air, nearly at rest
        root[e, 2], root[e, 3:7], root[e, 7:13] = 1.5, (0, 0, 0, 1), 0.05 * root[e, 7:13]
        dof[e, :, 0], dof[e, :, 1] = 0.0, 0.05 * dof[e, :, 1]
        dof[e, hip, 0] = -0.9
        target[e] = dof[e, :, 0] + 0.1 * (target[e] - parts[pick[e]][1][e, :, 0])
    nd = model.num_dof
    off, scale = rng.normal(0, 0.1, nd).astype(F), rng.uniform(0.5, 1.5, nd).astype(F)
    actions = ((target - off) / scale).astype(F)
    freeze = np.zeros(nd, np.int32)
    for nme in ("L_Hand", "R_Hand"):
        i = 3 * (names.index(nme) - 1)
        freeze[i:i + 3] = 1
    tgt = (off + (scale * actions).astype(F)).astype(F)   # A2: the product rounded on its own, then the sum
    tgt[:, freeze != 0] = 0.0
    assert np.abs(actions).min(axis=1).max() > 0 and np.abs(actions).mean() > 0.05
    return root.astype(F), dof.astype(F), off, scale, actions, freeze, tgt


@pytest.fixture(scope="module")
def scene():
    import hostemu_util as hu
    be = get_backend("hip")
    model, mstruct, keep = model_on(be)
    root, dof, off, scale, actions, freeze, tgt = _states(model)
    prm = abi.sim_params_struct(inertia_lag=1, self_collision=1)
    ref = hu.sim_step_f64(model, prm, root, dof, tgt, 2)   # once, for all sizes: envs are independent and every size runs a prefix
    return dict(be=be, model=model, mstruct=mstruct, keep=keep, root=root, dof=dof, off=off, scale=scale, actions=actions, freeze=freeze, tgt=tgt, prm=prm, ref=ref)


def _launch(sc, n, generic, prm=None, freeze=True, pd_ref=False):
    """-> (was the launch plain by the predicate, {tensor: numpy}) of one env step of the first n envs"""
    be, model = sc["be"], sc["model"]
    nb, nd = model.num_bodies, model.num_dof
    prm = prm or sc["prm"]
    a = dict(root=be.arr(sc["root"][:n]), dof=be.arr(sc["dof"][:n]), rbs=be.zeros((n, nb, 13)), cf=be.zeros((n, nb, 3)), df=be.zeros((n, nd)), pd=be.zeros((n, nd)))
    act, off, scale, frz = be.arr(sc["actions"][:n]), be.arr(sc["off"]), be.arr(sc["scale"]), be.arr(sc["freeze"]) if freeze else None
    ref_pos = be.arr(sc["dof"][:n, :, 0].copy()) if pd_ref else None
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"], pd_ref=ref_pos)
    plain = be.lib.phc_sim_is_plain(sc["mstruct"], prm, sim, abi.ptr(act), abi.ptr(frz), 2)
    old = be.lib.phc_sim_force_generic(int(generic))
    try:
        assert be.sim_step(sc["mstruct"], prm, sim, act, off, scale, frz, 2) == 0
        be.sync()
    finally:
        be.lib.phc_sim_force_generic(old)
    return bool(plain), {k: be.np(v) for k, v in a.items()}


@pytest.mark.parametrize("n", SIZES)
def test_plain_and_generic_paths_against_the_double_precision_recursion(scene, n):
    sc = scene
    model, ref = sc["model"], sc["ref"]
    plain_a, shipped = _launch(sc, n, generic=False)
    plain_b, generic = _launch(sc, n, generic=True)
    assert plain_a and plain_b, "the default task's launch must satisfy phc_sim_is_plain (the predicate does not look at the switch)"
    worst = {k: float(np.abs(shipped[k].astype(np.float64) - generic[k]).max()) for k in shipped}
    print(f"N {n}: largest |plain - generic| per tensor " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for name, out in (("plain", shipped), ("generic", generic)):
        assert np.array_equal(out["pd"], sc["tgt"][:n]), f"{name}: PD targets are not the formula's"
        vs = {k: float(np.abs(out[k].astype(np.float64) - ref[k][:n]).max()) for k in ("root", "rbs", "df", "cf")}
        print(f"N {n}: largest |{name} - fp64| " + ", ".join(f"{k} {v:.3e}" for k, v in vs.items()))
    for name, out in (("plain", shipped), ("generic", generic)):
        for e in range(n):
            check_step_against(model, {k: v[e] for k, v in out.items()}, ref["root"][e], ref["dof"][e], ref["rbs"][e], ref["df"][e], ref["cf"][e], f"{name} N {n} env {e}")
    # the two paths against each other, at the tolerance both are held to against fp64
    for e in range(n):
        check_step_against(model, {k: v[e] for k, v in shipped.items()}, generic["root"][e], generic["dof"][e], generic["rbs"][e], generic["df"][e], generic["cf"][e],
                           f"plain vs generic N {n} env {e}")
    assert any(worst[k] > 0 for k in worst) or n < 3, "the two paths returned the same bits everywhere: is the plain kernel launched at all?"
    # the scene does what its description says: body-body contact in the constructed envs, ground contact in the low ones
    if n >= 65:
        cf = np.abs(generic["cf"]).max(axis=(1, 2))
        assert (cf[1:n:4] > 50.0).all(), "the swung leg does not touch the other one"
        assert (cf[np.arange(n) % 3 == 2] > 1.0).mean() > 0.5


@pytest.mark.parametrize("case", ["no_freeze_mask", "pd_ref", "tgs"])
def test_a_launch_the_predicate_rejects_runs_the_generic_kernel(scene, case):
    sc = scene
    kw = dict(no_freeze_mask=dict(freeze=False), pd_ref=dict(pd_ref=True),
              tgs=dict(prm=abi.sim_params_struct(self_collision=1, contact_model="tgs")))[case]
    for n in (3, 66):
        plain_a, a = _launch(sc, n, generic=False, **kw)
        plain_b, b = _launch(sc, n, generic=True, **kw)
        assert not plain_a and not plain_b, case
        for k in a:
            assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{case} N {n}: {k} depends on the switch"
        assert np.isfinite(a["rbs"]).all() and np.abs(a["rbs"][:, :, 0:3] - sc["root"][:n, None, 0:3]).max() < 2.0   # (a step was taken, nothing blew up)
        if case == "no_freeze_mask":
            tgt = (sc["off"] + (sc["scale"] * sc["actions"][:n]).astype(F)).astype(F)
            assert np.array_equal(a["pd"], tgt)


def test_force_average_stays_plain_and_changes_only_the_published_forces(scene):
    sc = scene
    model, n = sc["model"], 65
    avg = abi.sim_params_struct(inertia_lag=1, self_collision=1, force_average=1)
    plain_0, last = _launch(sc, n, generic=False)
    plain_1, mean = _launch(sc, n, generic=False, prm=avg)
    plain_g, mean_g = _launch(sc, n, generic=True, prm=avg)
    assert plain_0 and plain_1 and plain_g
    for k in ("root", "dof", "rbs", "pd"):
        assert np.array_equal(last[k].view(np.int32), mean[k].view(np.int32)), f"force_average moved {k}"
    assert not np.array_equal(last["df"], mean["df"]) and np.abs(last["cf"] - mean["cf"]).max() > 0.0
    for e in range(n):   # the means of the two kernels, at the tolerance both are held to against fp64 for the last sub-step's values
        check_step_against(model, {k: v[e] for k, v in mean.items()}, mean_g["root"][e], mean_g["dof"][e], mean_g["rbs"][e], mean_g["df"][e], mean_g["cf"][e],
                           f"force_average plain vs generic env {e}")
