"""External body wrenches (phc_sim_step_wrench) and the push schedule (`+perturb.*`) on a machine without a GPU.

The stepper checks run through oracle/hostemu's emu_sim_step_wrench: the per-lane functions of phc_amd/csrc/phc_aba.h in the phase sequence of the kernel, with the
wrench handed to aba_body_init as the kernel's WRENCH instantiations hand it over -- at single precision and at double precision (the exact-arithmetic statement of
the same recursion).  Each physical statement is checked at 1e-9 between two fp64 runs and, for the fp32 run against that fp64 run, at the tolerances the fp32
stepper is held to against its references everywhere else (wrench_util.assert_standing)."""
import numpy as np
import pytest
import torch

import wrench_util as wu

F = np.float32


@pytest.fixture(scope="module")
def smpl():
    return wu.load("smpl_humanoid")


@pytest.fixture(scope="module")
def h1():
    return wu.load("h1_humanoid")


# ---- 1. null wrench ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["fp32", "fp64"])
@pytest.mark.parametrize("robot", ["smpl_humanoid", "h1_humanoid", "g1_humanoid"])
def test_null_wrench_is_the_host_emulation_bit_for_bit(robot, f64):
    """Without a wrench (null pointers, and a wrench with wrench_sim_calls = 0) emu_sim_step_wrench takes the plain route: it IS
    oracle/hostemu's emu_sim_step, same bits in every output."""
    model = wu.load(robot)
    if model.all_spherical:
        root, dof, target = wu.smpl_state(model, 2, "ground", seed=1)
        prm = wu.params(self_collision=1, inertia_lag=1)
    else:
        root, dof, target = wu.robot_rest_state(model, 2, 1.05 if robot == "h1_humanoid" else 0.80)
        dof[:, :, 1] = np.random.default_rng(2).normal(0, 0.3, dof[:, :, 1].shape)
        prm = wu.params(control_mode=2, sim_dt=1 / 200, limit_stiffness=2000.0, limit_damping=20.0, self_collision=1, inertia_lag=1)
    ref = wu.host_step(model, prm, root, dof, target, 2, f64=f64, reference=True)
    big = np.full((2, model.num_bodies, 3), 250.0)
    for kw in (dict(), dict(force=big, torque=big * 0.1, wrench_sim_calls=0)):
        out = wu.host_step(model, prm, root, dof, target, 2, f64=f64, **kw)
        for k in ("root", "dof", "rbs", "cf", "df"):
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    assert np.abs(ref["cf"]).sum() > 0


# ---- 2. a force m_i dg on every body is gravity ---------------------------------------------------------------------------------------------------------------
GRAVITY_CASES = [("ground", dict(inertia_lag=0)), ("ground", dict(inertia_lag=1)), ("ground", dict(contact_model="tgs")), ("air", dict(inertia_lag=0)),
                 ("air", dict(inertia_lag=1))]


@pytest.mark.parametrize("where,opts", GRAVITY_CASES, ids=["ground-fresh", "ground-lag", "ground-rigid", "air-fresh", "air-lag"])
def test_uniform_force_is_gravity(smpl, where, opts):
    """F_i = m_i (0, 0, dg) at every centre of mass, over the whole launch, is the same step as gravity_z + dg without a wrench."""
    root, dof, target = wu.smpl_state(smpl, 2, where, seed=3)
    prm = wu.params(**opts)
    rigid = opts.get("contact_model") == "tgs"
    ref = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, gravity_z=float(prm.gravity_z) + wu.DELTA_G)
    out64 = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, force=wu.gravity_wrench(smpl, 2, True), wrench_sim_calls=2)
    out32 = wu.host_step(smpl, prm, root, dof, target, 2, f64=False, force=wu.gravity_wrench(smpl, 2, False), wrench_sim_calls=2)
    plain = wu.host_step(smpl, prm, root, dof, target, 2, f64=True)
    wu.report(f"gravity {where} {opts} fp64", out64, ref)
    wu.report(f"gravity {where} {opts} fp32", out32, ref)
    assert np.abs(plain["rbs"][..., 7:10] - ref["rbs"][..., 7:10]).max() > 0.02, "the added gravity must matter"
    if where == "ground":
        assert np.abs(ref["cf"]).sum() > 0
    wu.assert_exact(out64, ref)
    wu.assert_standing(out32, ref, rigid=rigid)


# ---- 3. a torque couple across a joint is a joint torque ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("body", wu.COUPLE_JOINTS["h1_humanoid"])
def test_torque_couple_is_a_joint_torque(h1, body):
    """H1, `pd` drive held over the simulate call (control_mode 1), one sub-step, from rest: +dtau a on a link and -dtau a on its parent is the drive torque of that
    joint raised by dtau, i.e. its PD target raised by dtau / kp (30 N m, far inside the effort limit)."""
    root, dof, target = wu.robot_rest_state(h1, 2, 1.5)
    prm = wu.params(control_mode=1, substeps=1, sim_dt=1 / 200, limit_stiffness=2000.0, limit_damping=20.0)
    dtau = 30.0
    d = int(h1.dof_start[h1.body_names.index(body)])
    assert dtau < 0.5 * h1.dof_effort[d]
    torque, tgt = wu.couple_case(h1, root, dof, target, body, dtau)
    ref = wu.host_step(h1, prm, root, dof, tgt, 1, f64=True)
    out64 = wu.host_step(h1, prm, root, dof, target, 1, f64=True, torque=torque, wrench_sim_calls=1)
    out32 = wu.host_step(h1, prm, root, dof, target, 1, f64=False, torque=torque, wrench_sim_calls=1)
    plain = wu.host_step(h1, prm, root, dof, target, 1, f64=True)
    wu.report(f"couple {body} fp64", out64, ref)
    wu.report(f"couple {body} fp32", out32, ref)
    assert np.abs(plain["dof"][:, d, 1] - ref["dof"][:, d, 1]).min() > 0.05, "the raised target must move the joint"
    wu.assert_exact(out64, ref)
    wu.assert_standing(out32, ref)


# ---- 4. yaw covariance -------------------------------------------------------------------------------------------------------------------------------------------
def test_yaw_covariance(smpl):
    """State and wrench turned by 90 degrees about z give the turned result: catches a wrench read in the body frame, and swapped components."""
    root, dof, target, force, torque = wu.yaw_case(smpl, 2)
    prm = wu.params(inertia_lag=1)
    a64 = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=2)
    rroot, rforce, rtorque = wu.yaw90_state(root), wu.yaw90_vec(force), wu.yaw90_vec(torque)
    b64 = wu.host_step(smpl, prm, rroot, dof, target, 2, f64=True, force=rforce, torque=rtorque, wrench_sim_calls=2)
    b32 = wu.host_step(smpl, prm, rroot, dof, target, 2, f64=False, force=rforce, torque=rtorque, wrench_sim_calls=2)
    plain = wu.host_step(smpl, prm, root, dof, target, 2, f64=True)
    assert np.abs(plain["rbs"][..., 7:13] - a64["rbs"][..., 7:13]).max() > 0.05, "the wrench must matter"
    turned = dict(root=wu.yaw90_state(a64["root"]), dof=a64["dof"], rbs=wu.yaw90_state(a64["rbs"]))
    wu.report("yaw fp64", b64, turned)
    wu.report("yaw fp32", b32, turned)
    np.testing.assert_allclose(b64["root"][..., 0:3], turned["root"][..., 0:3], atol=1e-9)
    np.testing.assert_allclose(b64["root"][..., 7:13], turned["root"][..., 7:13], atol=1e-9)
    np.testing.assert_allclose(b64["dof"], turned["dof"], atol=1e-9)
    np.testing.assert_allclose(b64["rbs"][..., 0:3], turned["rbs"][..., 0:3], atol=1e-9)
    np.testing.assert_allclose(b64["rbs"][..., 7:13], turned["rbs"][..., 7:13], atol=1e-9)
    np.testing.assert_allclose(np.abs((b64["rbs"][..., 3:7] * turned["rbs"][..., 3:7]).sum(-1)), 1.0, atol=1e-12)
    wu.assert_standing(b32, turned)


# ---- 5. momentum theorem ----------------------------------------------------------------------------------------------------------------------------------------
def _momenta(model, out, e):
    """Linear momentum and angular momentum about the system's centre of mass of env e, from the published body states (fp64)."""
    rbs = out["rbs"][e]
    m = wu.body_mass(model, True)
    Rs = [wu.quat_to_mat(rbs[i, 3:7]) for i in range(model.num_bodies)]
    cs = np.array([rbs[i, 0:3] + Rs[i] @ model.com[i] for i in range(model.num_bodies)])
    C = (m[:, None] * cs).sum(0) / m.sum()
    P, Lc = np.zeros(3), np.zeros(3)
    for i in range(model.num_bodies):
        c, R = model.com[i], Rs[i]
        Icom = model.inertia_origin[i] - m[i] * (c @ c * np.eye(3) - np.outer(c, c))
        wv, v = rbs[i, 10:13], rbs[i, 7:10]
        vc = v + np.cross(wv, R @ c)
        P += m[i] * vc
        Lc += R @ Icom @ R.T @ wv + m[i] * np.cross(cs[i] - C, vc)
    return P, Lc, cs, C


def test_momentum_theorem(smpl):
    """Airborne SMPL at rest, PD targets at its pose, one sub-step: the change of total linear momentum converges to dt (sum F + M g) and the change of angular
    momentum about the system's centre of mass to dt (sum T + sum (c_i - C) x F_i) -- at second order in dt (error ratio 4 between dt and dt / 2; [3, 5] asked).
    Forces: horizontal at the pelvis' centre of mass and -- because the SMPL pelvis has its centre of mass AT its origin -- also at the left knee's, which has not;
    a torque on the torso.  The same forces applied at the body ORIGINS instead (expressed through the torque argument) must fail the angular half.
    The steps compared are 1/960 and 1/1920 s: the theorem is a statement about the limit, and at the shipped 1/120 s the implicit drive's dt^2 kp term is not yet
    small against the joint inertias, so the error still carries its cubic term there (measured ratios: 6.0 at 1/60 | 1/120, 5.1 at 1/240 | 1/480, 3.8 and 4.4 here)."""
    nb = smpl.num_bodies
    root, dof, target = wu.smpl_state(smpl, 1, "air", seed=6)
    root[:, 7:13] = 0
    dof[:, :, 1] = 0
    target = dof[:, :, 0].copy()
    knee, torso = smpl.body_names.index("L_Knee"), smpl.body_names.index("Torso")
    assert np.linalg.norm(smpl.com[knee]) > 0.05
    force, torque = np.zeros((1, nb, 3)), np.zeros((1, nb, 3))
    force[0, 0] = (200.0, -120.0, 0.0)
    force[0, knee] = (-80.0, 150.0, 0.0)
    torque[0, torso] = (25.0, 10.0, -30.0)
    g = float(F(-9.81))
    M = wu.body_mass(smpl, True).sum()

    def errors(at_origin):
        errs = []
        for dt in (1 / 960, 1 / 1920):
            prm = wu.params(sim_dt=dt, substeps=1, angular_damping=0.0)
            dt = float(prm.sim_dt)
            before = wu.host_step(smpl, prm, root, dof, target, 0, f64=True)
            P0, L0, cs, C = _momenta(smpl, before, 0)
            assert np.abs(P0).max() < 1e-12 and np.abs(L0).max() < 1e-12
            tq = torque.copy()
            if at_origin:   # F at the origin o_i = F at the centre of mass c_i plus the torque (o_i - c_i) x F
                for i in (0, knee):
                    tq[0, i] += np.cross(before["rbs"][0, i, 0:3] - cs[i], force[0, i])
            out = wu.host_step(smpl, prm, root, dof, target, 1, f64=True, force=force, torque=tq, wrench_sim_calls=1)
            P1, L1, _, _ = _momenta(smpl, out, 0)
            dP = dt * (force[0].sum(0) + np.array([0, 0, M * g]))
            dL = dt * (torque[0].sum(0) + sum(np.cross(cs[i] - C, force[0, i]) for i in range(nb)))
            errs.append((np.linalg.norm(P1 - dP), np.linalg.norm(L1 - dL), np.linalg.norm(dP), np.linalg.norm(dL)))
        return errs

    (eP1, eL1, nP, nL), (eP2, eL2, _, _) = errors(False)
    print(f"momentum: linear error {eP1:.3e} -> {eP2:.3e} (of {nP:.3e}), angular error {eL1:.3e} -> {eL2:.3e} (of {nL:.3e})")
    assert eP1 < 0.05 * nP and 3.0 <= eP1 / eP2 <= 5.0, (eP1, eP2)
    assert eL1 < 0.05 * nL and 3.0 <= eL1 / eL2 <= 5.0, (eL1, eL2)
    (_, oL1, _, _), (_, oL2, _, _) = errors(True)
    print(f"momentum, forces at the origins: angular error {oL1:.3e} -> {oL2:.3e}")
    assert not (3.0 <= oL1 / oL2 <= 5.0) and oL1 > 10 * eL1, "a force applied at the body origin must fail the angular momentum balance"


# ---- 6. duration -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["fp32", "fp64"])
def test_wrench_duration(smpl, f64):
    """num_sim_calls = 2 with wrench_sim_calls = 1 is a one-call launch with the wrench followed by a one-call launch without.  (The state passes through the
    simulator tensors between two launches -- exponential-map joint coordinates --, so the two ways agree to rounding, not to the bit: 1e-9 at double precision,
    the standing tolerances for the fp32 run against the fp64 split.)  wrench_sim_calls beyond num_sim_calls is clamped."""
    root, dof, target, force, torque = wu.yaw_case(smpl, 2)
    prm = wu.params(inertia_lag=1)
    one = wu.host_step(smpl, prm, root, dof, target, 2, f64=f64, force=force, torque=torque, wrench_sim_calls=1)
    s1 = wu.host_step(smpl, prm, root, dof, target, 1, f64=True, force=force, torque=torque, wrench_sim_calls=1)
    s2 = wu.host_step(smpl, prm, s1["root"], s1["dof"], target, 1, f64=True)
    both = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=2)
    assert np.abs(both["rbs"][..., 7:13] - s2["rbs"][..., 7:13]).max() > 0.05, "the second call's wrench must matter"
    wu.report(f"duration fp{64 if f64 else 32}", one, s2)
    if f64:
        wu.assert_exact(one, s2)
        clamped = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=7)
        for k in ("root", "dof", "rbs"):
            np.testing.assert_array_equal(clamped[k], both[k])
    else:
        wu.assert_standing(one, s2)


# ---- 7. published forces -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["fp32", "fp64"])
def test_wrench_is_not_part_of_the_published_forces(smpl, h1, f64):
    """contact_force (S4) and dof_force (S5) of an airborne env under a wrench are those of the same env without it.
    S4: exactly (zero in the air, with and without).  S5 publishes the torque the drive APPLIED over the sub-step:
      * H1 under the held `pd` drive (control_mode 1, one simulate call): the torque is fixed at the start of the call -- equal to the bit;
      * SMPL under the linearly-implicit drive: tau_explicit(t) - (dt kd + dt^2 kp) qdd, the drive's own reaction to the motion, which a push changes like any
        other cause of motion would.  There is nothing to hold equal there; the figure is printed."""
    nb = smpl.num_bodies
    root, dof, target = wu.smpl_state(smpl, 2, "air", seed=8)
    force, torque = np.full((2, nb, 3), 120.0), np.full((2, nb, 3), -20.0)
    prm = wu.params(substeps=1)
    plain = wu.host_step(smpl, prm, root, dof, target, 1, f64=f64)
    out = wu.host_step(smpl, prm, root, dof, target, 1, f64=f64, force=force, torque=torque, wrench_sim_calls=1)
    assert np.abs(out["rbs"] - plain["rbs"]).max() > 0.01
    np.testing.assert_array_equal(out["cf"], plain["cf"])
    assert np.abs(out["cf"]).max() == 0.0
    moved = np.abs(out["df"].astype(np.float64) - plain["df"].astype(np.float64)).max()
    print(f"SMPL, implicit drive, fp{64 if f64 else 32}: the applied drive torque follows the pushed motion, it moved by up to {moved:.3e} N m")
    # H1, held drive
    root, dof, target = wu.robot_rest_state(h1, 2, 1.5)
    target = target + 0.2
    prm = wu.params(control_mode=1, sim_dt=1 / 200, limit_stiffness=2000.0, limit_damping=20.0)
    f = np.full((2, h1.num_bodies, 3), 60.0)
    plain = wu.host_step(h1, prm, root, dof, target, 1, f64=f64)
    out = wu.host_step(h1, prm, root, dof, target, 1, f64=f64, force=f, torque=-0.2 * f, wrench_sim_calls=1)
    assert np.abs(out["rbs"] - plain["rbs"]).max() > 0.01 and np.abs(plain["df"]).max() > 1.0
    np.testing.assert_array_equal(out["cf"], plain["cf"])
    np.testing.assert_array_equal(out["df"], plain["df"])


# ---- 8. PushSchedule on the CPU device ---------------------------------------------------------------------------------------------------------------------------
NAMES = ["Pelvis", "L_Hip", "Torso", "Head"]


def _schedule(**kw):
    from phc_amd.perturb import PushSchedule
    cfg = dict(force=[200, 400], bodies=["Pelvis", "Torso"], interval_s=[0.2, 0.4], duration_s=0.1, direction="horizontal", seed=5)
    cfg.update(kw)
    return PushSchedule(cfg, 16, NAMES, 1 / 30, "cpu", default_seed=0)


def _run(s, steps, reset_at=None):
    hist = []
    for t in range(steps):
        s.advance(None if reset_at is None else torch.tensor([t == reset_at and e == 3 for e in range(s.num_envs)]))
        hist.append(s.force.clone())
    return torch.stack(hist)   # [T, N, NB, 3]


def test_push_schedule():
    state = torch.get_rng_state()
    a = _run(_schedule(), 100)
    assert torch.equal(torch.get_rng_state(), state), "the schedule must draw from its own generator"
    assert torch.equal(a, _run(_schedule(), 100)), "same seed, same pushes"
    assert not torch.equal(a, _run(_schedule(seed=6), 100))
    mag = a.norm(dim=-1)                                   # [T, N, NB]
    on = mag > 0
    assert on.any() and (mag[on] >= 200 - 1e-3).all() and (mag[on] <= 400 + 1e-3).all()
    assert (a[..., 2] == 0).all(), "horizontal pushes have no z component"
    assert not on[:, :, 1].any() and not on[:, :, 3].any() and on[:, :, 0].any() and on[:, :, 2].any(), "only the listed bodies are pushed"
    assert (on.sum(-1) <= 1).all(), "one body per push"
    # runs of pushed and of force-free steps per env: 0.1 s at dt = 1/30 is 3 steps; the pause is 6 .. 12 steps (0.2 .. 0.4 s)
    s = _schedule()
    a = _run(s, 100)
    pushed = (a.norm(dim=-1) > 0).any(-1).numpy()          # [T, N]
    started = 0
    for e in range(pushed.shape[1]):
        runs, t = [], 0
        while t < len(pushed):
            u = t
            while u < len(pushed) and pushed[u, e] == pushed[t, e]:
                u += 1
            runs.append((bool(pushed[t, e]), u - t))
            t = u
        started += sum(1 for p, _ in runs if p)
        assert not runs[0][0]
        for k, (p, n) in enumerate(runs[:-1]):
            assert (n == 3) if p else (6 <= n <= 12), (e, runs)
        # within a push the force is constant
    assert int(s.pushes) == started
    any_dir = _run(_schedule(direction="any"), 60)
    assert (any_dir[..., 2] != 0).any()


def test_push_schedule_reset_ends_the_push():
    s = _schedule()
    a = _run(s, 40)
    pushed = (a.norm(dim=-1) > 0).any(-1)[:, 3]
    t0 = int(torch.nonzero(pushed)[0])                     # first pushed step of env 3; reset it in the push's second step
    b = _run(_schedule(), 40, reset_at=t0 + 1)
    pb = (b.norm(dim=-1) > 0).any(-1)[:, 3]
    assert pb[t0] and not pb[t0 + 1:t0 + 1 + 5].any(), "a reset env's push ends at once and a new pause of >= 6 steps (this one included) begins"
    others = [e for e in range(16) if e != 3]
    assert torch.equal(a[:, others], b[:, others])


# ---- 9. errors and the binding -----------------------------------------------------------------------------------------------------------------------------------
def test_binding_types_the_new_symbol():
    from phc_amd import _lib
    assert "phc_sim_step_wrench" in _lib.EXPORTED_SYMBOLS
    fn = _lib.load().phc_sim_step_wrench
    assert len(fn.argtypes) == 12 and fn.restype is _lib.c_i32


def _host_task(*over, push=None):
    """The task as far as its host phases build it (no device): what the task-level guards read."""
    from phc_amd.config import compose
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    t = HumanoidIm.host_only(compose(["env.num_envs=2", *over]))
    t._push, t.device = push, "cpu"     # (the one-shot buffers of the last case below are made on `device`)
    return t


def test_task_level_errors():
    from phc_amd.learning.amp_agent import IMAmpAgent
    T = _host_task
    f = torch.zeros(2, 24, 3)
    with pytest.raises(NotImplementedError, match="has_shape_variation"):
        T("robot.has_shape_variation=True").apply_rigid_body_force_tensors(f)
    with pytest.raises(NotImplementedError, match="lane_mapping"):
        T("+solver.lane_mapping=3").apply_rigid_body_force_tensors(f)
    with pytest.raises(ValueError, match="schedule"):
        T(push=_schedule()).apply_rigid_body_force_tensors(f)
    with pytest.raises(ValueError, match="shape"):
        T().apply_rigid_body_force_tensors(torch.zeros(2, 3, 3))
    t = T()
    t.apply_rigid_body_force_tensors(f + 1.0, None, sim_calls=1)
    assert t._ext_pending == (True, False, 1) and float(t._ext_force.sum()) == 144.0 and t._ext_torque is None

    class A:
        task = T(push=_schedule())
    with pytest.raises(NotImplementedError, match="push schedule"):
        IMAmpAgent.train(A(), 1)


def test_schedule_config_errors():
    with pytest.raises(ValueError, match="no such body"):
        _schedule(bodies=["Tail"])
    with pytest.raises(ValueError, match="direction"):
        _schedule(direction="up")
    with pytest.raises(ValueError, match="unknown perturb option"):
        _schedule(force_n=3)
