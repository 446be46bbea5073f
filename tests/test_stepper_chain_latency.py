"""The stepper paths whose memory traffic was re-batched (profiles/stepper_chain_latency/README.md): the PD-target prologue, the level hand-overs of the
backward sweep (all children requested together; the lagged hand-over at its 16-byte aligned place), the ground-contact point pass (eight points in flight, the
body constants kept for the launch, the reference-point offsets in LDS) and the pair-list load.  No sum was reordered, so every check here is one the parent
commit passes as well: the targets bit for bit against the formula, everything else against the host emulation and the double-precision build of the same
recursion at exactly the tolerances of tests/test_stepper_options.py::test_stepper_equals_the_double_precision_recursion (test_dynamics.check_step_against)."""
import numpy as np
import pytest

from backends import BACKENDS, get_backend, model_on
from phc_amd import abi
from test_dynamics import check_step_against, random_states, run_step

F = np.float32
_REF = {}   # references computed once and shared by the backends


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _robot_case(name, n, seed, height, draw=None):
    """Random states the way test_stepper_equals_the_double_precision_recursion draws them, and the robot's stepper switches there.  `draw`: that many states are
    drawn and repeated to fill the n envs."""
    model, _, _ = model_on(get_backend("hostemu"), name=name)
    rng = np.random.default_rng(seed)
    if draw is not None:
        root, dof, target, kw = _robot_case(name, draw, seed, height)
        i = np.arange(n) % draw
        return root[i].copy(), dof[i].copy(), target[i].copy(), kw
    if model.all_spherical:
        root, dof, target = random_states(model, n, rng, height=height)
        kw = {}
    else:
        root, dof, target = random_states(model, n, rng, height=height, vel=0.5, pose=0.15)
        lo, hi = model.dof_limits()
        dof[:, :, 0] = np.clip(dof[:, :, 0], lo + 0.05, hi - 0.05)
        target = np.clip(target, lo, hi).astype(F)
        kw = dict(control_mode=1 if name == "h1_humanoid" else 2, sim_dt=1.0 / 200.0)
    return root, dof, target, kw


def _check_against_references(backend, name, root, dof, target, prm, key, on=None):
    """One env step on `backend` against the fp64 build of the recursion and, on the device, against the host emulation as well.
    `on(be)`: the model on a backend, as model_on returns it (default: the shipped model `name`)."""
    import hostemu_util as hu
    on = on or (lambda b: model_on(b, name=name))
    be = get_backend(backend)
    model, mstruct, keep = on(be)
    out = run_step(be, model, mstruct, root, dof, target, prm, 2)
    ref = _cached(("f64",) + key, lambda: hu.sim_step_f64(model, prm, root, dof, target, 2))
    refs = [("fp64 recursion", ref)]
    if backend == "hip":
        def emu():
            hb = get_backend("hostemu")
            hm, hs, hk = on(hb)
            return run_step(hb, hm, hs, root, dof, target, prm, 2)
        refs.append(("host emulation", _cached(("emu",) + key, emu)))
    for what, r in refs:
        worst = float(np.abs(out["rbs"] - r["rbs"]).max())
        print(f"{name} {key}: {backend} vs {what}, worst body-state difference {worst:.2e}")
        for e in range(root.shape[0]):
            check_step_against(model, {k: v[e] for k, v in out.items()}, r["root"][e], r["dof"][e], r["rbs"][e], r["df"][e], r["cf"][e], f"{name} {key} env {e} vs {what}")
    return model, out


# ---------------------------------------------------------------------------------------------------------------
# 1. PD targets
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,mode", [("hostemu", "plain"), ("hostemu", "freeze"),   # (the host emulation has no res_action path)
                                          pytest.param("hip", "plain", marks=pytest.mark.gpu), pytest.param("hip", "res_action", marks=pytest.mark.gpu),
                                          pytest.param("hip", "freeze", marks=pytest.mark.gpu), pytest.param("hip", "res_action_freeze", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("name", ["smpl_humanoid", "h1_humanoid"])
def test_pd_targets_equal_the_formula_bit_for_bit(backend, mode, name):
    """`sim.pd_target` after a launch with actions == float32(offset + float32(scale * action)); with a reference position (env.res_action)
    float32(ref + scale * action) kept within float32(pi / 2) of the joint position; frozen DoFs 0.  Three envs: the last wavefront is half empty."""
    be = get_backend(backend)
    model, mstruct, keep = model_on(be, name=name)
    n, nd = 3, model.num_dof
    rng = np.random.default_rng(23)
    root, dof, _ = random_states(model, n, rng, height=2.0, vel=0.2, pose=0.3)
    act = rng.normal(0, 2.0, (n, nd)).astype(F)
    off = rng.normal(0, 0.3, nd).astype(F)
    scale = rng.uniform(0.3, 2.0, nd).astype(F)
    ref = (dof[:, :, 0] + rng.normal(0, 0.4, (n, nd))).astype(F) if "res_action" in mode else None
    freeze = (rng.random(nd) < 0.3).astype(np.int32) if "freeze" in mode else None
    sa = (scale[None] * act).astype(F)
    if ref is not None:
        half_pi = F(1.57079637)
        q = dof[:, :, 0].astype(F)
        expect = np.maximum(np.minimum((ref + sa).astype(F), (q + half_pi).astype(F)), (q - half_pi).astype(F))
        hit = expect != (ref + sa).astype(F)
        assert hit.any() and not hit.all(), "the case must reach the clamp on some DoFs only"
    else:
        expect = (off[None] + sa).astype(F)
    if freeze is not None:
        assert freeze.any() and not freeze.all()
        expect[:, freeze != 0] = 0
    a = dict(root=be.arr(root), dof=be.arr(dof), rbs=be.zeros((n, model.num_bodies, 13)), cf=be.zeros((n, model.num_bodies, 3)), df=be.zeros((n, nd)),
             pd=be.arr(np.full((n, nd), 7.0, F)), act=be.arr(act), off=be.arr(off), scale=be.arr(scale))
    a["ref"] = None if ref is None else be.arr(ref)
    a["freeze"] = None if freeze is None else be.arr(freeze)
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"], pd_ref=a["ref"])
    prm = abi.sim_params_struct() if model.all_spherical else abi.sim_params_struct(sim_dt=1.0 / 200.0)
    assert be.sim_step(mstruct, prm, sim, a["act"], a["off"], a["scale"], a["freeze"], 1) == 0
    be.sync()
    got = be.np(a["pd"])
    assert np.array_equal(got.view(np.uint32), expect.astype(F).view(np.uint32)), f"{int((got != expect).sum())} of {got.size} targets differ, worst {np.abs(got - expect).max():.3e}"
    assert np.isfinite(be.np(a["root"])).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. level hand-overs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("name,height", [("smpl_humanoid", 0.85), ("h1_humanoid", 0.85), ("g1_humanoid", 0.70)])
def test_level_hand_overs(backend, lag, n, name, height):
    """SMPL (spherical joints, re-rooted solver tree, bodies with 0 / 1 / 2 / 3 solver children), H1 (revolute, 32-lane groups), G1 (64-lane groups); one, three and 65 envs
    (a lone env, a half-empty last wavefront, more than one workgroup row); fresh and lagged level-steps; self-collision on.  One env step.
    The states are the six that test_stepper_equals_the_double_precision_recursion draws for the robot (same generator, same seed), repeated over the envs: what 65 envs
    add is indexing, not states.  (65 independent draws hold a state -- env 26, H1, lagged -- at which the fp32 host emulation of the PARENT commit is 2.1e-2 m/s from the
    fp64 recursion in two body velocities of ~7 m/s, the explicit `pd` torque clipping on different sides: a property of that state, not of a build.)"""
    root, dof, target, kw = _cached(("case", name, n), lambda: _robot_case(name, n, 17, height, draw=6))
    prm = abi.sim_params_struct(inertia_lag=lag, self_collision=1, **kw)
    _check_against_references(backend, name, root, dof, target, prm, ("handover", name, n, lag))


# ---------------------------------------------------------------------------------------------------------------
# 3. ground contact
# ---------------------------------------------------------------------------------------------------------------
def _quat_rotate(q, v):
    """q xyzw [..., 4], v [..., 3]"""
    u, w = q[..., :3], q[..., 3:4]
    t = 2.0 * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def _point_depths(name, root, dof):
    """depth (> 0: below the plane) of every ground-contact point of every env, from the FK-only launch of the host emulation: [n, points]"""
    hb = get_backend("hostemu")
    model, ms, keep = model_on(hb, name=name)
    n = root.shape[0]
    a = dict(root=hb.arr(root), dof=hb.arr(dof), rbs=hb.zeros((n, model.num_bodies, 13)), cf=hb.zeros((n, model.num_bodies, 3)), df=hb.zeros((n, model.num_dof)),
             pd=hb.zeros((n, model.num_dof)))
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"])
    assert hb.refresh_body_state(ms, sim) == 0
    rbs = hb.np(a["rbs"]).astype(np.float64)
    cb = np.asarray(model.contact_body)
    pos = np.asarray(model.contact_pos, np.float64)
    rad = np.asarray(model.contact_radius, np.float64)
    z = rbs[:, cb, 2] + _quat_rotate(rbs[:, cb, 3:7], pos[None])[..., 2] - rad[None]
    return model, -z


def _ground_scene(scene):
    rng = np.random.default_rng(29)
    if scene in ("smpl_feet_flat", "smpl_in_the_air", "smpl_one_toe"):
        name = "smpl_humanoid"
        model, _, _ = model_on(get_backend("hostemu"), name=name)
        n, nd = 3, model.num_dof
        root = np.zeros((n, 13), F)
        root[:, 6] = 1
        dof = np.zeros((n, nd, 2), F)
        dof[:, :, 1] = rng.normal(0, 0.05, (n, nd))
        root[:, 7:13] = rng.normal(0, 0.05, (n, 6))
        root[:, 9] = -0.3   # moving down: the penalty contact is non-adhesive, a point that moves up fast enough carries no force
        names = list(model.body_names)
        feet = [names.index(b) for b in ("L_Ankle", "R_Ankle")]
        toes = [names.index(b) for b in ("L_Toe", "R_Toe")]
        cb = np.asarray(model.contact_body)
        root[:, 2] = 2.0
        if scene == "smpl_one_toe":   # the left toe joint turned until that toe's lowest point hangs more than 1 cm below every other body's; lowered until it is 4 mm in the ground
            j = 3 * (toes[0] - 1)
            for axis, angle in [(a, s) for a in range(3) for s in (0.9, -0.9)]:
                dof[:, j:j + 3, 0] = 0
                dof[:, j + axis, 0] = angle
                _, depth = _point_depths(name, root, dof)
                low = np.array([(-depth[0, cb == b]).min() for b in range(model.num_bodies)])
                if low.argmin() == toes[0] and np.sort(low)[1] - low.min() > 0.01:
                    break
            else:
                raise AssertionError("no toe angle leaves the toe alone lowest")
        _, depth = _point_depths(name, root, dof)
        if scene == "smpl_in_the_air":
            root[:, 2] = 3.0
        else:
            root[:, 2] = 2.0 - (-depth).min(axis=1) - (0.004 if scene == "smpl_one_toe" else 0.006)   # lowest point that far in the ground
        return name, root, dof, dof[:, :, 0].copy(), {}, dict(feet=feet, toes=toes, cb=cb)
    if scene == "g1_on_its_torso":
        name = "g1_humanoid"
        model, _, _ = model_on(get_backend("hostemu"), name=name)
        n, nd = 2, model.num_dof
        root = np.zeros((n, 13), F)
        root[:, 3:7] = np.array([0.0, -np.sqrt(0.5), 0.0, np.sqrt(0.5)], F)   # pitched by 90 degrees: the torso link is the lowest body
        dof = np.zeros((n, nd, 2), F)
        lo, hi = model.dof_limits()
        dof[:, :, 0] = np.clip(0.0, lo + 0.05, hi - 0.05)[None]
        dof[:, :, 1] = rng.normal(0, 0.05, (n, nd))
        root[:, 9] = -0.3
        root[:, 2] = 2.0
        _, depth = _point_depths(name, root, dof)
        root[:, 2] = 2.0 - (-depth).min(axis=1) - 0.02
        return name, root, dof, np.clip(dof[:, :, 0], lo, hi).astype(F), dict(control_mode=2, sim_dt=1.0 / 200.0), dict(cb=np.asarray(model.contact_body))
    raise KeyError(scene)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("lag", [0, 1])
@pytest.mark.parametrize("scene", ["smpl_feet_flat", "smpl_in_the_air", "smpl_one_toe", "g1_on_its_torso"])
def test_ground_contact_point_pass(backend, lag, scene):
    """Both feet flat (every box corner touches: the longest walk over the touching points), nothing within the broad-phase bound, one toe alone, and G1 lying on its
    torso: 40 ground-contact points on one body, the most of any shipped model.  (G1 has revolute joints: it takes the serial point pass.  The batched pass
    with more than one group of eight is test_ground_contact_with_more_than_eight_points_on_a_body.)"""
    name, root, dof, target, kw, info = _cached(("scene", scene), lambda: _ground_scene(scene))
    model, depth = _cached(("depth", scene), lambda: _point_depths(name, root, dof))
    cb = info["cb"]
    touching = depth > 0
    if scene == "smpl_feet_flat":
        for b in info["feet"] + info["toes"]:   # (a flat box rests on its four bottom corners: half of the body's eight points, on four bodies)
            assert (cb == b).sum() == 8 and (touching[:, cb == b].sum(axis=1) == 4).all(), "the four bottom corners of both feet and both toes are in the ground"
    elif scene == "smpl_in_the_air":
        assert not touching.any()
    elif scene == "smpl_one_toe":
        for e in range(root.shape[0]):
            assert len(set(cb[touching[e]])) == 1 and cb[touching[e]][0] in info["toes"], "one toe body alone touches"
    else:
        torso = max(set(cb), key=lambda b: int((cb == b).sum()))
        assert (cb == torso).sum() == 40, "the torso link carries 40 points"
        assert touching[:, cb == torso][:, 8:].any(axis=1).all(), "points behind the first eight touch"
    prm = abi.sim_params_struct(inertia_lag=lag, **kw)
    _, out = _check_against_references(backend, name, root, dof, target, prm, ("ground", scene, lag))
    fz = out["cf"][:, :, 2].sum(-1)
    assert (fz == 0).all() if scene == "smpl_in_the_air" else (fz > 1.0).all(), fz   # (every env carries ground force)


def _smpl_with_dense_soles(be):
    """The SMPL humanoid with more sole points than one group of eight: 9 further points on the left sole (17 on the body: two full groups and a third that holds
    one point) and 4 on the right (12: a full group and half a group).  They lie in the plane of the box's bottom corners, so model.pack() -- lowest points
    first -- puts the 13 / 8 sole points in front of the upper corners: standing flat, points 8..12 of the left foot touch."""
    from phc_amd.model import load_model
    from phc_amd.robots import apply_collision_filter
    m = load_model("smpl_humanoid")
    apply_collision_filter(m, "smpl")
    names = list(m.body_names)
    for body, extra in (("R_Ankle", 4), ("L_Ankle", 9)):   # (the later body first: the earlier body's indices stay valid)
        b = names.index(body)
        idx = np.flatnonzero(m.contact_body == b)
        pos, rad = m.contact_pos[idx], m.contact_radius[idx]
        sole = pos[np.argsort(pos[:, 2] - rad, kind="stable")[:4]]   # the four bottom corners
        w = np.random.default_rng(41 + extra).dirichlet(np.ones(4), extra)   # points inside their quadrilateral
        at = idx[-1] + 1
        m.contact_body = np.insert(m.contact_body, at, np.full(extra, b, m.contact_body.dtype))
        m.contact_pos = np.insert(m.contact_pos, at, w @ sole, axis=0)
        m.contact_radius = np.insert(m.contact_radius, at, np.full(extra, rad.min()))
    ints, floats = m.pack()
    keep = (be.arr(ints), be.arr(floats))
    return m, abi.model_struct(keep[0], keep[1], m.num_bodies, m.num_dof, m.max_level, len(m.contact_body)), keep


def _dense_scene():
    m, _, _ = _smpl_with_dense_soles(get_backend("hostemu"))
    n, nd = 3, m.num_dof
    rng = np.random.default_rng(31)
    root = np.zeros((n, 13), F)
    root[:, 6] = 1
    dof = np.zeros((n, nd, 2), F)
    dof[:, :, 1] = rng.normal(0, 0.05, (n, nd))
    root[:, 7:13] = rng.normal(0, 0.05, (n, 6))
    root[:, 9] = -0.3
    # rest pose, upright: body frames are world-aligned up to the root's, so the lowest point follows from the kinematic chain of offsets
    _, depth = _point_depths("smpl_humanoid", np.concatenate([root[:, :2], np.full((n, 1), 2.0, F), root[:, 3:]], 1), dof)
    root[:, 2] = 2.0 - (-depth).min(axis=1) - 0.006
    return m, root, dof


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("lag", [0, 1])
def test_ground_contact_with_more_than_eight_points_on_a_body(backend, lag):
    """The batched point pass (spherical joints, penalty contact) behind its first group of eight: the group loop, the clamp of a group's tail to the body's last
    point, the shift by the group's first index.  No shipped spherical model has more than eight points on a body, so the SMPL humanoid gets denser soles here.
    Standing flat on both feet, slightly in the ground."""
    m, root, dof = _cached(("dense_scene",), _dense_scene)
    names = list(m.body_names)
    per_body = np.bincount(m.contact_body, minlength=m.num_bodies)
    assert per_body[names.index("L_Ankle")] == 17 and per_body[names.index("R_Ankle")] == 12
    prm = abi.sim_params_struct(inertia_lag=lag)
    _, out = _check_against_references(backend, "smpl_dense_soles", root, dof, dof[:, :, 0].copy(), prm, ("dense", lag), on=_smpl_with_dense_soles)
    # the added points carry load: the foot ends the step with another velocity than under the shipped model from the same state
    def shipped():
        hb = get_backend("hostemu")
        pm, ps, keep = model_on(hb)   # (`keep` holds the model tables the struct points to)
        return run_step(hb, pm, ps, root, dof, dof[:, :, 0].copy(), prm, 2)
    plain = _cached(("dense_plain", lag), shipped)
    assert np.abs(out["cf"]).sum() > 10.0, "the case must exercise ground contact"   # (S4 is the LAST sub-step's force: a stiff sole may have left the ground by then)
    moved = float(np.abs(out["rbs"][:, names.index("L_Ankle"), 7:13] - plain["rbs"][:, names.index("L_Ankle"), 7:13]).max())
    print(f"left foot velocity, dense soles vs shipped soles: {moved:.3e}")
    assert moved > 3e-2, "13 sole points carry the foot differently from 4: ten times what the comparison above tolerates"


def test_batched_point_pass_equals_the_dense_oracle_with_more_than_eight_points_on_a_body():
    """The references of the test above compile the same point pass as the kernel, so an error in its group loop would pass there.  Here the double-precision
    build of the lane code steps the dense-sole model from the same state and is compared with the dense fp64 oracle (oracle/dyn_oracle.py), which walks
    `model.contact_pos` point by point in code of its own -- both with the fp32-rounded parameters of the C struct, as
    test_double_precision_build_of_the_recursion_is_the_dense_scheme does for the shipped models, at its bound (1e-9; a dropped or misplaced sole point moves the
    foot by 1e-2 and more).  And the oracle itself sees the points behind the first eight: without them its result differs."""
    import copy
    import dyn_oracle as do
    import hostemu_util as hu
    from test_dynamics import f32_params
    m, _, _ = _smpl_with_dense_soles(get_backend("hostemu"))
    _, root, dof = _cached(("dense_scene",), _dense_scene)
    target = dof[:, :, 0].copy()
    prm = abi.sim_params_struct()
    out = hu.sim_step_f64(m, prm, root, dof, target, 2)
    dp, sim_dt, substeps = f32_params(prm)
    # the model without the points that pack() puts behind the first eight of each foot (the lowest-first order pack() uses)
    cut = copy.deepcopy(m)
    keep = np.ones(len(m.contact_body), bool)
    for b in (list(m.body_names).index("L_Ankle"), list(m.body_names).index("R_Ankle")):
        idx = np.flatnonzero(m.contact_body == b)
        order = idx[np.argsort(m.contact_pos[idx, 2] - m.contact_radius[idx], kind="stable")]
        keep[order[8:]] = False
    cut.contact_body, cut.contact_pos, cut.contact_radius = m.contact_body[keep], m.contact_pos[keep], m.contact_radius[keep]
    worst, cut_off = 0.0, 0.0
    for e in range(root.shape[0]):
        r, d, rbs, tau, fc = do.sim_step(m, root[e], dof[e], target[e], params=dp, sim_dt=sim_dt, substeps=substeps, num_sim_calls=2)
        check_step_against(m, {k: v[e] for k, v in out.items()}, r, d, rbs, tau, fc, f"env {e}", scale=1e-5)
        worst = max(worst, float(np.abs(out["rbs"][e] - rbs).max()))
        rbs_cut = do.sim_step(cut, root[e], dof[e], target[e], params=dp, sim_dt=sim_dt, substeps=substeps, num_sim_calls=2)[2]
        cut_off = max(cut_off, float(np.abs(rbs_cut - rbs).max()))
    print(f"dense soles: fp64 recursion vs dense oracle {worst:.2e}; oracle without the points behind the first eight differs by {cut_off:.2e}")
    assert worst < 1e-9
    assert cut_off > 1e-3, "the points behind the first eight of a foot carry load in this scene"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("lag", [0, 1])
def test_ground_contact_with_two_shapes_in_one_wavefront(backend, lag):
    """Per-env body shapes: envs 0 and 1 share a wavefront and carry different shapes (different link offsets, masses and contact-point counts).  Every env against the
    fp64 recursion of its own shape's model and, on the device, against the host emulation of the same stacked launch."""
    import hostemu_util as hu
    from phc_amd.model import load_model, pack_shapes
    from phc_amd.robots import apply_collision_filter
    models = [load_model(f"smpl_{g}_humanoid") for g in range(3)]
    for m in models:
        apply_collision_filter(m, "smpl")
    ints, floats = pack_shapes(models)
    m0 = models[0]
    n = 4
    shape = np.array([0, 1, 2, 1], np.int32)
    root, dof, target = _cached(("shapes_case",), lambda: random_states(m0, n, np.random.default_rng(5), height=0.85))
    prm = abi.sim_params_struct(inertia_lag=lag)

    def run(be):
        keep = (be.arr(ints), be.arr(floats))
        stacked = abi.model_struct(keep[0], keep[1], m0.num_bodies, m0.num_dof, m0.max_level, max(len(m.contact_body) for m in models), num_shapes=3)
        a = dict(root=be.arr(root), dof=be.arr(dof), rbs=be.zeros((n, m0.num_bodies, 13)), cf=be.zeros((n, m0.num_bodies, 3)), df=be.zeros((n, m0.num_dof)),
                 pd=be.arr(target), es=be.arr(shape))
        sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"], env_shape=a["es"])
        assert be.sim_step(stacked, prm, sim, None, None, None, None, 2) == 0
        be.sync()
        return {k: be.np(v) for k, v in a.items()}

    out = run(get_backend(backend))
    assert np.abs(out["cf"]).sum() > 10.0, "the case must exercise ground contact"
    for e in range(n):
        g = int(shape[e])
        ref = _cached(("shapes_f64", lag, e), lambda: hu.sim_step_f64(models[g], prm, root[e:e + 1], dof[e:e + 1], target[e:e + 1], 2))
        check_step_against(models[g], {k: v[e] for k, v in out.items() if k != "es"}, ref["root"][0], ref["dof"][0], ref["rbs"][0], ref["df"][0], ref["cf"][0], f"shape {g} env {e} vs fp64")
    if backend == "hip":
        emu = _cached(("shapes_emu", lag), lambda: run(get_backend("hostemu")))
        for e in range(n):
            check_step_against(models[int(shape[e])], {k: v[e] for k, v in out.items() if k != "es"}, emu["root"][e], emu["dof"][e], emu["rbs"][e], emu["df"][e], emu["cf"][e],
                               f"env {e} vs host emulation")


# ---------------------------------------------------------------------------------------------------------------
# 4. pair list
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["smpl_humanoid", "g1_humanoid"])
def test_pair_list_with_touching_limbs(backend, name):
    """Self-collision with folded limbs, no ground in reach, no gravity: SMPL's candidate pairs fill the 18 x 32 pair slots only in part (the last slots are empty for
    every lane), G1's run over 64 lanes.  The net contact forces of an env sum to zero and the step equals the references."""
    def case():
        model, _, _ = model_on(get_backend("hostemu"), name=name)
        rng = np.random.default_rng(3)
        n = 3
        if model.all_spherical:
            root, dof, target = random_states(model, n, rng, height=5.0, vel=0.0, pose=1.0)
            kw = {}
        else:
            root, dof, target = random_states(model, n, rng, height=5.0, vel=0.0, pose=1.5)
            lo, hi = model.dof_limits()
            dof[:, :, 0] = np.clip(dof[:, :, 0], lo + 0.02, hi - 0.02)
            target = np.clip(target, lo, hi).astype(F)
            kw = dict(control_mode=2, sim_dt=1.0 / 200.0)
        dof[:, :, 1] = 0
        root[:, 7:13] = 0
        return root, dof, target, kw
    root, dof, target, kw = _cached(("pairs_case", name), case)
    prm = abi.sim_params_struct(self_collision=1, gravity_z=0.0, **kw)
    _, out = _check_against_references(backend, name, root, dof, target, prm, ("pairs", name))
    cf = out["cf"]
    assert (np.abs(cf).sum(axis=(1, 2)) > 1.0).all(), "limbs must touch in every env"
    np.testing.assert_allclose(cf.sum(axis=1), 0.0, atol=2e-3 * np.abs(cf).sum(axis=1).max())
