"""TEST INFRASTRUCTURE for tests/test_lag_regimes.py: constructed states for the decisions only the LAGGED stepping scheme (`inertia_lag` 1, the default) takes -- a ground
point that arrives, leaves or changes its friction regime between two fresh sub-steps, a joint limit that is held, engages or releases there, several lagged sub-steps in
a row -- in the style of tests/stepper_regimes.py, whose Regime rows, launches and comparisons are reused.

The witness comes from oracle/aba_oracle.py::sim_step(trace=...) alone (plain numpy, fp64; no backend and no build of the lane code is asked): per sub-step whether
it was lagged, per ground point depth, fn0, whether the kept I^A holds it and whether it pushed, per revolute DoF the limit error and whether the kept D^-1 holds the
limit.  `WITNESS[make]` asserts the regime with its margin, as a condition on the INPUTS (test_lag_regime_is_reached_with_its_margin).

MARGINS
  ground point against the plane    depth >= 1 mm on the stated side of 0 at the sub-steps named
  pushing / separating              |fn0| >= 5 % of k |depth| + c_n |u_z|, the two terms it is the difference of
  friction regime                   cone / viscous >= 1.05 (stick) or <= 0.95 (slip), as stepper_regimes
  joint limit                       limit error >= 1e-3 rad on the stated side at each sub-step named

CASES (every launch: 2 simulate() calls; sub-step s is lagged when s % substeps != 0).  Margins reached, as the witness prints them:
  arrive-smpl / -h1         the left foot 1.5 / 1.2 mm above the plane at sub-step 0 falling at 1.2 / 2.0 m/s is 8.0 / 3.5 mm deep at sub-step 1 (lagged): no force there;
                            it joins at sub-step 2 (fresh).  The right foot carries the body throughout.
  leave-smpl / -h1          the left foot 3 mm deep rising at 0.1 m/s pushes at sub-step 0; at sub-step 1 it separates (fn0 <= 0 at positive depth): F0 gone, impedance kept
  slip-smpl / -h1           both feet 3 mm deep; the left foot slides at 0.6 m/s at sub-step 0 (slip) and the contact has stopped it by sub-step 1 (stick): old c_t in the
                            kept I^A, new c_t in F0
  limits-h1 / -g1           three states, limit penalty 2000 N m/rad + 20 N m s/rad: HELD (0.05 rad beyond at sub-steps 0 and 1), LATE (2 mrad inside at sub-step 0,
                            beyond at sub-step 1: spring without damper), RELEASED (2 mrad beyond at sub-step 0, inside at sub-step 1).  H1: elbows and a shoulder; G1: the
                            14-gram finger links left_two / left_four / left_six
  deep-smpl / -h1           substeps 4: the left foot arrives in lagged sub-step 1 and stays silent through sub-steps 2 and 3"""
import numpy as np

import aba_oracle as ao
import stepper_edge_cases as ec
import stepper_regimes as sr

F = np.float32
LIMITS = dict(limit_stiffness=2000.0, limit_damping=20.0)

TABLE = [
    sr._r("arrive-smpl", "smpl_humanoid", "lag_arrive", "a foot above the plane at the fresh sub-step penetrates at the lagged one: no force until the next fresh one", (1,)),
    sr._r("arrive-h1", "h1_humanoid", "lag_arrive", "the same, revolute", (1,)),
    sr._r("leave-smpl", "smpl_humanoid", "lag_leave", "a point that pushed at the fresh sub-step separates at the lagged one: impedance kept, F0 gone", (1,)),
    sr._r("leave-h1", "h1_humanoid", "lag_leave", "the same, revolute", (1,)),
    sr._r("slip-smpl", "smpl_humanoid", "lag_slip", "a kept point slips at the fresh sub-step and sticks at the lagged one: old c_t kept, new c_t in F0", (1,)),
    sr._r("slip-h1", "h1_humanoid", "lag_slip", "the same, revolute", (1,)),
    sr._r("limits-h1", "h1_humanoid", "lag_limits", "joint limit held / engaging late (spring, no damper) / released in the lagged sub-step", (1,), **LIMITS),
    sr._r("limits-g1", "g1_humanoid", "lag_limits", "the same on G1's 14-gram finger links (64 lanes, `pd` mode 2)", (1,), **LIMITS),
    sr._r("deep-smpl", "smpl_humanoid", "lag_deep", "substeps 4: a foot arrives in lagged sub-step 1 and stays silent through sub-step 3", (1,), substeps=4),
    sr._r("deep-h1", "h1_humanoid", "lag_deep", "the same, revolute", (1,), substeps=4),
]
REGIMES = {r.id: r for r in TABLE}
ROWS = [(r.id, 1) for r in TABLE]

# Tolerances wider than check_step_against's, by the rule of stepper_regimes.WIDER (4 x the fp32 host emulation's error against the fp64 reference, measured on the CPU):
# none is needed -- every row meets check_step_against itself.
WIDER = {}


# ---- constructors -----------------------------------------------------------------------------------------------------------------------------------------------
def _feet(model, gap_l, vz_l, vx_l=0.0, root_vz=0.0):
    """Squatting on flat feet, PD targets at the pose: the right foot `depth_r` deep at rest, the left foot's lowest point `gap_l` above the plane (negative: inside)
    moving at (vx_l, 0, vz_l)."""
    depth_r = DEPTH_R[sr.smpl(model)]
    root, dof, target = sr.standing(model)
    sr.foot_gap_angle(model, root, dof, "L", gap_l + depth_r)
    target = dof[:, :, 0].copy()
    if vz_l or vx_l:
        sr.foot_rates(model, root[0], dof[0], "L", (vx_l, 0.0, vz_l))
    sr.lower(model, root[0], dof[0], depth_r, sr.FEET[sr.smpl(model)]["R"])
    root[0, 9] = root_vz
    return sr.done(root, dof, target)


# Depth of the right foot's lowest point.  H1's foot hull has points 1.5 and 3.0 mm above its lowest one: at 3 mm a point would sit ON the plane in the fresh sub-step 0,
# where fp32 and fp64 may take different sides of `depth > 0` (a pushing point adds its whole impedance: the one discontinuous decision of the penalty law).
DEPTH_R = {True: 0.003, False: 0.0042}
ARRIVE = {True: (0.0015, -1.2), False: (0.0012, -2.0)}   # (gap, v_z) of the left foot: SMPL (sub-steps of 1/120 s), robots (1/400 s)
DEEP = {True: (0.0012, -1.6), False: (0.0011, -2.5)}     # (sub-steps of 1/240 and 1/800 s)
LEAVE = {True: (-0.003, 0.14, 0.0, 0.0), False: (-0.0042, 0.25, 0.0, -0.1)}   # (gap, v_z, v_x of the left foot, v_z of the root)
SLIP = {True: (-0.003, -0.3, 1.0, -0.25), False: (-0.0042, -0.3, 0.6, 0.0)}


def make_arrive(model):
    return _feet(model, *ARRIVE[sr.smpl(model)])


def make_deep(model):
    return _feet(model, *DEEP[sr.smpl(model)])


def make_leave(model):
    gap, vz, vx, rvz = LEAVE[sr.smpl(model)]
    return _feet(model, gap, vz, vx_l=vx, root_vz=rvz)


def make_slip(model):
    gap, vz, vx, rvz = SLIP[sr.smpl(model)]
    return _feet(model, gap, vz, vx_l=vx, root_vz=rvz)


LIMIT_JOINTS = {"h1": (("left_elbow_link", "hi"), ("right_elbow_link", "hi"), ("left_shoulder_roll_link", "lo")),
                "g1": (("left_two_link", "lo"), ("left_four_link", "hi"), ("left_six_link", "hi"))}
LIMIT_RATE = {"h1": (2.0, 2.0), "g1": (2.0, 10.0)}   # rad/s across the limit, late / released: 5 mrad per sub-step of 1/400 s (G1's fingers: the limit damper takes 5/6 of it)


def make_limits(model):
    """Three states in the air at rest, targets at the pose; one joint each: held, late, released."""
    root, dof, target = sr.air(model, 3, quiet=True)
    lo, hi = model.dof_limits()
    for e, (body, end) in enumerate(LIMIT_JOINTS[sr.model_kind(model)]):
        d = sr.dofs_of(model, body)[0]
        out = 1.0 if end == "hi" else -1.0          # the direction that leaves the range
        lim = hi[d] if end == "hi" else lo[d]
        if e == 0:
            dof[e, d, 0] = lim + 0.05 * out
        elif e == 1:
            dof[e, d, 0], dof[e, d, 1] = lim - 0.002 * out, LIMIT_RATE[sr.model_kind(model)][0] * out
        else:
            dof[e, d, 0], dof[e, d, 1] = lim + 0.0015 * out, -LIMIT_RATE[sr.model_kind(model)][1] * out
        target[e, d] = dof[e, d, 0]
    return sr.done(root, dof, target)


sr.MAKE.update(lag_arrive=make_arrive, lag_deep=make_deep, lag_leave=make_leave, lag_slip=make_slip, lag_limits=make_limits)


# ---- the oracle on a case ------------------------------------------------------------------------------------------------------------------------------------------
def oracle(reg, num_sim_calls=2):
    """aba_oracle.sim_step at inertia_lag 1 on the case's states with the case's parameters (the numbers the C struct holds; body-body forces in the stepper's fixed point):
    ({tensor: [n, ...]} like a launch's outputs, [trace per state])."""
    def make():
        s, m = sr.states(reg), sr.model_of(reg)
        dp, sim_dt, substeps = sr.dense_params(sr.params_of(reg, 1))
        dp["self_force_fixed_point"] = sr.FIXED_POINT
        outs, traces = [], []
        for e in range(s["root"].shape[0]):
            tr = {}
            outs.append(ao.sim_step(m, s["root"][e], s["dof"][e], s["target"][e], dp, sim_dt, substeps, num_sim_calls, inertia_lag=1, trace=tr))
            traces.append(tr["substeps"])
        return {k: np.stack([o[i] for o in outs]) for i, k in enumerate(("root", "dof", "rbs", "df", "cf"))}, traces
    return ec.cached(("lag-oracle", reg.id, num_sim_calls), make)


# ---- witnesses ---------------------------------------------------------------------------------------------------------------------------------------------------
def _fn0_margin(reg, c):
    """|fn0| relative to the two terms it is the difference of (k depth and c_n u_z)."""
    prm = sr.params_of(reg, 1)
    k = float(prm.contact_stiffness)
    # fn0 = k depth - c_n u_z: the second term is what is left
    return abs(c["fn0"]) / (k * abs(c["depth"]) + abs(k * c["depth"] - c["fn0"]))


def _points(reg, sub, side):
    return [c for c in sub["contacts"] if sr._foot_points(sr.model_of(reg), side)(c)]


def _no_point_on_a_branch(reg, tr, lines):
    """In a FRESH sub-step a point that pushes adds its whole impedance to I^A, so `depth > 0` and `fn0 > 0` are discontinuous decisions there (in a lagged sub-step
    only F0 depends on them, and F0 -> 0 continuously at both).  fp32 carries a depth to ~1e-7 m and fn0 = k depth - c_n u_z to ~0.03 N: every point of every fresh
    sub-step stays 0.05 mm from the plane and, when inside, 0.3 N from fn0 = 0 -- five hundred and ten times those errors."""
    near, small = np.inf, np.inf
    for sub in tr:
        if sub["lagged"]:
            continue
        near = min(near, min(abs(c["depth"]) for c in sub["contacts"]))
        small = min([small] + [abs(c["fn0"]) for c in sub["contacts"] if c["fn0"] is not None])
    lines.append(f"fresh sub-steps, all points: nearest to the plane {near * 1e3:.3f} mm, smallest |fn0| {small:.2f} N")
    assert near >= 5e-5 and small >= 0.3


def _silent_then_joins(reg, tr, lines, silent, joins):
    """The left foot is above the plane at sub-step 0, at least one of its points penetrates and would push at every sub-step of `silent` (all lagged) without being
    allowed to, and pushes at the fresh sub-step `joins`; the right foot pushes throughout."""
    L0 = _points(reg, tr[0], "L")
    lines.append(f"sub-step 0 (fresh): left foot {len(L0)} points {-max(c['depth'] for c in L0) * 1e3:.2f} .. {-min(c['depth'] for c in L0) * 1e3:.2f} mm above the plane")
    assert not tr[0]["lagged"] and L0 and all(c["depth"] <= -0.001 and not c["pushed"] for c in L0)
    for k in silent:
        Lk = [c for c in _points(reg, tr[k], "L") if c["depth"] >= 0.001]
        assert tr[k]["lagged"] and Lk, f"sub-step {k}: no left-foot point 1 mm deep"
        lines.append(f"sub-step {k} (lagged): {len(Lk)} left-foot points {min(c['depth'] for c in Lk) * 1e3:.2f} .. {max(c['depth'] for c in Lk) * 1e3:.2f} mm deep, fn0 "
                     f"{min(c['fn0'] for c in Lk):.0f} .. {max(c['fn0'] for c in Lk):.0f} N (margin >= {min(_fn0_margin(reg, c) for c in Lk):.2f}): kept {any(c['kept'] for c in Lk)}, "
                     f"pushed {any(c['pushed'] for c in Lk)}")
        assert all(c["fn0"] > 0 and _fn0_margin(reg, c) >= 0.05 and c["kept"] is False and not c["pushed"] for c in Lk)
        assert not any(c["pushed"] for c in _points(reg, tr[k], "L"))
    Lj = [c for c in _points(reg, tr[joins], "L") if c["pushed"]]
    lines.append(f"sub-step {joins} (fresh): {len(Lj)} left-foot points push, {min(c['depth'] for c in Lj) * 1e3:.2f} .. {max(c['depth'] for c in Lj) * 1e3:.2f} mm deep")
    assert not tr[joins]["lagged"] and Lj and all(c["depth"] >= 0.001 and _fn0_margin(reg, c) >= 0.05 for c in Lj)
    for k, sub in enumerate(tr):
        assert any(c["pushed"] for c in _points(reg, sub, "R")), f"sub-step {k}: the right foot does not push"


def w_arrive(reg, s, traces, out):
    lines = sr.Lines()
    _silent_then_joins(reg, traces[0], lines, (1,), 2)
    _no_point_on_a_branch(reg, traces[0], lines)
    return lines


def w_deep(reg, s, traces, out):
    lines = sr.Lines()
    assert [t["lagged"] for t in traces[0]] == [False, True, True, True] * 2
    _silent_then_joins(reg, traces[0], lines, (1, 2, 3), 4)
    _no_point_on_a_branch(reg, traces[0], lines)
    return lines


def w_leave(reg, s, traces, out):
    lines, tr = sr.Lines(), traces[0]
    L0 = [c for c in _points(reg, tr[0], "L") if c["pushed"]]
    assert L0 and all(c["depth"] >= 0.001 and _fn0_margin(reg, c) >= 0.05 for c in L0)
    lines.append(f"sub-step 0 (fresh): {len(L0)} left-foot points push, {min(c['depth'] for c in L0) * 1e3:.2f} .. {max(c['depth'] for c in L0) * 1e3:.2f} mm deep, fn0 >= "
                 f"{min(c['fn0'] for c in L0):.0f} N (margin >= {min(_fn0_margin(reg, c) for c in L0):.2f})")
    kept = {c["point"] for c in L0}
    L1 = [c for c in _points(reg, tr[1], "L") if c["point"] in kept]
    assert tr[1]["lagged"] and all(c["kept"] for c in L1)
    for c in L1:   # every kept point: out of the plane by 1 mm, or in it by 1 mm and pushing / separating by the margin
        assert c["depth"] <= -0.001 or (c["depth"] >= 0.001 and _fn0_margin(reg, c) >= 0.05), c
    gone = [c for c in L1 if not c["pushed"]]
    assert gone, "no kept point leaves"
    sep = [c for c in gone if c["depth"] > 0]
    lines.append(f"sub-step 1 (lagged): {len(gone)} of the {len(L1)} kept points carry no force: {len(sep)} separating" +
                 (f" at {min(c['depth'] for c in sep) * 1e3:.2f} .. {max(c['depth'] for c in sep) * 1e3:.2f} mm depth with fn0 {min(c['fn0'] for c in sep):.0f} .. "
                  f"{max(c['fn0'] for c in sep):.0f} N (margin >= {min(_fn0_margin(reg, c) for c in sep):.2f})" if sep else "") + f", {len(gone) - len(sep)} above the plane")
    _no_point_on_a_branch(reg, traces[0], lines)
    return lines


def w_slip(reg, s, traces, out):
    lines, tr = sr.Lines(), traces[0]
    L0 = {c["point"]: c for c in _points(reg, tr[0], "L") if c["pushed"]}
    assert L0 and all(c["friction"] == "slip" and c["cone_ratio"] <= 0.95 and c["depth"] >= 0.001 and _fn0_margin(reg, c) >= 0.05 for c in L0.values())
    # the witness points: kept, still pushing by the margin, and now inside the cone by the margin (the friction clamp is a min: continuous for every other point)
    L1 = [c for c in _points(reg, tr[1], "L") if c["point"] in L0 and c["pushed"] and c["cone_ratio"] >= 1.05 and c["depth"] >= 0.001 and _fn0_margin(reg, c) >= 0.05]
    lines.append(f"sub-step 0 (fresh): {len(L0)} left-foot points slide at {min(c['slip_speed'] for c in L0.values()):.3f} m/s, cone / viscous <= {max(c['cone_ratio'] for c in L0.values()):.2f} "
                 f"(slip); sub-step 1 (lagged): {len(L1)} of them push at <= {max(c['slip_speed'] for c in L1):.4f} m/s, cone / viscous >= {min(c['cone_ratio'] for c in L1):.2f} (stick), "
                 f"{min(c['depth'] for c in L1) * 1e3:.2f} mm deep, fn0 margin >= {min(_fn0_margin(reg, c) for c in L1):.2f}")
    assert tr[1]["lagged"] and L1 and all(c["kept"] and c["friction"] == "stick" for c in L1)
    _no_point_on_a_branch(reg, traces[0], lines)
    return lines


def w_limits(reg, s, traces, out):
    m, lines = sr.model_of(reg), sr.Lines()
    want = (("held", True, True, True), ("late", False, True, False), ("released", True, False, True))   # (engaged at sub-step 0, at sub-step 1, in the kept D^-1 there)
    for e, ((body, end), (label, on0, on1, kept1)) in enumerate(zip(LIMIT_JOINTS[sr.model_kind(m)], want)):
        d = sr.dofs_of(m, body)[0]
        r0, r1 = (next(x for x in traces[e][k]["limits"] if x["dof"] == d) for k in (0, 1))
        past = lambda r: r["above"] if end == "hi" else r["below"]   # > 0: beyond the limit
        lines.append(f"state {e} {label}: {body} ({m.mass[list(m.body_names).index(body)] * 1e3:.0f} g) {past(r0) * 1e3:+.2f} mrad past its {end} limit at sub-step 0, "
                     f"{past(r1) * 1e3:+.2f} mrad at sub-step 1 (lagged); the kept D^-1 holds the limit: {r1['kept']}")
        assert not traces[e][0]["lagged"] and traces[e][1]["lagged"]
        assert (past(r0) >= 1e-3) if on0 else (past(r0) <= -1e-3), "sub-step 0: not on its side by 1 mrad"
        assert (past(r1) >= 1e-3) if on1 else (past(r1) <= -1e-3), "sub-step 1: not on its side by 1 mrad"
        assert (r0["e"] != 0) == on0 and (r1["e"] != 0) == on1 and r1["kept"] == kept1
        others = [x for k in (0, 1) for x in traces[e][k]["limits"] if x["dof"] != d]
        assert all(x["e"] == 0 and max(x["below"], x["above"]) <= -1e-3 for x in others), "another joint is at a limit"
    return lines


WITNESS = dict(lag_arrive=w_arrive, lag_deep=w_deep, lag_leave=w_leave, lag_slip=w_slip, lag_limits=w_limits)


def witness(reg):
    out, traces = oracle(reg)
    return WITNESS[reg.make](reg, sr.states(reg), traces, out)
