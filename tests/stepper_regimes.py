"""TEST INFRASTRUCTURE for tests/test_stepper_regimes.py: constructed states that put the stepper (phc_sim_step, csrc/phc_aba.h + csrc/phc_sim_kernel.h) on a chosen side of
each of its data-dependent branches, the witness that they got there, and the references.

The witness does not come from the code under test.  oracle/dyn_oracle.py::sim_step(trace=...) -- the fp64 dense scheme -- records per sub-step which side of every branch
it took and the deciding quantity as a ratio to its branch point; `WITNESS[make]` below asserts from that record that the regime was reached, with the margin of the
table, so that a correct fp32 kernel provably takes the same side.  The margin check is a condition on the INPUTS: it runs on the CPU with the oracle alone
(test_regime_is_reached_with_its_margin).  The two quat_* small-angle branches, the pi wrap, the pd_ref clamp and the body gate have no counterpart in the oracle's
formulation: their witness is formed from the fp64 inputs and from what the fp64 build of the recursion (oracle/hostemu/hostemu64.cpp) returns.

MARGINS (deciding quantity / branch point, in the fp64 reference; fp32 carries these quantities to ~1e-5 relative or better):
  rate cap                |rate| / max_angular_velocity         >= 1.05 (capped) or <= 0.95, for every joint named by the case
  effort clamp            torque / limit                         |.| >= 1.05 (saturated, sign as stated) or <= 0.95
  pd_ref clamp            (pd_ref + scale action - q) / (pi/2)  >= 1.05, <= -1.05 or |.| <= 0.95
  quat_from_rotvec        angle / 1e-4                           <= 0.55 (series) or >= 1.9
  quat_to_rotvec          sine / 1e-5                            <= 0.6 (small) or >= 2; q.w < 0: the angle is >= 0.04 rad beyond pi
  shortest arc            |angle - pi|                           >= 0.04 rad
  bounce                  approach speed / threshold             >= 1.05 or <= 0.95 at sub-step 0; >= 1.03 or <= 0.97 for EVERY point in range of every sub-step (the one
                                                                 discontinuous branch; 3 % of 0.2 m/s is twice the velocity tolerance the stepper is held to)
  depenetration cap       (depth / dt) / cap                     >= 1.05 or <= 0.95
  contact range           depth against 0 and -contact_offset    >= 1 mm away
  body gate               origin height - gate                   >= 4 mm away
  friction cone           mu F_n / (|u_t| c_max)                 >= 1.05 (stick: the viscous term is inside the cone) or <= 0.95 (slip: clamped to the cone)
  capsule closest points  s, t (and the re-solved s)             >= 0.02 from 0 and 1; penetration >= 1 mm; denom / (a e) >= 1e-3
A margin is asserted at the sub-steps the case names (sub-step 0 unless stated).  Every branch but the bounce threshold is continuous at its branch point (min / max / clamp
of continuous quantities), so a later sub-step that drifts near one changes the result by rounding only; the bounce margin is asserted on all sub-steps for that reason.

CASES (TABLE below states each row's regime and the inertia_lag values it runs; the dense check always runs inertia_lag 0).  Margin reached, as
test_regime_is_reached_with_its_margin prints it (ratios to the branch point):
  cap8-smpl, -occ3     wrist and hand driven to 1.79 .. 1.88 x the cap in every sub-step, the knee started at 100 rad/s 2.34 / 2.47 in sub-step 0 and 0.45 after; named slow
                       joints <= 0.64; capped and uncapped joints in every env and sub-step
  cap100-smpl          both hips 1.26 and 1.38 x 100 rad/s after sub-step 0, every other joint <= 0.74; nothing above 0.95 in the last sub-step
  cap8-h1 / cap8-g1    knee 3.9 -> 2.1 / 3.6 -> 1.9, elbow 2.6 -> 1.2, torso 2.4 -> 1.2 (H1: 0.88 in one sub-step); named slow joints <= 0.43 / 0.65
  expmap-smpl          (a) exact zeros; (b) angle / 1e-4 = 0.50 and 2.00, rate x dt / 1e-4 <= 0.007; (c) sine / 1e-5 = 0.50 before and 0.49 after the step;
                       (d) pi + 0.358 and pi + 2.842 in, 2.756 and 0.300 stored; (e) crosses pi by 0.160 rad; (f) PD error +3.09 -> +2.93 and -3.09 -> -3.00 along the axis
  effort-smpl          +-3.11, +-3.88, +-1.94 x the limit on the saturated axes, <= 0.16 on the unsaturated; 4 positive, 4 negative per state
  effort-smpl-aniso    1.16 .. 5.82 x the limit saturated (1.03 in a later sub-step: the clamp is continuous), <= 0.19 unsaturated
  effort-h1-m0/1/2     hip pitch +2.14, knee -1.43 x 350 N m (mirrored in state 1), 17 DoFs unsaturated; state 2: spring +60 N m against damper -450 N m, whole torque
                       -1.11 x the limit in the `pd` modes (mode 2 takes the sign from the whole torque), 0.17 in mode 0
  pdref-smpl / -h1     23 / 7 DoFs >= 1.08 x pi/2 above q, 23 / 6 <= -1.09 below, 23 / 6 within 0.19
  rigid-bounce-*       left foot 5.0 x the threshold (bounce target 2.1 / 1.25 x the depenetration target), right foot 0.5; every point in range >= 0.047 from the threshold
                       in every sub-step
  rigid-depen-*        right foot 30 mm deep: 3.6 / 3.5 x the cap; left foot 2 mm: 0.24 / 0.80
  rigid-spec-*         the left foot's nearest points (SMPL: its two heel corners, the feet pitched) 10 mm above the plane closing at 1.6 x gap / dt: they push (H1: 1.39
                       on the farthest pushing point); right foot 30 mm above: outside by 10 mm
  rigid-gate / pen-gate toe origin 5.00 mm under / over its gate; under it the farthest point pushes (15 mm above the plane closing at 3 m/s / 4.99 mm deep); over it no force
  pen-friction-*       left foot 2 m/s: cone / viscous 0.05 (slip); right foot 1 mm/s: 99.9 / 25 (stick)
  caps-smpl            interior pair 23.9 mm deep, s 0.85 t 0.94 (0.065 from a branch point); end-interior pair 28.5 mm, t -0.38 re-solved s 0.79 (0.21); end-end pair 11.3 mm,
                       t -1.03 re-solved s -0.66 (0.66); denom / (a e) >= 0.107
  caps-hi-smpl         end-interior pair through the t > 1 re-solve, 14.7 mm deep, t 1.71 re-solved s 0.63 (0.37); denom / (a e) 0.999
WIDER below holds every tolerance wider than test_dynamics.check_step_against's with the host-emulation error it was measured from (bound = 4 x the fp32 HOST EMULATION's
error against the fp64 recursion, measured on the CPU; never the HIP kernel's).  Every case also satisfies w_pair_coherence: the device kernel's documented pair skip.

LEFT OUT on purpose: the parallel-segment branch of seg_seg_closest (`denom <= 1e-7 a e`).  fp32 and fp64 cannot be made to take the same side of a 1e-7 relative
threshold with a margin: a e - b^2 of nearly parallel unit-length segments is a difference of two numbers that agree to seven digits, which fp32 does not carry.  Every
capsule case asserts denom / (a e) >= 1e-3 instead, three decades on the general side."""
from dataclasses import dataclass

import numpy as np

import dyn_oracle as do
import hostemu_util as hu
import stepper_edge_cases as ec
import wrench_util as wu
from backends import get_backend, model_on
from phc_amd import abi

F = np.float32
PI = np.pi


@dataclass(frozen=True)
class Regime:
    id: str
    model: str            # smpl_humanoid | smpl_aniso (backends.model_on(anisotropic=True)) | h1_humanoid | g1_humanoid
    make: str             # constructor in MAKE, witness in WITNESS
    opts: tuple = ()      # sim_params_struct keywords on top of stepper_edge_cases.params_of's (self_collision = 1, the robot switches)
    lags: tuple = (0,)    # inertia_lag values the backend rows run
    actions: str = ""     # "ref": through pd_ref (device only)
    what: str = ""

    @property
    def hip_only(self):
        return self.actions == "ref"


def _r(id, model, make, what, lags=(0,), actions="", **opts):
    return Regime(id, model, make, tuple(sorted(opts.items())), lags, actions, what)


RIGID = dict(contact_model="tgs")
TABLE = [
    _r("cap8-smpl", "smpl_humanoid", "cap8", "rate cap 8 rad/s, spherical: PD errors drive three joints above the cap, the rest stay below", (0, 1), max_angular_velocity=8.0),
    _r("cap8-smpl-occ3", "smpl_humanoid", "cap8", "the same through lane_mapping 3", (0,), max_angular_velocity=8.0, lane_mapping=3),
    _r("cap100-smpl", "smpl_humanoid", "cap100", "default cap 100 rad/s: two joints start far above it", (0, 1)),
    _r("cap8-h1", "h1_humanoid", "cap8", "rate cap 8 rad/s, revolute, `pd` mode 1", (0, 1), max_angular_velocity=8.0),
    _r("cap8-g1", "g1_humanoid", "cap8", "rate cap 8 rad/s, revolute, 64 lanes, `pd` mode 2", (1,), max_angular_velocity=8.0),
    _r("expmap-smpl", "smpl_humanoid", "expmap", "exp-map edges: exact zero, both sides of the two small-angle branches, |e| > pi, crossing pi, PD error around pi", (0, 1)),
    _r("effort-smpl", "smpl_humanoid", "effort", "effort clamp per axis, scalar gains: +, -, unsaturated on one joint", (0, 1)),
    _r("effort-smpl-aniso", "smpl_aniso", "effort", "effort clamp per axis, per-axis gains", (0, 1)),
    _r("effort-h1-m0", "h1_humanoid", "effort", "effort clamp, revolute, implicit drive", (1,), control_mode=0),
    _r("effort-h1-m1", "h1_humanoid", "effort", "effort clamp, revolute, held torque", (1,), control_mode=1),
    _r("effort-h1-m2", "h1_humanoid", "effort", "effort clamp, revolute, sampled spring (saturated: held)", (1,), control_mode=2),
    _r("pdref-smpl", "smpl_humanoid", "pdref", "pd_ref residual clamp to q +- pi/2", (1,), "ref"),
    _r("pdref-h1", "h1_humanoid", "pdref", "pd_ref residual clamp to q +- pi/2", (1,), "ref"),
    _r("rigid-bounce-smpl", "smpl_humanoid", "bounce", "rigid contact: one foot arrives at 1 m/s (bounces), the other at 0.1 m/s (below the threshold)", restitution=0.5, **RIGID),
    _r("rigid-bounce-h1", "h1_humanoid", "bounce", "the same, revolute", restitution=0.5, **RIGID),
    _r("rigid-depen-smpl", "smpl_humanoid", "depen", "rigid contact: one foot 3 cm deep (depenetration capped at 1 m/s), the other 2 mm", max_depenetration_velocity=1.0, **RIGID),
    _r("rigid-depen-h1", "h1_humanoid", "depen", "the same, revolute", max_depenetration_velocity=1.0, **RIGID),
    _r("rigid-spec-smpl", "smpl_humanoid", "spec", "rigid contact: one foot 1 cm above the plane closing at 1.6 x gap / dt (speculative, pushes), the other 3 cm above (no force)", **RIGID),
    _r("rigid-spec-h1", "h1_humanoid", "spec", "the same, revolute", **RIGID),
    _r("rigid-gate-smpl", "smpl_humanoid", "gate", "rigid contact: the left toe's origin 5 mm under (its farthest point pushes) / over the gate f[34] + contact_offset", **RIGID),
    _r("pen-gate-smpl", "smpl_humanoid", "gate", "penalty contact: the left toe's origin 5 mm under (its farthest point pushes) / over the gate f[34]", (0, 1)),
    _r("pen-friction-smpl", "smpl_humanoid", "friction", "penalty contact: one foot slides at 2 m/s (cone clamp), the other creeps at 1 mm/s (sticks)", (0, 1)),
    _r("pen-friction-h1", "h1_humanoid", "friction", "the same, revolute", (0, 1)),
    _r("caps-smpl", "smpl_humanoid", "capsules", "capsule pairs: interior-interior, end-interior (the t < 0 re-solve), end-end closest points, each penetrating", (0, 1)),
    _r("caps-hi-smpl", "smpl_humanoid", "capsules_hi", "capsule pair: end-interior through the t > 1 re-solve, penetrating", (0, 1)),
]
REGIMES = {r.id: r for r in TABLE}
ROWS = [(r.id, lag) for r in TABLE for lag in r.lags]

# Tolerances wider than check_step_against's.  {(id, lag): the error of the fp32 HOST EMULATION against the fp64 recursion, measured on the CPU, per quantity in units of
# check_step_against's tolerance for it (error_ratios below; the worst state of the case)}.  The bound of such a row is 4 x the measured value for every quantity, and
# never below check_step_against's own (1.0).  Rows not named here are held to check_step_against itself.
#   rigid-bounce-smpl: sixteen points of two flat feet under the rigid model, eight of them reversing 1 m/s with the impedance 1e5 N s/m -- forces of 4e4 N per point in
#   the first pass, of which the solve leaves ~1e3 N: three digits cancel in fp32.
WIDER = {("rigid-bounce-smpl", 0): dict(root=2.182, dofvel=0.918, dofpos=0.001, bodypos=0.036, bodyrot=0.045, bodyvel=0.680, df=1.463, cf=3.084)}


def wider(rid, lag):
    w = WIDER.get((rid, lag))
    return None if w is None else {k: (v, max(1.0, 4.0 * v)) for k, v in w.items()}


# ---- models, parameters -------------------------------------------------------------------------------------------------------------------------------------
def case_of(reg, lag, wrench=False, actions=None, **more):
    opts = dict(reg.opts)
    opts["inertia_lag"] = lag
    opts.update(more)
    return ec.Case(f"{reg.id}-lag{lag}", reg.model, tuple(sorted(opts.items())), "", False, wrench, reg.actions if actions is None else actions)


ec.MODEL_MAKERS["smpl_aniso"] = lambda be: model_on(be, anisotropic=True)


def models_on(be, reg):
    return ec.models_on(be, case_of(reg, 0))


def model_of(reg):
    return models_on(get_backend("hostemu"), reg)[0][0]


def params_of(reg, lag, **more):
    return ec.params_of(case_of(reg, lag, **more), [model_of(reg)])


def _header_constant(name):
    """A `#define NAME <float>f` of csrc/phc_aba.h, read from the header the stepper is built from."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "phc_amd", "csrc", "phc_aba.h")
    with open(path) as fh:
        found = re.findall(rf"^#define\s+{name}\s+([0-9.eE+-]+)f?\b", fh.read(), re.M)
    assert len(found) == 1, (name, found)
    return float(found[0])


FIXED_POINT = (_header_constant("PHC_SC_FSCALE"), _header_constant("PHC_SC_NSCALE"))   # force steps per N, moment steps per N m
SKIP_MARGIN = _header_constant("PHC_SC_SKIP_MARGIN")


def dense_params(prm):
    """The dense oracle's parameter dict holding exactly the numbers the C struct holds (test_dynamics.f32_params, plus the rigid contact model's)."""
    fl = ("gravity_z", "contact_stiffness", "contact_damping", "friction", "friction_viscous", "angular_damping", "max_angular_velocity", "limit_stiffness", "limit_damping",
          "self_stiffness_scale", "self_damping_ratio", "contact_impedance", "max_depenetration_velocity", "bounce_threshold_velocity", "restitution", "contact_offset")
    d = {k: float(getattr(prm, k)) for k in fl}
    d.update({k: int(getattr(prm, k)) for k in ("control_mode", "self_collision", "contact_model", "contact_iterations")})
    return d, float(prm.sim_dt), int(prm.substeps)


# ---- building blocks of the constructors --------------------------------------------------------------------------------------------------------------------
def smpl(model):
    return model.all_spherical


def dofs_of(model, body):
    """DoF indices of the joint of `body`."""
    j = list(model.body_names).index(body)
    return list(range(3 * (j - 1), 3 * j)) if smpl(model) else [int(model.dof_start[j])]


LEGS = {True: {"L": ("L_Hip", "L_Knee", "L_Ankle"), "R": ("R_Hip", "R_Knee", "R_Ankle")},
        False: {"L": ("left_hip_yaw_link", "left_hip_roll_link", "left_hip_pitch_link", "left_knee_link", "left_ankle_link"),
                "R": ("right_hip_yaw_link", "right_hip_roll_link", "right_hip_pitch_link", "right_knee_link", "right_ankle_link")}}
FEET = {True: {"L": ("L_Ankle", "L_Toe"), "R": ("R_Ankle", "R_Toe")}, False: {"L": ("left_ankle_link",), "R": ("right_ankle_link",)}}
PITCH = {True: {"L": ("L_Hip", "L_Knee", "L_Ankle"), "R": ("R_Hip", "R_Knee", "R_Ankle")},
         False: {"L": ("left_hip_pitch_link", "left_knee_link", "left_ankle_link"), "R": ("right_hip_pitch_link", "right_knee_link", "right_ankle_link")}}


def air(model, n, seed=3, quiet=False):
    """Benign states in the air (root 1.5 m up, upright, at rest): small pose, joint rates and PD errors (none with `quiet`)."""
    rng = np.random.default_rng(seed)
    nd = model.num_dof
    if smpl(model):
        root = np.zeros((n, 13))
        root[:, 2], root[:, 6] = 1.5, 1.0
        dof = np.zeros((n, nd, 2))
    else:
        root, dof, _ = (np.asarray(a, np.float64) for a in wu.robot_rest_state(model, n, 2.0))
    if not quiet:
        dof[:, :, 0] += rng.normal(0, 0.08, (n, nd))
        dof[:, :, 1] = rng.normal(0, 0.3, (n, nd))
    target = dof[:, :, 0] + (0 if quiet else rng.normal(0, 0.1, (n, nd)))
    return root, dof, target


def done(root, dof, target, **more):
    """The state dict of a case: fp32 tensors (what every backend and every reference reads)."""
    s = dict(root=np.asarray(root, F), dof=np.asarray(dof, F), target=np.asarray(target, F))
    s.update(more)
    return s


def frames(model, root_e, dof_e):
    st = do.State(np.asarray(root_e, np.float64), np.asarray(dof_e, np.float64), model)
    Q, R, p = do.kinematics(model, st)
    w, v = do.body_velocities(model, st, R, p)
    return R, p, w, v


def point_low(model, root_e, dof_e, bodies=None):
    """Height of the lowest surface point of every ground-contact point (of `bodies`: names; others +inf)."""
    R, p, _, _ = frames(model, root_e, dof_e)
    names = list(model.body_names)
    keep = None if bodies is None else {names.index(b) for b in bodies}
    return np.array([p[i][2] + (R[i] @ model.contact_pos[k])[2] - model.contact_radius[k] if keep is None or int(i) in keep else np.inf
                     for k, i in enumerate(model.contact_body)])


def squat(model, dof_e, side, phi):
    """Hip -phi, knee +2 phi, ankle -phi about the pitch axis: the foot stays flat under the hip."""
    for body, a in zip(PITCH[smpl(model)][side], (-phi, 2 * phi, -phi)):
        d = dofs_of(model, body)
        dof_e[d[1] if smpl(model) else d[0], 0] = a


def foot_rates(model, root_e, dof_e, side, v):
    """Joint rates of one leg (least squares, minimum norm) that give the foot body the linear velocity `v` at its origin and no angular velocity, the root at rest."""
    names = list(model.body_names)
    foot = names.index(FEET[smpl(model)][side][0])
    cols = [d for b in LEGS[smpl(model)][side] for d in dofs_of(model, b)]
    J = np.zeros((6, len(cols)))
    probe = np.array(dof_e, np.float64)
    probe[:, 1] = 0
    r0 = np.array(root_e, np.float64)
    r0[7:13] = 0
    for c, d in enumerate(cols):
        probe[d, 1] = 1.0
        _, _, w, vv = frames(model, r0, probe)
        J[:, c] = np.concatenate([vv[foot], w[foot]])
        probe[d, 1] = 0.0
    want = np.concatenate([np.asarray(v, np.float64), np.zeros(3)])
    x = np.linalg.lstsq(J, want, rcond=None)[0]
    assert np.abs(J @ x - want).max() < 1e-9, "the leg cannot produce this foot velocity"
    for c, d in enumerate(cols):
        dof_e[d, 1] = x[c]


def lower(model, root_e, dof_e, depth, bodies=None):
    """Moves the root vertically until the lowest contact point (of `bodies`) is `depth` inside the plane (negative: above it)."""
    root_e[2] -= point_low(model, root_e, dof_e, bodies).min() + depth


def standing(model, phi_l=0.4, phi_r=0.4):
    """One state: squatting on flat feet, at rest, PD targets at the pose, root at the origin height (use `lower`)."""
    root, dof, target = air(model, 1, quiet=True)
    squat(model, dof[0], "R", phi_r)
    if phi_l == phi_r:   # (the shipped SMPL shape is not symmetric: the left squat angle that puts both feet at one height)
        phi_l = foot_gap_angle(model, root, dof, "L", 0.0)
    squat(model, dof[0], "L", phi_l)
    return root, dof, dof[:, :, 0].copy()


def foot_gap_angle(model, root, dof, side, gap):
    """The squat angle of leg `side` (bisection, other leg as it is) at which its lowest foot point is `gap` above the other foot's; the leg is left at that angle."""
    other = "R" if side == "L" else "L"
    lo, hi = 0.2, 0.8
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        squat(model, dof[0], side, mid)
        g = point_low(model, root[0], dof[0], FEET[smpl(model)][side]).min() - point_low(model, root[0], dof[0], FEET[smpl(model)][other]).min()
        lo, hi = (mid, hi) if g < gap else (lo, mid)
    return mid


# ---- the constructors: -> state dict (1 to 3 states) ---------------------------------------------------------------------------------------------------------
def make_cap8(model):
    """Two states.  PD errors that drive named joints to a steady rate kp err / (kd + dt kp) far above 8 rad/s, others mildly (below), on top of a benign state."""
    root, dof, target = air(model, 2, seed=5)
    for e in range(2):
        for body, ax, err in CAP8[model_kind(model)]["fast"]:
            d = dofs_of(model, body)[ax]
            target[e, d] = dof[e, d, 0] + err * (1 if e == 0 else -1)
            if not smpl(model):
                dof[e, d, 1] = 20.0 * np.sign(err) * (1 if e == 0 else -1)   # (explicit `pd` drives: the rate is set, the torque keeps it)
        for body, ax, err in CAP8[model_kind(model)]["slow"]:
            d = dofs_of(model, body)[ax]
            target[e, d] = dof[e, d, 0] + err
        for body, ax, rate in CAP8[model_kind(model)].get("rate", ()):
            dof[e, dofs_of(model, body)[ax], 1] = rate * (1 if e == 0 else -1)
    return done(root, dof, target)


def model_kind(model):
    return "smpl" if smpl(model) else ("h1" if model.num_bodies == 20 else "g1")


# SMPL: the spring saturates at 500 N m, so a drive alone reaches 500 / (kd + dt kp): 5.8 rad/s at kp 800 and 15 rad/s at the wrists' and hands' kp 300 -- those are driven
# across the cap; the knee starts at 100 rad/s, of which the implicit damper leaves ~13 after the first sub-step.
CAP8 = {"smpl": dict(fast=[("L_Wrist", 1, 2.2), ("R_Hand", 0, -2.2), ("L_Knee", 1, 0.0)], slow=[("R_Knee", 1, 0.4), ("L_Elbow", 2, -0.3)], rate=[("L_Knee", 1, 100.0)]),
        "h1": dict(fast=[("left_knee_link", 0, 1.0), ("right_elbow_link", 0, -1.0), ("torso_link", 0, 0.8)],
                   slow=[("left_shoulder_pitch_link", 0, 0.2), ("left_elbow_link", 0, -0.2)]),
        "g1": dict(fast=[("left_knee_link", 0, 1.0), ("right_elbow_pitch_link", 0, -1.0), ("torso_link", 0, 0.8)],
                   slow=[("right_knee_link", 0, 0.2), ("left_elbow_pitch_link", 0, -0.2)])}
# (Chosen by a scan over every joint and axis: most joints at 300 rad/s either keep < 100 rad/s after the implicit damper of the first sub-step or -- the hips about y, the
# spine -- whip the rest of the body above 100 rad/s in the following sub-steps, where rate x dt ~ 1 and the explicit velocity-product terms of ANY first-order scheme
# amplify rounding tenfold per sub-step: such a state compares nothing; a swinging arm reaches the neck or the hip from beyond the kernel's pair skip margin
# (w_pair_coherence).  The two legs spreading end sub-step 0 at 126 and 138 rad/s, touch nothing and calm down afterwards.)
CAP100 = [("L_Hip", 0, 180.0), ("R_Hip", 0, -180.0)]


def make_cap100(model):
    """One state at the default cap: both hips start at 180 rad/s, the legs spreading (the implicit damper takes a third of it in the first sub-step; what is left is above 100)."""
    root, dof, target = air(model, 1, seed=6)
    for body, ax, rate in CAP100:
        dof[0, dofs_of(model, body)[ax], 1] = rate
    return done(root, dof, target)


EXPMAP = dict(zero="L_Wrist", series_lo=("R_Wrist", 5e-5), series_hi=("L_Elbow", 2e-4), near_identity=("R_Elbow", 1e-5),
              beyond_pi=("L_Shoulder", 3.5), near_two_pi=("R_Shoulder", 2 * PI - 0.3), crossing=("L_Knee", PI - 0.02, 6.0),
              err_below=("L_Hip", PI - 0.05), err_above=("R_Hip", PI + 0.05))
_AX = {"R_Wrist": (1.0, 0, 0), "L_Elbow": (0, 0.6, 0.8), "R_Elbow": (0, 0, 1.0), "L_Shoulder": (0.6, 0, 0.8), "R_Shoulder": (0, 1.0, 0), "L_Knee": (0, 1.0, 0),
       "L_Hip": (0, 0.8, 0.6), "R_Hip": (1.0, 0, 0)}


def make_expmap(model):
    """Three states, each otherwise at rest in the air with targets at the pose.  0 (quiet): (a) a joint at exactly 0 with rate 0, (b) |e| = 5e-5 and 2e-4 with rates of
    1e-3 rad/s, (c) |e| = 1e-5 held.  1: (d) |e| = 3.5 and 2 pi - 0.3 held at their rotation, (e) a joint at pi - 0.02 driven at +6 rad/s across pi.  2: (f) PD errors
    of pi - 0.05 and pi + 0.05 from the zero pose."""
    root, dof, target = air(model, 3, quiet=True)
    ax = {b: np.array(a) for b, a in _AX.items()}
    for key in ("series_lo", "series_hi", "near_identity"):
        b, ang = EXPMAP[key]
        d = dofs_of(model, b)
        dof[0, d, 0] = ang * ax[b]
        target[0, d] = dof[0, d, 0]
        if key != "near_identity":
            dof[0, d, 1] = 1e-3 * ax[b]
    for key in ("beyond_pi", "near_two_pi"):
        b, ang = EXPMAP[key]
        d = dofs_of(model, b)
        dof[1, d, 0] = ang * ax[b]
        target[1, d] = dof[1, d, 0]
    b, ang, rate = EXPMAP["crossing"]
    d = dofs_of(model, b)
    kp, kd = float(model.dof_kp[d[0]]), float(model.dof_kd[d[0]])
    dof[1, d, 0] = ang * ax[b]
    dof[1, d, 1] = rate * ax[b]
    target[1, d] = (ang + rate * (kd + kp / 120.0) / kp) * ax[b]   # (the PD error whose steady rate is `rate`)
    for key in ("err_below", "err_above"):
        b, ang = EXPMAP[key]
        target[2, dofs_of(model, b)] = ang * ax[b]
    return done(root, dof, target)


EFFORT = {"smpl": [("L_Hip", (2.5, -2.5, 0.1)), ("R_Knee", (-2.5, 0.1, 2.5)), ("Chest", (0.1, 2.5, -2.5)), ("L_Shoulder", (-2.5, 2.5, 0.1))],
          "h1": [("left_hip_pitch_link", (2.5,)), ("right_knee_link", (-2.5,))]}


def make_effort(model):
    """Two states (signs mirrored in the second; robots: a third, OPPOSED): targets +-2.5 rad away on chosen axes, 0.1 rad on the unsaturated one, from a benign state at rest."""
    root, dof, target = air(model, 2, seed=8)
    if smpl(model):
        dof[:, :, 0] = 0      # (the error of a spherical joint is the target's own rotation vector)
    dof[:, :, 1] *= 0.2
    target = dof[:, :, 0].copy()
    for e in range(2):
        for body, errs in EFFORT[model_kind(model)]:
            for d, err in zip(dofs_of(model, body), errs):
                target[e, d] = dof[e, d, 0] + err * (1 if e == 0 or abs(err) < 1 else -1)
    if not smpl(model):   # a third state: the damper term outweighs and opposes the spring of a saturated explicit drive
        r2, d2, t2 = air(model, 1, seed=8)
        d2[:, :, 1] *= 0.2
        t2 = d2[:, :, 0].copy()
        body, err, rate = OPPOSED
        d = dofs_of(model, body)[0]
        t2[0, d], d2[0, d, 1] = d2[0, d, 0] + err, rate
        root, dof, target = (np.concatenate([a, b]) for a, b in ((root, r2), (dof, d2), (target, t2)))
    return done(root, dof, target)


# kp 300, kd 7.5, limit 350 N m: spring +60 N m, damper -450 N m, whole torque -390 N m = -1.11 x the limit: `pd` modes 1 and 2 hold -350 N m, and mode 2 must take the
# sign from the whole torque, not from the spring; the implicit drive (mode 0) sees 0.17 x the limit
OPPOSED = ("left_hip_pitch_link", 0.2, 60.0)


def make_pdref(model):
    """Two states: pd_ref + scale action lands 2 rad above q on a third of the DoFs, 2 rad below on another third, within 0.3 rad on the rest."""
    rng = np.random.default_rng(9)
    root, dof, target = air(model, 2, seed=9)
    nd = model.num_dof
    q = np.asarray(dof[:, :, 0], F)
    want = np.where(np.arange(nd)[None] % 3 == 0, 2.0, np.where(np.arange(nd)[None] % 3 == 1, -2.0, 0.0)) + rng.uniform(-0.3, 0.3, (2, nd))
    want[1] = np.roll(want[1], 1)
    scale = rng.uniform(0.5, 1.5, nd).astype(F)
    act = rng.normal(0, 1.0, (2, nd)).astype(F)
    pd_ref = (q + want - scale[None] * act).astype(F)
    return done(root, dof, target, scale=scale, off=rng.normal(0, 0.1, nd).astype(F), act=act, pd_ref=pd_ref)


def make_bounce(model):
    root, dof, target = standing(model)
    foot_rates(model, root[0], dof[0], "L", (0, 0, -0.9))
    root[0, 9] = -0.1
    # (deep enough to be in contact by 1 mm and more, shallow enough that the bounce target 0.5 m/s exceeds the depenetration target depth / dt: 0.24 and 0.4 m/s)
    lower(model, root[0], dof[0], 0.002 if smpl(model) else 0.001)
    return done(root, dof, target)


def make_depen(model):
    root, dof, target = standing(model)
    foot_gap_angle(model, root, dof, "L", 0.028)
    target = dof[:, :, 0].copy()
    lower(model, root[0], dof[0], 0.030)
    return done(root, dof, target)


def make_spec(model):
    """One point 1 cm above the plane: the feet are pitched by 0.3 rad (SMPL; as stepper_edge_cases.heel_states does), so that the two heel corners of the left foot are its
    lowest points and the rest of it hangs up to 4 cm higher.  (With the foot flat all eight of its points push at once: eight coplanar constraints on one 1.5 kg body,
    each with the impedance dt c = 833 kg, are redundant, and what fp32 makes of the sub-step then sits at 0.2 to 0.9 of check_step_against's tolerance on the host
    emulation, whichever way it is compiled -- the state, not the regime, would decide whether an fp32 build passes.)"""
    root, dof, target = standing(model)
    if smpl(model):
        for body in ("L_Ankle", "R_Ankle"):
            dof[0, dofs_of(model, body)[1], 0] -= 0.3
    foot_gap_angle(model, root, dof, "R", 0.020)
    target = dof[:, :, 0].copy()
    # the whole body moves down at 1.6 x gap / dt, so that the speculative point has to push to close no more than its gap (a foot driven by joint rates alone is
    # stopped by the drives' own dampers within the sub-step and never needs the contact)
    root[0, 9] = -1.6 * 0.010 / (0.5 / (60.0 if smpl(model) else 200.0))
    lower(model, root[0], dof[0], -0.010)
    return done(root, dof, target)


def gate_bound(model, body):
    """f[34] of the body as the fp32 model table holds it."""
    _, fl = model.pack(1.0, 1.0)
    return float(np.asarray(fl).reshape(-1)[:model.num_bodies * 56].reshape(model.num_bodies, 56)[list(model.body_names).index(body), 34])


GATE_BODY = "L_Toe"   # a leaf: nothing hangs below it


def make_gate(model, offset=0.0):
    """Two states, legs straight, the left toe turned so that its contact point farthest from the origin points straight down -- the deepest any point of the body can
    reach, which is what the gate bounds; toe origin 5 mm under the gate (state 0, moving down: at 0.1 m/s, or -- rigid model, where that point is then 15 mm above the
    plane -- at 3 m/s, so that it has to push) and 5 mm over it (state 1, moving up at 0.5 m/s so that gravity does not bring it back inside the launch)."""
    root, dof, target = air(model, 2, quiet=True)
    names = list(model.body_names)
    j = names.index(GATE_BODY)
    ks = [k for k, i in enumerate(model.contact_body) if int(i) == j]
    k = max(ks, key=lambda k: np.linalg.norm(model.contact_pos[k]) + model.contact_radius[k])
    c = np.asarray(model.contact_pos[k], np.float64)
    u = c / np.linalg.norm(c)
    axis, ang = np.cross(u, [0, 0, -1.0]), np.arccos(np.clip(-u[2], -1, 1))   # the rotation that takes u to -z (every parent is at the identity)
    dof[:, dofs_of(model, GATE_BODY), 0] = (axis / np.linalg.norm(axis) * ang)[None]
    target = dof[:, :, 0].copy()
    for e, (dz, vz) in enumerate(((-0.005, -3.0 if offset else -0.1), (0.005, 0.5))):
        _, p, _, _ = frames(model, root[e], dof[e])
        root[e, 2] += gate_bound(model, GATE_BODY) + offset + dz - p[j][2]
        root[e, 9] = vz
    return done(root, dof, target)


def make_friction(model):
    root, dof, target = standing(model)
    foot_rates(model, root[0], dof[0], "L", (2.0, 0, 0))
    foot_rates(model, root[0], dof[0], "R", (1e-3, 0, 0))
    lower(model, root[0], dof[0], 0.002)
    return done(root, dof, target)


# the closest-point regimes of the two capsule cases: end_t is split by which re-solve it takes
CAPS_KINDS = {"capsules": ("interior", "end_t<0", "end_end"), "capsules_hi": ("end_t>1",)}


def pair_kind(p):
    return p["kind"] if p["kind"] != "end_t" else ("end_t<0" if p["t_raw"] < 0 else "end_t>1")


def pair_margin(p):
    """Distance of a recorded capsule pair from its branch points: min over the parameters that decided its kind."""
    vals = [p["s_raw"], p["t_raw"]] + ([p["s2_raw"]] if p["s2_raw"] is not None else [])
    return min(min(abs(x), abs(x - 1.0)) for x in vals if x is not None)


def make_capsules(model, kinds=CAPS_KINDS["capsules"]):
    """One state per kind, found by a fixed-seed search over poses at rest in the air (targets at the pose): state i holds a pair of kind kinds[i] that penetrates by more
    than 3 mm, and every pair of the state that penetrates or comes within 3 mm sits >= 0.03 from its branch points and >= 1e-2 from parallel."""
    rng = np.random.default_rng(12)
    found = {}
    prm = dict(do.DEFAULT_PARAMS, self_collision=1)
    for _ in range(3000):
        root, dof, target = air(model, 1, quiet=True)
        dof[0, :, 0] = rng.normal(0, 0.55, model.num_dof)
        R, p, w, v = frames(model, root[0], dof[0])
        rec = []
        do.self_collision_wrenches(model, R, p, w, v, prm, 1 / 120, rec)
        near = [q for q in rec if q["pen"] > -0.003]
        if not near or any(abs(q["pen"]) < 0.003 or pair_margin(q) < 0.03 or q["par"] < 1e-2 or q["pen"] > 0.04 for q in near):
            continue
        for kind in kinds:
            if kind not in found and any(pair_kind(q) == kind for q in near):
                found[kind] = (root, dof, dof[:, :, 0].copy())
                break
        if len(found) == len(kinds):
            break
    assert len(found) == len(kinds), f"the search found only {sorted(found)}"
    return done(*(np.concatenate([found[k][i] for k in kinds]) for i in range(3)))


MAKE = dict(cap8=make_cap8, cap100=make_cap100, expmap=make_expmap, effort=make_effort, pdref=make_pdref, bounce=make_bounce, depen=make_depen, spec=make_spec,
            gate=make_gate, friction=make_friction, capsules=make_capsules, capsules_hi=lambda model: make_capsules(model, CAPS_KINDS["capsules_hi"]))


def states(reg):
    def make():
        m = model_of(reg)
        if reg.make == "gate":
            return make_gate(m, 0.02 if dict(reg.opts).get("contact_model") == "tgs" else 0.0)
        return MAKE[reg.make](m)
    return ec.cached(("regime-states", reg.model, reg.make, reg.id if reg.make == "gate" else ""), make)


def formed_target(reg, s):
    """The PD target a launch of the case forms (bit for bit): the target handed over, or stepper_edge_cases.formula_targets' formula with pd_ref."""
    if reg.actions != "ref":
        return s["target"]
    sa = (s["scale"][None] * s["act"]).astype(F)
    half_pi, q = F(1.57079637), s["dof"][:, :, 0]
    return np.maximum(np.minimum((s["pd_ref"] + sa).astype(F), (q + half_pi).astype(F)), (q - half_pi).astype(F))


# ---- references ------------------------------------------------------------------------------------------------------------------------------------------------
def reference(reg, lag, wrench=False, target=None):
    """The fp64 build of the recursion on the case's states, with the target the launch forms (`target`: the one a launch through actions formed)."""
    def make():
        s = states(reg)
        n = s["root"].shape[0]
        m = model_of(reg)
        kw = dict(force=np.zeros((n, m.num_bodies, 3)), torque=np.zeros((n, m.num_bodies, 3)), wrench_sim_calls=1) if wrench else {}
        return hu.host_sim_step(m, params_of(reg, lag), s["root"], s["dof"], formed_target(reg, s) if target is None else target, 2, f64=True, **kw)
    return ec.cached(("regime-f64", reg.id, lag, wrench, target is not None), make)


def dense(reg):
    """The dense oracle on the case's states with the case's parameters at inertia_lag 0: [(root, dof, rbs, tau, fc)], [trace].  Body-body forces in the stepper's fixed
    point (dyn_oracle.DEFAULT_PARAMS self_force_fixed_point): with floating-point sums a state with a touching capsule pair -- H1's rest pose has some -- is 1e-3 to
    2e-2 of the stepper's tolerances from the fp64 recursion, with them 1e-9."""
    def make():
        s = states(reg)
        m = model_of(reg)
        dp, sim_dt, substeps = dense_params(params_of(reg, 0))
        dp["self_force_fixed_point"] = FIXED_POINT
        tgt = formed_target(reg, s)
        outs, traces = [], []
        for e in range(s["root"].shape[0]):
            tr = {}
            outs.append(do.sim_step(m, s["root"][e], s["dof"][e], tgt[e], params=dp, sim_dt=sim_dt, substeps=substeps, num_sim_calls=2, trace=tr))
            traces.append(tr["substeps"])
        return outs, traces
    return ec.cached(("regime-dense", reg.model, reg.make, reg.opts), make)


def error_ratios(model, out, ref):
    """Every comparison of test_dynamics.check_step_against as error / its tolerance (<= 1: check_step_against passes)."""
    o = {k: np.asarray(out[k], np.float64) for k in ("root", "dof", "rbs", "df", "cf")}
    rel = lambda a, b, atol, rtol: float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())
    r = dict(root=rel(o["root"], ref["root"], 3e-4, 1e-4), dofvel=rel(o["dof"][:, 1], ref["dof"][:, 1], 3e-3, 1e-3))
    if model.all_spherical:
        qa = np.array([do.quat_from_rotvec(o["dof"][3 * j:3 * j + 3, 0]) for j in range(model.num_bodies - 1)])
        qb = np.array([do.quat_from_rotvec(np.asarray(ref["dof"][3 * j:3 * j + 3, 0], np.float64)) for j in range(model.num_bodies - 1)])
        r["dofpos"] = float(np.abs(np.abs((qa * qb).sum(-1)) - 1).max() / (1e-6 + 1e-12))
    else:
        r["dofpos"] = rel(o["dof"][:, 0], ref["dof"][:, 0], 3e-4, 0)
    r["bodypos"] = rel(o["rbs"][:, 0:3], ref["rbs"][:, 0:3], 3e-4, 0)
    r["bodyrot"] = float(np.abs(np.abs((o["rbs"][:, 3:7] * ref["rbs"][:, 3:7]).sum(-1)) - 1).max() / (1e-5 + 1e-12))
    r["bodyvel"] = rel(o["rbs"][:, 7:13], ref["rbs"][:, 7:13], 3e-3, 1e-3)
    r["df"] = rel(o["df"], ref["df"], 0.15, 2e-3)
    r["cf"] = rel(o["cf"], ref["cf"], 0.5, 5e-3)
    return r


def assert_close(model, out, ref, e, tag, wide=None):
    """Env e of `out` against env e of `ref`: check_step_against itself, or -- for a row of WIDER -- its comparisons with the named quantities' bounds."""
    from test_dynamics import check_step_against
    o = {k: out[k][e] for k in ("root", "dof", "rbs", "df", "cf")}
    r = {k: ref[k][e] for k in ("root", "dof", "rbs", "df", "cf")}
    ratios = error_ratios(model, o, r)
    print(f"{tag} env {e}: error / tolerance " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    if wide is None:
        check_step_against(model, o, r["root"], r["dof"], r["rbs"], r["df"], r["cf"], f"{tag} env {e}")
        return ratios
    for k, v in ratios.items():
        bound = wide[k][1] if k in wide else 1.0
        assert v <= bound, f"{tag} env {e}: {k} is {v:.3f} x check_step_against's tolerance, bound {bound}"
    return ratios


# ---- launches ---------------------------------------------------------------------------------------------------------------------------------------------------
def launch_states(reg, s, wrench=False, through_actions=False):
    """The state dict stepper_edge_cases.launch reads for this way of launching: only the tensors the launch is handed."""
    d = dict(root=s["root"], dof=s["dof"], target=s["target"])
    n, m = s["root"].shape[0], model_of(reg)
    if reg.actions == "ref":
        d.update(act=s["act"], scale=s["scale"], off=s["off"], pd_ref=s["pd_ref"])
    elif through_actions:   # offset + scale * action ~ the target, no DoF frozen: what phc_sim_is_plain asks of the arguments
        rng = np.random.default_rng(23)
        scale, off = rng.uniform(0.5, 1.5, m.num_dof).astype(F), rng.normal(0, 0.1, m.num_dof).astype(F)
        d.update(scale=scale, off=off, act=((s["target"] - off[None]) / scale[None]).astype(F), freeze=np.zeros(m.num_dof, np.int32))
    if wrench:
        d.update(force=np.zeros((n, m.num_bodies, 3), F), torque=np.zeros((n, m.num_bodies, 3), F))
    return d


def action_target(d):
    return (d["off"][None] + (d["scale"][None] * d["act"]).astype(F)).astype(F)


def launch(be, reg, lag, s, rows, wrench=False, through_actions=False):
    """One launch with state rows[e] of `s` in env e -> {tensor: array}; guards and read-only tensors checked (stepper_edge_cases.launch)."""
    models_on(be, reg)
    case = case_of(reg, lag, wrench, "plain" if through_actions else None)
    rc, out, wrong = ec.launch(be, case, rows, states=launch_states(reg, s, wrench, through_actions))
    assert rc == 0, (reg.id, rc)
    assert not wrong, wrong
    return out


def is_plain(be, reg, lag, n=1):
    """phc_sim_is_plain for a launch of the case through actions and a freeze mask (the predicate reads pointers and fields only)."""
    m, ms = model_of(reg), models_on(be, reg)[1]
    t = {k: be.zeros(sh) for k, sh in dict(root=(n, 13), dof=(n, m.num_dof, 2), rbs=(n, m.num_bodies, 13), cf=(n, m.num_bodies, 3), df=(n, m.num_dof), pd=(n, m.num_dof)).items()}
    sim = abi.sim_state_struct(n, t["root"], t["dof"], t["rbs"], t["cf"], t["df"], t["pd"])
    act, frz = be.zeros((n, m.num_dof)), be.zeros((m.num_dof,), np.int32)
    return bool(be.lib.phc_sim_is_plain(ms, params_of(reg, lag), sim, abi.ptr(act), abi.ptr(frz), 2))


BENIGN = {"smpl_humanoid": "smpl-lag", "smpl_aniso": "smpl-lag", "h1_humanoid": "h1-lag", "g1_humanoid": "g1-lag"}


def beside_benign(reg, e):
    """State e of the case followed by two benign states of stepper_edge_cases.states_of (the random near-ground states of the model's lagged row)."""
    s, b = states(reg), ec.states_of(ec.CASES[BENIGN[reg.model]])
    d = {k: np.concatenate([s[k][e:e + 1], b[k][0:2]]) for k in ("root", "dof", "target")}
    if reg.actions == "ref":
        rng = np.random.default_rng(29)
        act = rng.normal(0, 0.15, (2, s["act"].shape[1])).astype(F)
        d.update(scale=s["scale"], off=s["off"], act=np.concatenate([s["act"][e:e + 1], act]),
                 pd_ref=np.concatenate([s["pd_ref"][e:e + 1], (b["target"][0:2] - s["scale"][None] * act).astype(F)]))
    return d


# ---- witnesses: -> lines "what: value (margin)"; assert the regime and its margin -----------------------------------------------------------------------------
class Lines(list):
    """The margins of a case as text; printed as they are found, so that a failing margin check shows what it had seen."""

    def append(self, line):
        print("    " + line)
        super().append(line)


def _side(x, lo=0.95, hi=1.05):
    assert not lo < x < hi, f"{x} sits between {lo} and {hi} of its branch point"
    return x >= hi


def joint_index(model, body):
    return list(model.body_names).index(body) - 1


def w_cap8(reg, s, traces, ref):
    m, lines = model_of(reg), Lines()
    spec = CAP8[model_kind(m)]
    for e, tr in enumerate(traces):
        capped = set()
        for k, sub in enumerate(tr):
            rr = sub["rate_ratio"]
            for body, _, _ in spec["fast"] + spec["slow"]:
                if rr[joint_index(m, body)] >= 1.05:
                    capped.add(body)
            lines.append(f"state {e} sub-step {k}: rate / cap of the named joints " + " ".join(f"{b} {rr[joint_index(m, b)]:.2f}" for b, _, _ in spec["fast"] + spec["slow"])
                         + f"; all joints: {int((rr > 1).sum())} capped, closest to the cap {rr[np.abs(rr - 1).argmin()]:.3f}")
        assert all(any(t["rate_ratio"][joint_index(m, b)] >= 1.05 for t in tr) for b, _, _ in spec["fast"]), "a fast joint never reaches the cap"
        assert all(all(t["rate_ratio"][joint_index(m, b)] <= 0.95 for t in tr) for b, _, _ in spec["slow"]), "a slow joint reaches the cap"
        assert capped and any((t["rate_ratio"] > 1.05).any() and (t["rate_ratio"] < 0.95).any() for t in tr), "capped and uncapped joints in one env"
    return lines


def w_cap100(reg, s, traces, ref):
    m, lines = model_of(reg), Lines()
    rr = traces[0][0]["rate_ratio"]
    for body, _, _ in CAP100:
        lines.append(f"sub-step 0: {body} rate / cap {rr[joint_index(m, body)]:.3f}")
        assert rr[joint_index(m, body)] >= 1.05
    others = np.delete(rr, [joint_index(m, b) for b, _, _ in CAP100])
    lines.append(f"sub-step 0: the other joints at most {others.max():.3f}; later sub-steps " + " ".join(f"{t['rate_ratio'].max():.3f}" for t in traces[0][1:]))
    assert others.max() <= 0.95
    assert max(t["rate_ratio"].max() for t in traces[0]) < 2.0 and traces[0][-1]["rate_ratio"].max() < 0.95, "the state calms down inside the launch"
    return lines


def _joint_e(x, model, body):
    return np.asarray(x, np.float64)[dofs_of(model, body)]


def w_expmap(reg, s, traces, ref):
    m, lines = model_of(reg), Lines()
    dt = float(params_of(reg, 0).sim_dt) / 2
    inp, out = s["dof"].astype(np.float64), np.asarray(ref["dof"], np.float64)
    b = EXPMAP["zero"]
    assert (_joint_e(inp[0, :, 0], m, b) == 0).all() and (_joint_e(inp[0, :, 1], m, b) == 0).all() and (_joint_e(s["target"][0], m, b) == 0).all()
    lines.append(f"(a) {b}: exp-map, rate and target exactly 0; after the step |e| {np.linalg.norm(_joint_e(out[0, :, 0], m, b)):.2e}")
    for key, small in (("series_lo", True), ("series_hi", False)):
        b, ang = EXPMAP[key]
        a = np.linalg.norm(_joint_e(inp[0, :, 0], m, b))
        lines.append(f"(b) {b}: input angle / 1e-4 = {a / 1e-4:.3f} ({'series' if small else 'quotient'} side), sine / 1e-5 = {np.sin(a / 2) / 1e-5:.2f}")
        assert (a / 1e-4 <= 0.55) if small else (a / 1e-4 >= 1.9)
        assert np.sin(a / 2) / 1e-5 >= 2.0
    rates = np.array([t["rate_ratio"] for t in traces[0]]) * float(params_of(reg, 0).max_angular_velocity)
    lines.append(f"(b) quiet state: largest rate x dt over all joints and sub-steps / 1e-4 = {rates.max() * dt / 1e-4:.4f} (the integrator's rotation vector stays on the series side)")
    assert rates.max() * dt / 1e-4 <= 0.5 and rates.max() > 0
    b, ang = EXPMAP["near_identity"]
    for name, x in (("input", inp[0, :, 0]), ("after the step", out[0, :, 0])):
        sn = np.sin(np.linalg.norm(_joint_e(x, m, b)) / 2)
        lines.append(f"(c) {b} {name}: sine / 1e-5 = {sn / 1e-5:.3f} (small side)")
        assert 0 < sn / 1e-5 <= 0.6
    for key in ("beyond_pi", "near_two_pi"):
        b, ang = EXPMAP[key]
        a_in, a_out = np.linalg.norm(_joint_e(inp[1, :, 0], m, b)), np.linalg.norm(_joint_e(out[1, :, 0], m, b))
        lines.append(f"(d) {b}: input |e| {a_in:.4f} = pi + {a_in - PI:.3f}: the quaternion's w is negative; stored |e| {a_out:.4f} = 2 pi - {2 * PI - a_out - 0:.4f}")
        assert a_in - PI >= 0.04 and abs((2 * PI - a_out) - a_in) < 0.1 and a_out <= PI - 0.04
    b, ang, rate = EXPMAP["crossing"]
    e_in, e_out = _joint_e(inp[1, :, 0], m, b), _joint_e(out[1, :, 0], m, b)
    ax = e_in / np.linalg.norm(e_in)
    lines.append(f"(e) {b}: input angle pi - {PI - np.linalg.norm(e_in):.3f}, rate {rate}; stored e along the input axis {e_out @ ax:.4f} = -(pi - {PI + e_out @ ax:.4f}): crossed pi by "
                 f"{PI + e_out @ ax:.4f} rad")
    assert PI - np.linalg.norm(e_in) >= 0.019 and e_out @ ax < 0 and PI + e_out @ ax >= 0.04
    for key, sign in (("err_below", 1.0), ("err_above", -1.0)):
        b, ang = EXPMAP[key]
        d = dofs_of(m, b)
        axv = np.array(_AX[b])
        er = np.array([t["effort_ratio"][d] for t in traces[2]]) * float(m.dof_effort[d[0]]) / float(m.dof_kp[d[0]])   # the PD error per sub-step (rad)
        along = er @ axv
        lines.append(f"(f) {b}: target angle pi {'-' if ang < PI else '+'} 0.05; PD error along the target axis per sub-step " + " ".join(f"{x:.4f}" for x in along))
        assert (np.sign(along) == sign).all() and (np.abs(along) <= PI - 0.04).all() and abs(abs(along[0]) - (PI - 0.05)) < 1e-6
    return lines


def w_effort(reg, s, traces, ref):
    m, lines = model_of(reg), Lines()
    if len(traces) == 3:
        body, err, rate = OPPOSED
        d = dofs_of(m, body)[0]
        r = traces[2][0]["effort_ratio"][d]
        mode = int(params_of(reg, 0).control_mode)
        lines.append(f"state 2 {body}: spring {float(m.dof_kp[d]) * err:+.0f} N m, damper {-float(m.dof_kd[d]) * rate:+.0f} N m; torque / limit in sub-step 0 {r:+.3f} (control mode {mode})")
        assert float(m.dof_kp[d]) * err > 0 and ((r <= -1.05) if mode else (0 < r <= 0.95))
    for e, tr in enumerate(traces[:2]):
        closest = np.inf
        for body, errs in EFFORT[model_kind(m)]:
            d = dofs_of(m, body)
            for k, sub in enumerate(tr):
                r = sub["effort_ratio"][d]
                if k == 0:
                    lines.append(f"state {e} {body}: torque / limit per axis, sub-step 0: " + " ".join(f"{x:+.2f}" for x in r))
                    assert (np.abs(r) >= 1.05).sum() == sum(abs(x) > 1 for x in errs) and (np.abs(r) <= 0.95).sum() == sum(abs(x) < 1 for x in errs)
                    if len(errs) == 3:
                        assert (r >= 1.05).any() and (r <= -1.05).any()
                closest = min(closest, float(np.abs(np.abs(r) - 1).min()))
        r0 = tr[0]["effort_ratio"]
        lines.append(f"state {e}: over all sub-steps the named DoFs stay >= {closest:.3f} from the limit (the clamp is continuous there: asserted at sub-step 0 only)")
        lines.append(f"state {e}: saturated DoFs in sub-step 0: {int((r0 >= 1.05).sum())} positive, {int((r0 <= -1.05).sum())} negative, {int((np.abs(r0) <= 0.95).sum())} unsaturated")
        assert (r0 >= 1.05).any() and (r0 <= -1.05).any() and not ((np.abs(r0) > 0.95) & (np.abs(r0) < 1.05)).any()
    return lines


def w_pdref(reg, s, traces, ref):
    q = s["dof"][:, :, 0].astype(np.float64)
    r = (s["pd_ref"].astype(np.float64) + s["scale"].astype(np.float64)[None] * s["act"] - q) / (PI / 2)
    lines = Lines()
    for e in range(r.shape[0]):
        up, dn, mid = r[e] >= 1.05, r[e] <= -1.05, np.abs(r[e]) <= 0.95
        lines.append(f"state {e}: (pd_ref + scale action - q) / (pi / 2): {int(up.sum())} DoFs above (>= {r[e][up].min():.2f}), {int(dn.sum())} below (<= {r[e][dn].max():.2f}), "
                     f"{int(mid.sum())} inside (|.| <= {np.abs(r[e][mid]).max():.2f})")
        assert up.sum() >= 3 and dn.sum() >= 3 and mid.sum() >= 3 and (up | dn | mid).all()
    t = formed_target(reg, s)
    assert (np.abs(np.abs(t - s["dof"][:, :, 0]) - F(1.57079637)) < 1e-6).sum() >= 6, "the clamp is active"
    return lines


def _foot_points(model, side):
    names = list(model.body_names)
    bodies = {names.index(b) for b in FEET[smpl(model)][side]}
    return lambda c: c["body"] in bodies


def _all_bounce_margins(traces):
    worst = np.inf
    for tr in traces:
        for sub in tr:
            for c in sub["contacts"]:
                if c.get("bounce_ratio") is not None and c["kind"] != "outside":
                    _side(c["bounce_ratio"], 0.97, 1.03)
                    worst = min(worst, abs(c["bounce_ratio"] - 1))
    return worst


def w_bounce(reg, s, traces, ref):
    m, sub = model_of(reg), traces[0][0]
    L, R = [c for c in sub["contacts"] if _foot_points(m, "L")(c) and c["active"]], [c for c in sub["contacts"] if _foot_points(m, "R")(c) and c["active"]]
    lines = Lines()
    lines.append(f"sub-step 0: left foot {len(L)} pushing points, approach / threshold {min(c['bounce_ratio'] for c in L):.2f} .. {max(c['bounce_ratio'] for c in L):.2f}, bounce target / "
             f"depenetration target >= {min(c['bounce_over_depen'] for c in L):.2f}; right foot {len(R)} pushing points, {min(c['bounce_ratio'] for c in R):.2f} .. {max(c['bounce_ratio'] for c in R):.2f}")
    assert L and R and all(c["bounced"] and c["bounce_ratio"] >= 1.05 and c["bounce_over_depen"] >= 1.05 for c in L) and all(not c["bounced"] and c["bounce_ratio"] <= 0.95 for c in R)
    lines.append(f"all sub-steps, all points in range: |approach / threshold - 1| >= {_all_bounce_margins(traces):.3f}")
    return lines


def w_depen(reg, s, traces, ref):
    m, sub = model_of(reg), traces[0][0]
    L, R = [c for c in sub["contacts"] if _foot_points(m, "L")(c) and c["active"]], [c for c in sub["contacts"] if _foot_points(m, "R")(c) and c["active"]]
    lines = Lines()
    lines.append(f"sub-step 0: right foot {len(R)} pushing points {min(c['depth'] for c in R) * 1e3:.1f} .. {max(c['depth'] for c in R) * 1e3:.1f} mm deep, (depth / dt) / cap >= "
             f"{min(c['depen_ratio'] for c in R):.2f}; left foot {len(L)} points {min(c['depth'] for c in L) * 1e3:.1f} .. {max(c['depth'] for c in L) * 1e3:.1f} mm, <= {max(c['depen_ratio'] for c in L):.2f}")
    assert L and R and all(c["depen_capped"] and c["depen_ratio"] >= 1.05 for c in R) and all(not c["depen_capped"] and c["depen_ratio"] <= 0.95 for c in L)
    assert max(c["depth"] for c in R) > 0.029 and any(0.001 <= c["depth"] <= 0.0021 for c in L)
    return lines


def w_spec(reg, s, traces, ref):
    m, lines = model_of(reg), Lines()
    off, dt = float(params_of(reg, 0).contact_offset), float(params_of(reg, 0).sim_dt) / 2
    sub = traces[0][0]
    L = [c for c in sub["contacts"] if _foot_points(m, "L")(c) and c["kind"] == "speculative"]
    lines.append(f"sub-step 0: left foot {len(L)} speculative points {-max(c['depth'] for c in L) * 1e3:.1f} .. {-min(c['depth'] for c in L) * 1e3:.1f} mm above the plane, "
                 f"{sum(c['active'] for c in L)} of them push")
    assert L and any(c["active"] for c in L) and all(-off + 0.001 <= c["depth"] <= -0.001 for c in L if c["active"])
    act = [c for c in L if c["active"]]
    lines.append(f"sub-step 0: approach speed / (gap / dt) of the pushing points >= {min(c['approach'] / (-c['depth'] / dt) for c in act):.2f}")
    assert all(c["approach"] / (-c["depth"] / dt) >= 1.05 for c in act)
    assert any(abs(c["depth"] + 0.010) < 1e-4 for c in L)
    Rp = [c for c in sub["contacts"] if _foot_points(m, "R")(c)]
    assert Rp and all(c["kind"] == "outside" and c["depth"] <= -off - 0.001 for c in Rp) and abs(max(c["depth"] for c in Rp) + 0.030) < 1e-4
    lines.append(f"sub-step 0: right foot {len(Rp)} points, all outside, the nearest {-max(c['depth'] for c in Rp) * 1e3:.1f} mm above the plane (offset {off * 1e3:.0f} mm); it comes "
                 f"into range in sub-step {next((k for k, t in enumerate(traces[0]) if any(_foot_points(m, 'R')(c) and c['kind'] != 'outside' for c in t['contacts'])), None)}: "
                 "test_point_outside_the_contact_offset_carries_no_force launches sub-step 0 alone")
    return lines


def w_gate(reg, s, traces, ref):
    m, lines = model_of(reg), Lines()
    rigid = dict(reg.opts).get("contact_model") == "tgs"
    names = list(m.body_names)
    for e, (want, label) in enumerate(((-0.005, "under"), (0.005, "over"))):
        for body in (GATE_BODY,):
            j = names.index(body)
            gate = gate_bound(m, body) + (float(params_of(reg, 0).contact_offset) if rigid else 0.0)
            _, p, _, _ = frames(m, s["root"][e], s["dof"][e])
            z_in, z_out = p[j][2] - gate, float(np.asarray(ref["rbs"])[e, j, 2]) - gate
            pts = [c for c in traces[e][0]["contacts"] if c["body"] == j]
            lines.append(f"state {e} {body}: origin - gate {z_in * 1e3:+.2f} mm at the start, {z_out * 1e3:+.2f} mm after the step (fp64 recursion); sub-step 0: deepest point "
                         f"{max(c['depth'] for c in pts) * 1e3:+.2f} mm, {sum(c['active'] for c in pts)} pushing")
            assert abs(z_in - want) < 1e-3 and abs(z_in) >= 0.004, f"{label}: not on its side by 4 mm"
            assert e == 0 or z_out >= 0.004, "over the gate for the whole launch"
            if e == 0:
                assert any(c["active"] for c in pts) and (rigid or max(c["depth"] for c in pts) >= 0.004), "under the gate the farthest point pushes"
            else:
                assert not any(c["active"] for c in pts) and (np.asarray(ref["cf"])[e, j] == 0).all()
    return lines


def w_friction(reg, s, traces, ref):
    m, sub = model_of(reg), traces[0][0]
    L, R = [c for c in sub["contacts"] if _foot_points(m, "L")(c) and c["active"]], [c for c in sub["contacts"] if _foot_points(m, "R")(c) and c["active"]]
    lines = Lines()
    lines.append(f"sub-step 0: left foot {len(L)} pushing points slide at {min(c['slip_speed'] for c in L):.3f} .. {max(c['slip_speed'] for c in L):.3f} m/s, cone / viscous <= "
             f"{max(c['cone_ratio'] for c in L):.3f} (slip); right foot {len(R)} points creep at {max(c['slip_speed'] for c in R) * 1e3:.3f} mm/s, cone / viscous >= {min(c['cone_ratio'] for c in R):.1f} (stick)")
    assert L and R and all(c["friction"] == "slip" and c["cone_ratio"] <= 0.95 for c in L) and all(c["friction"] == "stick" and c["cone_ratio"] >= 1.05 for c in R)
    return lines


def w_capsules(reg, s, traces, ref):
    lines = Lines()
    for e, kind in enumerate(CAPS_KINDS[reg.make]):
        for k, sub in enumerate(traces[e]):
            pen = [p for p in sub["pairs"] if p["pen"] > 0]
            if k == 0:
                mine = [p for p in pen if pair_kind(p) == kind]
                assert mine, f"state {e}: no penetrating {kind} pair"
                for p in mine:
                    lines.append(f"state {e}: {kind} pair {p['shapes']} penetrates {p['pen'] * 1e3:.1f} mm, s {p['s_raw']}, t {p['t_raw']:.3f}, re-solved s {p['s2_raw']}, "
                                 f"distance to a branch point {pair_margin(p):.3f}, denom / (a e) {p['par']:.3f}")
                    assert p["pen"] >= 0.001 and pair_margin(p) >= 0.02 and p["par"] >= 1e-3
                    if kind == "end_t<0":
                        assert p["t_raw"] <= -0.02 and 0.02 <= p["s2_raw"] <= 0.98
                    if kind == "end_t>1":
                        assert p["t_raw"] >= 1.02 and 0.02 <= p["s2_raw"] <= 0.98
            if pen:
                lines.append(f"state {e} sub-step {k}: {len(pen)} penetrating pairs {sorted(p['kind'] for p in pen)}, nearest to a branch point {min(pair_margin(p) for p in pen):.3f}, "
                             f"smallest denom / (a e) {min(p['par'] for p in pen):.3f}")
                assert all(pair_margin(p) >= 0.02 and p["par"] >= 1e-3 for p in pen if p["pen"] >= 0.001)
    return lines


WITNESS = dict(cap8=w_cap8, cap100=w_cap100, expmap=w_expmap, effort=w_effort, pdref=w_pdref, bounce=w_bounce, depen=w_depen, spec=w_spec, gate=w_gate,
               friction=w_friction, capsules=w_capsules, capsules_hi=w_capsules)


def w_pair_coherence(traces):
    """The device kernel tests every candidate capsule pair in the first sub-step of a launch and afterwards only those whose surfaces were then closer than
    PHC_SC_SKIP_MARGIN = 0.12 m (csrc/phc_aba.h, "temporal coherence": a pair that closes faster than ~5 m/s from beyond the margin is picked up one env step late);
    the host emulation and both fp64 references test every pair in every sub-step.  A state is inside what the kernel promises when every pair that touches in a
    later sub-step started within the margin: asserted with 2 cm to spare, so that the comparison with the references is a comparison of the same scheme."""
    worst = np.inf
    for e, tr in enumerate(traces):
        first = {p["shapes"]: p["pen"] for p in tr[0]["pairs"]}
        for k, sub in enumerate(tr[1:], 1):
            for p in sub["pairs"]:
                if p["pen"] > 0:
                    gap0 = -first.get(p["shapes"], -np.inf)
                    assert gap0 <= SKIP_MARGIN - 0.02, f"state {e}: pair {p['shapes']} touches in sub-step {k} and was {gap0:.3f} m apart in sub-step 0: the kernel skips it"
                    worst = min(worst, SKIP_MARGIN - gap0)
    return worst


def witness(reg):
    """Asserts the case's regime and margin from the dense oracle's trace (and, where the table says so, the fp64 inputs and the fp64 recursion); -> the lines to print."""
    s = states(reg)
    traces = dense(reg)[1]
    lines = WITNESS[reg.make](reg, s, traces, reference(reg, 0 if 0 in reg.lags else reg.lags[0]))
    worst = w_pair_coherence(traces)
    lines.append("no capsule pair touches after sub-step 0" if worst == np.inf else
                 f"every capsule pair that touches after sub-step 0 started inside the kernel's skip margin, by >= {worst * 1e3:.0f} mm")
    return lines
