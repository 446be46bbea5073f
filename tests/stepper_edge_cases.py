"""TEST INFRASTRUCTURE for tests/test_stepper_launch_edges.py: the table of stepper configurations, their states, a launcher that puts every tensor of a launch
into a guarded buffer, and the bit-for-bit comparison.

Guarded buffers.  Every tensor a launch WRITES (root, dof, rbs, cf, df, pd_target, force_sensor) is a slice of a larger buffer: GUARD floats, `k` lead floats, the
payload, GUARD floats; guards, lead and -- for the pure outputs -- the payload hold one fixed quiet-NaN bit pattern before the launch.  The allocators of both backends
hand out buffers aligned to 256 bytes or more (asserted on the device), so k = 0 gives a 16-byte aligned tensor, k = 2 an 8-byte and k = 1, 3 a 4-byte aligned one.
Every float tensor a launch only READS (actions, offset, scale, pd_ref, wrench force and torque) is followed by GUARD NaN floats: a lane that read past the end would
poison its workgroup and the finite-output checks fail.  Float tensors need 4-byte alignment only (include/phc_amd.h, phc_sim_state_t)."""
from dataclasses import dataclass

import numpy as np

import hostemu_util as hu
import wrench_util as wu
from backends import get_backend, model_on
from phc_amd import abi

F = np.float32
GUARD = 64
PATTERN = np.uint32(0x7FC5A5A5)   # a quiet NaN no computation produces
NUM_STATES = 5
WRITTEN = ("root", "dof", "rbs", "cf", "df", "pd", "fs")
UNSUPPORTED = -2   # PHC_EUNSUPPORTED
EINVAL = -1        # PHC_EINVAL


@dataclass(frozen=True)
class Case:
    id: str
    model: str                      # a shipped model, or "smpl_shapes": the three stacked SMPL shapes
    opts: tuple = ()                # sim_params_struct keywords on top of self_collision = 1 (and the robot's switches)
    states: str = "random"          # "random": test_dynamics.random_states near the ground (_robot_case); "ground": wrench_util.smpl_state(.., "ground"); "heels": heel_states;
                                    # "rest": robot_ground_states
    sensors: bool = False           # two force sensors (ankles), force_sensor tensor given
    wrench: bool = False            # through phc_sim_step_wrench, force and torque per state, wrench_sim_calls = 1 of 2
    actions: str = ""               # "" | "plain" | "freeze" | "ref" (pd_ref: device only, the host emulation has no res_action path)

    @property
    def rigid(self):
        return dict(self.opts).get("contact_model") == "tgs"

    @property
    def hip_only(self):
        return self.actions == "ref"


def _c(id, model, states="random", sensors=False, wrench=False, actions="", **opts):
    return Case(id, model, tuple(sorted(opts.items())), states, sensors, wrench, actions)


HEIGHT = {"smpl_humanoid": 0.85, "smpl_shapes": 0.85, "h1_humanoid": 0.85, "g1_humanoid": 0.70}
_TABLE = [
    _c("smpl-fresh", "smpl_humanoid", inertia_lag=0),
    _c("smpl-lag", "smpl_humanoid", inertia_lag=1),
    _c("smpl-lag-avg", "smpl_humanoid", inertia_lag=1, force_average=1),
    _c("smpl-rigid", "smpl_humanoid", "ground", contact_model="tgs"),
    _c("smpl-rigid-avg", "smpl_humanoid", "ground", contact_model="tgs", force_average=1),
    _c("smpl-sensors", "smpl_humanoid", "heels", sensors=True, inertia_lag=1),
    _c("smpl-sensors-rigid", "smpl_humanoid", "heels", sensors=True, contact_model="tgs"),
    _c("smpl-shapes-lag", "smpl_shapes", inertia_lag=1),
    _c("smpl-shapes-rigid", "smpl_shapes", "ground", contact_model="tgs"),
    _c("smpl-occ3", "smpl_humanoid", lane_mapping=3, inertia_lag=0),
    _c("h1-fresh", "h1_humanoid", inertia_lag=0),
    _c("h1-lag", "h1_humanoid", inertia_lag=1),
    _c("h1-rigid", "h1_humanoid", "rest", contact_model="tgs"),
    _c("g1-lag", "g1_humanoid", inertia_lag=1),
    # (g1-rigid: refused -- G1's torso link carries 40 contact points, the rigid model's masks hold 32; test_g1_with_rigid_contact_is_refused)
    _c("smpl-lag-wrench", "smpl_humanoid", wrench=True, inertia_lag=1),
    _c("smpl-rigid-wrench", "smpl_humanoid", "ground", wrench=True, contact_model="tgs"),
    _c("h1-lag-wrench", "h1_humanoid", wrench=True, inertia_lag=1),
    _c("g1-lag-wrench", "g1_humanoid", wrench=True, inertia_lag=1),
    _c("smpl-lag-act", "smpl_humanoid", actions="plain", inertia_lag=1),
    _c("smpl-lag-act-freeze", "smpl_humanoid", actions="freeze", inertia_lag=1),
    _c("smpl-lag-act-ref", "smpl_humanoid", actions="ref", inertia_lag=1),
    _c("h1-lag-act", "h1_humanoid", actions="plain", inertia_lag=1),
    _c("h1-lag-act-freeze", "h1_humanoid", actions="freeze", inertia_lag=1),
    _c("h1-lag-act-ref", "h1_humanoid", actions="ref", inertia_lag=1),
]
CASES = {c.id: c for c in _TABLE}
TWO_PER_WAVEFRONT = ["smpl-lag-avg", "smpl-rigid", "smpl-sensors", "smpl-shapes-lag", "h1-lag", "smpl-lag-wrench"]   # the rows of the guard and null-output tests
REFRESH_MODELS = ["smpl-lag", "h1-lag", "g1-lag", "smpl-shapes-lag"]   # rows whose model and states the refresh tests take

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- models -------------------------------------------------------------------------------------------------------------------------------------------------
def _shape_models():
    from phc_amd.model import load_model
    from phc_amd.robots import apply_collision_filter
    models = [load_model(f"smpl_{g}_humanoid") for g in range(3)]
    for m in models:
        apply_collision_filter(m, "smpl")
    return models


MODEL_MAKERS = {}   # {model name: be -> (ArticulationModel, model struct, keep)} for models a case table adds on top of the shipped ones (tests/stepper_regimes.py)


def models_on(be, case):
    """-> ([ArticulationModel per shape block], model struct, what the struct points to), once per backend and model."""
    def make():
        if case.model in MODEL_MAKERS:
            m, ms, keep = MODEL_MAKERS[case.model](be)
            return [m], ms, keep
        if case.model != "smpl_shapes":
            m, ms, keep = model_on(be, name=case.model)
            return [m], ms, keep
        from phc_amd.model import pack_shapes
        models = _shape_models()
        ints, floats = pack_shapes(models)
        keep = (be.arr(ints), be.arr(floats))
        m0 = models[0]
        return models, abi.model_struct(keep[0], keep[1], m0.num_bodies, m0.num_dof, m0.max_level, max(len(m.contact_body) for m in models), num_shapes=3), keep
    return cached(("model", be.name, case.model), make)


def params_of(case, models):
    kw = dict(self_collision=1)
    if case.model in ("h1_humanoid", "g1_humanoid"):   # (the robot switches of test_stepper_chain_latency._robot_case)
        kw.update(control_mode=1 if case.model == "h1_humanoid" else 2, sim_dt=1.0 / 200.0)
    kw.update(dict(case.opts))
    if case.sensors:
        names = list(models[0].body_names)
        kw["force_sensor_bodies"] = (names.index("L_Ankle"), names.index("R_Ankle"))
    return abi.sim_params_struct(**kw)


# ---- states -------------------------------------------------------------------------------------------------------------------------------------------------
def heel_states(model, n, seed=11):
    """wrench_util.smpl_state(.., "ground") with the legs straight, both ankles pitched by 0.3 rad so that the heels of the ANKLE bodies are the lowest points (4 to
    4 + n mm in the plane) and the toes hang 4 cm above them, and the root moving down at 1 m/s.  The sensor rows need it: the generators of the other rows rest on
    the toes, and under rigid contact a foot that is not pressed down has left the plane by the launch's last sub-step -- the ankle sensors then read zero."""
    import dyn_oracle as do
    rng = np.random.default_rng(seed)
    nd, names = model.num_dof, list(model.body_names)
    legs = [3 * (names.index(b) - 1) + k for b in names if b[2:] in ("Hip", "Knee", "Ankle", "Toe") for k in range(3)]
    root = np.zeros((n, 13), F)
    root[:, 6] = 1.0
    dof = np.zeros((n, nd, 2), F)
    dof[:, :, 0] = rng.normal(0, 0.08, (n, nd))
    dof[:, legs, 0] = 0
    for b in ("L_Ankle", "R_Ankle"):
        dof[:, 3 * (names.index(b) - 1) + 1, 0] = -0.3
    dof[:, :, 1] = rng.normal(0, 0.3, (n, nd))
    target = (dof[:, :, 0] + rng.normal(0, 0.1, (n, nd))).astype(F)
    target[:, legs] = dof[:, legs, 0]
    root[:, 7:10] = rng.normal(0, 0.05, (n, 3))
    root[:, 9] = -1.0
    cb = np.asarray(model.contact_body)
    for e in range(n):
        Q, R, p = do.kinematics(model, do.State(root[e].astype(np.float64), dof[e].astype(np.float64), model))
        low = np.array([p[i][2] + (R[i] @ model.contact_pos[k])[2] - model.contact_radius[k] for k, i in enumerate(cb)])
        assert cb[low.argmin()] in (names.index("L_Ankle"), names.index("R_Ankle")) and low[cb == names.index("L_Toe")].min() - low.min() > 0.02
        root[e, 2] = -low.min() - 0.004 - 0.001 * e
    return root, dof, target


def robot_ground_states(model, n, seed=11):
    """wrench_util.robot_rest_state with joint rates (as test_ext_wrench_gpu.test_robots_match_the_double_precision_recursion adds them), lowered until the lowest
    contact point is 4 to 4 + n mm in the plane, moving down.  The rigid robot row takes it: among the violent random states of the other robot rows is one (state 1,
    joint rates up to 47 rad/s) at which the fp32 HOST EMULATION is 1.8e-2 rad/s from the fp64 recursion in one joint rate under rigid contact -- a property of that
    state, the bound is 1e-2."""
    import dyn_oracle as do
    rng = np.random.default_rng(seed)
    root, dof, target = wu.robot_rest_state(model, n, 2.0)
    dof[:, :, 1] = rng.normal(0, 0.3, dof[:, :, 1].shape)
    root[:, 7:10] = rng.normal(0, 0.05, (n, 3))
    root[:, 9] = -0.3
    for e in range(n):
        Q, R, p = do.kinematics(model, do.State(root[e].astype(np.float64), dof[e].astype(np.float64), model))
        low = min(p[i][2] + (R[i] @ model.contact_pos[k])[2] - model.contact_radius[k] for k, i in enumerate(model.contact_body))
        root[e, 2] -= low + 0.004 + 0.001 * e
    return root, dof, target


def states_of(case, n=NUM_STATES):
    """n distinct states of the case's model and everything else a launch of the case reads, row i belonging to state i."""
    def make():
        from test_dynamics import random_states
        from test_stepper_chain_latency import _robot_case
        models = models_on(get_backend("hostemu"), case)[0]
        m0 = models[0]
        nb, nd = m0.num_bodies, m0.num_dof
        shapes = case.model == "smpl_shapes"
        if case.states == "rest":
            root, dof, target = robot_ground_states(m0, n)
        elif case.states == "heels":
            root, dof, target = heel_states(m0, n)
        elif case.states == "ground":
            per = [wu.smpl_state(m, n, "ground", seed=11) for m in models]   # (the same draws for every shape; the root height is the shape's own)
            pick = np.arange(n) % len(models)
            root, dof, target = (np.stack([per[pick[i]][k][i] for i in range(n)]) for k in range(3))
        elif shapes:
            root, dof, target = random_states(m0, n, np.random.default_rng(5), height=HEIGHT[case.model])
        else:
            root, dof, target, _ = _robot_case(case.model, n, 17, HEIGHT[case.model])
        s = dict(root=root.astype(F), dof=dof.astype(F), target=target.astype(F))
        rng = np.random.default_rng(23)
        if shapes:
            s["env_shape"] = (np.arange(n) % 3).astype(np.int32)
        if case.actions:
            # offset + scale * action (or pd_ref + scale * action) lands near the state's own target
            s["scale"] = rng.uniform(0.5, 1.5, nd).astype(F)
            s["off"] = rng.normal(0, 0.1, nd).astype(F)
            if case.actions == "ref":
                s["act"] = rng.normal(0, 0.15, (n, nd)).astype(F)
                s["pd_ref"] = (s["target"] - s["scale"][None] * s["act"]).astype(F)
            else:
                s["act"] = ((s["target"] - s["off"][None]) / s["scale"][None]).astype(F)
            if case.actions == "freeze":
                s["freeze"] = (rng.random(nd) < 0.3).astype(np.int32)
                assert s["freeze"].any() and not s["freeze"].all()
        if case.wrench:   # wrench_util's magnitudes: m dg on every body, a push on the root body, a torque on the torso; all of them different per state
            names = list(m0.body_names)
            torso = names.index("Torso" if "Torso" in names else "torso_link")
            force = wu.gravity_wrench(m0, n, False) * (1.0 + 0.15 * np.arange(n))[:, None, None]
            torque = np.zeros((n, nb, 3))
            for e in range(n):
                force[e, 0] += (150.0 + 20.0 * e, -90.0 + 30.0 * e, 0.0)
                torque[e, torso] = (20.0, -15.0 + 5.0 * e, 30.0)
            assert np.abs(force).max() <= 300.0 and np.abs(torque).max() <= 50.0
            s["force"], s["torque"] = force.astype(F), torque.astype(F)
        return s
    return cached(("states", case.id, n), make)


# ---- guarded launch -----------------------------------------------------------------------------------------------------------------------------------------
class _Guarded:
    """GUARD pattern floats | k pattern floats | payload | GUARD pattern floats, on a backend."""

    def __init__(self, be, payload, k, name):
        payload = np.ascontiguousarray(payload, F)
        self.be, self.shape, self.n, self.k, self.name = be, payload.shape, payload.size, k, name
        full = np.full(GUARD + k + self.n + GUARD, PATTERN, np.uint32)
        full[GUARD + k:GUARD + k + self.n] = payload.reshape(-1).view(np.uint32)
        self.full = be.arr(full.view(F))
        self.view = self.full[GUARD + k:GUARD + k + self.n]
        if be.name == "hip":
            assert self.full.data_ptr() % 256 == 0, "the lead floats set the alignment only on a 256-byte base"
            assert self.view.data_ptr() == self.full.data_ptr() + 4 * (GUARD + k)

    def read(self):
        """-> (payload, number of guard / lead words that no longer hold the pattern)"""
        bits = np.ascontiguousarray(self.be.np(self.full)).view(np.uint32)
        lo, hi = GUARD + self.k, GUARD + self.k + self.n
        broken = int((bits[:lo] != PATTERN).sum() + (bits[hi:] != PATTERN).sum())
        return bits[lo:hi].view(F).reshape(self.shape).copy(), broken


def _padded(be, x):
    """A read-only float tensor followed by GUARD NaN floats."""
    x = np.ascontiguousarray(x, F)
    full = be.arr(np.concatenate([x.reshape(-1), np.full(GUARD, np.nan, F)]))
    return full, full[:x.size]


def _pattern(shape):
    return np.full(shape, PATTERN, np.uint32).view(F)


def launch(be, case, rows, lead=0, null=(), entry="step", env_ids=None, num=None, states=None):
    """One launch of `case` on backend `be` with state rows[e] in env e.  `lead`: the lead floats k of every written tensor, or {tensor: k} (0 where absent).
    `null`: written tensors handed over as null pointers (their buffers stay allocated).  `entry`: "step", "refresh", "refresh_indexed" (env_ids, num).
    -> (return code, {tensor: array [n, ...]}, [what is wrong with the guards])."""
    models, mstruct, keep = models_on(be, case)
    m0 = models[0]
    s = states or states_of(case)
    rows = np.asarray(rows)
    n, nb, nd = len(rows), m0.num_bodies, m0.num_dof
    k_of = (lambda t: lead.get(t, 0)) if isinstance(lead, dict) else (lambda t: lead)
    prm = params_of(case, models)
    init = dict(root=s["root"][rows], dof=s["dof"][rows], pd=s["target"][rows], rbs=_pattern((n, nb, 13)), cf=_pattern((n, nb, 3)), df=_pattern((n, nd)))
    if case.sensors:
        init["fs"] = _pattern((n, 2, 6))
    g ={t: _Guarded(be, v, k_of(t), t) for t, v in init.items()}
    p = {t: (None if t in null else g[t].view) for t in g}
    hold = {}
    for t in ("act", "pd_ref", "force", "torque"):
        if t in s and entry == "step":
            hold[t] = _padded(be, s[t][rows])
    for t in ("off", "scale"):
        if t in s and entry == "step":
            hold[t] = _padded(be, s[t])
    ints = {t: be.arr(v) for t, v in (("freeze", s.get("freeze")), ("env_shape", s["env_shape"][rows] if "env_shape" in s else None)) if v is not None}
    get = lambda t: hold[t][1] if t in hold else None
    sim = abi.sim_state_struct(n, p["root"], p["dof"], p["rbs"], p["cf"], p["df"], p["pd"], force_sensor=p.get("fs"), env_shape=ints.get("env_shape"),
                               pd_ref=get("pd_ref"))
    if entry == "step":
        extra = dict(force=get("force"), torque=get("torque"), wrench_sim_calls=1) if case.wrench else {}
        rc = be.sim_step(mstruct, prm, sim, get("act"), get("off"), get("scale"), ints.get("freeze"), 2, **extra)
    elif entry == "refresh":
        rc = be.refresh_body_state(mstruct, sim)
    else:
        ids = None if env_ids is None else be.arr(np.asarray(env_ids, np.int64))
        rc = be.refresh_body_state_indexed(mstruct, sim, len(env_ids) if num is None else num, ids)
    be.sync()
    out, wrong = {}, []
    for t, b in g.items():
        out[t], broken = b.read()
        if broken:
            wrong.append(f"{t}: {broken} guard words overwritten (lead {b.k})")
        if t in null and not np.array_equal(out[t].view(np.uint32), np.ascontiguousarray(init[t], F).view(np.uint32)):
            wrong.append(f"{t}: handed over as null and written all the same")
    for t, (full, view) in hold.items():   # (a launch writes none of what it only reads)
        if not np.array_equal(np.ascontiguousarray(be.np(view)).view(np.uint32), np.ascontiguousarray(s[t][rows] if t in ("act", "pd_ref", "force", "torque") else s[t], F).reshape(-1).view(np.uint32)):
            wrong.append(f"{t}: a read-only tensor was written")
    return rc, out, wrong


def outputs_of(case, null=()):
    return [t for t in WRITTEN if (t != "fs" or case.sensors) and t not in null]


# ---- comparison ---------------------------------------------------------------------------------------------------------------------------------------------
def mismatches(got, want, keys, tag, envs=None, want_envs=None):
    """Rows of `got` that are not, bit for bit, the rows of `want`: one line per tensor and env with the count and the worst absolute difference.
    `envs` / `want_envs`: the rows to pair (default: all, in order)."""
    lines = []
    for t in keys:
        a, b = got[t], want[t]
        ea = range(a.shape[0]) if envs is None else envs
        eb = ea if want_envs is None else want_envs
        for i, j in zip(ea, eb):
            x, y = np.ascontiguousarray(a[i]), np.ascontiguousarray(b[j])
            bad = x.view(np.uint32) != y.view(np.uint32)
            if bad.any():
                with np.errstate(invalid="ignore"):
                    d = np.abs(x.astype(np.float64) - y.astype(np.float64))[bad]
                worst = "nan" if np.isnan(d).any() else f"{d.max():.3e}"
                lines.append(f"{tag} {t} env {i}: {int(bad.sum())} of {bad.size} words differ, worst {worst}")
    return lines


def stack_refs(refs, rows):
    return {t: np.concatenate([refs[i][t] for i in rows]) for t in refs[0]}


def references(backend, case):
    """The case's five states stepped ALONE (N = 1, every tensor 16-byte aligned) on `backend`, once; with the preconditions of every test that compares with them."""
    def make():
        be = get_backend(backend)
        refs = []
        for i in range(NUM_STATES):
            rc, out, wrong = launch(be, case, [i])
            assert rc == 0, (case.id, rc)
            assert not wrong, wrong
            refs.append(out)
        keys = outputs_of(case)
        for i, r in enumerate(refs):
            for t in keys:
                assert np.isfinite(r[t]).all(), f"{case.id}: reference {t} of state {i} is not finite (or was not written)"
        assert any(np.abs(r["cf"]).sum() > 0 for r in refs), f"{case.id}: no state carries contact force"
        if case.sensors:
            assert any(np.abs(r["fs"]).sum() > 0 for r in refs), f"{case.id}: no force sensor reads anything"
        for i in range(NUM_STATES):
            for j in range(i):
                for t in ("root", "dof", "rbs", "df"):
                    assert not np.array_equal(refs[i][t], refs[j][t]), f"{case.id}: {t} of states {i} and {j} are equal, a row swap could pass"
        return refs
    return cached(("refs", backend, case.id), make)


def formula_targets(case):
    """What `pd_target` holds after a launch of the case, from the formula (tests/test_stepper_chain_latency.py::test_pd_targets_equal_the_formula_bit_for_bit):
    float32(offset + float32(scale * action)); with pd_ref float32(pd_ref + ..) kept within float32(pi / 2) of the joint position; frozen DoFs 0; the targets handed
    over where the launch has no actions."""
    s = states_of(case)
    if not case.actions:
        return s["target"]
    sa = (s["scale"][None] * s["act"]).astype(F)
    if case.actions == "ref":
        half_pi, q = F(1.57079637), s["dof"][:, :, 0]
        t = np.maximum(np.minimum((s["pd_ref"] + sa).astype(F), (q + half_pi).astype(F)), (q - half_pi).astype(F))
    else:
        t = (s["off"][None] + sa).astype(F)
    if "freeze" in s:
        t[:, s["freeze"] != 0] = 0
        assert (t[:, s["freeze"] == 0] != 0).all(), "a frozen DoF must differ from its neighbours"
    return t


def fp64_reference(case, i, target):
    """State i of the case through the double-precision build of the recursion, with `target` as its PD target."""
    def make():
        models = models_on(get_backend("hostemu"), case)[0]
        s = states_of(case)
        m = models[int(s["env_shape"][i]) if "env_shape" in s else 0]
        kw = dict(force=s["force"][i:i + 1], torque=s["torque"][i:i + 1], wrench_sim_calls=1) if case.wrench else {}
        return m, hu.host_sim_step(m, params_of(case, models), s["root"][i:i + 1], s["dof"][i:i + 1], target, 2, f64=True, **kw)
    return cached(("f64", case.id, i), make)
