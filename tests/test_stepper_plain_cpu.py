"""CPU: the plain launch of the stepper (phc_amd/csrc/phc_sim_plain.h) against the structs the default task really builds.

The header lists, once, what `phc_sim_step` is called with by the default SMPL task -- launch options, nullable pointers, the call's own arguments -- and the facts
of the shipped SMPL model its plain kernel assumes; `sim_is_plain` / `sim_model_facts` (host) and `pin_sim_plain` / `SimPlainModel` (device) are generated from the two
lists.  Here both lists are parsed back out of the header, so a new entry is tested without touching this file:

  1. the default `compose([...])` task's structs and the arguments of its `_physics_step` satisfy `phc_sim_is_plain`, and every listed entry holds the listed value;
  2. each listed entry moved off its value, one at a time, does not; neither does a model fact moved off its value in the HOST tables;
  3. a model with one anisotropic joint, or with 33 contact points on one body, is not plain; H1, G1, a shape-variation task, and structs whose facts were never
     examined are not plain; an unaligned state tensor is not plain, an odd env count is;
  4. the switch `phc_sim_force_generic` is a host flag that returns the old value and leaves the predicate alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from phc_amd import _lib as L
from phc_amd import abi
from test_task_plain_cpu import G1_OVER, H1_OVER, clone, cpu_structs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "phc_amd", "csrc", "phc_sim_plain.h")
MB, NTAB, BODY_FLOATS = 64, 21, 56
FACTS_PLAIN = 0x504c4e01   # PHC_SIM_FACTS_PLAIN


def _macro(name):
    txt = open(HEADER).read()
    body = txt[txt.index(f"#define {name}("):]
    return body[:body.index("\n\n")].split("\n", 1)[1]


def plain_fields():
    """[(kind, struct, field, value or None)] of PHC_SIM_PLAIN_FIELDS."""
    body = _macro("PHC_SIM_PLAIN_FIELDS")
    out = []
    for kind, s, f, v in re.findall(r"\b(VAL|NUL|SET)\((prm|sim|arg), (\w+)(?:, (-?\d+))?\)", body):
        assert (kind == "VAL") == (v != ""), (kind, f)
        out.append((kind, s, f, int(v) if kind == "VAL" else None))
    assert len(re.findall(r"\b(?:VAL|NUL|SET)\(", body)) == len(out), "an entry of the list does not parse"
    return out


def model_facts():
    """[(name, value)] of PHC_SIM_PLAIN_MODEL."""
    body = _macro("PHC_SIM_PLAIN_MODEL")
    out = [(n, int(v)) for n, v in re.findall(r"\bFACT\((\w+), (-?\d+)\)", body)]
    assert len(re.findall(r"\bFACT\(", body)) == len(out), "an entry of the list does not parse"
    return out


# where each model fact lives in the packed tables (model.py pack(); phc_aba.h): (int table, slot), or a field of the struct
FACT_WORD = {"solver_depth": (11, 2), "rerooted": (11, 3), "jump_steps": (11, 4), "extra_shapes": (11, 5)}
FACT_FIELD = {"num_bodies", "num_dof"}


class Launch:
    """What `_physics_step` hands phc_sim_step for the task `compose(over)` builds, with host addresses."""

    def __init__(self, *over):
        t = cpu_structs(*over)[0]
        self.task, self.model, self.prm, self.sim = t, t._model_struct, t._sim_params, t._sim_struct
        self.actions, self.freeze, self.num_sim_calls = t.actions.data_ptr(), t._freeze_mask.data_ptr(), t.control_freq_inv
        self.ints, self.floats = t._up["ints"], t._up["floats"]

    def args(self, **kw):
        a = dict(model=self.model, prm=self.prm, sim=self.sim, actions=self.actions, freeze=self.freeze, num_sim_calls=self.num_sim_calls)
        a.update(kw)
        return a


def is_plain(model, prm, sim, actions, freeze, num_sim_calls):
    return L.load().phc_sim_is_plain(model, prm, sim, actions, freeze, num_sim_calls)


def facts_of(model, ints, floats):
    """phc_sim_model_facts of `model` with the given HOST tables."""
    h = clone(model)
    ints, floats = np.ascontiguousarray(ints), np.ascontiguousarray(floats)
    h.ints, h.floats = ints.ctypes.data, floats.ctypes.data
    return L.load().phc_sim_model_facts(h)


@pytest.fixture(scope="module")
def default():
    return Launch()


def test_the_lists_name_real_fields_and_the_default_launch_is_plain(default):
    d = default
    fields, facts = plain_fields(), model_facts()
    assert len(fields) >= 12 and len({(s, f) for _, s, f, _ in fields}) == len(fields)
    assert len(facts) >= 6 and set(n for n, _ in facts) == set(FACT_WORD) | FACT_FIELD
    names = {"prm": dict(L.SimParams._fields_), "sim": dict(L.SimState._fields_), "arg": {"actions": L.c_p, "freeze": L.c_p, "num_sim_calls": L.c_i32}}
    have = {"prm": d.prm, "sim": d.sim, "arg": type("A", (), dict(actions=d.actions, freeze=d.freeze, num_sim_calls=d.num_sim_calls))}
    for kind, s, f, v in fields:
        assert f in names[s], f"{s}.{f} is not a field of the struct"
        assert (names[s][f] is L.c_p) == (kind != "VAL"), f"{s}.{f}: pointers are listed as NUL / SET, values as VAL"
        got = getattr(have[s], f)
        if kind == "VAL":
            assert got == v, f"the default task's {s}.{f} is {got!r}, the list says {v!r}"
        else:
            assert bool(got) == (kind == "SET"), f"the default task's {s}.{f} is {got!r}, the list says {kind}"
    # the model facts, read from the tables the task packed
    ints = d.ints.reshape(-1)
    for n, v in facts:
        got = getattr(d.model, n) if n in FACT_FIELD else int(ints[4 + FACT_WORD[n][0] * MB + FACT_WORD[n][1]])
        assert (got != 0) == (v != 0) if n == "rerooted" else got == v, f"the shipped SMPL model's {n} is {got}, the list says {v}"
    assert facts_of(d.model, d.ints, d.floats) == FACTS_PLAIN == d.model.sim_plain_facts   # (abi.model_struct asked at upload)
    assert is_plain(**d.args()) == 1
    # what the lists leave alone may take any value
    p2, s2 = clone(d.prm), clone(d.sim)
    p2.sim_dt, p2.contact_stiffness, p2.friction, p2.control_freq_inv, p2.contact_iterations, p2.angular_damping = 1 / 50, 5e4, 0.7, 5, 9, 0.3
    s2.num_envs = 4097
    assert is_plain(**d.args(prm=p2, sim=s2)) == 1
    assert is_plain(**d.args(model=None)) == 0 and is_plain(**d.args(prm=None)) == 0 and is_plain(**d.args(sim=None)) == 0


@pytest.mark.parametrize("entry", plain_fields(), ids=lambda e: f"{e[1]}.{e[2]}")
def test_one_listed_entry_off_its_value_leaves_the_plain_set(default, entry):
    d = default
    kind, s, f, v = entry
    others = [v + 1, v - 1] + ([0] if v else []) if kind == "VAL" else ([0x1000] if kind == "NUL" else [None])
    for other in others:
        p2, s2 = clone(d.prm), clone(d.sim)
        kw = dict(prm=p2, sim=s2)
        if s == "arg":
            kw[f] = other
        else:
            setattr({"prm": p2, "sim": s2}[s], f, other)
        assert is_plain(**d.args(**kw)) == 0, f"{s}.{f} = {other} still counts as plain"
    assert is_plain(**d.args(prm=clone(d.prm), sim=clone(d.sim))) == 1


@pytest.mark.parametrize("fact", model_facts(), ids=lambda e: e[0])
def test_one_model_fact_off_its_value_leaves_the_plain_set(default, fact):
    d = default
    n, v = fact
    for other in ([v + 1, v - 1] if n != "rerooted" else [0]):
        m2, ints = clone(d.model), d.ints.copy()
        if n in FACT_FIELD:
            setattr(m2, n, other)
        else:
            ints.reshape(-1)[4 + FACT_WORD[n][0] * MB + FACT_WORD[n][1]] = other
        assert facts_of(m2, ints, d.floats) == 0, f"{n} = {other} still counts as plain"
        if n in FACT_FIELD:   # (these the launch predicate sees in the struct itself, whatever the stored answer says)
            assert is_plain(**d.args(model=m2)) == 0


def test_anisotropic_joints_and_33_contact_points_are_not_plain(default):
    d = default
    nb = d.model.num_bodies
    for col in (13, 14, 17, 18, 19, 21):   # one axis of kp / kd / armature of ONE joint
        fl = d.floats.copy()
        fl.reshape(-1)[5 * BODY_FLOATS + col] *= 1.5
        assert facts_of(d.model, d.ints, fl) == 0, col
    fl = d.floats.copy()
    fl.reshape(-1)[0 * BODY_FLOATS + 13] = 7.0   # (the root has no joint: its gain slots play no part)
    assert facts_of(d.model, d.ints, fl) == FACTS_PLAIN
    for pts, want in ((32, FACTS_PLAIN), (33, 0)):
        ints, m2 = d.ints.copy(), clone(d.model)
        ints.reshape(-1)[4 + 9 * MB + (nb - 1)] = pts
        m2.max_body_contact_pts = max(pts, d.model.max_body_contact_pts)
        assert facts_of(m2, ints, d.floats) == want, pts
        m3 = clone(d.model)   # ... and the table is read, not only the struct's summary of it
        assert facts_of(m3, ints, d.floats) == want, pts
        m2.sim_plain_facts = FACTS_PLAIN   # a stale answer does not outvote the struct's own summary
        assert is_plain(**d.args(model=m2)) == (1 if pts <= 32 else 0)
    # the answer is asked by abi.model_struct, from the very tables it is given -- on the host here, after a device copy in a real task
    fl = d.floats.copy()
    fl.reshape(-1)[7 * BODY_FLOATS + 16] *= 2.0
    t = d.task
    mk = lambda floats: abi.model_struct(d.ints, floats, t.num_bodies, t.num_dof, t.model.max_level, d.model.num_contact_pts)
    assert mk(d.floats).sim_plain_facts == FACTS_PLAIN and mk(fl).sim_plain_facts == 0
    assert is_plain(**d.args(model=mk(fl))) == 0
    m0 = clone(d.model)
    m0.sim_plain_facts = 0     # never examined (a caller that zero-fills the struct): generic
    assert is_plain(**d.args(model=m0)) == 0
    m0.sim_plain_facts = 1
    assert is_plain(**d.args(model=m0)) == 0


def test_robots_shape_variation_alignment_and_odd_env_counts(default):
    d = default
    for over in (H1_OVER, G1_OVER, ["robot.has_shape_variation=True", "robot.has_shape_obs=True", "robot.has_shape_obs_disc=True"]):
        o = Launch(*over)
        assert o.model.sim_plain_facts == 0 and is_plain(**o.args()) == 0, over
    assert is_plain(**Launch("+solver.force_average=1").args()) == 1   # (not listed: it never changes the states, and both values must run one kernel)
    for over in (["+solver.inertia_lag=0"], ["+solver.contact=tgs"], ["+solver.self_collision=0"], ["env.self_obs_v=3"], ["env.res_action=True"]):
        try:
            o = Launch(*over)
        except Exception as e:   # (an override this config tree does not take is no evidence either way)
            pytest.fail(f"{over}: {e}")
        if over == ["env.res_action=True"] and not o.sim.pd_ref:
            s2 = clone(o.sim)
            s2.pd_ref = 0x1000
            assert is_plain(**o.args(sim=s2)) == 0
            continue
        assert is_plain(**o.args()) == 0, over
    # the staged epilogue's alignment is the host's to check: one tensor 4 bytes off is not plain
    for f in ("root_states", "dof_state", "rigid_body_state", "contact_force", "dof_force"):
        s2 = clone(d.sim)
        setattr(s2, f, getattr(d.sim, f) + 4)
        assert is_plain(**d.args(sim=s2)) == 0, f
    s2 = clone(d.sim)
    s2.pd_target = d.sim.pd_target + 4   # (not part of the epilogue)
    assert is_plain(**d.args(sim=s2)) == 1
    # the tail wavefront of an odd env count keeps its run-time test in the kernel: any count is plain
    for n in (1, 3, 65, 4095):
        s2 = clone(d.sim)
        s2.num_envs = n
        assert is_plain(**d.args(sim=s2)) == 1, n


def test_force_generic_is_a_host_flag(default):
    lib_ = L.load()
    assert {"phc_sim_force_generic", "phc_sim_is_plain", "phc_sim_model_facts"} <= set(L.EXPORTED_SYMBOLS)
    assert C.sizeof(L.Model) == 56   # the facts word took the struct's tail padding: layout of ABI 37
    old = lib_.phc_sim_force_generic(1)
    try:
        assert old == 0
        assert lib_.phc_sim_force_generic(7) == 1 and lib_.phc_sim_force_generic(0) == 1 and lib_.phc_sim_force_generic(1) == 0
        assert is_plain(**default.args()) == 1   # the predicate reports the structs, not the switch
    finally:
        lib_.phc_sim_force_generic(old)
    assert lib_.phc_sim_force_generic(old) == old
