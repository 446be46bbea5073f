"""Launch edges of k_sim_step and the refresh entry points: what the stepper writes for an env depends on that env's inputs only -- not on the env's slot, on
which epilogue its wavefront took, on the alignment of the tensors or on which optional outputs exist.  Stated bit for bit (uint32 views, no tolerance) on both
backends of tests/backends.py; cases, guarded buffers and the comparison are tests/stepper_edge_cases.py.

Instantiations of k_sim_step the table of stepper_edge_cases.py launches (joint type x lanes per env x contact x scheme x shapes x OCC x wrench):
  spherical, 32 lanes, penalty, fresh                       smpl-fresh
  spherical, 32 lanes, penalty, lagged                      smpl-lag, smpl-lag-avg (force_average), smpl-sensors, smpl-lag-act / -act-freeze / -act-ref
  spherical, 32 lanes, rigid                                smpl-rigid, smpl-rigid-avg, smpl-sensors-rigid
  spherical, 32 lanes, penalty, lagged, per-env shapes      smpl-shapes-lag
  spherical, 32 lanes, rigid, per-env shapes                smpl-shapes-rigid
  spherical, 32 lanes, penalty, fresh, OCC = 3              smpl-occ3 (lane_mapping 3: its first comparison with anything)
  spherical, 32 lanes, penalty lagged / rigid, WRENCH       smpl-lag-wrench, smpl-rigid-wrench
  revolute, 32 lanes, penalty fresh / lagged, rigid         h1-fresh, h1-lag (+ -act / -act-freeze / -act-ref), h1-rigid
  revolute, 32 lanes, penalty, lagged, WRENCH               h1-lag-wrench
  revolute, 64 lanes, penalty, lagged (+ WRENCH)            g1-lag, g1-lag-wrench
  STEP = false (the refresh entry points)                   spherical, spherical with shapes, revolute 32 lanes, revolute 64 lanes
Not launched here: the fresh per-env-shapes and fresh 64-lane instantiations and the remaining WRENCH twins (fresh; rigid revolute).

Mutation check.  Each of these one-line changes of phc_sim_kernel.h (all of them keep every access inside its allocation) was built in a scratch copy and this file run
once against it on an MI355X; the tests that failed:
  1. stage_flush copies the dof_force slice from stage + o.contact     test_placement (22 rows: every 32-lane row), test_guards_and_alignment (12), test_optional_outputs_may_be_null (6)
  2. aba_force_accumulate is handed favg_all + lane * 6                 test_placement[smpl-lag-avg, smpl-rigid-avg], test_guards_and_alignment[smpl-lag-avg-4, -3]
  3. the direct epilogue publishes body state to row `grp`            test_placement (all 24 rows), test_guards_and_alignment (12), test_optional_outputs_may_be_null (5), both refresh tests (4 + 4)
  4. pd_targets_of reads the freeze flags from `freeze`               not a slot error (the single-env reference is wrong the same way): caught by the formula comparison of
                                                                       test_single_env_references_equal_the_double_precision_recursion[*-act-freeze], which was added for it
  5. the indexed refresh uses `slot` instead of env_ids[slot]         test_refresh_body_state_indexed (all 4 models)
  (6., stage_aligned without sim.dof_force in the OR, was NOT tried: it makes the staged epilogue issue float2 / float4 global stores at a 4-byte offset, and nothing
   at hand confirms that those are ordinary unaligned accesses on gfx950.  What it stands for -- one pointer alone off 16 bytes -- is launched by
   test_guards_and_alignment with the unmutated kernel, which then takes the direct epilogue.)

Left out of what was asked, and why:
  * g1-rigid: phc_sim_step refuses it (40 contact points on G1's torso link, 32-bit masks); test_g1_with_rigid_contact_is_refused states the refusal instead.
  * The host emulation has no indexed refresh and no res_action path: test_refresh_body_state_indexed and the `-act-ref` rows are device only.
  * The sensor rows and h1-rigid take states from generators of stepper_edge_cases.py (heel_states, robot_ground_states; reasons in their docstrings) that are
    modelled on wrench_util's; every other row uses the existing generators unchanged.
  * No bit equality had to become a bound: every comparison but the fp64 anchor is exact on both backends.
"""
import numpy as np
import pytest

import stepper_edge_cases as ec
import wrench_util as wu
from backends import BACKENDS, get_backend
from test_dynamics import check_step_against

F = np.float32


def _over(ids):
    """(backend, case id) for both backends; rows the host emulation has no path for on the device only."""
    out = []
    for i in ids:
        if not ec.CASES[i].hip_only:
            out.append(("hostemu", i))
        out.append(pytest.param("hip", i, marks=pytest.mark.gpu))
    return out


def _run(be, case, rows, **kw):
    rc, out, wrong = ec.launch(be, case, rows, **kw)
    assert rc == 0, (case.id, rc)
    return out, wrong


# ---------------------------------------------------------------------------------------------------------------
# 1. placement
# ---------------------------------------------------------------------------------------------------------------
PLACEMENTS = [("2", [0, 1]), ("3", [0, 1, 2]), ("5", [0, 1, 2, 3, 4]), ("5 reversed", [4, 3, 2, 1, 0]), ("131", [e % 5 for e in range(131)])]


@pytest.mark.parametrize("backend,cid", _over(list(ec.CASES)))
def test_placement(backend, cid):
    """ref[i]: state i stepped alone.  Then 2, 3, 5, 5 reversed and 131 envs (state e % 5 in env e: 66 workgroups, the last one half filled; 131 for G1): every row
    of every written tensor is, bit for bit, the ref of the state it holds, and no guard word around any tensor changed."""
    case, be = ec.CASES[cid], get_backend(backend)
    refs = ec.references(backend, case)
    keys = ec.outputs_of(case)
    lines = []
    for tag, rows in PLACEMENTS:
        out, wrong = _run(be, case, rows)
        lines += [f"N = {tag}: {w}" for w in wrong]
        lines += ec.mismatches(out, ec.stack_refs(refs, rows), keys, f"N = {tag}:")
    assert not lines, f"{cid} on {backend}: {len(lines)} problems\n" + "\n".join(lines[:40])


# ---------------------------------------------------------------------------------------------------------------
# 2. anchor
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,cid", _over(list(ec.CASES)))
def test_single_env_references_equal_the_double_precision_recursion(backend, cid):
    """The only numerical statement of the file: the five single-env references against the fp64 build of the recursion (hostemu_util.host_sim_step) at the
    tolerances the stepper is held to everywhere else -- test_dynamics.check_step_against, wrench_util.assert_standing for rigid contact.  With actions the PD target
    the launch formed is the recursion's target, and is first compared bit for bit with the formula (every DoF's own offset, scale and freeze flag).  `smpl-occ3` runs the states of `smpl-fresh`."""
    case = ec.CASES[cid]
    refs = ec.references(backend, case)
    lines = ec.mismatches(ec.stack_refs(refs, range(ec.NUM_STATES)), dict(pd=ec.formula_targets(case)), ("pd",), "pd_target vs the formula:")
    assert not lines, "\n".join(lines)
    for i, r in enumerate(refs):
        m, ref = ec.fp64_reference(case, i, r["pd"])
        wu.report(f"{cid} state {i} on {backend}", r, ref)
        if case.rigid:
            wu.assert_standing(r, ref, rigid=True, tag=f"{cid} state {i}")
        else:
            check_step_against(m, {k: r[k][0] for k in ("root", "dof", "rbs", "df", "cf")}, ref["root"][0], ref["dof"][0], ref["rbs"][0], ref["df"][0], ref["cf"][0],
                               f"{cid} state {i}")


@pytest.mark.parametrize("backend", BACKENDS)
def test_g1_with_rigid_contact_is_refused(backend):
    """`g1-rigid` of the table does not exist: G1's torso link carries 40 ground-contact points and the rigid model's active / removed masks hold 32
    (phc_sim_check.h).  The launch is refused and nothing is written."""
    be = get_backend(backend)
    case = ec.Case("g1-rigid", "g1_humanoid", (("contact_model", "tgs"),))
    assert ec.models_on(be, case)[1].max_body_contact_pts == 40
    rc, out, wrong = ec.launch(be, case, [0, 1, 2], states=ec.states_of(ec.CASES["g1-lag"]))
    assert rc == ec.UNSUPPORTED and not wrong
    for t in ("rbs", "cf", "df"):
        assert (out[t].view(np.uint32) == ec.PATTERN).all(), t


# ---------------------------------------------------------------------------------------------------------------
# 3. guards and alignment
# ---------------------------------------------------------------------------------------------------------------
def _lead_cases(case):
    written = ec.outputs_of(case)
    cases = [("all k = 1", 1), ("all k = 2", 2), ("all k = 3", 3)]
    for t in written:   # one tensor off 16 bytes, the others on: stage_aligned ORs five pointers
        cases += [(f"{t} alone k = 1", {t: 1}), (f"{t} alone k = 2", {t: 2})]
    return cases


@pytest.mark.parametrize("n", [4, 3])
@pytest.mark.parametrize("backend,cid", _over(ec.TWO_PER_WAVEFRONT))
def test_guards_and_alignment(backend, cid, n):
    """Two envs per wavefront, N = 4 (two full wavefronts) and N = 3 (the last one half filled).  Every written tensor 16-byte aligned (staged epilogue), all of them 4 /
    8 / 4 bytes off together (direct epilogue with two full envs per wavefront: group 1 stores for itself), and each one alone 4 and 8 bytes off with the others
    aligned: the outputs are bit-equal to the aligned run and to the single-env references, and every guard word is intact."""
    case, be = ec.CASES[cid], get_backend(backend)
    refs = ec.references(backend, case)
    keys = ec.outputs_of(case)
    rows = list(range(n))
    base, wrong = _run(be, case, rows)
    lines = [f"k = 0: {w}" for w in wrong] + ec.mismatches(base, ec.stack_refs(refs, rows), keys, "k = 0 vs ref:")
    for tag, lead in _lead_cases(case):
        out, wrong = _run(be, case, rows, lead=lead)
        lines += [f"{tag}: {w}" for w in wrong]
        lines += ec.mismatches(out, base, keys, f"{tag} vs k = 0:")
        lines += ec.mismatches(out, ec.stack_refs(refs, rows), keys, f"{tag} vs ref:")
    assert not lines, f"{cid} N = {n} on {backend}: {len(lines)} problems\n" + "\n".join(lines[:40])


# ---------------------------------------------------------------------------------------------------------------
# 4. optional outputs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,cid", _over(ec.TWO_PER_WAVEFRONT))
def test_optional_outputs_may_be_null(backend, cid):
    """`dof_force`, `contact_force`, both, and `force_sensor` handed over as null pointers (stage_layout moves every later slice; aba_store_state,
    aba_publish_body, aba_publish_contact_rigid and aba_publish_sensors test for null), N = 4, aligned (staged) and 4 bytes off (direct): every remaining output is
    bit-equal to the all-present run, the buffers of the absent ones and every guard stay untouched."""
    case, be = ec.CASES[cid], get_backend(backend)
    rows = [0, 1, 2, 3]
    lines = []
    for lead in (0, 1):
        full, wrong = _run(be, case, rows, lead=lead)
        lines += [f"all present, k = {lead}: {w}" for w in wrong]
        for null in [("df",), ("cf",), ("cf", "df")] + ([("fs",), ("cf", "df", "fs")] if case.sensors else []):
            out, wrong = _run(be, case, rows, lead=lead, null=null)
            tag = f"null {'+'.join(null)}, k = {lead}:"
            lines += [f"{tag} {w}" for w in wrong]
            lines += ec.mismatches(out, full, ec.outputs_of(case, null), tag)
    assert not lines, f"{cid} on {backend}: {len(lines)} problems\n" + "\n".join(lines[:40])


# ---------------------------------------------------------------------------------------------------------------
# 5. refresh entry points
# ---------------------------------------------------------------------------------------------------------------
def _refresh_alone(backend, case):
    """rigid_body_state of each of the seven states from the N = 1 refresh"""
    def make():
        be = get_backend(backend)
        s = ec.states_of(case, 7)
        alone = []
        for i in range(7):
            rc, out, wrong = ec.launch(be, case, [i], entry="refresh", states=s)
            assert rc == 0 and not wrong, (rc, wrong)
            assert np.isfinite(out["rbs"]).all()
            alone.append(out)
        for i in range(7):
            for j in range(i):
                assert not np.array_equal(alone[i]["rbs"], alone[j]["rbs"])
        return alone
    return ec.cached(("refresh", backend, case.id), make)


@pytest.mark.parametrize("backend,cid", _over(ec.REFRESH_MODELS))
def test_refresh_body_state(backend, cid):
    """phc_refresh_body_state over five states (and reversed): every env's rigid_body_state is, bit for bit, what the N = 1 refresh of its state gives; root_states,
    dof_state and every tensor the refresh does not own are unchanged; guards intact.  rigid_body_state 16-byte aligned and 4 bytes off."""
    case, be = ec.CASES[cid], get_backend(backend)
    s = ec.states_of(case, 7)
    alone = _refresh_alone(backend, case)
    lines = []
    for rows in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0]):
        for lead in (0, {"rbs": 1}):
            rc, out, wrong = ec.launch(be, case, rows, lead=lead, entry="refresh", states=s)
            assert rc == 0
            tag = f"rows {rows} lead {lead}:"
            lines += [f"{tag} {w}" for w in wrong]
            lines += ec.mismatches(out, ec.stack_refs(alone, rows), ("rbs",), tag)
            want = dict(root=s["root"][rows], dof=s["dof"][rows], pd=s["target"][rows], cf=ec._pattern(out["cf"].shape), df=ec._pattern(out["df"].shape))
            lines += ec.mismatches(out, want, ("root", "dof", "pd", "cf", "df"), tag + " untouched")
    assert not lines, "\n".join(lines[:40])


LISTS = [[6], [0], [3, 0, 6], [5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5, 6]]


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ec.REFRESH_MODELS)
def test_refresh_body_state_indexed(cid):
    """phc_refresh_body_state_indexed over seven states, rigid_body_state pre-filled with the guard pattern: the last env alone, the first alone, an odd unordered list
    (`slot >= num_listed` in the second group of the last wavefront), six in descending order, all seven.  Listed rows are the full refresh's rows, unlisted rows still
    hold the pattern; an empty list returns 0 and a null list with num > 0 PHC_EINVAL (include/phc_amd.h), neither with a launch.  (Device only: the host emulation has no
    indexed refresh.)"""
    case, be = ec.CASES[cid], get_backend("hip")
    s = ec.states_of(case, 7)
    alone = _refresh_alone("hip", case)
    rows = list(range(7))
    lines = []
    rc, full, wrong = ec.launch(be, case, rows, entry="refresh", states=s)
    assert rc == 0 and not wrong
    lines += ec.mismatches(full, ec.stack_refs(alone, rows), ("rbs",), "full refresh:")
    for ids in LISTS:
        rc, out, wrong = ec.launch(be, case, rows, entry="refresh_indexed", env_ids=ids, states=s)
        assert rc == 0
        tag = f"list {ids}:"
        lines += [f"{tag} {w}" for w in wrong]
        lines += ec.mismatches(out, full, ("rbs",), tag, envs=ids)
        rest = [e for e in rows if e not in ids]
        lines += ec.mismatches(out, dict(rbs=ec._pattern(out["rbs"].shape)), ("rbs",), tag + " unlisted", envs=rest)
        lines += ec.mismatches(out, dict(root=s["root"][rows], dof=s["dof"][rows]), ("root", "dof"), tag + " untouched")
    for ids, num, code in (([0, 1], 0, 0), (None, 3, ec.EINVAL)):
        rc, out, wrong = ec.launch(be, case, rows, entry="refresh_indexed", env_ids=ids, num=num, states=s)
        assert rc == code and not wrong, (ids, num, rc, wrong)
        assert (out["rbs"].view(np.uint32) == ec.PATTERN).all(), "nothing may be launched"
    assert not lines, "\n".join(lines[:40])
