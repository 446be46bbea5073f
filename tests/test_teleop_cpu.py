"""HumanoidTeleop's reward launch (phc_teleop_rewards) and task options on a machine without a GPU:
  1. the host build of phc_amd/csrc/phc_teleop.h (tests/teleop_shim.cpp) against the reference's own reward methods (tests/golden/teleop_rewards.npz, made by
     tests/gen_golden_teleop.py): every term alone and all together, three chained steps, floats within 2e-5 max(1, |x|), flags and counters exact;
  2. columns: order and width of the combined reward_raw; a term that is off reads none of its nullable inputs;
  3. the recovery counter against the push law of phc_dr_advance (tests/dr_shim.cpp);
  4. the ABI: symbol, struct size, version; what the argument check refuses (a host function: no device needed);
  5. HumanoidTeleop.host_only: reward names, widths, defaulted imitation gains, every refusal by its message."""
import ctypes as C

import numpy as np
import pytest

import teleop_util as tu
from phc_amd import _lib as L
from phc_amd import abi

F = np.float32
EINVAL = -1


@pytest.fixture(scope="module")
def gold(golden):
    return golden("teleop_rewards")


def _names(g, tag):
    return [str(n)[2:] for n in g[f"{tag}/reward_names"]]


@pytest.mark.parametrize("tag", ["h1", "g1"])
def test_all_terms_three_steps_against_the_reference(gold, tag):
    """All eleven terms in the fixture's column order and scales; the state of each step is what the host build itself wrote in the step before."""
    x, names = tu.golden_case(gold, tag), _names(gold, tag)
    scales = dict(zip(names, (float(v) for v in gold[f"{tag}/reward_scales"])))
    run = tu.Runner(x, tu.host_launch, names, scales)
    worst = 0.0
    for s in range(3):
        rew, raw = run.step(s)
        assert raw.shape == (16, 5 + 11)
        np.testing.assert_array_equal(raw[:, :5], x["reward_im"][s])
        worst = max(worst, tu.close(raw[:, 5:], gold[f"{tag}/columns"][s], f"{tag} step {s} columns"), tu.close(rew, gold[f"{tag}/rew_out"][s], f"{tag} step {s} rew_buf"))
        st = run.state_np()
        np.testing.assert_array_equal(st["last_contacts"].astype(bool), gold[f"{tag}/last_contacts"][s])
        np.testing.assert_array_equal(st["last_actions"], gold[f"{tag}/last_actions"][s])
        np.testing.assert_array_equal(st["last_dof_vel"], gold[f"{tag}/last_dof_vel"][s])
        worst = max(worst, tu.close(st["feet_air_time"], gold[f"{tag}/feet_air_time"][s], f"{tag} step {s} feet_air_time"))
        assert not st["recovery_counter"].any()
    print(f"{tag}: largest error {worst:.3e}")


@pytest.mark.parametrize("term", tu.TERMS)
def test_each_term_alone_against_the_reference(gold, term):
    """A mask of one bit, scale 1, every input the term does not read passed as null: the column is the reference's raw value."""
    for tag in ("h1", "g1"):
        x, names = tu.golden_case(gold, tag), _names(gold, tag)
        col = names.index(term)
        run = tu.Runner(x, tu.host_launch, [term], with_state=term in ("dof_acc", "action_rate"))
        for s in range(3):
            rew, raw = run.step(s)
            assert raw.shape == (16, 6)
            ref = gold[f"{tag}/raw"][s][:, col]
            if term == "stumble":
                np.testing.assert_array_equal(raw[:, 5], ref)   # a flag: exact
            tu.close(raw[:, 5], ref, f"{tag} {term} step {s}")
            tu.close(rew, x["rew_in"][s].astype(np.float64) + ref, f"{tag} {term} step {s} rew_buf")
            given = {n for n, _ in L.TeleopArgs._fields_ if n in tu.INPUTS + tu.STATE and getattr(run.last_args, n)}
            assert given == run.used(), given
        if term == "feet_air_time_teleop":
            np.testing.assert_array_equal(run.state_np()["last_contacts"].astype(bool), gold[f"{tag}/last_contacts"][2])


def test_columns_follow_the_order_given_and_no_term_leaves_the_copy():
    x = tu.random_case(5, 7, [1, 3], steps=1, seed=3)
    order = ["stumble", "dof_vel", "feet_ori", "torques"]
    one = {t: tu.Runner(x, tu.host_launch, [t], {t: 0.5}).step(0)[1][:, 5] for t in order}
    for perm in (order, order[::-1], [order[2], order[0], order[3], order[1]]):
        rew, raw = tu.Runner(x, tu.host_launch, perm, {t: 0.5 for t in perm}, im_cols=4).step(0)
        assert raw.shape == (5, 8)
        np.testing.assert_array_equal(raw[:, :4], x["reward_im"][0][:, :4])
        for c, t in enumerate(perm):
            np.testing.assert_array_equal(raw[:, 4 + c], one[t])
        acc = x["rew_in"][0].copy()
        for t in perm:   # rew_buf += column, in column order, in fp32
            acc = (acc + one[t]).astype(F)
        np.testing.assert_array_equal(rew, acc)
    # R = 0: the imitation columns are copied, rew_buf is untouched, no nullable input is given (the state arrays neither)
    run = tu.Runner(x, tu.host_launch, [], with_state=False)
    rew, raw = run.step(0)
    np.testing.assert_array_equal(raw, x["reward_im"][0])
    np.testing.assert_array_equal(rew, x["rew_in"][0])
    assert not any(getattr(run.last_args, n) for n in tu.INPUTS + tu.STATE)


def test_gated_env_looks_the_reference_speed_up_one_step_later():
    """An env whose recovery counter is positive had its progress held by the post-physics launch: the air-time gate reads the frame of progress + 1."""
    x = tu.random_case(4, 3, [0, 1], steps=2, seed=11)
    x["ref_root_vel"][0, :, :2] = 0.0          # frame 1: standing
    x["ref_root_vel"][1, :, :2] = [0.3, 0.0]   # frame 2: moving
    x["feet_air_time0"][:] = 0.5
    x["contact_force"][0][:, :2] = [0, 0, 50]  # both feet land in step 0: first contact with 0.5 s of air time
    run = tu.Runner(x, tu.host_launch, ["feet_air_time_teleop"])
    run.state["recovery_counter"][:] = [0, 2, 0, 1]
    run.progress = [np.array([1, 1, 2, 1])]    # env 2 is one step ahead, envs 1 and 3 are gated at progress 1
    _, raw = run.step(0)
    expect = (F(0.5) + F(x["dt"]) - F(0.25)) * 2
    np.testing.assert_allclose(raw[:, 5], [0, expect, expect, expect], rtol=1e-6)


def test_recovery_counter_is_written_exactly_when_the_dr_launch_pushes_one_step_later():
    import dr_util as du
    n, d, interval, steps = 4, 3, 3, 3
    x = tu.random_case(n, d, [0, 1], steps=1, seed=5)
    dr = du.HostDr(n, d, delay=(0, 0), push_interval=interval, max_push_vel_xy=1.0)
    run = tu.Runner(x, tu.host_launch, [], push_interval=interval, recovery_steps=steps, with_state=False)
    progress = np.zeros(n, np.int64)
    written = []
    for step in range(10):
        dr.root_states[:, 7:9] = 0
        if step == 6:
            progress[2] = 0                          # env 2 was reset just before the push step: phc_dr_advance does not push it
        dr.advance(np.zeros((n, d), F), progress)
        pushed = np.abs(dr.root_states[:, 7:9]).sum(-1) > 0
        if step > 0:
            expect = written[-1] & ~(progress == 0)  # the envs the previous step's launch marked, minus those reset in between
            np.testing.assert_array_equal(pushed, expect)
        run.dr_k = dr.k.copy()
        run.state["recovery_counter"][:] = 0         # (the post-physics launch counts it down: here only the write is watched)
        run.step(0)
        rc = run.state_np()["recovery_counter"]
        assert set(rc.tolist()) <= {0, steps + 1}
        written.append(rc == steps + 1)
        progress += 1
    assert not written[0].any()                      # k = 1 after the first step
    assert [bool(w.all()) for w in written] == [False, False, True, False, False, True, False, False, True, False]
    # k == 0 (no step counted yet) writes nothing
    run.dr_k = np.zeros(n, np.int32)
    run.state["recovery_counter"][:] = 0
    run.step(0)
    assert not run.state_np()["recovery_counter"].any()


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbol_struct_size_and_version():
    assert "phc_teleop_rewards" in L.EXPORTED_SYMBOLS and hasattr(L.load(), "phc_teleop_rewards")
    assert L.load().phc_abi_version() == 37   # (phc_teleop_args_t and the PHC_TELEOP_* macros against their mirrors: tests/test_abi_and_host.py)


def _good_args(terms=tu.TERMS):
    x = tu.random_case(3, 4, [0, 1], steps=1, seed=1)
    run = tu.Runner(x, tu.host_launch, list(terms), push_interval=2)
    run.step(0)
    return run


def test_argument_check_returns_the_documented_codes():
    """Both the host build's check and the library's entry point (the check runs before any device work, so it needs no device)."""
    run = _good_args()
    lib_entry = lambda lib, a: L.load().phc_teleop_rewards(lib, a, None)
    checks = [lambda lib, a: tu.shim().teleop_args_check_of(lib, a), lib_entry]

    def rc_with(check, lib=True, **changes):
        a = L.TeleopArgs()
        C.memmove(C.byref(a), C.byref(run.last_args), C.sizeof(a))
        for k, v in changes.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
        return check(C.byref(run.lib) if lib else None, C.byref(a))

    for check in checks:
        if check is not lib_entry:
            assert rc_with(check) == 0
        assert check(C.byref(run.lib), None) == EINVAL
        for field in ("rew_buf", "reward_raw", "reward_im", "dof_state", "dof_limits_lower", "dof_limits_upper", "torque_limits", "dof_force", "actions",
                      "contact_force", "rigid_body_state", "progress_buf", "motion_start_times", "motion_start_times_offset", "dr_k", "recovery_counter",
                      "last_actions", "last_dof_vel", "feet_air_time", "last_contacts"):
            assert rc_with(check, **{field: None}) == EINVAL, field
        bad = [dict(num_envs=-1), dict(num_dof=0), dict(num_feet=-1), dict(num_feet=9), dict(num_feet=1), dict(num_bodies=0), dict(num_bodies=65),
               dict(feet=(1, 99)), dict(feet=(0, -1)), dict(num_im_cols=-1), dict(num_im_cols=9), dict(term_mask=1 << 11), dict(term_mask=0xFFFFFFFF),
               dict(order=(0, 11)), dict(order=(1, run.last_args.order[0])), dict(dt=0.0), dict(dt=float("nan")), dict(push_interval=-1), dict(recovery_steps=-1)]
        for b in bad:
            assert rc_with(check, **b) == EINVAL, b
        assert rc_with(check, lib=False) == EINVAL                # the air-time term without a motion library
        nolib = L.MotionLib()
        a = L.TeleopArgs()
        C.memmove(C.byref(a), C.byref(run.last_args), C.sizeof(a))
        assert check(C.byref(nolib), C.byref(a)) == EINVAL        # ... or with an empty one
        assert rc_with(check, num_envs=0) == 0                    # nothing to do: no launch
    # without the air-time term no library is needed; sampled_motion_ids is nullable; feet_ori with fewer than two feet is what num_feet=1 hit above
    run2 = _good_args([t for t in tu.TERMS if t != "feet_air_time_teleop"])
    assert tu.shim().teleop_args_check_of(None, C.byref(run2.last_args)) == 0
    a = L.TeleopArgs()
    C.memmove(C.byref(a), C.byref(run2.last_args), C.sizeof(a))
    a.num_feet, a.term_mask = 1, 1 << L.TELEOP_TERMS.index("feet_ori")
    a.order[0] = L.TELEOP_TERMS.index("feet_ori")
    assert tu.shim().teleop_args_check_of(None, C.byref(a)) == EINVAL
    a.num_feet = 2
    assert tu.shim().teleop_args_check_of(None, C.byref(a)) == 0


# ---- the task, host phases only ----------------------------------------------------------------------------------------------------------------------------
def _cfg(*extra, base=tu.H1_OVER):
    from phc_amd.config import compose
    return compose(list(base) + ["env.task=HumanoidTeleop", "env.num_envs=4", "env.motion_file=armswing:4"] + list(extra))


def test_task_reward_names_widths_and_defaulted_imitation_gains():
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    from phc_amd.env.tasks.humanoid_teleop import HumanoidTeleop
    from phc_amd.env.tasks import vec_task
    t = HumanoidTeleop.host_only(_cfg("+env.reward_specs.r_action_rate=-0.01", "+env.reward_specs.r_dof_vel=0", "+env.reward_specs.r_torques=-1e-5",
                                      "+env.reward_specs.r_feet_contact_forces=-0.01", "+env.reward_specs.max_contact_force=350"))
    assert t.reward_names == ["r_action_rate", "r_torques", "r_feet_contact_forces"]          # the dict's order, the zero scale dropped
    assert t.reward_scales == {"r_action_rate": -0.01 * t.dt, "r_torques": -1e-5 * t.dt, "r_feet_contact_forces": -0.01 * t.dt}
    assert t.max_contact_force == 350.0
    ref = HumanoidIm.host_only(_cfg())
    assert {k: t.reward_specs[k] for k in ("k_pos", "k_rot", "k_vel", "k_ang_vel", "w_pos", "w_rot", "w_vel", "w_ang_vel")} == ref.reward_specs
    assert t.num_im_reward_columns == (5 if t.power_reward else 4) and t.num_reward_columns == t.num_im_reward_columns + 3
    assert t._feet == [t._body_names.index(b) for b in t.cfg["env"]["contact_bodies"]] and t._recovery_steps == 60
    assert HumanoidTeleop.host_only(_cfg("env.push_recovery_steps=3"))._recovery_steps == 3
    assert HumanoidTeleop._post_physics_launch is not None and HumanoidIm._post_physics_launch is None
    assert HumanoidTeleop.post_physics_step is HumanoidIm.post_physics_step and HumanoidTeleop.step is HumanoidIm.step
    # no r_* key at all, no domain_rand, the SMPL family: the task is HumanoidIm plus an empty launch
    plain = HumanoidTeleop.host_only(_cfg(base=[]))
    assert plain.reward_names == [] and plain.num_reward_columns == plain.num_im_reward_columns and plain._dr is None
    smpl = HumanoidTeleop.host_only(_cfg("+env.reward_specs.r_dof_acc=-2.5e-7", "+env.reward_specs.r_stumble=-1", base=[]))
    assert smpl.reward_names == ["r_dof_acc", "r_stumble"] and smpl.reward_specs["k_pos"] == 100
    import inspect
    assert "HumanoidTeleop" in inspect.getsource(vec_task.parse_task)


def test_task_refusals_each_by_its_message():
    from phc_amd.env.tasks.humanoid_teleop import HumanoidTeleop
    h = HumanoidTeleop.host_only
    with pytest.raises(ValueError, match="r_feet_in_the_air"):
        h(_cfg("+env.reward_specs.r_feet_in_the_air=1.0"))
    for term in ("torques", "torque_limits"):
        with pytest.raises(NotImplementedError, match=f"r_{term} needs control.control_mode=pd"):
            h(_cfg(f"+env.reward_specs.r_{term}=-1e-5", "control.control_mode=isaac_pd"))
        with pytest.raises(NotImplementedError, match=f"r_{term} needs control.control_mode=pd"):
            h(_cfg(f"+env.reward_specs.r_{term}=-1e-5", base=[]))          # the SMPL family has no explicit-PD mode
        h(_cfg(f"+env.reward_specs.r_{term}=0", "control.control_mode=isaac_pd"))   # a zero scale asks for nothing
    with pytest.raises(NotImplementedError, match="control.action_filter"):
        h(_cfg("control.action_filter=True"))
    with pytest.raises(NotImplementedError, match="env.cycle_motion"):
        h(_cfg("env.cycle_motion=True"))
    with pytest.raises(ValueError, match="r_feet_ori needs two feet"):
        h(_cfg("+env.reward_specs.r_feet_ori=-1", "env.contact_bodies=[left_ankle_link]"))
    with pytest.raises(ValueError, match="max_contact_force"):
        h(_cfg("+env.reward_specs.r_feet_contact_forces=-0.01"))
