"""The whole-step task oracle (oracle/task_oracle.py) against the reference's own outputs: in fp32 it reproduces every post-physics and reset golden
the task kernels are compared against (tests/test_task_parity.py, tests/test_h1.py), at the tolerances those tests use for the same arrays, flags and
counters exactly.  An oracle that has not met the reference's outputs decides nothing in tests/test_task_regimes.py.  CPU only, no backend."""
import numpy as np
import pytest

import task_oracle as to
import task_regimes as tr

F = np.float32


def golden_state(g, N, **over):
    """The `st` of task_oracle.post_step from a task_fns-style golden (`progress` there is the value AFTER the increment)."""
    st = dict(motion_ids=g["env_motion"].astype(np.int64), progress=(g["progress"] - 1).astype(np.int64), start=g["start_times"].astype(F),
              start_off=np.zeros(N, F), goff=np.zeros((N, 3), F), body_pos=g["body_pos"], body_rot=g["body_rot"], body_vel=g["body_vel"],
              body_ang_vel=g["body_ang_vel"], dof_pos=g["dof_pos"], dof_vel=g["dof_vel"], dof_force=g["dof_force"])
    st.update(over)
    return st


@pytest.fixture(scope="module")
def smpl(golden):
    g = golden("task_fns")
    su = tr.setup("smpl")
    np.testing.assert_array_equal(tr.oracle_cfg("smpl")["reset_ids"], np.sort(g["reset_body_ids"]))
    np.testing.assert_array_equal(tr.oracle_cfg("smpl")["key_ids"], g["key_body_ids"])
    np.testing.assert_array_equal(np.unique(g["dof_subset"] // 3) + 1, tr.oracle_cfg("smpl")["amp_joint_bodies"])
    return su, g, g["body_pos"].shape[0]


@pytest.mark.parametrize("use_mean", [False, True])
def test_post_physics_golden(smpl, use_mean):
    su, g, N = smpl
    cfg = tr.oracle_cfg("smpl", use_mean_termination=use_mean)
    trace = {}
    o = to.post_step(su.lib, cfg, golden_state(g, N), F, trace)
    assert all(v.dtype == F for k, v in o.items() if k in tr.POST_FLOAT and v is not None)
    np.testing.assert_array_equal(o["progress"], g["progress"])
    np.testing.assert_array_equal(trace["t_rew"], g["motion_times"])
    np.testing.assert_array_equal(trace["pass_time"], g["pass_time"].astype(bool))
    np.testing.assert_allclose(o["reward_raw"][:, :4], g["reward_raw"], atol=1e-5)
    np.testing.assert_allclose(o["reward_raw"][:, 4], g["power_reward"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(o["reward"], g["reward"] + g["power_reward"], atol=1e-5)
    np.testing.assert_array_equal(o["reset"], g["reset_mean" if use_mean else "reset"])
    np.testing.assert_array_equal(o["terminate"], g["terminate_mean" if use_mean else "terminate"])
    np.testing.assert_allclose(o["self_obs"], g["self_obs"], atol=1e-5)
    np.testing.assert_allclose(o["task_obs"], g["task_obs"], atol=1e-5)
    np.testing.assert_allclose(o["amp_obs"], g["amp_obs"], atol=1e-5)
    np.testing.assert_allclose(o["ref1_pos"], g["ref1_pos"], atol=2e-5)
    np.testing.assert_allclose(o["ref1_rot"], g["ref1_rot"], atol=2e-5)
    np.testing.assert_allclose(o["ref1_vel"], g["ref1_vel"], atol=2e-5)
    # the fp64 run: same decisions on these goldens, floats within the fp32 formulas' own error (slerp of two mocap frames divides sin(t acos c) by
    # sqrt(1 - c^2) at c ~ 1 - 1e-4, where an ulp of c is 6e-4 of either: up to 2e-4 on the reference rotations and on the reward's rotation term)
    o64 = to.post_step(su.lib, cfg, golden_state(g, N), np.float64)
    assert o64["task_obs"].dtype == np.float64 and o64["reward"].dtype == np.float64
    for k in ("progress", "reset", "terminate"):
        np.testing.assert_array_equal(o64[k], o[k])
    for k in ("self_obs", "amp_obs"):
        np.testing.assert_allclose(o64[k], o[k], atol=1e-5)
    for k in ("task_obs", "reward"):
        np.testing.assert_allclose(o64[k], o[k], atol=1e-3)


def test_cycle_motion_zero_out_far_golden(smpl, golden):
    su, _, _ = smpl
    g = golden("task_fns_cfg3")
    N = g["body_pos"].shape[0]
    cfg = tr.oracle_cfg("smpl", power_coefficient=0.00005, cycle_motion=True, zero_out_far=True, close_distance=0.25, far_distance=3.0)
    gg = dict(g, dof_pos=np.zeros((N, 69), F))
    st = golden_state(gg, N, start_off=g["start_off"].astype(F), goff=g["global_offset"].astype(F), cycle_counter=g["cycle_counter_in"],
                      point_goal=g["point_goal_prev"], cycle_phase=g["cycle_phase"])
    trace = {}
    o = to.post_step(su.lib, cfg, st, F, trace)
    np.testing.assert_array_equal(o["progress"], g["progress"])
    np.testing.assert_array_equal(o["cycle_counter"], g["cycle_counter_out"])
    np.testing.assert_array_equal(o["start"], g["start_times_out"])
    np.testing.assert_array_equal(o["start_off"], g["start_off_out"])
    np.testing.assert_allclose(o["goff"], g["global_offset_out"], atol=1e-6)
    np.testing.assert_allclose(o["reward_raw"], g["reward_raw"], atol=2e-5)
    np.testing.assert_allclose(o["reward"], g["reward"], atol=3e-5)
    np.testing.assert_array_equal(o["reset"], g["reset"])
    np.testing.assert_array_equal(o["terminate"], g["terminate"])
    np.testing.assert_allclose(o["point_goal"], g["point_goal_out"], atol=1e-5)
    np.testing.assert_allclose(o["task_obs"], g["task_obs"], atol=2e-5)
    np.testing.assert_array_equal(trace["pass_len"], g["pass_len"].astype(bool))
    np.testing.assert_array_equal(trace["zof_close"], g["zeros_subset"].astype(bool))
    np.testing.assert_array_equal(trace["zof_far"], g["far_subset"].astype(bool))
    np.testing.assert_array_equal(trace["reward_far"], g["reward_far"].astype(bool))
    # the random offsets of a restart (humanoid_im.py:1131-1140)
    uv = np.random.default_rng(8).random((N, 2)).astype(F)
    cycled = g["pass_len"].astype(bool)
    for kw, add in ((dict(cycle_motion_xp=True), uv), (dict(zero_out_far_train=True), to.disk_offset(uv, F))):
        o2 = to.post_step(su.lib, dict(cfg, **kw), dict(st, offset_rand=uv), F)
        want = g["global_offset_out"].astype(F).copy()
        want[cycled, :2] += add[cycled]
        np.testing.assert_allclose(o2["goff"], want, atol=3e-6)
        np.testing.assert_array_equal(o2["start"], g["start_times_out"])


@pytest.mark.parametrize("obs_v,mask,use_mean", [(6, "fixed", False), (6, "random", True), (7, "random", False), (8, "fixed", True), (8, "random", False)])
def test_occlusion_golden(smpl, golden, obs_v, mask, use_mean):
    su, g, N = smpl
    go = golden("task_occl")
    cfg = tr.oracle_cfg("smpl", obs_v=obs_v, use_mean_termination=use_mean, termination_distances=np.full(24, go["term_dist"][int(use_mean)], F))
    o = to.post_step(su.lib, cfg, golden_state(g, N, occl_mask=go[f"mask_{mask}"]), F)
    np.testing.assert_allclose(o["task_obs"], go[f"v{obs_v}_{mask}"], atol=2e-5)
    np.testing.assert_allclose(o["self_obs"], g["self_obs"], atol=1e-5)
    np.testing.assert_array_equal(o["terminate"], go[f"terminate_{mask}_mean{int(use_mean)}"])
    np.testing.assert_array_equal(o["reset"], go[f"reset_{mask}_mean{int(use_mean)}"])
    np.testing.assert_allclose(o["reward"], g["reward"] + g["power_reward"], atol=1e-5)


def test_three_point_and_keypoint_goldens(smpl, golden):
    su, g, N = smpl
    gv, g7 = golden("task_fns_vr"), golden("task_fns_v7")
    vr = ["Head", "L_Hand", "R_Hand"]
    o = to.post_step(su.lib, tr.oracle_cfg("smpl", track=vr, reset=vr), golden_state(g, N), F)
    np.testing.assert_allclose(o["task_obs"], gv["task_obs"], atol=1e-5)
    np.testing.assert_array_equal(o["reset"], gv["reset"])
    np.testing.assert_array_equal(o["terminate"], gv["terminate"])
    np.testing.assert_allclose(o["reward_raw"][:, :4], g["reward_raw"], atol=1e-5)
    for track, key in ((None, "task_obs"), (vr, "task_obs_vr")):
        o = to.post_step(su.lib, tr.oracle_cfg("smpl", track=track, obs_v=7), golden_state(g, N), F)
        np.testing.assert_allclose(o["task_obs"], g7[key], atol=1e-5)


@pytest.mark.parametrize("obs_v,upright", [(1, True), (2, True), (3, True), (8, True), (9, True), (2, False), (8, False), (9, False)])
def test_task_obs_versions_golden(smpl, golden, obs_v, upright):
    su, g, N = smpl
    want = golden("task_obs_versions")[f"v{obs_v}_u{int(upright)}"]
    cfg = tr.oracle_cfg("smpl", obs_v=obs_v, remove_base_rot=not upright)
    assert tr.obs_sizes(cfg)[1] == want.shape[1]
    o = to.post_step(su.lib, cfg, golden_state(g, N), F)
    np.testing.assert_allclose(o["task_obs"], want, atol=2e-5)


@pytest.mark.parametrize("local_root,upright", [(True, True), (True, False), (False, True), (False, False)])
def test_upright_start_golden(smpl, golden, local_root, upright):
    su, g, N = smpl
    gs = golden("obs_shape_upright")
    tag = f"l{int(local_root)}u{int(upright)}"
    o = to.post_step(su.lib, tr.oracle_cfg("smpl", local_root_obs=local_root, remove_base_rot=not upright), golden_state(g, N), F)
    np.testing.assert_allclose(o["self_obs"], gs[f"self_{tag}"][:, :358], atol=1e-5)       # (the golden's last 21 columns are the shape / limb constants)
    np.testing.assert_allclose(o["amp_obs"], gs[f"amp_{tag}"][:, :196], atol=1e-5)
    np.testing.assert_allclose(o["task_obs"], gs[f"task_v6_u{int(upright)}"], atol=1e-5)
    o7 = to.post_step(su.lib, tr.oracle_cfg("smpl", obs_v=7, remove_base_rot=not upright), golden_state(g, N), F)
    np.testing.assert_allclose(o7["task_obs"], gs[f"task_v7_u{int(upright)}"], atol=1e-5)


@pytest.mark.parametrize("upright", [True, False])
def test_self_obs_v2_history_golden(smpl, golden, upright):
    su, g, N = smpl
    g2 = golden("self_obs_v2")
    o = to.post_step(su.lib, tr.oracle_cfg("smpl", remove_base_rot=not upright), golden_state(g, N, body_state_hist=g2["hist"]), F)
    np.testing.assert_allclose(o["self_obs"], g2[f"l1u{int(upright)}"], atol=1e-5)
    np.testing.assert_array_equal(o["body_state_hist"][:, :4], g2["hist"][:, 1:])
    np.testing.assert_array_equal(o["body_state_hist"][:, 4, :, :3], g["body_pos"])


def test_self_obs_v3_force_sensors_golden(smpl, golden):
    su, g, N = smpl
    g3 = golden("self_obs_v3")
    o = to.post_step(su.lib, tr.oracle_cfg("smpl"), golden_state(g, N, force_sensor=g3["sensors"]), F)
    np.testing.assert_allclose(o["self_obs"], g3["self_obs_v3"], atol=1e-5)
    np.testing.assert_array_equal(o["self_obs"][:, 358:], g3["sensors"])


@pytest.mark.parametrize("obs_v,upright", [(6, True), (7, True), (9, True), (6, False), (9, False)])
def test_fut_tracks_golden(smpl, golden, obs_v, upright):
    su, g, N = smpl
    gv = golden("task_obs_fut_tracks")
    cfg = tr.oracle_cfg("smpl", obs_v=obs_v, remove_base_rot=not upright, num_traj_samples=3, traj_sample_timestep=1 / 30)
    o = to.post_step(su.lib, cfg, golden_state(g, N, start_off=gv["start_off"].astype(F)), F)
    np.testing.assert_allclose(o["task_obs"], gv[f"v{obs_v}_u{int(upright)}"], atol=3e-5)


def test_track_body_reward_golden(smpl, golden):
    su, g, N = smpl
    gr = golden("reward_track_bodies")
    track = [su.names[i] for i in gr["track_ids"]]
    o = to.post_step(su.lib, tr.oracle_cfg("smpl", track=track, power_reward=False, track_body_reward=True), golden_state(g, N), F)
    np.testing.assert_allclose(o["reward"], gr["reward"], atol=1e-5)
    np.testing.assert_allclose(o["reward_raw"], gr["reward_raw"], atol=1e-5)


@pytest.mark.parametrize("rb", ["h1", "g1"])
def test_robot_post_physics_golden(golden, rb):
    su = tr.setup(rb)
    g = golden(f"task_fns_{rb}")
    N = g["body_pos"].shape[0]
    cfg = tr.oracle_cfg(rb)
    np.testing.assert_array_equal(cfg["ext_parent"], g["ext_parent"])
    np.testing.assert_array_equal(cfg["ext_pos"], g["ext_pos"])
    np.testing.assert_array_equal(cfg["key_ids"], g["key_body_ids"])
    o = to.post_step(su.lib, cfg, golden_state(g, N), F)
    np.testing.assert_allclose(o["reward_raw"][:, :4], g["reward_raw"], atol=1e-5)
    np.testing.assert_allclose(o["reward_raw"][:, 4], g["power_reward"], atol=1e-5, rtol=1e-5)
    np.testing.assert_allclose(o["reward"], g["reward"] + g["power_reward"], atol=1e-5)
    np.testing.assert_array_equal(o["reset"], g["reset"])
    np.testing.assert_array_equal(o["terminate"], g["terminate"])
    np.testing.assert_allclose(o["self_obs"], g["self_obs"], atol=1e-5)
    np.testing.assert_allclose(o["task_obs"], g["task_obs"], atol=2e-5)
    np.testing.assert_allclose(o["amp_obs"], g["amp_obs"], atol=1e-5)
    np.testing.assert_allclose(o["ref1_pos"], g["ref1_pos"], atol=2e-5)
    np.testing.assert_allclose(o["ref1_dof_pos"], g["ref1_dof_pos"], atol=2e-5)


def test_without_a_trace_the_results_are_the_same_bits(smpl):
    su, g, N = smpl
    cfg = tr.oracle_cfg("smpl")
    a, b = to.post_step(su.lib, cfg, golden_state(g, N), F), to.post_step(su.lib, cfg, golden_state(g, N), F, {})
    for k in a:
        if a[k] is not None:
            np.testing.assert_array_equal(a[k], b[k])
