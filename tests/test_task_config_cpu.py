"""CPU: what a task's constructor decides before it touches the device -- `HumanoidIm.host_only(cfg)` runs the host phases alone.

  1. the observation / AMP sizes the learner's networks are shaped by, per configuration (the numbers tests/test_env_gpu.py and
     tests/test_config_sizes_gpu.py assert on the device, copied, not recomputed)
  2. every refusal of the host phases, and that the first of two wins
  3. the stepper switches as they arrive in phc_sim_params_t
  4. the synthetic motion specs (`phc_amd.utils.synthetic_motion.motion_from_spec`) against the generators called directly"""
import numpy as np
import pytest

from phc_amd.config import compose
from phc_amd.utils import synthetic_motion as sm

H1_OVER = ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"]
G1_OVER = ["robot=unitree_g1", "env=env_im_g1_phc", "sim=robot_sim", "control=robot_control"]
GETUP = ["env.task=HumanoidImGetup", "env.recoveryEpisodeProb=0.5", "env.recoverySteps=8", "env.fallInitProb=0.5"]   # (the task's three required options)
SHAPES = ["robot.has_shape_variation=True", "robot.has_shape_obs=True", "robot.has_shape_obs_disc=True", "robot.has_weight_obs=True"]
FUT = ["env.fut_tracks=True", "env.numTrajSamples=3"]
PUSH = ["+perturb.force_n=[50,100]"]


def host_task(*over):
    from phc_amd.env.tasks import humanoid_im, humanoid_im_getup, humanoid_im_mcp, humanoid_im_mcp_getup
    cfg = compose(["env.num_envs=8", *over])
    for mod in (humanoid_im, humanoid_im_getup, humanoid_im_mcp, humanoid_im_mcp_getup):
        cls = getattr(mod, cfg["env"]["task"], None)
        if cls is not None:
            return cls.host_only(cfg)
    raise KeyError(cfg["env"]["task"])


# ---- 1. sizes ----------------------------------------------------------------------------------------------------------------------------------------
def _default(t):
    assert (t.num_obs, t.get_self_obs_size(), t.get_num_amp_obs(), t.num_actions) == (934, 358, 1960, 69)
    assert t.cfg["env"]["numObservations"] == 934 and t.cfg["env"]["numActions"] == 69 and type(t)._use_reset_list is True


def _h1(t):
    assert (t.get_self_obs_size(), t.get_task_obs_size(), t.num_obs, t.get_num_amp_obs()) == (298, 480, 298 + 480, 630)
    assert t.humanoid_type == "h1" and t.num_bodies == 20 and t.control_mode == "pd" and t.control_freq_inv == 4 and t.dt == pytest.approx(0.02, abs=1e-12)


def _g1(t):
    assert (t.get_self_obs_size(), t.get_task_obs_size(), t.num_obs, t.get_num_amp_obs()) == (568, 912, 568 + 912, 990)
    assert t.humanoid_type == "g1" and t.num_bodies == 38 and t.num_extend_bodies == 1


def _vr(t):
    assert (t.get_self_obs_size(), t.get_task_obs_size(), t.num_obs) == (358, 72, 358 + 72)
    assert list(t._track_bodies) == ["Head", "L_Hand", "R_Hand"]


def _sensors(t):
    assert (t.get_self_obs_size(), t.num_obs) == (370, 370 + 576)


def _body_history(t):
    assert (t.get_self_obs_size(), t.num_obs) == (6 * 358, 6 * 358 + 576)


def _shapes(t):
    assert t.get_self_obs_size() == 358 + 11 + 10 and t._num_amp_obs_per_step == 196 + 11 and len(t.shape_models) == 3
    assert t._env_shape.tolist() == [0, 1, 2, 0, 1, 2, 0, 1]


def _fut(block):
    def check(t):
        assert host_task(f"env.obs_v={t.obs_v}").get_task_obs_size() == block                  # the single-sample task's block ...
        assert t.get_task_obs_size() == 3 * block and t.num_obs == 358 + 3 * block and t._num_traj_samples == 3   # ... three times
    return check


def _hist(t):
    assert t.num_obs == 934 + 1960 and t._hist_obs_cols == 1960


def _v5(t):
    assert t.num_obs == 934 + 30


def _v4(t):
    assert t.num_obs == 934


def _no_disc_rot(t):
    assert t._num_amp_obs_per_step == 25 and t.get_num_amp_obs() == 250 and len(t.dof_subset) == 0


def _getup(t):
    assert (t.num_obs, t.get_self_obs_size(), t.get_num_amp_obs(), t.num_actions) == (934, 358, 1960, 69)
    assert type(t).__name__ == "HumanoidImGetup" and type(t)._use_reset_list is False and t._use_reset_list is False and t._recovery_steps == 8


def _mcp_getup(t):
    assert type(t).__name__ == "HumanoidImMCPGetup" and t.num_actions == 3 and t.get_dof_action_size() == 69 and t.cfg["env"]["numActions"] == 3
    assert type(t)._use_reset_list is False


@pytest.mark.parametrize("over,check", [
    ([], _default), (H1_OVER, _h1), (G1_OVER, _g1), (["env=env_vr"], _vr), (["env.self_obs_v=3"], _sensors), (["env.self_obs_v=2"], _body_history),
    (SHAPES, _shapes),
    (FUT + ["env.obs_v=6"], _fut(24 * 24)), (FUT + ["env.obs_v=7"], _fut(9 * 24)), (FUT + ["env.obs_v=9"], _fut(18 * 24 + 6)),   # (the single-sample blocks: humanoid_im.py:486-520)
    (["+env.enableHistObs=True"], _hist), (["env.obs_v=5"], _v5), (["env.obs_v=4", "+env.past_track_steps=1"], _v4),
    (["+env.remove_disc_rot=True"], _no_disc_rot), (GETUP, _getup), (["env=env_im_getup_mcp", "learning=im_mcp", "env.num_prim=3"], _mcp_getup),
], ids=["default", "h1", "g1", "vr", "force_sensors", "body_history", "shapes", "fut_v6", "fut_v7", "fut_v9", "hist_obs", "obs_v5", "obs_v4", "no_disc_rot", "getup",
        "mcp_getup"])
def test_sizes(over, check):
    check(host_task(*over))


# ---- 2. refusals: one row per raise of the host phases, in the constructor's order ---------------------------------------------------------------
REFUSALS = [
    (["robot.humanoid_type=smplx"], NotImplementedError, "humanoid_type='smplx'"),
    (["+env.kin_loss=True"], NotImplementedError, "kin_loss=True is outside the hot path"),
    (["env.obs_v=10"], NotImplementedError, "built: obs_v 1 - 9"),
    (["env.obs_v=4", "+env.past_track_steps=5"], NotImplementedError, "past_track_steps"),
    (["env.obs_v=5", "env.fut_tracks=True"], NotImplementedError, "fut_tracks: built for the time-major"),
    (FUT + ["env.obs_v=1"], NotImplementedError, "fut_tracks: built for the time-major"),
    (FUT + ["env.obs_v=7", "+env.fut_tracks_dropout=True"], NotImplementedError, "fut_tracks_dropout"),
    (FUT + ["env.zero_out_far=True"], NotImplementedError, "fut_tracks with zero_out_far"),
    (["env.self_obs_v=2", "robot.has_shape_obs=True"], NotImplementedError, "self_obs_v=2: SMPL family"),
    (H1_OVER + ["robot.has_shape_variation=True"], NotImplementedError, "SMPL-family options"),
    (["control.control_mode=pd"], NotImplementedError, "control_mode='pd'"),
    (["env.stateInit=Hybrid"], NotImplementedError, "stateInit"),
    (["+env.ampRootHeightObs=False"], NotImplementedError, "ampRootHeightObs"),
    (H1_OVER + ["+env.amp_obs_v=2"], NotImplementedError, "amp_obs_v=2"),
    (H1_OVER + ["env.self_obs_v=3"], NotImplementedError, r"self_obs_v=3 \(foot force sensors\)"),
    (["+env.remove_disc_rot=True", "robot.has_dof_subset=False"], NotImplementedError, "remove_disc_rot empties dof_subset"),
    (["+env.enableHistObs=True", "env.self_obs_v=2"], NotImplementedError, "enableHistObs with self_obs_v=2"),
    (["env=env_vr", "env.obs_v=2"], NotImplementedError, "index the root as the first tracked body"),          # (get_task_obs_size, called for num_obs)
    (G1_OVER + ["+solver.contact=tgs"], ValueError, "at most 32 ground-contact points"),                          # (G1: 40 points on one body)
    (SHAPES[:1] + PUSH, NotImplementedError, "perturb: external wrenches .*has_shape_variation"),
    (["+solver.lane_mapping=3"] + PUSH, NotImplementedError, "perturb: external wrenches .*lane_mapping=3"),
    (["env=env_vr", "env.zero_out_far=True"], NotImplementedError, "zero_out_far needs the root"),
    (["env=env_vr", "+env.occl_training=True"], NotImplementedError, "occl_training"),
    # two options wrong at once: the earlier message wins; the later one alone gives its own
    (["env.obs_v=4", "+env.past_track_steps=5", "control.control_mode=pd"], NotImplementedError, "past_track_steps"),
    (["env.obs_v=4", "+env.past_track_steps=1", "control.control_mode=pd"], NotImplementedError, "control_mode='pd'"),
]


@pytest.mark.parametrize("over,exc,match", REFUSALS, ids=[f"{i:02d}-{m[:24].split('=')[0].split(':')[0].strip()}" for i, (_, _, m) in enumerate(REFUSALS)])
def test_refusals(over, exc, match):
    with pytest.raises(exc, match=match):
        host_task(*over)


def test_a_real_construction_refuses_a_missing_device_first(monkeypatch):
    """The two device checks stay in front of every option: a doubly-wrong call hears about the device."""
    import torch
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    bad = compose(["env.num_envs=8", "env.obs_v=10"])
    with pytest.raises(RuntimeError, match="HIP device only"):
        HumanoidIm(bad, device_type="cpu")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no HIP device visible"):
        HumanoidIm(bad)


# ---- 3. stepper switches through the config ---------------------------------------------------------------------------------------------------------
def test_stepper_switches_through_the_config():
    p = host_task()._sim_params
    assert (p.inertia_lag, p.force_average, p.contact_model, p.control_mode) == (1, 0, 0, 0)      # penalty contact, lagged inertias, isaac_pd
    assert host_task("+solver.inertia_lag=0")._sim_params.inertia_lag == 0
    tgs = host_task("+solver.contact=tgs")._sim_params
    assert tgs.inertia_lag == 0 and tgs.contact_model == 1
    assert host_task("+solver.force_average=1")._sim_params.force_average == 1
    assert host_task(*H1_OVER)._sim_params.control_mode == 2                                       # pd, continuous damping
    assert host_task(*H1_OVER, "+solver.pd_damping=held")._sim_params.control_mode == 1


# ---- 4. motion specs ----------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b)
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    else:
        assert type(a) is type(b) and a == b


@pytest.fixture(scope="module")
def models():
    from phc_amd.model import load_model
    from phc_amd.robots import ROBOTS
    return {"smpl": (load_model("smpl_humanoid"), None), **{r: (load_model(f"{r}_humanoid"), ROBOTS[r]["default_dof_pos"]) for r in ("h1", "g1")}}


SMPL_SPECS = {
    "stand": lambda m: {"stand_00000": sm.make_stand_clip(m, 10.0)},
    "stand:1": lambda m: {"stand_00000": sm.make_stand_clip(m, 1.0)},
    "armswing": lambda m: {"armswing_00000": sm.make_armswing_clip(m, 10.0)},
    "armswing:1.5": lambda m: {"armswing_00000": sm.make_armswing_clip(m, 1.5)},
    "squat": lambda m: {"squat_00000": sm.make_gait_clip(m, "squat", 10.0)},
    "squat:2": lambda m: {"squat_00000": sm.make_gait_clip(m, "squat", 2.0)},
    "stepinplace": lambda m: {"stepinplace_00000": sm.make_gait_clip(m, "stepinplace", 10.0)},
    "stepinplace:2": lambda m: {"stepinplace_00000": sm.make_gait_clip(m, "stepinplace", 2.0)},
    "walk": lambda m: {"walk_00000": sm.make_gait_clip(m, "walk", 10.0)},
    "walk:2": lambda m: {"walk_00000": sm.make_gait_clip(m, "walk", 2.0)},
    "locomotion:4": lambda m: sm.make_locomotion_library(m, 4, 0, 8.0),
    "locomotion:4:3:1": lambda m: sm.make_locomotion_library(m, 4, 3, 1.0),
    "synthetic": lambda m: sm.make_motion_dict(m.parent, 1, seed=0, body_names=m.body_names, mean_seconds=8.0, min_frames=30, base_rot=None),
    "synthetic:3:1": lambda m: sm.make_motion_dict(m.parent, 3, seed=1, body_names=m.body_names, mean_seconds=8.0, min_frames=30, base_rot=None),
    "synthetic:2:5:1.5": lambda m: sm.make_motion_dict(m.parent, 2, seed=5, body_names=m.body_names, mean_seconds=1.5, min_frames=30, base_rot=None),
}
ROBOT_SPECS = {
    "stand": lambda m, q: {"stand_00000": sm.make_robot_stand_clip(m, q, 10.0, num_extend=3, arm_swing=0.0)},
    "stand:1": lambda m, q: {"stand_00000": sm.make_robot_stand_clip(m, q, 1.0, num_extend=3, arm_swing=0.0)},
    "armswing": lambda m, q: {"armswing_00000": sm.make_robot_stand_clip(m, q, 10.0, num_extend=3, arm_swing=0.5)},
    "armswing:2": lambda m, q: {"armswing_00000": sm.make_robot_stand_clip(m, q, 2.0, num_extend=3, arm_swing=0.5)},
    "synthetic": lambda m, q: sm.make_robot_motion_dict(m, 1, seed=0, mean_seconds=8.0, num_extend=3, min_frames=30),
    "synthetic:2:1:1.0": lambda m, q: sm.make_robot_motion_dict(m, 2, seed=1, mean_seconds=1.0, num_extend=3, min_frames=30),
}


@pytest.mark.parametrize("spec", list(SMPL_SPECS))
def test_smpl_motion_specs_equal_the_generators(models, spec):
    m, _ = models["smpl"]
    got = sm.motion_from_spec(spec, m)
    assert isinstance(got, dict)
    _same(got, SMPL_SPECS[spec](m))


@pytest.mark.parametrize("robot", ["h1", "g1"])
@pytest.mark.parametrize("spec", list(ROBOT_SPECS))
def test_robot_motion_specs_equal_the_generators(models, robot, spec):
    m, q = models[robot]
    got = sm.motion_from_spec(spec, m, True, q, num_extend=3)
    assert isinstance(got, dict)
    _same(got, ROBOT_SPECS[spec](m, q))


def test_motion_spec_options_reach_the_generators(models, monkeypatch):
    m, _ = models["smpl"]
    _same(sm.motion_from_spec("synthetic:2:1:1.0", m, min_frames=45, base_rot=sm.BASE_ROT),
          sm.make_motion_dict(m.parent, 2, seed=1, body_names=m.body_names, mean_seconds=1.0, min_frames=45, base_rot=sm.BASE_ROT))
    h1, q = models["h1"]
    _same(sm.motion_from_spec("synthetic:2:1:1.0", h1, True, q, num_extend=1, min_frames=45),
          sm.make_robot_motion_dict(h1, 2, seed=1, mean_seconds=1.0, num_extend=1, min_frames=45))
    # the bare `locomotion` is 64 clips of 8 s (seconds of generation): its defaults, through a recorder
    seen = []
    monkeypatch.setattr(sm, "make_locomotion_library", lambda *a: seen.append(a) or {"x": 1})
    assert sm.motion_from_spec("locomotion", m) == {"x": 1} and seen == [(m, 64, 0, 8.0)]


def test_what_is_no_spec_passes_through(models):
    m, _ = models["smpl"]
    h1, q = models["h1"]
    d = {"clip": {"fps": 30}}
    assert sm.motion_from_spec(d, m) is d
    # a path that merely begins with a spec word is a path (before the exact head-word match, `startswith` made these clips)
    for path in ("standup_clips.pkl", "armswing_set/a.pkl", "locomotion_v2.pkl", "synthetic_amass.pkl", "walking.pkl", "data/stand:1"):
        assert sm.motion_from_spec(path, m) is path
        assert sm.motion_from_spec(path, h1, True, q, num_extend=3) is path
    # SMPL-only words with a robot model
    for spec in ("squat:2", "stepinplace", "walk:2", "locomotion:4"):
        assert sm.motion_from_spec(spec, h1, True, q, num_extend=3) is spec
