"""CPU: the plain feature set of the task kernels (phc_amd/csrc/phc_im_plain.h) against the structs the tasks really build.

The header lists, once, the value every feature selector of phc_im_params_t / phc_im_buffers_t has in the default SMPL task; `im_is_plain` (host) and
`pin_plain` (device) are both generated from that list.  Here the list is parsed back out of the header, so a new entry is tested without touching this file:

  1. the default `compose([...])` task's structs satisfy `phc_im_is_plain` -- the structs come from the constructor's own phases (`HumanoidIm.host_only`, then
     the device phases run on CPU tensors: the very code that fills the structs of a real task, only the addresses are host addresses);
  2. flipping any ONE listed field makes the predicate false, and the list is not empty / names real struct fields;
  3. H1 and G1 structs, and an SMPL struct whose env needs 64 lanes, are not plain; neither are the shipped feature configs;
  4. the switch `phc_task_force_generic` is a host flag that returns the old value and leaves the predicate alone."""
import ctypes as C
import os
import re

import pytest
import torch

from phc_amd import _lib as L
from phc_amd.config import compose

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "phc_amd", "csrc", "phc_im_plain.h")
H1_OVER = ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"]
G1_OVER = ["robot=unitree_g1", "env=env_im_g1_phc", "sim=robot_sim", "control=robot_control"]


def plain_fields():
    """[(struct, field, value or None for a NULL pointer)] of PHC_IM_PLAIN_FIELDS."""
    txt = open(HEADER).read()
    body = txt[txt.index("#define PHC_IM_PLAIN_FIELDS(VAL, NUL)"):]
    body = body[:body.index("\n\n")]
    out = []
    for kind, s, f, v in re.findall(r"\b(VAL|NUL)\((prm|buf), (\w+)(?:, (-?\d+))?\)", body.split("\n", 1)[1]):
        assert (kind == "VAL") == (v != ""), (kind, f)
        out.append((s, f, int(v) if kind == "VAL" else None))
    assert len(re.findall(r"\b(?:VAL|NUL)\(", body.split("\n", 1)[1])) == len(out), "an entry of the list does not parse"
    return out


def cpu_structs(*over):
    """(task, model, lib, prm, buf) of the task `compose(over)` builds, with host addresses."""
    from phc_amd.env.tasks import humanoid_im, humanoid_im_getup
    cfg = compose(["env.num_envs=8", *over])
    cls = getattr(humanoid_im_getup, cfg["env"]["task"], None) or getattr(humanoid_im, cfg["env"]["task"])
    t = cls.host_only(cfg)
    t.device = "cpu"
    t._lib = L.load()
    for phase in ("_upload_model", "_upload_character_props", "_allocate_buffers", "_setup_action_scaling", "_allocate_im_state"):
        getattr(t, phase)()
    ids = t._sampled_motion_ids   # (the identity check of the clip-id table asks the device whether a capture is running: answered here)
    t.__dict__["_ids_identity_cache"] = (ids, ids._version, bool(torch.equal(ids, torch.arange(t.num_envs))))
    S = t._num_amp_obs_steps
    buf = t._buffers_uncached(t._amp_window(S), t._amp_window(S - 1))
    lib = L.MotionLib()   # what MotionLib.struct holds of the articulation (the frame tables play no part in the predicate)
    lib.num_bodies, lib.dofs_per_joint, lib.num_ext_bodies = t.num_bodies, t._im_params.dofs_per_joint, t._im_params.num_ext_bodies
    return t, t._model_struct, lib, t._im_params, buf


def is_plain(model, lib, prm, buf):
    return L.load().phc_im_is_plain(model, lib, prm, buf)


def clone(s):
    c = type(s)()
    C.memmove(C.byref(c), C.byref(s), C.sizeof(s))
    return c


@pytest.fixture(scope="module")
def default():
    return cpu_structs()


def test_the_list_names_struct_fields_and_the_default_task_is_plain(default):
    _, model, lib, prm, buf = default
    fields = plain_fields()
    assert len(fields) >= 15 and len(set(fields)) == len(fields)
    names = {"prm": dict(L.ImParams._fields_), "buf": dict(L.ImBuffers._fields_)}
    for s, f, v in fields:
        assert f in names[s], f"{s}.{f} is not a field of the struct"
        assert (names[s][f] is L.c_p) == (v is None), f"{s}.{f}: pointers are listed as NUL, values as VAL"
        have = getattr({"prm": prm, "buf": buf}[s], f)
        assert have == v, f"the default task's {s}.{f} is {have!r}, the list says {v!r}"
    assert is_plain(model, lib, prm, buf) == 1
    # what the list leaves alone may take any value
    p2 = clone(prm)
    p2.enable_early_termination, p2.use_mean_termination, p2.disable_collision_check, p2.max_episode_length, p2.k_pos = 0, 1, 1, 77, 3.0
    b2 = clone(buf)
    b2.reset_list, b2.reset_slot = None, 2
    assert is_plain(model, lib, p2, b2) == 1
    assert is_plain(None, lib, prm, buf) == 0 and is_plain(model, None, prm, buf) == 0 and is_plain(model, lib, None, buf) == 0 and is_plain(model, lib, prm, None) == 0


@pytest.mark.parametrize("entry", plain_fields(), ids=lambda e: f"{e[0]}.{e[1]}")
def test_flipping_one_listed_field_leaves_the_plain_set(default, entry):
    _, model, lib, prm, buf = default
    s, f, v = entry
    p2, b2 = clone(prm), clone(buf)
    for other in ([0x1000] if v is None else [v + 1, v - 1] + ([0] if v else [])):   # (a value of 0 is not read as the default by the predicate either)
        setattr({"prm": p2, "buf": b2}[s], f, other)
        assert is_plain(model, lib, p2, b2) == 0, f"{s}.{f} = {other} still counts as plain"
    setattr({"prm": p2, "buf": b2}[s], f, v)
    assert is_plain(model, lib, p2, b2) == 1


def test_robots_and_64_lane_models_are_not_plain(default):
    _, model, lib, prm, buf = default
    for over in (H1_OVER, G1_OVER):
        t, m, l, p, b = cpu_structs(*over)
        assert p.dofs_per_joint == 1 and is_plain(m, l, p, b) == 0
        # ... and not only for their features: the joint family alone decides
        p2, l2 = clone(prm), clone(lib)
        p2.dofs_per_joint = 1
        assert is_plain(model, lib, p2, buf) == 0
        l2.dofs_per_joint = 1
        assert is_plain(model, l2, prm, buf) == 0
    assert model.num_bodies == 24
    for nb, ext, want in ((32, 0, 1), (33, 0, 0), (24, 8, 1), (24, 9, 0), (64, 0, 0)):   # 32 lanes while bodies + extended bodies <= 32
        m2, p2 = clone(model), clone(prm)
        m2.num_bodies, p2.num_ext_bodies = nb, ext
        assert is_plain(m2, lib, p2, buf) == want, (nb, ext)


@pytest.mark.parametrize("over", [["env.zero_out_far=True"], ["env.obs_v=7"], ["env.fut_tracks=True", "env.numTrajSamples=3"], ["env.occl_training=True"],
                                  ["env.self_obs_v=2"], ["env.self_obs_v=3"], ["env.amp_obs_v=2"], ["env.cycle_motion=True"], ["env.power_reward=False"],
                                  ["robot.has_shape_variation=True", "robot.has_shape_obs=True", "robot.has_shape_obs_disc=True"],
                                  ["env.task=HumanoidImGetup", "env.recoveryEpisodeProb=0.5", "env.recoverySteps=8", "env.fallInitProb=0.5"]],
                         ids=lambda o: o[0].split(".", 1)[1])
def test_feature_configs_are_not_plain(over):
    _, m, l, p, b = cpu_structs(*over)
    assert is_plain(m, l, p, b) == 0


def test_rebuilding_the_parameter_struct_rechooses(default):
    """What a captured launch is keyed by (`_im_params_gen`) moves with every `_rebuild_im_params`, and the rebuilt struct carries the toggled feature.
    (No launch is captured here.  The nullable buffers are not part of `launch_generation()`: the constructor alone allocates them, and the last lines only show
    that a buffer bound later reaches the struct through `_buffer_tensors()`, not that a capture made before would be dropped.)"""
    t = cpu_structs()[0]
    lib = default[2]
    S = t._num_amp_obs_steps
    buf = lambda: t._buffers_uncached(t._amp_window(S), t._amp_window(S - 1))
    gen = t._im_params_gen
    assert is_plain(t._model_struct, lib, t._im_params, buf()) == 1
    t.self_obs_v = 3
    t._rebuild_im_params()
    assert t._im_params_gen != gen and is_plain(t._model_struct, lib, t._im_params, buf()) == 0
    gen = t._im_params_gen
    t.self_obs_v = 1
    t._rebuild_im_params()
    assert t._im_params_gen != gen and is_plain(t._model_struct, lib, t._im_params, buf()) == 1
    t._occl_mask = torch.zeros((t.num_envs, len(t._track_bodies)), dtype=torch.uint8)   # what env.occl_training allocates
    assert is_plain(t._model_struct, lib, t._im_params, buf()) == 0
    # the buffers cache serves a struct only while every tensor it was built from still is the task's: the new mask is seen
    assert any(x is t._occl_mask for x in t._buffer_tensors())


def test_force_generic_is_a_host_flag(default):
    _, model, lib, prm, buf = default
    lib_ = L.load()
    assert {"phc_task_force_generic", "phc_im_is_plain"} <= set(L.EXPORTED_SYMBOLS) and lib_.phc_abi_version() == 37
    old = lib_.phc_task_force_generic(1)
    try:
        assert old == 0
        assert lib_.phc_task_force_generic(7) == 1 and lib_.phc_task_force_generic(0) == 1 and lib_.phc_task_force_generic(1) == 0
        assert is_plain(model, lib, prm, buf) == 1   # the predicate reports the structs, not the switch
    finally:
        lib_.phc_task_force_generic(old)
    assert lib_.phc_task_force_generic(old) == old
