"""-m gpu: phc_sim_step_wrench -- the WRENCH instantiations of k_sim_step -- through the C ABI against the double-precision host statement of the same recursion
(emu_sim_step_wrench of oracle/hostemu/hostemu64.cpp), the push schedule's plumbing in HumanoidIm, and the evaluation sweep under pushes.  States, wrenches and tolerances are those of
tests/test_ext_wrench_cpu.py (tests/wrench_util.py)."""
import numpy as np
import pytest
import torch

import wrench_util as wu
from backends import get_backend, model_on
from phc_amd import abi

pytestmark = pytest.mark.gpu
F = np.float32
OUT = ("root", "dof", "rbs", "cf", "df")


def hip_step(name, prm, root, dof, target, num_sim_calls=2, force=None, torque=None, wrench_sim_calls=0, plain=False, pad_envs=0):
    """One launch through the C ABI.  `plain`: phc_sim_step.  `pad_envs`: the wrench tensors hold that many envs more than the launch has, filled with NaN."""
    be = get_backend("hip")
    model, mstruct, keep = model_on(be, name=name)
    n, nb, nd = root.shape[0], model.num_bodies, model.num_dof
    a = dict(root=be.arr(np.asarray(root, F)), dof=be.arr(np.asarray(dof, F)), rbs=be.zeros((n, nb, 13)), cf=be.zeros((n, nb, 3)), df=be.zeros((n, nd)),
             pd=be.arr(np.asarray(target, F)))
    sim = abi.sim_state_struct(n, a["root"], a["dof"], a["rbs"], a["cf"], a["df"], a["pd"])

    def dev(w):
        if w is None:
            return None
        full = np.full((n + pad_envs, nb, 3), np.nan, F)
        full[:n] = w
        return be.arr(full)
    fo, to = dev(force), dev(torque)
    s = torch.cuda.current_stream().cuda_stream
    if plain:
        rc = be.lib.phc_sim_step(mstruct, prm, sim, None, None, None, None, num_sim_calls, s)
    else:
        rc = be.lib.phc_sim_step_wrench(mstruct, prm, sim, None, None, None, None, num_sim_calls, abi.ptr(fo), abi.ptr(to), wrench_sim_calls, s)
    assert rc == 0, rc
    be.sync()
    return {k: be.np(a[k]) for k in OUT}


# ---- 1. null wrench ----------------------------------------------------------------------------------------------------------------------------------------
def test_null_wrench_launches_phc_sim_step():
    smpl = wu.load("smpl_humanoid")
    root, dof, target = wu.smpl_state(smpl, 3, "ground", seed=1)
    prm = wu.params(self_collision=1, inertia_lag=1)
    ref = hip_step("smpl_humanoid", prm, root, dof, target, plain=True)
    big = np.full((3, smpl.num_bodies, 3), 250.0)
    for kw in (dict(), dict(force=big, torque=big * 0.1, wrench_sim_calls=0)):
        out = hip_step("smpl_humanoid", prm, root, dof, target, **kw)
        for k in OUT:
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    pushed = hip_step("smpl_humanoid", prm, root, dof, target, force=big, wrench_sim_calls=1)
    assert np.abs(pushed["rbs"] - ref["rbs"]).max() > 0.01


def test_unsupported_configurations_are_refused():
    be = get_backend("hip")
    smpl, mstruct, keep = model_on(be)
    root, dof, target = wu.smpl_state(smpl, 2, "air")
    a = [be.arr(x) for x in (root, dof, np.zeros((2, 24, 13), F), np.zeros((2, 24, 3), F), np.zeros((2, 69), F), target)]
    sim = abi.sim_state_struct(2, *a)
    f = be.arr(np.zeros((2, 24, 3), F))
    s = torch.cuda.current_stream().cuda_stream
    assert be.lib.phc_sim_step_wrench(mstruct, wu.params(lane_mapping=3), sim, None, None, None, None, 2, abi.ptr(f), None, 1, s) == -2
    mstruct.num_shapes = 2
    mstruct.int_stride = mstruct.float_stride = 1
    assert be.lib.phc_sim_step_wrench(mstruct, wu.params(), sim, None, None, None, None, 2, abi.ptr(f), None, 1, s) == -2
    be.sync()


# ---- 2. the kernel against the fp64 statement of the recursion -------------------------------------------------------------------------------------------------
SMPL_OPTS = {"lag": dict(inertia_lag=1), "fresh": dict(inertia_lag=0), "rigid": dict(contact_model="tgs"), "self-collision": dict(inertia_lag=1, self_collision=1)}


@pytest.mark.parametrize("opts", list(SMPL_OPTS))
@pytest.mark.parametrize("wrench", ["gravity", "yaw"])
def test_smpl_matches_the_double_precision_recursion(wrench, opts):
    """N = 3: one full two-env workgroup (staged epilogue) and one half-filled one (tail path).  The wrench tensors hold one env more than the launch, NaN: a lane
    of the missing fourth env that read them would poison the workgroup's shared state."""
    smpl = wu.load("smpl_humanoid")
    prm = wu.params(**SMPL_OPTS[opts])
    if wrench == "gravity":
        root, dof, target = wu.smpl_state(smpl, 3, "ground", seed=3)
        force, torque = wu.gravity_wrench(smpl, 3, False), None
        ref = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, gravity_z=float(prm.gravity_z) + wu.DELTA_G)
    else:
        root, dof, target, force, torque = wu.yaw_case(smpl, 3)
        ref = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=2)
    out = hip_step("smpl_humanoid", prm, root, dof, target, force=force, torque=torque, wrench_sim_calls=2, pad_envs=1)
    wu.report(f"hip smpl {wrench} {opts}", out, ref)
    assert np.abs(ref["cf"]).sum() > 0
    wu.assert_standing(out, ref, rigid=opts == "rigid")


@pytest.mark.parametrize("body", wu.COUPLE_JOINTS["h1_humanoid"])
def test_h1_torque_couple(body):
    h1 = wu.load("h1_humanoid")
    root, dof, target = wu.robot_rest_state(h1, 3, 1.5)
    prm = wu.params(control_mode=1, substeps=1, sim_dt=1 / 200, limit_stiffness=2000.0, limit_damping=20.0)
    torque, tgt = wu.couple_case(h1, root, dof, target, body, 30.0)
    ref = wu.host_step(h1, prm, root, dof, tgt, 1, f64=True)
    out = hip_step("h1_humanoid", prm, root, dof, target, 1, torque=torque, wrench_sim_calls=1, pad_envs=1)
    wu.report(f"hip h1 couple {body}", out, ref)
    wu.assert_standing(out, ref)


@pytest.mark.parametrize("lag", [0, 1])
def test_robots_match_the_double_precision_recursion(lag):
    """H1 (N = 3, two envs per wavefront) and G1 (N = 2, the 64-lane mapping) near the ground under the continuous `pd` drive: a force m dg on every body plus a
    torque on the torso link."""
    for name, n, height in (("h1_humanoid", 3, 1.05), ("g1_humanoid", 2, 0.80)):
        m = wu.load(name)
        root, dof, target = wu.robot_rest_state(m, n, height)
        dof[:, :, 1] = np.random.default_rng(2).normal(0, 0.3, dof[:, :, 1].shape)
        prm = wu.params(control_mode=2, sim_dt=1 / 200, limit_stiffness=2000.0, limit_damping=20.0, self_collision=1, inertia_lag=lag)
        force = wu.gravity_wrench(m, n, False)
        torque = np.zeros((n, m.num_bodies, 3))
        torque[:, m.body_names.index("torso_link")] = (10.0, -20.0, 15.0)
        ref = wu.host_step(m, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=2)
        out = hip_step(name, prm, root, dof, target, force=force, torque=torque, wrench_sim_calls=2, pad_envs=1)
        plain = hip_step(name, prm, root, dof, target, plain=True)
        wu.report(f"hip {name} lag {lag}", out, ref)
        assert np.abs(plain["rbs"][..., 7:13] - out["rbs"][..., 7:13]).max() > 0.02
        wu.assert_standing(out, ref)


def test_corner_entries_and_independence_of_the_other_envs():
    """A wrench on body 0 of env 0 and on the last body of the last env only; env 1's entries hold a large value.  Envs 0 and 2 must come out as the fp64
    recursion gives them when it sees THEIR wrench alone: no lane reads a neighbour's entry."""
    smpl = wu.load("smpl_humanoid")
    nb = smpl.num_bodies
    root, dof, target = wu.smpl_state(smpl, 3, "ground", seed=9)
    prm = wu.params(inertia_lag=1)
    force, torque = np.zeros((3, nb, 3)), np.zeros((3, nb, 3))
    force[0, 0], torque[0, 0] = (180.0, 100.0, -50.0), (20.0, 0.0, -10.0)
    force[2, nb - 1], torque[2, nb - 1] = (-60.0, 40.0, 80.0), (3.0, -4.0, 2.0)
    ref = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=2)
    force[1], torque[1] = 500.0, -100.0
    out = hip_step("smpl_humanoid", prm, root, dof, target, force=force, torque=torque, wrench_sim_calls=2, pad_envs=1)
    sel = [0, 2]
    wu.report("hip corners", {k: out[k][sel] for k in ("root", "dof", "rbs")}, {k: ref[k][sel] for k in ("root", "dof", "rbs")})
    assert np.abs(out["rbs"][1] - ref["rbs"][1]).max() > 0.1 and np.isfinite(out["rbs"]).all()
    wu.assert_standing({k: out[k][sel] for k in ("root", "dof", "rbs")}, {k: ref[k][sel] for k in ("root", "dof", "rbs")})


# ---- 3. duration -------------------------------------------------------------------------------------------------------------------------------------------------
def test_wrench_duration():
    smpl = wu.load("smpl_humanoid")
    root, dof, target, force, torque = wu.yaw_case(smpl, 3)
    prm = wu.params(inertia_lag=1)
    s1 = wu.host_step(smpl, prm, root, dof, target, 1, f64=True, force=force, torque=torque, wrench_sim_calls=1)
    s2 = wu.host_step(smpl, prm, s1["root"], s1["dof"], target, 1, f64=True)
    both = wu.host_step(smpl, prm, root, dof, target, 2, f64=True, force=force, torque=torque, wrench_sim_calls=2)
    assert np.abs(both["rbs"][..., 7:13] - s2["rbs"][..., 7:13]).max() > 0.05
    one = hip_step("smpl_humanoid", prm, root, dof, target, force=force, torque=torque, wrench_sim_calls=1)
    wu.report("hip duration", one, s2)
    wu.assert_standing(one, s2)
    clamped = hip_step("smpl_humanoid", prm, root, dof, target, force=force, torque=torque, wrench_sim_calls=9)
    wu.assert_standing(clamped, both)


# ---- 4. the schedule's plumbing ----------------------------------------------------------------------------------------------------------------------------------
PUSH = ["+perturb.force=[200,400]", "+perturb.bodies=[Pelvis,Torso]", "+perturb.interval_s=[0.1,0.2]", "+perturb.duration_s=0.1", "+perturb.seed=3"]


def _task(extra=(), num_envs=4):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    return parse_task(compose([f"env.num_envs={num_envs}", "env.motion_file=synthetic:4:0"] + list(extra)))


def test_schedule_reaches_the_stepper():
    """HumanoidIm with a schedule, 40 steps: inside a push the stepper's outputs are, bit for bit, those of a direct phc_sim_step_wrench call on the pre-step
    snapshot with the schedule's force buffer.  The one-shot API is refused on such a task; without `perturb` the task has no schedule."""
    task, env = _task(PUSH)
    env.reset()
    n, nb, nd = task.num_envs, task.num_bodies, task.num_dof
    dev = task.device
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    checked = 0
    for step in range(40):
        act = (torch.rand(n, nd, device=dev, generator=g) * 2 - 1) * 0.2
        root0, dof0 = task._root_states.clone(), task._dof_state.clone()
        task.step(act)
        if float(task._push.force.abs().sum()) == 0 or checked >= 2:
            continue
        rbs, cf, df, pd = torch.zeros(n, nb, 13, device=dev), torch.zeros(n, nb, 3, device=dev), torch.zeros(n, nd, device=dev), torch.zeros(n, nd, device=dev)
        sim = abi.sim_state_struct(n, root0, dof0, rbs, cf, df, pd)
        a = task.actions.contiguous()
        rc = task._lib.phc_sim_step_wrench(task._model_struct, task._sim_params, sim, a.data_ptr(), task._pd_action_offset.data_ptr(),
                                           task._pd_action_scale.data_ptr(), task._freeze_mask.data_ptr(), task.control_freq_inv,
                                           task._push.force.data_ptr(), None, task.control_freq_inv, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        for got, want, what in ((task._root_states, root0, "root"), (task._dof_state, dof0, "dof"), (task._rigid_body_state, rbs.view(-1), "body state"),
                                (task._contact_forces, cf, "contact force"), (task.dof_force_tensor, df, "dof force")):
            assert torch.equal(got.reshape(-1), want.reshape(-1)), f"step {step}: {what}"
        checked += 1
    assert checked == 2 and int(task._push.pushes) >= checked
    with pytest.raises(ValueError, match="schedule"):
        task.apply_rigid_body_force_tensors(torch.zeros(n, nb, 3, device=dev))


def test_one_shot_wrench_acts_in_the_next_step_only():
    task, env = _task()
    assert task._push is None
    env.reset()
    n, nb, nd = task.num_envs, task.num_bodies, task.num_dof
    dev = task.device
    act = torch.zeros(n, nd, device=dev)
    root0, dof0 = task._root_states.clone(), task._dof_state.clone()
    f = torch.zeros(n, nb, 3, device=dev)
    f[:, 0, 0] = 300.0

    def run(push):
        task._root_states.copy_(root0)
        task._dof_state.copy_(dof0)
        if push:
            task.apply_rigid_body_force_tensors(f, None, sim_calls=1)
        task.step(act)
        a = task._root_states.clone()
        task.step(act)
        return a, task._root_states.clone()
    p1, p2 = run(False)
    q1, q2 = run(True)
    assert task._ext_pending is None
    assert float((q1[:, 7] - p1[:, 7]).min()) > 0.02, "the push must act in the step after the call"
    # direct check of "then cleared": the second step from the pushed state equals a plain step from that state
    task._root_states.copy_(root0)
    task._dof_state.copy_(dof0)
    task.apply_rigid_body_force_tensors(f, None, sim_calls=1)
    task.step(act)
    r1, d1 = task._root_states.clone(), task._dof_state.clone()
    task.step(act)
    with_clear = task._root_states.clone()
    task._root_states.copy_(r1)
    task._dof_state.copy_(d1)
    task.step(act)
    assert torch.equal(with_clear, task._root_states)


# ---- 5. evaluation under pushes ----------------------------------------------------------------------------------------------------------------------------------
SMALL = ["learning.params.config.minibatch_size=64", "learning.params.config.amp_obs_demo_buffer_size=512", "learning.params.config.amp_replay_buffer_size=512"]


def _sweep(extra, mode):
    from phc_amd.learning.amp_agent import IMAmpAgent
    task, env = _task(SMALL + list(extra) + [f"+learning.params.config.eval_metrics={mode}"])
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    info, failed = agent.eval(log=None)
    torch.cuda.synchronize()
    return info, agent


@pytest.mark.parametrize("mode", ["host", "device"])
def test_evaluation_under_pushes(mode):
    a, agent = _sweep(PUSH, mode)
    b, _ = _sweep(PUSH, mode)
    print(mode, a)
    assert a["perturb_pushes"] > 0
    assert all(np.isfinite(v) for k, v in a.items() if k != "perturb_pushes"), a
    assert a == b, "same seeds, same sweep"
    c, _ = _sweep([p if "seed" not in p else "+perturb.seed=4" for p in PUSH], mode)
    assert c["perturb_pushes"] > 0 and {k: v for k, v in c.items() if k.startswith("eval/mpjpe")} != {k: v for k, v in a.items() if k.startswith("eval/mpjpe")}
    plain, _ = _sweep([], mode)
    assert "perturb_pushes" not in plain and set(plain) == set(a) - {"perturb_pushes"}
    with pytest.raises(NotImplementedError, match="push schedule"):
        agent.train(1)
