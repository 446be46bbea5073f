"""-m gpu: phc_sim_step_dr -- the DR instantiations of k_sim_step -- and phc_dr_advance through the C ABI, and `domain_rand=h1_dr` in HumanoidIm.

The oracle of the stepper cases is the double-precision host stepper run ONCE PER ENV on that env's own statically modified model and friction
(tests/dr_util.py `oracle`); torque noise as the shifted PD target, one 1-call launch per simulate call, chained.  Tolerances are the project's
(wrench_util.assert_standing: 3e-4 / 3e-3, rigid 5e-4 / 1e-2), and every comparison first asserts that the randomisation moves the fp64 result by at least ten
times the velocity tolerance against the nominal run.  N = 3 with 32-lane groups: one full two-env workgroup (staged epilogue) and a half-filled one; the
per-env tensors hold one env more than the launch, NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

import dr_util as du
import wrench_util as wu
from phc_amd import _lib as L
from phc_amd import abi

pytestmark = pytest.mark.gpu
F = np.float32
OUT = ("root", "dof", "rbs", "cf", "df", "pd")
FRICTION = [0.3, 1.0, 0.6]


@pytest.fixture(scope="module")
def h1():
    m = wu.load("h1_humanoid")
    return m, du.sliding_state(m, 3, True)


def _sub(d, sel):
    return {k: d[k][sel] for k in ("root", "dof", "rbs")}


def _compare(name, out, ref, nominal, rigid=False, changed=None):
    """`changed`: the envs whose physics differ from the nominal run (all by default) -- each must differ by 10 x the velocity tolerance."""
    n = ref["root"].shape[0]
    need = 10 * (du.VEL_TOL_RIGID if rigid else du.VEL_TOL)
    for e in (range(n) if changed is None else changed):
        eff = du.effect(_sub(ref, [e]), _sub(nominal, [e]))
        print(f"{name}: env {e} differs from the nominal run by {eff:.3f} (needs {need})")
        assert eff >= need, (name, e, eff)
    wu.report(name, out, ref)
    assert np.isfinite(out["rbs"]).all()
    wu.assert_standing(out, ref, rigid=rigid, tag=name)


# ---- 1. null dr ----------------------------------------------------------------------------------------------------------------------------------------
def test_null_dr_launches_phc_sim_step(h1):
    smpl = wu.load("smpl_humanoid")
    cases = [([smpl], wu.params(self_collision=1, inertia_lag=1), wu.smpl_state(smpl, 3, "ground", seed=1), 2),
             ([h1[0]], du.robot_params(1, self_collision=1), h1[1], 4)]
    for models, prm, (root, dof, target), calls in cases:
        ref = du.hip_step_dr(models, None, prm, root, dof, target, calls, plain=True)
        for kw in (dict(null_dr=True), dict()):   # a null pointer; a struct whose tensors are both null
            out = du.hip_step_dr(models, None, prm, root, dof, target, calls, **kw)
            for k in OUT:
                np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
        slid = du.hip_step_dr(models, None, prm, root, dof, target, calls, friction=[0.2, 0.2, 0.2])
        assert np.abs(slid["rbs"] - ref["rbs"]).max() > 1e-3


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched(h1):
    m, (root, dof, target) = h1
    smpl = wu.load("smpl_humanoid")
    sroot, sdof, starget = wu.smpl_state(smpl, 3, "ground", seed=1)
    amp = np.tile(0.01 * m.dof_effort, (3, 1)).astype(F)
    noise = (amp, [1, 2, 3], du.KEY, 0)

    def untouched(out, r, d):
        np.testing.assert_array_equal(out["root"], np.asarray(r, F))
        np.testing.assert_array_equal(out["dof"], np.asarray(d, F))
        assert not out["rbs"].any() and not out["cf"].any() and not out["df"].any()
    untouched(du.hip_step_dr([m], None, wu.params(lane_mapping=3), root, dof, target, 2, friction=FRICTION, expect=-2), root, dof)
    untouched(du.hip_step_dr([m], None, du.robot_params(1, mode=0), root, dof, target, 2, noise=noise, expect=-2), root, dof)
    untouched(du.hip_step_dr([smpl], None, wu.params(), sroot, sdof, starget, 2, noise=(np.zeros((3, 69), F), [1, 2, 3], du.KEY, 0), expect=-2), sroot, sdof)
    untouched(du.hip_step_dr([m], None, du.robot_params(1), root, dof, target, 2, noise=(amp, [1, 2, 3], du.KEY, -1), expect=-1), root, dof)
    untouched(du.hip_step_dr([m], None, du.robot_params(1), root, dof, target, 2, noise=(amp, [1, 2, 3], du.KEY, (1 << 32) // 19), expect=-1), root, dof)
    # torque noise without k; env-shape blocks without env_shape; and phc_sim_step keeps refusing blocks of a revolute model
    from backends import get_backend, model_on
    be = get_backend("hip")
    _, ms, keep = model_on(be, name="h1_humanoid")
    a = [be.arr(np.asarray(x, F)) for x in (root, dof, np.zeros((3, 20, 13)), np.zeros((3, 20, 3)), np.zeros((3, 19)), target)]
    sim = abi.sim_state_struct(3, *a)
    amp_d = be.arr(amp)
    dr = L.SimDr()
    dr.torque_noise = abi.ptr(amp_d)
    s = torch.cuda.current_stream().cuda_stream
    assert be.lib.phc_sim_step_dr(ms, du.robot_params(1), sim, None, None, None, None, 2, C.byref(dr), s) == -1
    ms.num_shapes, ms.int_stride, ms.float_stride = 2, 1, 1
    assert be.lib.phc_sim_step_dr(ms, du.robot_params(1), sim, None, None, None, None, 2, None, s) == -1
    assert be.lib.phc_sim_step(ms, du.robot_params(1), sim, None, None, None, None, 2, s) == -2
    be.sync()
    np.testing.assert_array_equal(be.np(a[0]), np.asarray(root, F))
    assert not be.np(a[2]).any()


# ---- 3. friction ---------------------------------------------------------------------------------------------------------------------------------------
SMPL_OPTS = {"lag": dict(inertia_lag=1), "fresh": dict(inertia_lag=0), "tgs": dict(contact_model="tgs")}


@pytest.mark.parametrize("opts", list(SMPL_OPTS))
def test_smpl_per_env_friction(opts):
    smpl = wu.load("smpl_humanoid")
    root, dof, target = du.sliding_state(smpl, 3, False, seed=3)
    prm = wu.params(**SMPL_OPTS[opts])
    nominal = du.oracle([smpl], None, prm, root, dof, target, 2)
    ref = du.oracle([smpl], None, prm, root, dof, target, 2, friction=FRICTION)
    out = du.hip_step_dr([smpl], None, prm, root, dof, target, 2, friction=FRICTION)
    _compare(f"smpl friction {opts}", out, ref, nominal, rigid=opts == "tgs", changed=[0, 2])


@pytest.mark.parametrize("lag", [0, 1])
def test_h1_per_env_friction(h1, lag):
    m, (root, dof, target) = h1
    prm = du.robot_params(lag)
    nominal = du.oracle([m], None, prm, root, dof, target, 4)
    ref = du.oracle([m], None, prm, root, dof, target, 4, friction=FRICTION)
    out = du.hip_step_dr([m], None, prm, root, dof, target, 4, friction=FRICTION)
    _compare(f"h1 friction lag {lag}", out, ref, nominal, changed=[0, 2])


# ---- 4. model blocks -----------------------------------------------------------------------------------------------------------------------------------
def test_h1_model_blocks(h1):
    """K = 3 blocks -- mass x 1.3 on pelvis / torso / one hip; torso CoM + (0.1, -0.1, 0.2); kp x 1.25, kd x 0.75 -- and env_shape = [2, 0, 1]."""
    m, (root, dof, target) = h1
    models = [du.variant(m, w) for w in ("mass", "com", "gain")]
    shape = [2, 0, 1]
    prm = du.robot_params(1)
    nominal = du.oracle([m], None, prm, root, dof, target, 4)
    ref = du.oracle(models, shape, prm, root, dof, target, 4)
    out = du.hip_step_dr(models, shape, prm, root, dof, target, 4)
    _compare("h1 blocks", out, ref, nominal)


def test_g1_model_blocks():
    """The 64-lane mapping: N = 2, K = 2, env_shape = [1, 0]; block 1 changes masses, the torso's CoM and the gains."""
    g1 = wu.load("g1_humanoid")
    root, dof, target = du.sliding_state(g1, 2, True, height=0.8)
    models = [g1, du.variant(g1, "all")]
    prm = du.robot_params(1)
    nominal = du.oracle([g1], None, prm, root, dof, target, 4)
    ref = du.oracle(models, [1, 0], prm, root, dof, target, 4)
    out = du.hip_step_dr(models, [1, 0], prm, root, dof, target, 4)
    _compare("g1 blocks", out, ref, nominal, changed=[0])
    np.testing.assert_array_equal(out["pd"], np.asarray(target, F))


# ---- 5. torque noise -----------------------------------------------------------------------------------------------------------------------------------
def _noise_case(m, target):
    """Amplitude 0.01 x the effort limit (3.5 N m) on every DoF: on the fp64 reference alone it moves joint rates by 1.0 (mode 2) to 1.2 rad/s (mode 1) over
    two simulate calls from the standing, sliding state (0.02 gives 2 rad/s in mode 2 but 20 rad/s in mode 1, whose held damper is unstable on H1's light
    links; 0.1 gives 8 rad/s in one call).  One drive saturates with and without the noise: the torso joint, its target 1.5 rad beyond its angle (kp x 1.5 =
    90 N m) and its effort limit lowered to 40 N m in the model both sides get -- H1's own 350 N m, saturated, throws the links to 50 - 100 rad/s within two
    calls, far outside what the fp32 tolerances cover."""
    import copy
    m = copy.copy(m)
    m.dof_effort = m.dof_effort.copy()
    j = m.dof_names.index("torso_joint")
    m.dof_effort[j] = 40.0
    amp = np.tile(0.01 * m.dof_effort, (3, 1)).astype(F)
    tgt = np.array(target, F)
    tgt[:, j] += 1.5
    assert 1.5 * m.dof_kp[j] > 2.0 * m.dof_effort[j] + amp[0, j]
    return m, amp, tgt


@pytest.mark.parametrize("mode", [1, 2])
def test_h1_torque_noise(h1, mode):
    m, (root, dof, target) = h1
    m, amp, tgt = _noise_case(m, target)
    noise = (amp, [3, 7, 11], du.KEY, 5)
    prm = du.robot_params(1, mode=mode)
    nominal = du.oracle([m], None, prm, root, dof, tgt, 2)
    ref = du.oracle([m], None, prm, root, dof, tgt, 2, noise=noise)
    rate = np.abs(ref["dof"][..., 1] - nominal["dof"][..., 1]).max()
    print(f"torque noise mode {mode}: joint rates move by up to {rate:.3f} rad/s on the reference")
    assert 0.1 <= rate <= 3.0
    out = du.hip_step_dr([m], None, prm, root, dof, tgt, 2, noise=noise)
    _compare(f"h1 torque noise mode {mode}", out, ref, nominal)
    np.testing.assert_array_equal(out["pd"], tgt)   # the published target stays the un-noised one
    again = du.hip_step_dr([m], None, prm, root, dof, tgt, 2, noise=(amp, [4, 7, 11], du.KEY, 5))
    assert np.abs(again["dof"][0] - out["dof"][0]).max() > 1e-3 and np.array_equal(again["dof"][1:], out["dof"][1:]), "k moves env 0's draws alone"


# ---- 6. all three --------------------------------------------------------------------------------------------------------------------------------------
def test_h1_friction_blocks_and_noise_with_self_collision(h1):
    m, (root, dof, target) = h1
    m, amp, tgt = _noise_case(m, target)
    noise = (amp, [2, 5, 9], du.KEY, 64)
    models = [du.variant(m, w) for w in ("mass", "com", "gain")]
    shape = [2, 0, 1]
    prm = du.robot_params(1, self_collision=1)
    nominal = du.oracle([m], None, prm, root, dof, tgt, 2)
    ref = du.oracle(models, shape, prm, root, dof, tgt, 2, friction=FRICTION, noise=noise)
    out = du.hip_step_dr(models, shape, prm, root, dof, tgt, 2, friction=FRICTION, noise=noise)
    _compare("h1 all three", out, ref, nominal)


# ---- 7. phc_dr_advance ---------------------------------------------------------------------------------------------------------------------------------
def test_dr_advance_equals_the_host_build_bit_for_bit():
    actions, progress = du.script()
    n, d = du.SCRIPT_N, du.SCRIPT_D
    host = du.HostDr(n, d, delay=(1, 3), push_interval=4, max_push_vel_xy=0.3, env_offset=11)
    host.root_states[:] = np.random.default_rng(0).normal(0, 1, (n, 13)).astype(F)
    dev = {k: torch.from_numpy(getattr(host, k).copy()).cuda() for k in du.HostDr.STATE}
    a = L.DrArgs()
    C.memmove(C.byref(a), C.byref(host.args), C.sizeof(a))
    for k in du.HostDr.STATE:
        setattr(a, k, dev[k].data_ptr())
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    for t in range(du.SCRIPT_STEPS):
        act, prog = torch.from_numpy(actions[t]).cuda(), torch.from_numpy(progress[t]).cuda()
        a.actions, a.progress_buf = act.data_ptr(), prog.data_ptr()
        assert lib.phc_dr_advance(C.byref(a), s) == 0
        torch.cuda.synchronize()
        host.advance(actions[t], progress[t])
        for k in du.HostDr.STATE:
            np.testing.assert_array_equal(dev[k].cpu().numpy(), getattr(host, k), err_msg=f"step {t}: {k}")
    assert (host.k == du.SCRIPT_STEPS).all()
    a.num_envs = -1
    assert lib.phc_dr_advance(C.byref(a), s) == -1
    a.num_envs = 0
    assert lib.phc_dr_advance(C.byref(a), s) == 0


# ---- 8. the task ---------------------------------------------------------------------------------------------------------------------------------------
def _task(*extra, seed=0):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(seed)
    return parse_task(compose(["env.num_envs=4", "env.motion_file=synthetic:3:2:2.0", "env.enableEarlyTermination=False", *du.H1_OVER, *extra]))


def _actions(t):
    g = torch.Generator().manual_seed(100 + t)
    return ((torch.rand(4, 19, generator=g) * 2 - 1) * 0.3).cuda()


def _rollout(task, env, steps):
    env.reset()
    for t in range(steps):
        task.reset_done()
        env.step(_actions(t))
    torch.cuda.synchronize()
    return [x.clone() for x in (task._root_states, task._dof_state, task._rigid_body_state, task.obs_buf)]


def test_humanoid_im_under_h1_dr():
    task, env = _task("domain_rand=h1_dr")
    assert task._dr is not None and task._dr.model_struct.num_shapes == 64 and task._model_struct.num_shapes == 1
    a = _rollout(task, env, 8)
    assert all(torch.isfinite(x).all() for x in a)
    assert (task._dr.k == 8).all() and int(task._dr.delay.min()) >= 1 and int(task._dr.delay.max()) <= 3
    assert task.actions.data_ptr() != task._dr.delayed_actions.data_ptr() and not torch.equal(task.actions, task._dr.delayed_actions)
    task_b, env_b = _task("domain_rand=h1_dr")
    b = _rollout(task_b, env_b, 8)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "same seed, same bits"
    task_c, env_c = _task("domain_rand=h1_dr", "domain_rand.has_domain_rand=False")
    assert task_c._dr is None
    c = _rollout(task_c, env_c, 8)
    assert float((a[0] - c[0]).abs().max()) > 1e-3 and float((a[1] - c[1]).abs().max()) > 1e-3

    # 4 replays of one captured reset_done + step against 4 eager steps of the twin (no env ends inside them: the captured unit's reset list stays empty)
    act = _actions(50)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        task.reset_done()
        task.step(act)
    torch.cuda.synchronize()
    for x, y in zip((task._root_states, task._dr.k, task._dr.action_queue), (task_b._root_states, task_b._dr.k, task_b._dr.action_queue)):
        assert torch.equal(x, y), "a capture launches nothing"
    for t in range(4):
        g.replay()
        task_b.reset_done()
        task_b.step(act)
    torch.cuda.synchronize()
    assert (task._dr.k == 12).all() and int(task.reset_buf.sum()) == 0 and int(task_b.reset_buf.sum()) == 0
    for name in ("_root_states", "_dof_state", "_rigid_body_state", "_pd_target"):
        assert torch.equal(getattr(task, name), getattr(task_b, name)), name
    for name in ("k", "delay", "action_queue", "delayed_actions"):
        assert torch.equal(getattr(task._dr, name), getattr(task_b._dr, name)), name
