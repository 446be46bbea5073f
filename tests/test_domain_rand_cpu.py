"""CPU: domain randomisation (`domain_rand=h1_dr`) as far as it runs without a device --

  1. the built-in `h1_dr` group against the reference's yaml, key by key
  2. the sampler (phc_amd/domain_rand.py): ranges, buckets, nominal variant 0, mass / CoM / inertia bookkeeping, determinism, rank offsets
  3. what check_sim_step_dr and phc_dr_advance refuse (the host functions the entry points call before any device work; tests/dr_shim.cpp)
  4. the per-lane code of csrc/phc_dr.h through its host build: torque-noise draws, the delay law, 12 scripted steps of the action ring against a numpy
     statement of the reference's shift queue, push instants
  5. the task's host phases: refusals, the one-line notice, and `has_domain_rand: False` building exactly what the task builds without the group"""
import ctypes as C
import os

import numpy as np
import pytest

import dr_util as du
import hostemu_util as hu
import wrench_util as wu
from phc_amd import _lib as L
from phc_amd import abi
from phc_amd.config import compose

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = np.float32


# ---- 1. config ------------------------------------------------------------------------------------------------------------------------------------------
def _plain(x):
    return {k: _plain(v) for k, v in x.items()} if isinstance(x, dict) else ([_plain(v) for v in x] if isinstance(x, (list, tuple)) else x)


def test_h1_dr_group_equals_the_reference_yaml():
    ours = _plain(compose(["domain_rand=h1_dr"]).domain_rand)
    ref = _plain(compose(["domain_rand=h1_dr"], cfg_dir=os.path.join(GOLDEN, "ref_cfg")).domain_rand)
    assert set(ours) == set(ref)
    for k in ref:
        assert ours[k] == ref[k], k
    default = _plain(compose([]).domain_rand)
    assert len(default) == 10 and all(v is False for v in default.values()), "default_dr gains nothing: its ten switches, all off"


# ---- 2. sampler -----------------------------------------------------------------------------------------------------------------------------------------
def _sampler(n=256, model=None, env_offset=0, **over):
    from phc_amd.domain_rand import DomainRand
    cfg = dict(_plain(compose(["domain_rand=h1_dr"]).domain_rand), **over)
    return DomainRand(cfg, n, model or wu.load("h1_humanoid"), plane_friction=1.0, dt=0.02, default_seed=7, env_offset=env_offset)


def test_sampler_ranges_buckets_and_nominal_variant():
    h1 = wu.load("h1_humanoid")
    dr = _sampler(model=h1)
    # friction: 64 buckets of U(-0.6, 1.2), averaged with the plane's 1.0, clamped at 0
    assert dr.env_friction.dtype == F and dr.env_friction.shape == (256,) and len(np.unique(dr.env_friction)) <= 64 and len(np.unique(dr.env_friction)) > 20
    assert dr.env_friction.min() >= 0.2 - 1e-6 and dr.env_friction.max() <= 1.1 + 1e-6
    assert ((dr.friction_buckets >= -0.6) & (dr.friction_buckets <= 1.2)).all()
    # variants
    assert len(dr.models) == 64 and dr.models[0] is h1 and dr.env_shape.dtype == np.int32 and dr.env_shape.min() >= 0 and dr.env_shape.max() <= 63
    assert len(np.unique(dr.env_shape)) > 40
    listed = [h1.body_names.index(b) for b in compose(["domain_rand=h1_dr"]).domain_rand.randomize_link_body_names]
    torso = h1.body_names.index("torso_link")
    for m in dr.models[1:]:
        s = m.mass / h1.mass
        assert ((s[listed] >= 0.7) & (s[listed] <= 1.3)).all() and np.array_equal(np.delete(s, listed), np.ones(h1.num_bodies - len(listed)))
        assert m.total_mass == pytest.approx(float((h1.mass * s).sum()), rel=1e-12)
        d = m.com - h1.com
        assert np.abs(d[torso]).max() > 0 and (np.abs(d[torso]) <= [0.1, 0.1, 0.2]).all() and not np.delete(d, torso, axis=0).any()
        for r, g0, g in (((0.75, 1.25), h1.dof_kp, m.dof_kp), ((0.75, 1.25), h1.dof_kd, m.dof_kd)):
            q = g[g0 != 0] / g0[g0 != 0]
            assert (q >= r[0]).all() and (q <= r[1]).all() and len(np.unique(q)) > 1
        # inertia about the CoM: scaled with the mass, untouched by the CoM shift -- i.e. inertia_origin is the parallel-axis formula
        for j in range(h1.num_bodies):
            c0, c1 = h1.com[j], m.com[j]
            icom0 = h1.inertia_origin[j] - h1.mass[j] * (c0 @ c0 * np.eye(3) - np.outer(c0, c0))
            want = icom0 * s[j] + m.mass[j] * (c1 @ c1 * np.eye(3) - np.outer(c1, c1))
            np.testing.assert_allclose(m.inertia_origin[j], want, rtol=0, atol=1e-12)
    ints, floats = dr.pack()
    assert ints.shape[0] == floats.shape[0] == 64
    i0, f0 = h1.pack()
    np.testing.assert_array_equal(ints[0, :i0.size], i0)
    np.testing.assert_array_equal(floats[0, :f0.size], f0)
    np.testing.assert_array_equal(ints, np.broadcast_to(ints[0], ints.shape))   # one topology, one geometry
    # torque noise: rfi_lim x effort (randomize_rfi_lim False), and with the scale on
    np.testing.assert_allclose(dr.torque_noise, np.tile(0.1 * h1.dof_effort, (256, 1)).astype(F))
    q = _sampler(model=h1, randomize_rfi_lim=True).torque_noise / (0.1 * h1.dof_effort)
    assert (q >= 0.5 - 1e-6).all() and (q <= 1.5 + 1e-6).all() and len(np.unique(q)) > 1000
    assert dr.delay_range == (1, 3) and dr.push_interval == 250 and dr.max_push_vel_xy == pytest.approx(0.3)
    assert dr.ignored == ["add_noise", "added_mass_range", "noise_level", "noise_scales"]


def test_sampler_is_deterministic_and_rank_offsets_tile_one_run():
    a, b, c = _sampler(), _sampler(), _sampler(seed=8)
    for x, y in ((a.env_friction, b.env_friction), (a.env_shape, b.env_shape), (a.torque_noise, b.torque_noise), (a.pack()[1], b.pack()[1])):
        np.testing.assert_array_equal(x, y)
    assert a.key == b.key != c.key and not np.array_equal(a.env_friction, c.env_friction) and not np.array_equal(a.pack()[1], c.pack()[1])
    lo, hi = _sampler(128, randomize_rfi_lim=True), _sampler(128, env_offset=128, randomize_rfi_lim=True)
    one = _sampler(256, randomize_rfi_lim=True)
    for name in ("env_friction", "env_shape", "torque_noise"):
        np.testing.assert_array_equal(np.concatenate([getattr(lo, name), getattr(hi, name)]), getattr(one, name), err_msg=name)
    np.testing.assert_array_equal(lo.pack()[1], one.pack()[1])   # the variants are the run's, not a rank's
    assert hi.env_offset == 128


def test_sampler_switches_and_refusals():
    from phc_amd.domain_rand import DomainRand
    off = _sampler(randomize_friction=False, randomize_link_mass=False, randomize_base_com=False, randomize_pd_gain=False, randomize_torque_rfi=False,
                   randomize_ctrl_delay=False, push_robots=False)
    assert off.env_friction is None and off.env_shape is None and len(off.models) == 1 and off.torque_noise is None and off.delay_range is None
    assert off.push_interval == 0
    assert len(_sampler(num_buckets=5).models) == 5
    with pytest.raises(ValueError, match="randomize_base_mass"):
        _sampler(randomize_base_mass=True)
    cfg = _plain(compose(["domain_rand=h1_dr"]).domain_rand)
    smpl = wu.load("smpl_humanoid")
    with pytest.raises(NotImplementedError, match="randomize_torque_rfi"):
        DomainRand(cfg, 4, smpl, is_robot=False, explicit_pd=False)
    with pytest.raises(NotImplementedError, match="randomize_torque_rfi"):
        DomainRand(cfg, 4, wu.load("h1_humanoid"), is_robot=True, explicit_pd=False)
    # the friction, mass, CoM, gain and delay parts work for the SMPL family
    s = DomainRand(dict(cfg, randomize_torque_rfi=False, randomize_link_body_names=["Pelvis", "Torso"], base_com_body="Torso"), 16, smpl, is_robot=False,
                   explicit_pd=False)
    assert len(s.models) == 64 and s.env_friction is not None and s.delay_range == (1, 3)
    with pytest.raises(ValueError, match="no such body"):
        DomainRand(dict(cfg, randomize_torque_rfi=False), 16, smpl, is_robot=False, explicit_pd=False)


# ---- 3. refusals of the two entry points ------------------------------------------------------------------------------------------------------------------
def _check(model_struct, prm, sim, dr):
    return du.shim().check_sim_step_dr_of(hu.P(model_struct), hu.P(prm), hu.P(sim), None, None, None, 2, hu.P(dr))


def _host_case(name, n=3):
    m, ms, keep = hu.np_model(name)
    nb, nd = m.num_bodies, m.num_dof
    a = [np.zeros((n, 13), F), np.zeros((n, nd, 2), F), np.zeros((n, nb, 13), F), np.zeros((n, nb, 3), F), np.zeros((n, nd), F), np.zeros((n, nd), F)]
    return m, ms, keep, a, abi.sim_state_struct(n, *a)


def test_check_sim_step_dr_refusals():
    h1, ms, keep, arrs, sim = _host_case("h1_humanoid")
    amp, k, fr = np.zeros((3, 19), F), np.zeros(3, np.int32), np.ones(3, F)
    shape = np.zeros(3, np.int32)

    def dr_of(noise=True, with_k=True, friction=False, env_offset=0):
        d = L.SimDr()
        d.torque_noise, d.k = (amp.ctypes.data if noise else None), (k.ctypes.data if with_k else None)
        d.env_friction, d.key, d.env_offset = (fr.ctypes.data if friction else None), du.KEY, env_offset
        return d
    ok = du.robot_params(1)
    assert _check(ms, ok, sim, dr_of()) == 0 and _check(ms, ok, sim, dr_of(friction=True)) == 0 and _check(ms, ok, sim, None) == 0
    assert _check(ms, du.robot_params(1, mode=1), sim, dr_of()) == 0
    # PHC_EUNSUPPORTED
    assert _check(ms, wu.params(lane_mapping=3), sim, dr_of(noise=False, friction=True)) == -2
    assert _check(ms, du.robot_params(1, mode=0), sim, dr_of()) == -2
    smpl, ms_s, keep_s, arrs_s, sim_s = _host_case("smpl_humanoid")
    assert _check(ms_s, wu.params(), sim_s, dr_of()) == -2
    assert _check(ms_s, wu.params(), sim_s, dr_of(noise=False, friction=True)) == 0
    # PHC_EINVAL
    assert _check(ms, ok, sim, dr_of(with_k=False)) == -1
    assert _check(ms, ok, sim, dr_of(env_offset=-1)) == -1
    assert _check(ms, ok, sim, dr_of(env_offset=(1 << 32) // 19 - 2)) == -1 and _check(ms, ok, sim, dr_of(env_offset=(1 << 32) // 19 - 3)) == 0
    assert _check(None, ok, sim, dr_of()) == -1 and _check(ms, None, sim, dr_of()) == -1 and _check(ms, ok, None, dr_of()) == -1
    # env-shape blocks: accepted for the revolute model here with env_shape, PHC_EINVAL without it or without strides; check_sim_step's own refusals stand
    ms.num_shapes, ms.int_stride, ms.float_stride = 2, keep[0].size, keep[1].size
    assert _check(ms, ok, sim, dr_of(noise=False)) == -1
    sim2 = abi.sim_state_struct(3, *arrs, env_shape=shape)
    assert _check(ms, ok, sim2, dr_of(noise=False)) == 0 and _check(ms, ok, sim2, None) == 0
    ms.float_stride = 0
    assert _check(ms, ok, sim2, dr_of(noise=False)) == -1
    ms.float_stride = keep[1].size
    assert _check(ms, wu.params(contact_model="tgs", contact_iterations=4), sim2, dr_of(noise=False)) == 0
    bad = du.robot_params(1)
    bad.substeps = 0
    assert _check(ms, bad, sim2, dr_of(noise=False)) == -1


def test_dr_advance_argument_refusals():
    def args(**kw):
        h = du.HostDr(4, 19, delay=kw.pop("delay", (1, 3)), push_interval=kw.pop("push_interval", 5), max_push_vel_xy=kw.pop("v", 0.3),
                      env_offset=kw.pop("env_offset", 0))
        act = np.zeros((4, 19), F)
        h.args.actions = act.ctypes.data
        for k, v in kw.items():
            setattr(h.args, k, v)
        return h, act
    chk = lambda h: du.shim().dr_args_check_of(C.byref(h[0].args))
    assert chk(args()) == 0 and chk(args(delay=(0, 0), action_queue=None)) == 0 and chk(args(push_interval=0, root_states=None)) == 0
    assert chk(args(num_envs=0)) == 0
    assert du.shim().dr_args_check_of(None) == -1
    for bad in (dict(actions=None), dict(delayed_actions=None), dict(delay=None), dict(k=None), dict(action_queue=None), dict(root_states=None),
                dict(num_envs=-1), dict(num_dof=0), dict(delay_lo=-1), dict(delay_lo=4), dict(delay_hi=1024), dict(push_interval=-1), dict(v=-0.1),
                dict(v=float("inf")), dict(v=float("nan")), dict(env_offset=-1), dict(env_offset=(1 << 32) - 3)):
        if "delay" in bad and bad["delay"] is None:   # (the pointer, not the range)
            h = args()
            h[0].args.delay = None
            assert chk(h) == -1, bad
            continue
        assert chk(args(**bad)) == -1, bad


# ---- 4. phc_dr.h through the host build -------------------------------------------------------------------------------------------------------------------
def test_noise_draws_and_target_shift():
    base = du.noise_u(du.KEY, 3, 0, 0, 4096)
    assert base.dtype == F and base.min() >= -1.0 and base.max() < 1.0 and abs(float(base.mean())) < 0.05 and base.std() == pytest.approx(1 / np.sqrt(3), abs=0.02)
    assert len(np.unique(base)) > 4000                                         # over env and DoF (the index)
    for other in (du.noise_u(du.KEY, 4, 0, 0, 4096), du.noise_u(du.KEY, 3, 1, 0, 4096), du.noise_u(du.KEY + 1, 3, 0, 0, 4096)):   # over k, call, key
        assert np.abs(np.corrcoef(base, other)[0, 1]) < 0.06 and (base != other).mean() > 0.99
    np.testing.assert_array_equal(du.noise_u(du.KEY, 3, 0, 19 * 7, 19), base[19 * 7:19 * 8])   # env_offset + env and dof enter as one index
    s = du.shim()
    assert s.dr_shifted_target(0.25, 0.5, 30.0, 200.0) == pytest.approx(0.25 + 0.5 * 30.0 / 200.0, rel=1e-6)
    assert s.dr_shifted_target(0.25, 0.5, 30.0, 0.0) == 0.25                   # kp == 0: no noise


def test_delay_law():
    s = du.shim()
    got = [s.dr_delay_law(1, 3, float(u)) for u in np.linspace(0, 1, 301, endpoint=False)]
    assert set(got) == {1, 2, 3} and got == sorted(got) and all(99 <= got.count(v) <= 102 for v in (1, 2, 3))
    assert s.dr_delay_law(1, 3, float(np.nextafter(F(1), F(0)))) == 3 and s.dr_delay_law(1, 3, 1.0) == 3 and s.dr_delay_law(2, 2, 0.7) == 2
    assert s.dr_delay_law(0, 5, 0.0) == 0


def shift_queue_reference(actions, progress, delay_rows, hi):
    """The reference's control delay, as humanoid_teleop.py states it: a queue [N, hi + 1, D]; a reset zeroes the env's queue; each step the queue shifts by
    one, takes the new action at slot 0 and the action applied is slot delay[env].  `delay_rows` [T, N]: the delay in force at each step."""
    T, N, D = actions.shape
    queue = np.zeros((N, hi + 1, D), F)
    out = np.zeros_like(actions)
    for t in range(T):
        for e in range(N):
            if t == 0 or progress[t, e] == 0:
                queue[e] = 0
        queue[:, 1:] = queue[:, :-1].copy()
        queue[:, 0] = actions[t]
        out[t] = queue[np.arange(N), delay_rows[t]]
    return out


def test_action_ring_equals_the_shift_queue_over_a_scripted_episode():
    actions, progress = du.script()
    h = du.HostDr(du.SCRIPT_N, du.SCRIPT_D, delay=(1, 3))
    got, delays = [], []
    for t in range(du.SCRIPT_STEPS):
        h.advance(actions[t], progress[t])
        got.append(h.delayed_actions.copy())
        delays.append(h.delay.copy())
        assert (h.k == t + 1).all()
    got, delays = np.array(got), np.array(delays)
    assert delays.min() >= 1 and delays.max() <= 3 and len(np.unique(delays)) >= 2   # (nine draws: the law itself is test_delay_law)
    for t in range(1, du.SCRIPT_STEPS):   # the delay is redrawn at a reset and only there
        keep = progress[t] != 0
        np.testing.assert_array_equal(delays[t][keep], delays[t - 1][keep])
    assert (delays[4][1] != delays[3][1]) or (delays[9][1] != delays[8][1]) or (delays[6][3] != delays[5][3]) or (delays[11][4] != delays[10][4])
    np.testing.assert_array_equal(got, shift_queue_reference(actions, progress, delays, 3))
    assert not got[0].any() and not got[4][1].any(), "a freshly reset env applies zeros for `delay` steps"
    # no delay: the actions pass through, no queue
    p = du.HostDr(du.SCRIPT_N, du.SCRIPT_D, delay=(0, 0))
    p.args.action_queue = None
    p.advance(actions[0], progress[0])
    np.testing.assert_array_equal(p.delayed_actions, actions[0])
    # a fixed delay of 2
    q = du.HostDr(du.SCRIPT_N, du.SCRIPT_D, delay=(2, 2))
    for t in range(5):
        q.advance(actions[t], None)
    np.testing.assert_array_equal(q.delayed_actions, actions[2])


def test_push_instants_and_untouched_reset_envs():
    actions, progress = du.script()
    h = du.HostDr(du.SCRIPT_N, du.SCRIPT_D, delay=(1, 3), push_interval=4, max_push_vel_xy=0.3)
    h.root_states[:] = 7.0
    pushed = []
    for t in range(du.SCRIPT_STEPS):
        before = h.root_states.copy()
        h.advance(actions[t], progress[t])
        changed = (h.root_states != before)
        assert not changed[:, :7].any() and not changed[:, 9:].any()
        pushed.append(changed[:, 7:9].all(axis=1))
        assert (changed[:, 7:9].all(axis=1) == changed[:, 7:9].any(axis=1)).all()
        h.root_states[:] = 7.0
    pushed = np.array(pushed)
    want = np.zeros_like(pushed)
    want[4], want[8] = True, True
    want[4, 1] = False   # env 1 was reset in step 4: not pushed
    np.testing.assert_array_equal(pushed, want)
    # the values: two draws in [-v, v), different per env and instant
    g = du.HostDr(3, 2, delay=(0, 0), push_interval=1, max_push_vel_xy=0.3)
    vals = []
    for t in range(40):
        g.advance(np.zeros((3, 2), F), None)
        vals.append(g.root_states[:, 7:9].copy())
    vals = np.array(vals[1:])
    assert np.abs(vals).max() < 0.3 and np.abs(vals).max() > 0.25 and len(np.unique(vals)) == vals.size


# ---- 5. the task's host phases ---------------------------------------------------------------------------------------------------------------------------
def host_task(*over):
    from phc_amd.env.tasks import humanoid_im
    return humanoid_im.HumanoidIm.host_only(compose(["env.num_envs=8", *over]))


def test_task_refusals_and_notice(capsys):
    t = host_task(*du.H1_OVER, "domain_rand=h1_dr")
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if "domain_rand" in l]
    assert len(lines) == 1 and all(k in lines[0] for k in ("add_noise", "noise_level", "noise_scales", "added_mass_range")) and "NOT applied" in lines[0]
    assert t._dr is not None and len(t._dr.models) == 64 and t._dr.push_interval == 250 and t._dr.delay_range == (1, 3) and t._dr.torque_noise.shape == (8, 19)
    assert t._dr.models[0] is t.model and float(t._dr.models[0].dof_kp.max()) > 0, "the sampler sees the robot's gains"
    assert t._env_shape is None and t._up["ints"].ndim == 1, "every other consumer keeps the single block"
    with pytest.raises(ValueError, match="randomize_base_mass"):
        host_task(*du.H1_OVER, "domain_rand=h1_dr", "domain_rand.randomize_base_mass=True")
    with pytest.raises(NotImplementedError, match="perturb"):
        host_task(*du.H1_OVER, "domain_rand=h1_dr", "+perturb.force=[50,100]")
    with pytest.raises(NotImplementedError, match="lane_mapping"):
        host_task(*du.H1_OVER, "domain_rand=h1_dr", "+solver.lane_mapping=3", "+solver.inertia_lag=0")
    with pytest.raises(NotImplementedError, match="randomize_torque_rfi"):
        host_task(*du.H1_OVER, "domain_rand=h1_dr", "control.control_mode=isaac_pd")
    with pytest.raises(NotImplementedError, match="randomize_torque_rfi"):
        host_task("domain_rand=h1_dr")
    smpl_ok = ["domain_rand=h1_dr", "domain_rand.randomize_torque_rfi=False", "domain_rand.randomize_link_body_names=[Pelvis,Torso]", "+domain_rand.base_com_body=Torso"]
    with pytest.raises(NotImplementedError, match="has_shape_variation"):
        host_task(*smpl_ok, "robot.has_shape_variation=True")
    s = host_task(*smpl_ok)
    assert s._dr is not None and len(s._dr.models) == 64 and s._dr.torque_noise is None


def test_has_domain_rand_false_builds_todays_task(capsys):
    a, b = host_task(*du.H1_OVER), host_task(*du.H1_OVER, "domain_rand=h1_dr", "domain_rand.has_domain_rand=False")
    assert "domain_rand" not in capsys.readouterr().out
    assert a._dr is None and b._dr is None
    assert bytes(a._sim_params) == bytes(b._sim_params)
    for k in ("ints", "floats"):
        np.testing.assert_array_equal(a._up[k], b._up[k])
    assert a._env_shape is None and b._env_shape is None
