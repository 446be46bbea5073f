"""-m gpu: thrown projectiles (`+projectile.*`): phc_proj_advance through the C ABI against the host build of phc_amd/csrc/phc_proj.h (tests/proj_shim.cpp) in
random runs and on the constructed regimes of tests/test_projectile_cpu.py, its refusals, a captured launch against eager ones, a task next to its twin
without projectiles, training with whole-step graphs, resuming, play and the evaluation sweep."""
import numpy as np
import pytest
import torch

import proj_util as pu
import test_projectile_cpu as cpu

pytestmark = pytest.mark.gpu
STEPS = 40
# The device against the host build: the same arithmetic in the same order but for the sinf / cosf of a throw.  The device's differ from glibc's by a few ulp
# of the direction cosines: 8 u d on the start point and 8 u s on the start velocity, which then travel through the flight like the round-off of K = 8 more
# operations per env step.  The bound is proj_util.float_bounds with K = (64 + 8) x the steps flown: the derived bound plus the transcendental term.
K_DEVICE = 64 + 8
# The stream key of the random runs, chosen on the fp64 oracle alone: over the twelve configurations below it drops one env of 70 in one of them (SMPL, four slots:
# 280 projectiles decide four times as often as 70) and none elsewhere; the cap of 2 % admits one of 70 and none of 1 or 9.
KEY = 40


class DevProj:
    """Caller-side state of phc_proj_advance in device memory, laid out like pu.HostProj and copied from one; every written array is followed by guard words."""
    NAMES = pu.INT_NAMES + ("k", "pos", "vel", "mass", "force", "torque")

    def __init__(self, host):
        from phc_amd import _lib as L
        self.L, self.host = L, host
        self.keep = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (host.bodies, host.tab["capsules"], host.tab["owner"], host.tab["com"],
                                                                                host.tab["inv_mass"], host.tab["inv_inertia"], host.rbs)]
        a = self.args = L.ProjArgs()
        for f, _ in L.ProjArgs._fields_[:24]:   # the sizes, ranges, key and env_offset
            setattr(a, f, getattr(host.args, f))
        a.bodies, a.capsules, a.owner, a.body_com, a.body_inv_mass, a.body_inv_inertia, a.rigid_body_state = (t.data_ptr() for t in self.keep)
        self.bufs, self.views = {}, {}
        for name in self.NAMES:
            src = getattr(host, name)
            buf = torch.full((src.size + pu.PAD,), pu.GUARD, dtype=torch.int32, device="cuda")
            view = buf[:src.size].view(torch.float32 if src.dtype == np.float32 else torch.int32).view(src.shape)
            view.copy_(torch.from_numpy(src))
            self.bufs[name], self.views[name] = buf, view
            setattr(a, name, view.data_ptr())
        self.progress = torch.zeros(host.n, dtype=torch.int64, device="cuda")

    def advance(self, progress=None):
        if progress is not None:
            self.progress.copy_(torch.from_numpy(np.asarray(progress, dtype=np.int64)))
        self.args.progress_buf = None if progress is None else self.progress.data_ptr()
        return self.L.load().phc_proj_advance(self.args, torch.cuda.current_stream().cuda_stream)

    def get(self, name):
        return self.views[name].cpu().numpy()

    def guards_intact(self):
        return all(bool((b[-pu.PAD:] == pu.GUARD).all()) for b in self.bufs.values())


# ---- the kernel against the host build ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 4])
@pytest.mark.parametrize("robot", ["smpl_humanoid", "g1_humanoid"], ids=["smpl-G32", "g1-G64"])
@pytest.mark.parametrize("n", [1, 9, 70])   # one group; one env past a 256-thread block at G = 32; a partial last block
def test_kernel_equals_the_host_build(n, robot, count):
    """40 steps of tests/test_projectile_cpu.py's random run (random progress zeros, the nullable pointer): integer state equal outside the envs the fp64 oracle
    flagged (decision margin below 1e-5), at most 2 % of them; floats within the derived bound plus the transcendental term; guards intact."""
    box = {}

    def on_step(step, h, progress, alive):
        dev = box["dev"]
        assert dev.advance(progress) == 0
        torch.cuda.synchronize()
        for name in pu.INT_NAMES + ("k",):
            np.testing.assert_array_equal(dev.get(name)[..., alive], getattr(h, name)[..., alive], err_msg=f"step {step}: {name}")
        o = box["oracle"]
        age = int((o.life_steps - o.life)[o.life > 0].max(initial=0)) + 1
        bounds = pu.float_bounds(o, 12.0, K=K_DEVICE * age)
        fly = (h.life > 0) & alive[None]
        w = [np.abs(dev.get("pos") - h.pos)[fly].max(initial=0.0), np.abs(dev.get("vel") - h.vel)[fly].max(initial=0.0),
             np.abs(dev.get("force") - h.force)[alive].max(initial=0.0), np.abs(dev.get("torque") - h.torque)[alive].max(initial=0.0)]
        for x, b, name in zip(w, bounds, ("pos", "vel", "force", "torque")):
            assert x <= b, f"step {step}: {name} differs by {x:.3e}, bound {b:.3e}"
        box["worst"] = np.maximum(box.get("worst", np.zeros(4)), w)
        assert dev.guards_intact(), f"step {step}"

    def on_start(h, o):
        box["dev"], box["oracle"] = DevProj(h), o
    h, o, alive, _ = cpu.random_run(robot, count, on_start=on_start, on_step=on_step, n=n, steps=STEPS, env_offset=1000, key=KEY)
    dropped = int((~alive).sum())
    print(f"N = {n}, {robot}, count {count}: {int(h.thrown.sum())} thrown, {int(h.hits.sum())} hits, {dropped} envs dropped; worst |kernel - host build| "
          f"pos, vel, force, torque = {box['worst']}")
    assert dropped <= max(0.02 * n, 1 if n >= 50 else 0)
    assert h.thrown.sum() >= 3 * n * count and h.hits.sum() >= n * count, "a run without impacts shows nothing"
    assert (box["dev"].get("k") == STEPS).all()


REGIMES = [(cpu.test_hit_on_a_cylinder_side_and_on_an_end_cap, dict(where="side")), (cpu.test_hit_on_a_cylinder_side_and_on_an_end_cap, dict(where="cap")),
           (cpu.test_hit_on_an_extra_shape_lands_on_the_owner_row, {}), (cpu.test_a_millimetre_decides, dict(gap_mm=1)), (cpu.test_a_millimetre_decides, dict(gap_mm=-1)),
           (cpu.test_overlapping_but_separating_is_no_hit, {}), (cpu.test_two_shapes_entered_in_one_sub_interval, dict(kind="deepest")),
           (cpu.test_two_shapes_entered_in_one_sub_interval, dict(kind="tie")), (cpu.test_a_spinning_body_flips_the_sign_of_vn, dict(kind="recedes")),
           (cpu.test_a_spinning_body_flips_the_sign_of_vn, dict(kind="catches_up")), (cpu.test_hit_in_the_first_and_in_the_last_sub_interval, dict(sub=1)),
           (cpu.test_hit_in_the_first_and_in_the_last_sub_interval, dict(sub=8)), (cpu.test_a_second_overlap_later_in_the_step_is_ignored, {}),
           (cpu.test_two_projectiles_on_one_body_add, {}), (cpu.test_ground_bounce, dict(kind="sticking")), (cpu.test_ground_bounce, dict(kind="sliding")),
           (cpu.test_expiry_parks_and_a_reset_in_mid_flight_zeroes_the_rows, {}), (cpu.test_the_last_body_of_the_last_env, {})]


@pytest.mark.parametrize("robot,count", [("smpl_humanoid", 1), ("smpl_humanoid", 4), ("g1_humanoid", 1), ("g1_humanoid", 4)], ids=["smpl-1", "smpl-4", "g1-1", "g1-4"])
def test_constructed_regimes_through_the_c_abi(robot, count, monkeypatch):
    """Every constructed case of tests/test_projectile_cpu.py with the launch next to the host build: none of them throws, so no elementary function runs and
    the kernel equals the host build bit for bit, floats included; the case's own assertions then hold for the kernel's output."""
    real_run = cpu.run
    ran = []

    def run(h, what, progress=None, speed=12.0):
        dev = DevProj(h)
        assert dev.advance(progress) == 0
        torch.cuda.synchronize()
        o = real_run(h, what, progress, speed)
        for name in DevProj.NAMES:
            got, want = dev.get(name), getattr(h, name)
            assert got.tobytes() == want.tobytes(), f"{what}: {name}"
        assert dev.guards_intact(), what
        ran.append(what)
        return o
    monkeypatch.setattr(cpu, "run", run)
    for fn, kw in REGIMES:
        c = max(count, 2) if fn is cpu.test_two_projectiles_on_one_body_add else count
        fn(robot, c, **kw)
    assert len(ran) == len(REGIMES) + 1   # (the second-overlap case runs two steps)


def test_entry_point_refuses_bad_arguments():
    """The checks of `phc_proj_advance` itself.  Every pointer is device memory, so that a check that stopped refusing would show as a failed assertion and
    nothing else; the sizes tried never exceed what the arrays hold except where the check under test refuses them."""
    m = pu.model("smpl_humanoid")
    host = pu.HostProj(m, 4, pu.posed_rbs(m, 4), count=2)
    dev = DevProj(host)
    fn, stream = dev.L.load().phc_proj_advance, torch.cuda.current_stream().cuda_stream
    assert fn(None, stream) == -1
    for f, bad in cpu.BAD_ARGS:
        keep = getattr(dev.args, f)
        setattr(dev.args, f, bad)
        assert fn(dev.args, stream) == -1, (f, bad)
        setattr(dev.args, f, keep)
    for f in cpu.POINTERS:
        keep = getattr(dev.args, f)
        setattr(dev.args, f, None)
        assert fn(dev.args, stream) == -1, f
        setattr(dev.args, f, keep)
    torch.cuda.synchronize()
    assert (dev.get("k") == 0).all() and (dev.get("force") == 0).all() and (dev.get("pos")[..., 2] == -1000).all() and dev.guards_intact(), "a refused call launches nothing"
    dev.args.num_envs = 0
    assert fn(dev.args, stream) == 0
    torch.cuda.synchronize()
    assert (dev.get("k") == 0).all(), "no envs: nothing to launch"
    dev.args.num_envs = 4
    assert dev.advance() == 0
    torch.cuda.synchronize()
    assert (dev.get("k") == 1).all() and dev.guards_intact()


def test_rows_snapshot_and_select():
    """phc_proj_rows against the host build of its per-env code, byte for byte, guards intact; a refused call launches nothing."""
    from phc_amd import _lib as L
    lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
    n, count, widths = 70, 3, (13, 138, 312, 1)
    base, shadow, last_hit, _ = pu.rows_case(n, count, widths)
    last_hit[1, 33] = 7

    def padded(x):
        buf = torch.full((x.size + pu.PAD,), pu.GUARD, dtype=torch.int32, device="cuda")
        view = buf[:x.size].view(torch.float32 if x.dtype == np.float32 else torch.int32).view(x.shape)
        view.copy_(torch.from_numpy(x))
        return buf, view
    dbase, dshadow, dhit = [padded(x) for x in base], [padded(x) for x in shadow], padded(last_hit)
    for mode in (L.PROJ_SELECT, L.PROJ_SNAPSHOT):
        host = pu.rows_args([x.ctypes.data for x in base], [x.ctypes.data for x in shadow], widths, last_hit.ctypes.data, n, count, mode)
        dev = pu.rows_args([v.data_ptr() for _, v in dbase], [v.data_ptr() for _, v in dshadow], widths, dhit[1].data_ptr(), n, count, mode)
        bad = pu.rows_args([v.data_ptr() for _, v in dbase], [v.data_ptr() for _, v in dshadow], widths, dhit[1].data_ptr(), n, count, 2)
        before = [v.clone() for _, v in dbase + dshadow]
        assert lib.phc_proj_rows(bad, stream) == -1 and lib.phc_proj_rows(None, stream) == -1
        torch.cuda.synchronize()
        assert all(torch.equal(x, v) for x, (_, v) in zip(before, dbase + dshadow)), "a refused call launches nothing"
        pu.shim().proj_rows_host(host)
        assert lib.phc_proj_rows(dev, stream) == 0
        torch.cuda.synchronize()
        for h, (buf, v) in zip(base + shadow, dbase + dshadow):
            assert v.cpu().numpy().tobytes() == h.tobytes() and bool((buf[-pu.PAD:] == pu.GUARD).all())
    assert not np.array_equal(base[0][0], base[0][1]) and (base[1][33] >= 100).all() and (base[1][0] < 100).all()


# ---- the schedule --------------------------------------------------------------------------------------------------------------------------------------------------
CFG = dict(mass=[1, 5], bodies=["Pelvis", "Torso", "Head"], interval_s=[0.1, 0.2], life_s=0.3, distance=[1, 2], speed=[8, 10], count=2, seed=11)


def _schedule(n=70, **kw):
    from phc_amd.projectile import ProjectileSchedule
    m = pu.model("smpl_humanoid")
    rbs = torch.from_numpy(pu.posed_rbs(m, n, seed=1)).cuda().view(-1, 13)
    env_offset = kw.pop("env_offset", 0)
    return ProjectileSchedule(dict(CFG, **kw), n, m, rbs, 1 / 30, "cuda", env_offset=env_offset)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in ((a._istate, b._istate), (a._k, b._k), (a._fstate, b._fstate), (a.force, b.force), (a.torque, b.torque)))


def test_graph_replay_draws_anew():
    """One captured `advance`, replayed 40 times, against 40 eager launches of a twin: equal bit for bit -- a stream frozen at capture would repeat a step."""
    a, b = _schedule(), _schedule()
    assert a.capturable and a.opt.pause_steps == (3, 6) and a.opt.life_steps == 9
    progress = torch.ones(70, dtype=torch.int64, device="cuda")
    for s in (a, b):            # (the first launch loads the code object: outside the capture)
        s.advance(progress)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.advance(progress)
    torch.cuda.synchronize()
    assert _same(a, b), "a capture launches nothing"
    forces = []
    for t in range(STEPS):
        progress.fill_(1)
        progress[t % 70] = 0    # one env reset per step
        g.replay()
        b.advance(progress)
        torch.cuda.synchronize()
        assert _same(a, b), t
        forces.append(a.force.clone())
    assert int(a.thrown) == int(b.thrown) > 140 and int(a.hits) > 70 and a.thrown.dim() == 0 and a.hits.dim() == 0
    assert len({f.cpu().numpy().tobytes() for f in forces}) > STEPS // 2, "the replays must move on"
    assert (a._k == STEPS + 1).all()
    other = _schedule(seed=12)
    for _ in range(STEPS + 1):
        other.advance(None)
    assert not _same(other, b)
    with pytest.raises(ValueError, match="progress_buf"):
        a.advance(progress == 0)


def test_state_dict_round_trip_and_env_offset():
    a = _schedule()
    for _ in range(15):
        a.advance()
    sd = a.state_dict()
    assert not sd["int"].is_cuda
    b = _schedule()
    b.load_state_dict(sd)
    for _ in range(15):
        a.advance()
        b.advance()
    assert _same(a, b) and int(a.hits) > 0
    with pytest.raises(ValueError, match="another size"):
        _schedule(n=71).load_state_dict(sd)
    big, r1 = _schedule(n=140), _schedule(n=70, env_offset=70)      # the ranks of one run: rank 1's envs continue rank 0's global numbering
    r1._rbs.copy_(big._rbs.view(140, -1)[70:].reshape(r1._rbs.shape))
    for _ in range(20):
        big.advance()
        r1.advance()
    assert torch.equal(big.force[70:], r1.force) and torch.equal(big._istate[:, :, 70:], r1._istate) and not torch.equal(big._istate[:, :, :70], r1._istate)


# ---- the task, the learner, play and the sweep ---------------------------------------------------------------------------------------------------------------------
SMALL = ["learning.params.config.minibatch_size=64", "learning.params.config.amp_obs_demo_buffer_size=512", "learning.params.config.amp_replay_buffer_size=512"]
PROJ = ["+projectile.mass=[1,5]", "+projectile.bodies=[Pelvis,Torso,Head]", "+projectile.interval_s=[0.1,0.2]", "+projectile.life_s=0.4", "+projectile.distance=[1,1.5]",
        "+projectile.speed=[8,10]", "+projectile.seed=3"]


def _task(extra=(), num_envs=4, motion="synthetic:4:0"):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(0)
    return parse_task(compose([f"env.num_envs={num_envs}", f"env.motion_file={motion}"] + list(extra)))


def _momentum(task, rbs):
    """Total linear momentum [N, 3] from body states [N, NB, 13] (fp64): sum m_b (v_b + w_b x R_b c_b), as tests/test_ext_wrench_cpu.py::_momenta reads them."""
    rbs = rbs.detach().cpu().numpy().astype(np.float64).reshape(task.num_envs, task.num_bodies, 13)
    m, c = task.model.mass, task.model.com
    vc = rbs[..., 7:10] + np.cross(rbs[..., 10:13], pu.quat_rot(rbs[..., 3:7], c[None]))
    return (m[None, :, None] * vc).sum(1)


TWIN = ["+projectile.mass=[3,5]", "+projectile.bodies=[Pelvis,Torso]", "+projectile.interval_s=0.15", "+projectile.life_s=0.5", "+projectile.distance=[1,1.5]",
        "+projectile.speed=[8,10]", "+projectile.elevation_deg=[0,10]", "+projectile.seed=5"]
STATE = ("_root_states", "_dof_state", "_rigid_body_state", "_contact_forces", "dof_force_tensor", "obs_buf", "rew_buf", "reset_buf", "progress_buf")


def _twins():
    a, ea = _task(TWIN, num_envs=16, motion="stand:4")
    b, eb = _task([], num_envs=16, motion="stand:4")
    assert b._proj is None and a._proj is not None and a._proj.opt.pause_steps[0] >= 4
    torch.manual_seed(3)
    ea.reset()
    torch.manual_seed(3)
    eb.reset()
    return a, b


def test_twin_tasks_with_a_late_first_throw():
    """A 16-env SMPL task with projectiles next to its twin without, equal actions; the first throw comes in step 4 or later (interval_s = 0.15 s: 4 or 5 steps).
    Bit-equal in every state until the step of the first hit; in that step the struck envs differ and the others do not, and an env stays its twin's, bit for
    bit, until it is struck itself.  (The task steps every env through the launch its twin takes and a shadow copy through phc_sim_step_wrench, whose
    instantiation differs from the plain one by fast-math rounding even with zero buffers -- 1.5e-7 on the root state after one step -- and takes the shadow's
    rows for the struck envs only.)
    The task's own hit step, quantitatively: phc_sim_step_wrench called directly on the pre-step snapshot of every simulator tensor with the kernel's force and
    torque buffers held over control_freq_inv simulate calls gives, bit for bit, the struck envs' rows of the task's root, dof, body state, contact force and dof
    force; phc_sim_step on the same snapshot gives the unstruck envs' rows.  A swapped or dropped buffer, another duration or a wrong shadow tensor in
    HumanoidIm._physics_step would show here.
    The impulse: the same direct call, with the kernel's buffers and with zero buffers, on that snapshot lifted 2 m off the ground -- standing, the ground's
    reaction inside the step takes part of the impulse, so the momentum statement is made airborne, and the bit-equality above ties it to the task's step: the
    difference of the struck env's momentum change equals dt * sum_b force[b].  Tolerance, two terms recorded apart: round-off, 4 times the twin's own momentum
    error |dP_twin - M g dt| (the parent's behaviour, measured here: 1.3e-3 N s); and a model term for the joint-space integrator, whose momentum balance holds
    in the limit dt -> 0 with an error of second order in the step that grows with the velocities a hit leaves behind -- the 5 % of the impulse that
    tests/test_ext_wrench_cpu.py::test_momentum_theorem admits for this path.  Measured: 2.2e-2 of a 22.6 N s impulse, 1.1e-1 of 36.9 N s, 4.8e-2 of 27.3 N s
    (0.1 - 0.3 %)."""
    from phc_amd import abi
    a, b = _twins()
    n, nb, nd, dev = a.num_envs, a.num_bodies, a.num_dof, a.device
    act = torch.zeros(n, nd, device=dev)
    names, zeros = STATE, torch.zeros(n, nb, 3, device=dev)
    first_hit = None
    for step in range(30):
        sim0 = [t.clone() for t in (a._root_states, a._dof_state, a._rigid_body_state, a._contact_forces, a.dof_force_tensor, a._pd_target)]
        root0, dof0, rbs0 = sim0[:3]
        a.step(act)
        b.step(act)
        torch.cuda.synchronize()
        hit_now = (a._proj.last_hit >= 0).any(0)
        if not bool(hit_now.any()):
            for name in names:
                assert torch.equal(getattr(a, name), getattr(b, name)), f"step {step}: {name} before the first hit"
            assert float(a._proj.force.abs().sum()) == 0
            if step < 3:
                assert int(a._proj.thrown) == 0, "the first throw comes after step 3"
            continue
        first_hit = step
        break
    assert first_hit is not None and first_hit > 3 and int(a._proj.thrown) > 0
    struck = hit_now.cpu().numpy()
    ra, rb_ = a._rigid_body_state.view(n, nb, 13), b._rigid_body_state.view(n, nb, 13)
    differs = (ra != rb_).flatten(1).any(1).cpu().numpy()
    assert (differs == struck).all(), "the struck envs differ, the others do not"
    # the impulse, on the lifted snapshot
    force, torque = a._proj.force, a._proj.torque
    J = (force.sum(1) * a.dt).cpu().numpy().astype(np.float64)

    def replay(f, t, lift=0.0):
        """The stepper called directly on the pre-step snapshot: phc_sim_step_wrench with buffers f, t (f None: phc_sim_step) -> root, dof, rbs, cf, df."""
        root, dof, rbs, cf, df, pd = (x.clone() for x in sim0)
        root[:, 2] += lift
        sim = abi.sim_state_struct(n, root, dof, rbs, cf, df, pd)
        args = (a._model_struct, a._sim_params, sim, a.actions.contiguous().data_ptr(), a._pd_action_offset.data_ptr(), a._pd_action_scale.data_ptr(),
                a._freeze_mask.data_ptr(), a.control_freq_inv)
        s = torch.cuda.current_stream().cuda_stream
        rc = a._lib.phc_sim_step(*args, s) if f is None else a._lib.phc_sim_step_wrench(*args, f.data_ptr(), t.data_ptr(), a.control_freq_inv, s)
        assert rc == 0
        torch.cuda.synchronize()
        return root, dof, rbs, cf, df

    # the task's own step: the struck envs' rows are the direct wrench call's, the others' the plain launch's, bit for bit
    hit = torch.from_numpy(struck).to(dev)
    assert float(torque[hit].abs().sum()) > 0 and float(force[~hit].abs().sum()) == 0
    mine = (a._root_states, a._dof_state, a._rigid_body_state, a._contact_forces, a.dof_force_tensor)
    for got, w, p, what in zip(mine, replay(force, torque), replay(None, None), ("root", "dof", "body state", "contact force", "dof force")):
        got, w, p = got.view(n, -1), w.view(n, -1), p.view(n, -1)
        assert torch.equal(got[hit], w[hit]), f"{what}: the struck envs' rows are the wrench launch's on the kernel's buffers"
        assert torch.equal(got[~hit], p[~hit]), f"{what}: the other envs' rows are the plain launch's"
        if what in ("root", "body state"):
            assert not torch.equal(w[hit], p[hit])
    swapped = replay(torque, force)[0].view(n, -1)
    assert not torch.equal(swapped[hit], a._root_states.view(n, -1)[hit]), "(the comparison tells the two buffers apart)"

    def direct(wrench):
        f, t = (force, torque) if wrench else (zeros, zeros)   # (the twin through the same launch, with zero buffers)
        out = replay(f, t, lift=2.0)
        assert float(out[3].abs().sum()) == 0, "airborne"
        return _momentum(a, out[2])
    p0 = _momentum(a, rbs0)
    dP_w, dP_t = direct(True) - p0, direct(False) - p0
    g = np.array([0.0, 0.0, float(a._sim_params.gravity_z)]) * a.model.total_mass * a.dt
    twin_err = float(np.abs(dP_t - g).max())
    worst = 0.0
    for e in np.nonzero(struck)[0]:
        err = float(np.abs((dP_w[e] - dP_t[e]) - J[e]).max())
        round_tol, model_tol = 4 * twin_err, 0.05 * float(np.linalg.norm(J[e]))
        tol = round_tol + model_tol
        worst = max(worst, err)
        print(f"first hit in step {first_hit}, env {e}: impulse {J[e]} N s, momentum change against the twin {dP_w[e] - dP_t[e]}, error {err:.3e}, "
              f"twin's own error {twin_err:.3e}, tolerance {round_tol:.3e} (round-off) + {model_tol:.3e} (integrator)")
        assert np.linalg.norm(J[e]) > 0.5 and err <= tol
    for e in np.nonzero(~struck)[0]:
        assert (J[e] == 0).all() and np.abs(dP_w[e] - dP_t[e]).max() == 0
    ever, compared = torch.from_numpy(struck).to(dev), 0
    for _ in range(5):   # and the task goes on: an env that nothing has struck yet is still its twin's
        a.step(act)
        b.step(act)
        ever |= (a._proj.last_hit >= 0).any(0)
        compared += int((~ever).sum())
        for name in ("_root_states", "_dof_state", "_rigid_body_state", "_contact_forces", "dof_force_tensor", "obs_buf", "rew_buf"):
            x, y = getattr(a, name).view(n, -1), getattr(b, name).view(n, -1)
            assert torch.equal(x[~ever], y[~ever]), name
    assert torch.isfinite(a._root_states).all() and compared > 0, "envs not yet struck were compared in these steps"
    with pytest.raises(ValueError, match="thrown projectiles"):
        a.apply_rigid_body_force_tensors(torch.zeros(n, nb, 3, device=dev))


def test_training_logs_hits_and_resume_restores_the_state(tmp_path):
    """64 envs, horizon 8, three epochs (the third replays captured whole steps): `projectile/hits` per epoch, `("step", n, ...)` graphs; the checkpoint carries
    the projectiles' state into a same-size training run and not into play."""
    from phc_amd.learning.amp_agent import IMAmpAgent
    from phc_amd.utils.flags import flags
    over = ["learning.params.config.horizon_length=8", "learning.params.config.minibatch_size=512", "learning.params.config.mini_epochs=2",
            "learning.params.config.amp_obs_demo_buffer_size=512", "learning.params.config.amp_replay_buffer_size=512", "+learning.params.config.hip_graph=True"] + PROJ

    def agent_of():
        task, env = _task(over, num_envs=64, motion="stand:4")
        torch.manual_seed(1)
        return IMAmpAgent(env, task.cfg), task
    agent, task = agent_of()
    assert task.whole_step_capturable()
    infos, real = [], agent.train_epoch

    def recorded():
        infos.append(real())
        return infos[-1]
    agent.train_epoch = recorded
    agent.train(3, log=None)
    torch.cuda.synchronize()
    hits = [i["projectile/hits"] for i in infos]
    print("projectile/hits per epoch:", hits, "thrown:", int(task._proj.thrown))
    assert len(hits) == 3 and sum(hits) == int(task._proj.hits) > 0 and hits[2] > 0
    assert {k[1] for k in agent._roll_graphs if k[0] == "step"} == set(range(8)), "whole-step graphs in use"
    assert (task._proj._k == 24).all(), "one launch per env step, captured ones included"
    assert all(torch.isfinite(p).all() for p in agent.model.parameters())
    assert "projectile/hits" in agent.assemble_train_info(infos[-1])
    path = str(tmp_path / "Humanoid.pth")
    agent.save(path)
    want = task._proj.state_dict()
    same, t_same = agent_of()
    same.restore(path)
    got = t_same._proj.state_dict()
    assert all(torch.equal(want[k], got[k]) for k in want)
    play, t_play = agent_of()
    flags.test = True
    try:
        play.restore(path, load_optimizer=False)
    finally:
        flags.test = False
    assert (t_play._proj._k == 0).all(), "play and the sweep start the configured projectiles, not the training run's"


def _sweep(mode):
    from phc_amd.learning.amp_agent import IMAmpAgent
    # (16 envs on the standing clips, throws from 1 - 1.5 m every 4 - 5 steps as in the twin test: they land whatever the untrained policy does)
    task, env = _task(SMALL + TWIN + [f"+learning.params.config.eval_metrics={mode}"], num_envs=16, motion="stand:4")
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    info, failed = agent.eval(log=None)
    torch.cuda.synchronize()
    return info, agent, task, env


def test_play_and_evaluation_return_the_counts():
    from phc_amd.run import play
    host, agent, task, env = _sweep("host")
    device = _sweep("device")[0]
    print(host, device)
    for info in (host, device):
        assert info["projectile_thrown"] > 0 and info["projectile_hits"] > 0 and all(np.isfinite(v) for v in info.values())
    assert (host["projectile_thrown"], host["projectile_hits"]) == (device["projectile_thrown"], device["projectile_hits"])
    before = int(task._proj.thrown), int(task._proj.hits)
    out = play(agent, task, env, steps=40)
    assert out["projectile_thrown"] == int(task._proj.thrown) - before[0] > 0 and out["projectile_hits"] == int(task._proj.hits) - before[1] > 0
    assert np.isfinite(out["mean_episode_reward"])
