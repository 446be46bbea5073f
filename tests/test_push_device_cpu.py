"""The device push schedule (`+perturb.rng=device`, phc_push_advance) on a machine without a GPU: phc_amd/csrc/phc_push.h built for the host with g++
(tests/push_shim.cpp).  Its transition against `PushSchedule` under the same uniforms, its draws, the whole host path's structure, the guards and
the binding."""
import numpy as np
import pytest
import torch

import push_util as pu

NAMES = ["Pelvis", "L_Hip", "Torso", "Head"]   # tests/test_ext_wrench_cpu.py::_schedule: 16 envs, pause 6 .. 12 steps, duration 3
N, DT, SEED, STEPS = 16, 1 / 30, 5, 100
FORCE_TOL = 1e-3   # newtons.  At 400 N one fp32 ulp is 3e-5 N; cosf / sinf against torch's cos / sin differ by a few ulp


def _cfg(**kw):
    cfg = dict(force=[200, 400], bodies=["Pelvis", "Torso"], interval_s=[0.2, 0.4], duration_s=0.1, direction="horizontal", seed=SEED)
    cfg.update(kw)
    return cfg


def _torch_run(cfg, reset_at):
    """PushSchedule on the CPU for STEPS steps, env 3 reset at step `reset_at` -> per step (remaining, countdown, pushed body or -1, pushes, force)."""
    from phc_amd.perturb import PushSchedule
    s = PushSchedule(cfg, N, NAMES, DT, "cpu")
    hist = []
    for t in range(STEPS):
        s.advance(torch.tensor([t == reset_at and e == 3 for e in range(N)]))
        on = s.force.norm(dim=-1) > 0
        body = torch.where(on.any(-1), on.float().argmax(-1), torch.full((N,), -1))
        hist.append((s.remaining.numpy().copy(), s.countdown.numpy().copy(), body.numpy().copy(), int(s.pushes), s.force.numpy().copy()))
    return s, hist


@pytest.mark.parametrize("over", [{}, {"direction": "any"}, {"bodies": ["Head"]}], ids=["horizontal", "any", "one_body"])
def test_transition_equals_the_torch_schedule_under_its_uniforms(over):
    cfg = _cfg(**over)
    _, free = _torch_run(cfg, reset_at=-1)
    t0 = next(t for t, h in enumerate(free) if h[2][3] >= 0)   # first pushed step of env 3; the reset comes in the push's second step
    s, want = _torch_run(cfg, reset_at=t0 + 1)
    assert want[t0][2][3] >= 0 and want[t0 + 1][2][3] < 0 and free[t0 + 1][2][3] >= 0, "the reset must end a running push"
    listed = [NAMES.index(b) for b in cfg["bodies"]]
    h = pu.HostPush(N, len(NAMES), listed, pause=s.pause_steps, duration=s.duration_steps, direction=int(cfg["direction"] == "any"), force=s.force_range)
    assert (s.pause_steps, s.duration_steps) == ((6, 12), 3)
    gen = torch.Generator()
    gen.manual_seed(SEED)
    u_ctor = torch.rand(N, generator=gen)
    h.countdown[:] = [h.pause_of(u) for u in u_ctor]   # the constructor's pause draw
    worst = 0.0
    for t in range(STEPS):
        u = torch.rand((5, N), generator=gen).numpy()
        h.step_given(u, [t == t0 + 1 and e == 3 for e in range(N)])
        rem, cnt, body, pushes, force = want[t]
        np.testing.assert_array_equal(h.remaining, rem, err_msg=f"remaining, step {t}")
        np.testing.assert_array_equal(h.countdown, cnt, err_msg=f"countdown, step {t}")
        np.testing.assert_array_equal(h.body, body, err_msg=f"pushed body, step {t}")
        assert int(h.started.sum()) == pushes, t
        worst = max(worst, float(np.abs(h.force - force).max()))
    print(f"{over or 'default'}: max |host lane - torch schedule| force = {worst:.3e} N over {STEPS} steps, {want[-1][3]} pushes")
    assert want[-1][3] > N and worst <= FORCE_TOL
    assert torch.equal(torch.rand(3, generator=gen), torch.rand(3, generator=s.gen)), "the twin generator must have followed the schedule's"


KEY = 0x0123456789ABCDEF
# (field, value) pairs phc_push_advance must refuse, for a schedule of 4 envs, 4 bodies, pause 6 .. 12, force 200 .. 400
BAD_ARGS = (("num_envs", -1), ("num_bodies", 0), ("num_bodies", 65), ("num_listed", 0), ("num_listed", 65), ("pause_lo", -1), ("pause_hi", 5),
            ("pause_hi", (1 << 24) + 1), ("duration", 0), ("direction", 2), ("direction", -1), ("force_lo", -1.0), ("force_lo", 500.0),
            ("force_hi", float("inf")), ("force_hi", float("nan")), ("env_offset", -1), ("env_offset", (1 << 32) - 3))


def test_draws():
    d = pu.draws(KEY, 0, 64, 0, 1024)          # [k, env, i]: 2^16 (k, env) pairs, five draws each
    assert d.dtype == np.float32 and (d >= 0).all() and (d < 1).all()
    assert np.array_equal(d, pu.draws(KEY, 0, 64, 0, 1024)), "same (key, env, k, i), same bits"
    assert not np.array_equal(d, pu.draws(KEY + 1, 0, 64, 0, 1024))
    m = 1 << 24
    assert np.array_equal(d * m, np.floor(d * m)), "24-bit uniforms"
    for i in range(5):
        for j in range(i + 1, 5):
            assert (d[..., i] != d[..., j]).mean() > 0.999, (i, j)      # the five draw indices differ
    assert (d[1:] != d[:-1]).mean() > 0.999                          # consecutive k
    assert (d[:, 1:] != d[:, :-1]).mean() > 0.999                    # neighbouring envs
    bound = 5.0 / np.sqrt(12.0 * (1 << 16))
    for i in range(5):
        mean = float(d[..., i].astype(np.float64).mean())
        print(f"draw {i}: mean of 2^16 = {mean:.5f} (bound 0.5 +- {bound:.5f})")
        assert abs(mean - 0.5) <= bound, i
    # an env's stream depends on its global index only
    assert np.array_equal(pu.draws(KEY, 0, 16, 0, 50), d[:50, :16])
    assert np.array_equal(pu.draws(KEY, 16, 16, 0, 50), d[:50, 16:32])
    assert np.array_equal(pu.draws(KEY, 0, 64, 7, 3), d[7:10])


def test_env_offset_continues_the_stream_of_a_larger_run():
    """Envs 0..15 of a 64-env run equal a 16-env run; env_offset = 16 on a 16-env run equals envs 16..31 of it (whole host path)."""
    big, a, b = pu.HostPush(64, 4, [0, 2]), pu.HostPush(16, 4, [0, 2]), pu.HostPush(16, 4, [0, 2], env_offset=16)
    for _ in range(60):
        for s in (big, a, b):
            s.advance()
        assert np.array_equal(big.state[:, :16], a.state) and np.array_equal(big.force[:16], a.force)
        assert np.array_equal(big.state[:, 16:32], b.state) and np.array_equal(big.force[16:32], b.force)
    assert a.started.sum() > 0 and not np.array_equal(a.force, b.force)


def _host_run(steps=STEPS, **kw):
    s = pu.HostPush(N, 4, [0, 2], **kw)
    hist = []
    for _ in range(steps):
        s.advance()
        hist.append(s.force.copy())
    return s, np.stack(hist)   # [T, N, NB, 3]


def test_whole_host_path_has_the_schedules_structure():
    """`push_draws` and `push_lane` composed as the kernel composes them: the structural assertions of tests/test_ext_wrench_cpu.py::test_push_schedule."""
    s, a = _host_run()
    assert np.array_equal(a, _host_run()[1]), "same key, same pushes"
    assert not np.array_equal(a, _host_run(key=KEY)[1])
    mag = np.linalg.norm(a, axis=-1)                # [T, N, NB]
    on = mag > 0
    assert on.any() and (mag[on] >= 200 - 1e-3).all() and (mag[on] <= 400 + 1e-3).all()
    assert (a[..., 2] == 0).all(), "horizontal pushes have no z component"
    assert not on[:, :, 1].any() and not on[:, :, 3].any() and on[:, :, 0].any() and on[:, :, 2].any(), "only the listed bodies are pushed"
    assert (on.sum(-1) <= 1).all(), "one body per push"
    pushed = on.any(-1)                             # [T, N]
    started = 0
    for e in range(N):
        runs, t = [], 0
        while t < len(pushed):
            u = t
            while u < len(pushed) and pushed[u, e] == pushed[t, e]:
                u += 1
            runs.append((bool(pushed[t, e]), t, u - t))
            t = u
        started += sum(1 for p, _, _ in runs if p)
        assert not runs[0][0]
        for p, t, n in runs[:-1]:
            assert (n == 3) if p else (6 <= n <= 12), (e, runs)
            if p:
                assert (a[t:t + n, e] == a[t, e]).all(), "within a push the force is constant"
    assert int(s.started.sum()) == started and (s.state[3] == STEPS).all()
    any_dir = _host_run(60, direction=1)[1]
    assert (any_dir[..., 2] != 0).any()
    assert np.abs(np.linalg.norm(any_dir, axis=-1)[np.linalg.norm(any_dir, axis=-1) > 0]).min() >= 200 - 1e-3


def test_progress_zero_ends_the_push():
    s, a = _host_run(40)
    t0 = int(np.nonzero((np.linalg.norm(a, axis=-1) > 0).any(-1)[:, 3])[0][0])
    r = pu.HostPush(N, 4, [0, 2])
    hist = []
    for t in range(40):
        progress = np.full(N, 7, dtype=np.int64)
        progress[3] = 0 if t == t0 + 1 else 7
        r.advance(progress)
        hist.append(r.force.copy())
    b = np.stack(hist)
    pb = (np.linalg.norm(b, axis=-1) > 0).any(-1)[:, 3]
    assert pb[t0] and not pb[t0 + 1:t0 + 1 + 5].any(), "a reset env's push ends at once and a new pause of >= 6 steps (this one included) begins"
    assert (b[t0 + 1, 3] == 0).all()
    others = [e for e in range(N) if e != 3]
    assert np.array_equal(a[:, others], b[:, others])


# ---- guards and the binding ----------------------------------------------------------------------------------------------------------------------------------------
def test_binding_and_struct_size():
    from phc_amd import _lib as L
    assert "phc_push_advance" in L.EXPORTED_SYMBOLS
    fn = L.load().phc_push_advance
    assert len(fn.argtypes) == 2 and fn.restype is L.c_i32   # (phc_push_args_t against its mirror: tests/test_abi_and_host.py)


def test_argument_checks():
    """`push_args_check` (phc_push.h), the function `phc_push_advance` asks before it launches, through the host build: nothing here reaches a launch, so
    arguments that must never get one (null pointers, host memory) are safe to try.  The entry point itself: tests/test_push_device_gpu.py."""
    check = pu.shim().push_args_check_of
    h = pu.HostPush(4, 4, [0, 2])
    EINVAL = -1
    assert check(h.args) == 0 and check(None) == EINVAL
    for f in ("bodies", "remaining", "countdown", "body", "k", "started", "force"):
        keep = getattr(h.args, f)
        setattr(h.args, f, None)
        assert check(h.args) == EINVAL, f
        setattr(h.args, f, keep)
    h.args.progress_buf = None
    assert check(h.args) == 0, "progress_buf is nullable"
    for f, bad in BAD_ARGS:
        keep = getattr(h.args, f)
        setattr(h.args, f, bad)
        assert check(h.args) == EINVAL, (f, bad)
        setattr(h.args, f, keep)
    for f, good in (("num_envs", 0), ("pause_lo", 0), ("pause_hi", 1 << 24), ("force_lo", 0.0), ("env_offset", (1 << 32) - 4), ("num_bodies", 64), ("num_listed", 64)):
        keep = getattr(h.args, f)
        setattr(h.args, f, good)
        assert check(h.args) == 0, (f, good)
        setattr(h.args, f, keep)


def test_rng_option():
    from phc_amd.perturb import DevicePushSchedule, PushSchedule, make_schedule

    def run(s):
        out = []
        for _ in range(30):
            s.advance()
            out.append(s.force.clone())
        return torch.stack(out)
    a = run(PushSchedule(_cfg(), N, NAMES, DT, "cpu"))
    b = PushSchedule(_cfg(rng="torch"), N, NAMES, DT, "cpu")
    assert torch.equal(a, run(b)) and a.abs().sum() > 0 and b.capturable is False
    assert type(make_schedule(_cfg(), N, NAMES, DT, "cpu")) is PushSchedule and type(make_schedule(_cfg(rng="torch"), N, NAMES, DT, "cpu")) is PushSchedule
    for build in (PushSchedule, DevicePushSchedule, make_schedule):
        with pytest.raises(ValueError, match="perturb.rng"):
            build(_cfg(rng="philox"), N, NAMES, DT, "cpu")
    with pytest.raises(ValueError, match="perturb.rng"):
        PushSchedule(_cfg(rng="device"), N, NAMES, DT, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        make_schedule(_cfg(rng="device"), N, NAMES, DT, "cpu")
    assert DevicePushSchedule.capturable is True


def test_train_refuses_the_torch_schedule_only():
    from phc_amd.learning.amp_agent import IMAmpAgent
    from phc_amd.perturb import PushSchedule

    class Task:
        def __init__(self, push):
            self._push = push

    class Agent:
        def __init__(self, push):
            self.task = Task(push)

    with pytest.raises(NotImplementedError, match="push schedule") as e:
        IMAmpAgent.train(Agent(PushSchedule(_cfg(), N, NAMES, DT, "cpu")), 1)
    assert "+perturb.rng=device" in str(e.value)

    class Capturable:
        capturable = True
    with pytest.raises(AttributeError, match="init_train"):   # past the guard: the stub has nothing to train
        IMAmpAgent.train(Agent(Capturable()), 1)
