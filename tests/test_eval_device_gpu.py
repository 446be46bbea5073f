"""-m gpu: the evaluation sweep's device metric path (`+learning.params.config.eval_metrics=device`): `phc_eval_accumulate` through the C ABI against
the fp64 host formulas of learning/im_eval.py, its failure flag / loop-control words against the host loop's rules, and whole sweeps with both
settings (same env steps, same simulation state, same results)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
H1_OVER = {"robot": "unitree_h1", "env": "env_im_h1_phc", "sim": "robot_sim", "control": "robot_control"}
G1_OVER = {"robot": "unitree_g1", "env": "env_im_g1_phc", "sim": "robot_sim", "control": "robot_control"}
SMALL = {"learning.params.config.minibatch_size": 64, "learning.params.config.amp_obs_demo_buffer_size": 512,
         "learning.params.config.amp_replay_buffer_size": 512}


def make_task(num_envs, motion, seed=0, **over):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(seed)
    return parse_task(compose([f"env.num_envs={num_envs}", f"env.motion_file={motion}"] + [f"{k}={v}" for k, v in over.items()]))


_TASKS = {}


def _lib_of(kind):
    """(motion library with one loaded clip per env, N, NB, dt) of a model; built once per kind."""
    if kind not in _TASKS:
        n, over = {"smpl": (9, {}), "h1": (2, H1_OVER), "g1": (5, G1_OVER)}[kind]
        task, _ = make_task(n, "synthetic:3:2:2.0", **over)
        _TASKS[kind] = (task._motion_lib, n, task.num_bodies, float(np.float32(task.dt)))
    return _TASKS[kind]


def tol(want):
    return 1e-3 + 1e-5 * np.abs(want)   # mm


class Acc:
    """Caller-side state of phc_eval_accumulate for N envs, and one launch."""

    def __init__(self, lib, n, nb, dt, clip_steps, bound=None, goff=None):
        from phc_amd import _lib as L
        dev = "cuda"
        self.L, self.lib, self.n, self.nb = L, lib, n, nb
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
        self.rbs = z((n, nb, 13), torch.float32)
        self.progress = torch.ones(n, dtype=torch.int64, device=dev)
        self.terminate = z(n, torch.int64)
        self.ids = torch.arange(n, dtype=torch.int64, device=dev)
        self.start = torch.arange(n, dtype=torch.float32, device=dev) * 0.07
        self.start_off = z(n, torch.float32)
        self.start_off[n - 1] = 0.013
        self.goff = z((n, 3), torch.float32) if goff is None else goff.to(dev)
        self.clip_steps = torch.as_tensor(clip_steps, dtype=torch.int32, device=dev)
        self.history, self.sums = z((n, 2, 2, nb, 3), torch.float32), z((n, 5), torch.float64)
        self.count, self.failed, self.status = z(n, torch.int32), z(n, torch.int32), z(2, torch.int32)
        self.mpjpe, self.gt_out = z(n, torch.float32), z((n, nb, 3), torch.float32)
        a = L.EvalArgs()
        a.num_envs, a.num_bodies, a.root_idx, a.bound, a.dt = n, nb, 0, n if bound is None else bound, dt
        for k, t in dict(rigid_body_state=self.rbs, progress_buf=self.progress, terminate_buf=self.terminate, motion_ids=self.ids,
                         motion_start_times=self.start, motion_start_times_offset=self.start_off, global_offset=self.goff, clip_steps=self.clip_steps,
                         history=self.history, sums=self.sums, count=self.count, failed=self.failed, status=self.status, mpjpe_step=self.mpjpe,
                         gt_out=self.gt_out).items():
            setattr(a, k, t.data_ptr())
        self.args, self.dt = a, dt

    def launch(self, step):
        self.args.step = step
        return self.L.load().phc_eval_accumulate(self.lib.struct, self.args, torch.cuda.current_stream().cuda_stream)

    def times(self):
        return self.progress * self.dt + self.start + self.start_off   # humanoid_im.py post_physics_step's evaluation time


def _run_metrics(kind, T, clip_steps, x_shift=0.0, seed=0):
    """T launches on scripted predictions; -> (Acc, P [T, N, NB, 3], G [T, N, NB, 3] fp64 host copies, per-step torch mpjpe [T, N])."""
    lib, n, nb, dt = _lib_of(kind)
    g = torch.Generator(device="cuda").manual_seed(seed)
    goff = torch.tensor([[0.3 * i + x_shift, -0.2 * i, 0.05] for i in range(n)], dtype=torch.float32)
    acc = Acc(lib, n, nb, dt, clip_steps, goff=goff)
    c, s = np.cos(0.4), np.sin(0.4)
    rot = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1.0]], dtype=torch.float32, device="cuda")
    reset = next(i for i, cs in enumerate(clip_steps) if cs - 1 > T)   # an env that counts every one of the T frames
    P, G, M = [], [], []
    for step in range(T):
        if step == 4:
            acc.progress[reset] = 0   # the mid-batch reset: this env's clip restarts, its frames keep counting and are differenced across the jump
        gt = lib.get_motion_state(acc.ids, acc.times(), acc.goff)["rg_pos"]
        pred = gt + 0.02 * torch.randn(gt.shape, device="cuda", generator=g)
        root = gt[:, :1]
        pred[n - 1, :, 0] = 2 * root[n - 1, :, 0] - pred[n - 1, :, 0]                  # mirrored about the root's x
        pred[n - 2] = root[n - 2] + 1.3 * (gt[n - 2] - root[n - 2]) @ rot.T             # rotated + scaled about the root, no noise
        acc.rbs[:, :, 0:3] = pred
        acc.rbs[:, :, 3:] = 7.0                                                         # (nothing but the position is read)
        assert acc.launch(step) == 0
        assert torch.equal(acc.gt_out, gt), f"gt_out differs from phc_motion_state's rg_pos at step {step}"
        M.append(((acc.rbs[:, :, 0:3] - gt).norm(dim=-1).mean(dim=-1), acc.mpjpe.clone()))
        P.append(acc.rbs[:, :, 0:3].double().cpu().numpy())
        G.append(gt.double().cpu().numpy())
        acc.progress += 1
    torch.cuda.synchronize()
    for want, got in M:
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), atol=1e-6, rtol=0)
    P, G = np.stack(P), np.stack(G)
    jump = np.abs(G[4, reset] - G[3, reset]).max()
    assert jump > 1e-3, jump   # the reset moved the reference four frames back: over 1 mm (metres here), a thousand times the tolerance
    return acc, P, G, reset


def _check_metrics(acc, P, G, clip_steps, T, reset):
    from phc_amd.learning.im_eval import METRICS, compute_metrics_per_clip, metrics_from_sums
    frames = [max(min(int(cs) - 1, T), 0) for cs in clip_steps]
    assert frames[reset] == T > 6   # the env that was reset at step 4 counts that frame and the ones after it
    want = compute_metrics_per_clip([P[:n, i] for i, n in enumerate(frames)], [G[:n, i] for i, n in enumerate(frames)])
    np.testing.assert_array_equal(acc.count.cpu().numpy(), frames)
    got = metrics_from_sums(acc.sums.cpu().numpy(), acc.count.cpu().numpy(), acc.nb)
    for k in METRICS:
        w, g = want[k], got[k]
        print(k, "host", np.round(w, 4), "max |device - host| (mm)", np.nanmax(np.abs(g - w)) if np.isfinite(w).any() else None)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=k)
        ok = ~np.isnan(w)
        assert (np.abs(g - w)[ok] <= tol(w)[ok]).all(), (k, g, w)


T8 = 8
CASES = {"smpl": [0, 1, 2, 3, 4, T8 + 5, T8 + 1, T8 + 5, T8 + 5], "h1": [3, T8 + 5], "g1": [1, 2, 3, 4, T8 + 5]}   # n = 0, 1, 2, 3 and > T (h1, two envs: 2 and > T)


@pytest.mark.parametrize("kind", ["smpl", "h1", "g1"])
def test_metrics_match_the_fp64_host_formulas(kind):
    """SMPL (24 bodies, 32-lane groups, 9 envs: one beyond a block), H1 (20 bodies + extended reference bodies in the record), G1 (38 bodies,
    64-lane groups, 5 envs: one beyond a block).  SMPL and G1 have clips of 0 / 1 / 2 / 3 / more than T counted frames; H1's two envs are the rotated +
    scaled one (2 frames) and the mirrored one (more than T).  In every case an env that counts all T frames has its progress set back to 0 at step 4 (a
    reset in mid-batch: SMPL a plain-noise env, H1 and G1 the mirrored one), so frames 4.. are summed and the velocity / acceleration differences are
    taken across the jump.  Oracle: compute_metrics_per_clip on the fp64 casts of the same arrays."""
    lib, n, nb, _ = _lib_of(kind)
    assert (nb, n) == {"smpl": (24, 9), "h1": (20, 2), "g1": (38, 5)}[kind] and (kind != "h1" or lib.num_ext_bodies > 0)
    acc, P, G, reset = _run_metrics(kind, T8, CASES[kind])
    assert reset == {"smpl": 5, "h1": 1, "g1": 4}[kind]
    _check_metrics(acc, P, G, CASES[kind], T8, reset)


def test_metrics_hold_over_forty_frames_thirty_metres_out():
    """T = 40 with the clips translated to x = 30 m (fp32 spacing 1.9e-6 m there): fp32 totals or a wrong history slot would show."""
    T = 40
    cs = [0, 1, 2, 3, 4, T + 5, 21, 30, T + 5]
    acc, P, G, reset = _run_metrics("smpl", T, cs, x_shift=30.0, seed=3)
    assert P[..., 0].min() > 25.0
    _check_metrics(acc, P, G, cs, T, reset)


@pytest.mark.parametrize("bound", [5, 2, 1])
def test_failure_flag_and_status_follow_the_host_loop(bound):
    lib, _, nb, dt = _lib_of("smpl")
    n, T = 5, 9
    cs = np.array([3, 3, 6, 4, 8])
    term = np.zeros((T, n), dtype=np.int64)
    term[2, 0] = 1     # at step == clip_steps - 1: a failure
    term[3, 1] = 1     # at step == clip_steps: not a failure
    term[1, 3] = 1     # early
    term[7, 2] = 1     # long after the clip's end
    term[6, 4] = 1     # the longest clip fails late
    acc = Acc(lib, n, nb, dt, cs, bound=bound)
    acc.rbs[:, :, 0:3] = lib.get_motion_state(acc.ids, acc.times(), acc.goff)["rg_pos"]
    state = np.zeros(n, dtype=bool)
    for step in range(T):
        acc.terminate.copy_(torch.from_numpy(term[step]))
        assert acc.launch(step) == 0
        state |= (step <= cs - 1) & (term[step] != 0)          # im_eval's host loop
        alive = ~state
        want = [int(alive.sum()), int(cs[:bound][alive[:bound]].max()) if alive[:bound].any() else 0]
        assert acc.status.cpu().tolist() == want, (step, acc.status.cpu().tolist(), want)
        assert acc.failed.cpu().numpy().astype(bool).tolist() == state.tolist()
    assert state.tolist() == [True, False, False, True, True]


def test_argument_checks_and_struct_size():
    from phc_amd import _lib as L
    lib, n, nb, dt = _lib_of("smpl")
    acc = Acc(lib, n, nb, dt, [5] * n)
    fn, stream = L.load().phc_eval_accumulate, torch.cuda.current_stream().cuda_stream
    EINVAL = -1
    assert fn(None, acc.args, stream) == EINVAL and fn(lib.struct, None, stream) == EINVAL
    required = [f for f, _ in L.EvalArgs._fields_[6:] if f not in ("motion_ids", "gt_out")]
    assert len(required) == 13
    for f in required:
        keep = getattr(acc.args, f)
        setattr(acc.args, f, None)
        assert fn(lib.struct, acc.args, stream) == EINVAL, f
        setattr(acc.args, f, keep)
    for f, bad in (("num_bodies", 65), ("num_bodies", 0), ("num_bodies", nb - 1), ("root_idx", -1), ("root_idx", nb), ("bound", -1), ("bound", n + 1),
                   ("step", -1), ("num_envs", -1)):
        keep = getattr(acc.args, f)
        setattr(acc.args, f, bad)
        assert fn(lib.struct, acc.args, stream) == EINVAL, (f, bad)
        setattr(acc.args, f, keep)
    acc.args.motion_ids, acc.args.gt_out = None, None          # the two nullable ones: ids default to the env's own index
    acc.rbs[:, :, 0:3] = lib.get_motion_state(acc.ids, acc.times(), acc.goff)["rg_pos"]
    assert acc.launch(0) == 0
    torch.cuda.synchronize()
    assert acc.mpjpe.abs().max().item() == 0.0 and acc.status.cpu().tolist() == [n, 5]


def _sweep(mode, num_envs, motion, over):
    """One evaluation sweep of an untrained agent; -> what the two settings are compared on."""
    from phc_amd.learning.amp_agent import IMAmpAgent
    extra = {} if mode is None else {"+learning.params.config.eval_metrics": mode}
    task, env = make_task(num_envs, motion, seed=0, **dict(SMALL, **over, **extra))
    torch.manual_seed(1)
    agent = IMAmpAgent(env, task.cfg)
    steps, infos = [0], []
    real_step = env.step

    def counted(actions):
        steps[0] += 1
        out = real_step(actions)
        infos.append(set(out[3]))
        return out
    env.step = counted
    info, failed = agent.eval(log=None)
    env.step = real_step
    torch.cuda.synchronize()
    return dict(info=info, failed=[str(k) for k in failed], steps=steps[0], info_keys=infos, per_clip=agent.last_eval_per_clip,
                prob=task._motion_lib._sampling_prob.cpu().numpy(), root=task._root_states.cpu().numpy(), obs=task.obs_buf.cpu().numpy(),
                progress=task.progress_buf.cpu().numpy(), task=task, agent=agent)


def _same_scalars(a, b):
    from phc_amd.learning.im_eval import METRICS
    assert a["info"].keys() == b["info"].keys()
    for k in a["info"]:
        x, y = a["info"][k], b["info"][k]
        print(k, x, y)
        assert (np.isnan(x) and np.isnan(y)) or abs(x - y) <= tol(x), (k, x, y)
    for k in METRICS:
        x, y = a["per_clip"][k], b["per_clip"][k]
        np.testing.assert_array_equal(np.isnan(x), np.isnan(y), err_msg=k)
        assert (np.abs(x - y)[~np.isnan(x)] <= tol(x)[~np.isnan(x)]).all(), (k, x, y)


def test_whole_sweep_is_the_same_with_both_settings():
    """5 clips on 2 envs: 3 batches, the last with one real clip (the `bound` rule).  Host and device metrics: same failed keys, success rate, env
    steps, sampler weights and -- bit for bit -- simulation state afterwards; the metrics agree to 1e-3 mm + 1e-5."""
    over = {"env.auto_pmcp_soft": True}
    host = _sweep("host", 2, "synthetic:5:4:1.2", over)
    dev = _sweep("device", 2, "synthetic:5:4:1.2", over)
    assert host["failed"] == dev["failed"] and host["info"]["eval/success_rate"] == dev["info"]["eval/success_rate"]
    assert host["steps"] == dev["steps"] > 0
    np.testing.assert_array_equal(host["prob"], dev["prob"])
    for k in ("root", "obs", "progress"):
        np.testing.assert_array_equal(host[k], dev[k], err_msg=k)
    assert host["per_clip"]["keys"] == dev["per_clip"]["keys"] and host["per_clip"]["failed"].tolist() == dev["per_clip"]["failed"].tolist()
    _same_scalars(host, dev)
    assert all("mpjpe" in k and "body_pos" not in k and "body_pos_gt" not in k for k in dev["info_keys"])
    assert all("mpjpe" in k and "body_pos" in k for k in host["info_keys"])
    assert dev["task"]._eval_acc is None
    # any other value is refused before the sweep touches the task
    agent, task = dev["agent"], dev["task"]
    agent.config["eval_metrics"] = "gpu"
    lib0 = task._motion_lib
    with pytest.raises(ValueError, match="eval_metrics"):
        agent.eval(log=None)
    assert task._motion_lib is lib0


def test_h1_sweep_scalars_are_the_same_with_both_settings():
    """The H1 config line of the README with its built-in arm-swing clip on 2 envs (20 bodies, extended reference bodies in the record)."""
    host = _sweep("host", 2, "armswing:2", H1_OVER)
    dev = _sweep("device", 2, "armswing:2", H1_OVER)
    assert host["steps"] == dev["steps"] > 0 and host["failed"] == dev["failed"]
    _same_scalars(host, dev)
