"""Tracking of streamed keypoints on the MI355X: the phc_stream_track kernel against the host build of phc_amd/csrc/phc_stream.h (tests/stream_shim.cpp), and
HumanoidImDemo / HumanoidImMCPDemo end to end against the fp64 restatement of tests/stream_util.py fed from the task's own tensors."""
import os

import numpy as np
import pytest
import torch

import stream_util as su
from phc_amd import _lib as L

pytestmark = pytest.mark.gpu
F = np.float32
STEPS = 35


@pytest.fixture(autouse=True)
def _training_flags():
    """The process-global flags as a training run has them (an in-process play or sweep of an earlier test module may have left its own behind)."""
    from phc_amd.utils.flags import flags
    old = (flags.test, flags.im_eval, flags.no_collision_check)
    flags.test = flags.im_eval = flags.no_collision_check = False
    yield
    flags.test, flags.im_eval, flags.no_collision_check = old


def _to(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _back(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _device_launch(model, prm, a):
    return L.load().phc_stream_track(model, prm, a, torch.cuda.current_stream().cuda_stream)


def _inputs(n, nb, seed):
    rng = np.random.default_rng(seed)
    r = np.array([0.0, 1.5, 4.5])[np.arange(n) % 3]
    ang = rng.uniform(0, 2 * np.pi, n)
    frames = su.keypoint_stream(STEPS, n, nb, seed=seed + 1, offset=np.stack([r * np.cos(ang), r * np.sin(ang), np.zeros(n)], axis=-1), drift=0.1)
    rbs = su.body_states(STEPS, n, nb, seed=seed + 2)
    rbs[:, :, 0, :3] = rng.uniform(-0.05, 0.05, (STEPS, n, 3))
    return frames, rbs


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [24, 38])
def test_kernel_equals_the_host_build(nb):
    """N = 1 (a lone env), 3 (a partial wavefront), 9 (one env past a block of eight); 35 steps, so the ring fills and wraps; SMPL's 24 bodies with the
    limb scale, G1's 38 (second lane round) without.  Counters and flags bit-equal, floats within the project's bound; env e has the same bits at N = 3
    and N = 9."""
    frames, rbs = _inputs(9, nb, seed=40 + nb)
    o = su.options(nb)
    track = list(range(nb))
    kept = {}
    for n in (1, 3, 9):
        host = su.Runner(n, nb, track, o, su.host_launch, close_distance=0.5)
        dev = su.Runner(n, nb, track, o, _device_launch, to=_to, back=_back, close_distance=0.5)
        trace = []
        for s in range(STEPS):
            h, d = host.step(frames[s, :n], rbs[s, :n]), dev.step(frames[s, :n], rbs[s, :n])
            for k in ("head", "count", "has_prev", "reset_buf", "terminate_buf"):
                np.testing.assert_array_equal(d[k], h[k], err_msg=f"N={n} step {s}: {k}")
            for k in ("ring_body", "ring_root", "cur_ref", "cur_vel", "obs_buf", "track_err"):
                su.close(d[k], h[k], f"N={n} NB={nb} step {s} {k}")
            trace.append(d)
        obs = dev.step(None, rbs[0, :n], mode=L.STREAM_OBSERVE)
        hobs = host.step(None, rbs[0, :n], mode=L.STREAM_OBSERVE)
        su.close(obs["obs_buf"], hobs["obs_buf"], f"N={n} observe")
        for k in su.STATE:
            np.testing.assert_array_equal(obs[k], trace[-1][k], err_msg=f"observe touched {k}")
        kept[n] = trace + [obs]
    for s, (a, b) in enumerate(zip(kept[3], kept[9])):
        for k in a:
            assert a[k].tobytes() == b[k][:3].tobytes(), f"step {s}: {k} of envs 0..2 depends on the env count"


def test_broadcast_row_and_smpl_order_on_the_device():
    nb, n = 24, 9
    frames, rbs = _inputs(n, nb, seed=77)
    o = su.options(nb, order="smpl", up="y")
    host = su.Runner(n, nb, list(range(nb)), o, su.host_launch, remove_base_rot=True)
    dev = su.Runner(n, nb, list(range(nb)), o, _device_launch, to=_to, back=_back, remove_base_rot=True)
    for s in range(5):
        h, d = host.step(frames[s, :1], rbs[s]), dev.step(frames[s, :1], rbs[s])
        for k in ("cur_ref", "cur_vel", "obs_buf", "track_err"):
            su.close(d[k], h[k], f"step {s} {k}")


# ---- the task ------------------------------------------------------------------------------------------------------------------------------------------
def _task(*extra, task="HumanoidImDemo", n=9, seed=0, motion="synthetic:3:1"):
    from phc_amd.config import compose
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(seed)
    return parse_task(compose([f"env.num_envs={n}", f"env.motion_file={motion}", f"env.task={task}", "env.obs_v=7", *extra]))


def _restated(task, rs, frame):
    """The restatement's (ref, vel, obs, err) of this step from the task's own tensors."""
    torch.cuda.synchronize()
    ref, vel = rs.advance(frame.cpu().numpy())
    return (ref, vel) + _observed(task, ref, vel)


def _observed(task, ref, vel):
    track = task._track_bodies_id.cpu().numpy().tolist()
    rbs = task._rigid_body_state.view(task.num_envs, task.num_bodies, 13).cpu().numpy()
    obs, err, _ = su.observe(rbs, ref, vel, track, bool(task.zero_out_far), task.close_distance, task.far_distance, not task._has_upright_start)
    return obs, err


def _run(task, env, rs, frames=None, steps=STEPS):
    """`steps` zero-action steps; with `frames` they are staged by hand.  Checks every step against the restatement; -> (fed frames, obs / ref clones)."""
    ns = task.get_self_obs_size()
    torch.manual_seed(3)
    env.reset()
    fed, out = [], []
    for s in range(steps):
        if frames is not None:
            task.set_keypoints(frames[s])
        env.step(torch.zeros(task.num_envs, task.num_actions, device=task.device))
        frame = task._stream_cur
        ref, vel, obs, err = _restated(task, rs, frame)
        su.close(task.ref_body_pos.cpu().numpy(), ref, f"step {s} ref_body_pos")
        su.close(task.ref_body_vel.cpu().numpy(), vel, f"step {s} ref_body_vel")
        su.close(task.obs_buf[:, ns:].cpu().numpy(), obs, f"step {s} task block")
        su.close(task.extras["stream_err"].cpu().numpy(), err, f"step {s} stream_err")
        assert not task.reset_buf.any() and not task._terminate_buf.any()
        fed.append(frame.clone())
        out.append((task.obs_buf.clone(), task.ref_body_pos.clone(), task.ref_body_vel.clone(), task._rigid_body_state.clone()))
    return fed, out


def test_end_to_end_against_the_restatement_and_by_hand():
    far = ["env.zero_out_far=True", "env.zero_out_far_train=False"]   # the gating on, as the reference's demo configs have it
    task, env = _task("+stream.motion=synthetic:3:1", *far)
    assert type(task).__name__ == "HumanoidImDemo" and task._stream_source is not None and not task.whole_step_capturable() and task.zero_out_far
    rs = su.Restate(task.num_envs, task.num_bodies, task._stream_opts)
    fed, out = _run(task, env, rs)
    assert not torch.equal(fed[0], fed[7]) and tuple(fed[0].shape) == (9, 24, 3)
    # a reset of some envs: their task block is the restatement's observation of the stored reference on the reset state
    ids = torch.tensor([1, 4, 7], device=task.device)
    before = task.obs_buf.clone()
    env.reset(ids)
    torch.cuda.synchronize()
    ns = task.get_self_obs_size()
    obs, _ = _observed(task, task.ref_body_pos.cpu().numpy().astype(np.float64), task.ref_body_vel.cpu().numpy().astype(np.float64))
    su.close(task.obs_buf[:, ns:].cpu().numpy(), obs, "task block after reset(ids)")
    keep = [e for e in range(9) if e not in (1, 4, 7)]
    assert torch.equal(task.obs_buf[keep], before[keep]) and not torch.equal(task.obs_buf[ids], before[ids])
    assert (task._stream_count == 30).all() and not task.reset_buf.any()
    # restart_stream: the next frame of these envs has zero velocity
    task.restart_stream([2, 5])
    env.step(torch.zeros(9, task.num_actions, device=task.device))
    assert not task.ref_body_vel[[2, 5]].any() and task.ref_body_vel[[0, 1, 3]].any()
    assert task._stream_count.tolist() == [30, 30, 1, 30, 30, 1, 30, 30, 30]
    task.close()
    # the same run with the frames staged by hand: identical bits
    hand, env_h = _task(*far)
    assert hand._stream_source is None
    with pytest.raises(RuntimeError, match="no keypoints staged"):
        hand.step(torch.zeros(9, hand.num_actions, device=hand.device))
    _, out_h = _run(hand, env_h, su.Restate(9, hand.num_bodies, hand._stream_opts), frames=[f.cpu().numpy() for f in fed])
    for s, (a, b) in enumerate(zip(out, out_h)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), f"step {s}: staged by hand differs from the source"
    hand.close()


def test_nothing_else_moved():
    """Same seed and actions: HumanoidImDemo and HumanoidIm agree bit for bit in the body state, the self observation and the AMP observation."""
    extra = ["env.enableEarlyTermination=False", "env.stateInit=Start"]
    runs = []
    for name, more in (("HumanoidIm", []), ("HumanoidImDemo", ["+stream.motion=synthetic:3:1"])):
        task, env = _task(*extra, *more, task=name, seed=2)
        torch.manual_seed(4)
        env.reset()
        g = torch.Generator(device=task.device).manual_seed(9)
        ns, rows = task.get_self_obs_size(), []
        for _ in range(20):   # (the clips are at least 30 frames long: none ends)
            obs, _, _, info = env.step((torch.rand(task.num_envs, task.num_actions, device=task.device, generator=g) * 2 - 1) * 0.3)
            rows.append((task._rigid_body_state.clone(), obs[:, :ns].clone(), info["amp_obs"].clone()))
        if name == "HumanoidIm":
            assert not task.reset_buf.any(), "a clip ended: the comparison needs steps before that"
        runs.append(rows)
        task.close()
    for s, (a, b) in enumerate(zip(*runs)):
        for x, y, what in zip(a, b, ("rigid_body_state", "self observation", "amp observation")):
            assert torch.equal(x, y), f"step {s}: {what}"


def test_mcp_demo_composes_primitives_on_the_stream():
    from test_env_gpu import _pnn_checkpoint
    task, env = _task("+stream.motion=synthetic:3:1", "env.num_prim=3", "env.has_pnn=True", task="HumanoidImMCPDemo")
    assert task.get_action_size() == task.num_prim == 3 and task.close_distance == 0.5
    task.load_primitives(_pnn_checkpoint(task, 3)[0])
    env.reset()
    rs = su.Restate(9, task.num_bodies, task._stream_opts)
    ns = task.get_self_obs_size()
    for s in range(3):
        task.step(torch.softmax(torch.randn(9, 3, device=task.device), dim=-1))
        ref, vel, obs, err = _restated(task, rs, task._stream_cur)
        su.close(task.obs_buf[:, ns:].cpu().numpy(), obs, f"step {s} task block")
        assert tuple(task.actions.shape) == (9, task.num_dof) and not task.reset_buf.any()
    task.close()


def test_recording_shows_the_stream(tmp_path):
    task, env = _task("+stream.motion=synthetic:3:1", "+render.video=" + str(tmp_path / "frames"), "+render.envs=2", "+render.width=96", "+render.height=64",
                      "+render.markers=True")
    env.reset()
    rs = su.Restate(9, task.num_bodies, task._stream_opts)
    for s in range(2):
        env.step(torch.zeros(9, task.num_actions, device=task.device))
        ref = _restated(task, rs, task._stream_cur)[0]
        task.render()
    torch.cuda.synchronize()
    assert task._stream_struct().cur_ref == task.ref_body_pos.data_ptr()   # what the renderer's markers read is what the launch writes
    su.close(task.ref_body_pos.cpu().numpy(), ref, "markers")
    task.close()
    assert len([f for f in os.listdir(tmp_path / "frames") if f.endswith(".png")]) == 2
