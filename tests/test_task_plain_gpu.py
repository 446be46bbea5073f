"""GPU: the plain instantiations of the task kernels (phc_amd/csrc/phc_kernels_plain.hip) against the generic ones, bit for bit.

phc_kernels_plain.hip is compiled like phc_kernels.hip -- no fast-math, no contraction -- and differs from it only in uniform branches folded at compile time, so
not one result bit may move.  A default SMPL task is stepped twice from the same seeds, once as shipped (plain kernels) and once under
`phc_task_force_generic(1)`, and after EVERY step every tensor the post-physics and reset launches write is compared through its int32 view.

  N = 3: a half-empty last wavefront; N = 9: a second 256-thread block; N = 130: `env >> 3` beyond the 16 reset sub-lists.
  12 steps of the benchmark's idiom (`reset_done()` then `step(fixed random actions)`): the AMP window wraps (S = 10), steps with progress <= 3 and beyond occur
  (the power reward's switch), envs finish and are reset.  Three of the twelve resets take the other launches: before step 5 `phc_im_reset` on the LIST of the
  finished envs with a phase array (the reference's `reset(reset_buf.nonzero())`), before step 8 `phc_im_reset`'s masked mode with a phase array, before step 10
  `phc_im_reset_done` as the masked sweep (`reset_list` cleared); the others are `phc_im_reset_done` on the device-built list, and the initial `reset()` is
  `phc_im_reset` on the list of all envs.
Each run asserts that at least one env was reset during the rollout and at least one NEVER was, and that each of the three special launches had finished and
unfinished envs in front of it: otherwise the comparison proves nothing.  SEEDS holds a seed per N for which this is so
(profiles/task_plain_instantiation/README.md says how they were found and how rare they are).
Not covered here: a launch captured in a hipGraph being re-chosen (the tests show that the keys a capture is dropped by -- `launch_generation()` -- move
whenever `is_plain()` can change; the nullable buffers are allocated by the constructor only and are not part of that key).

Routing: tasks outside the plain set report so and do not change under the switch (zero_out_far, obs_v 7, fut_tracks, occl_training)."""
import pytest
import torch

from phc_amd import _lib as L
from phc_amd import abi
from phc_amd.config import compose

pytestmark = pytest.mark.gpu

SEEDS = {3: 4078, 9: 529, 130: 1}   # num_envs -> torch seed of both runs (see above)
STEPS = 12
# the order of a sub-list's entries is the arrival order of its atomics: compared as sets per sub-list (below), everything else as bits
WRITTEN = ("obs_buf", "rew_buf", "reward_raw", "reset_buf", "_terminate_buf", "progress_buf", "_amp_strip", "ref_body_pos", "ref_body_rot", "ref_body_vel",
           "ref_dof_pos", "_root_states", "_dof_state", "_rigid_body_state", "_pd_target", "_contact_forces", "dof_force_tensor", "_motion_start_times",
           "_motion_start_times_offset", "_global_offset", "_cycle_counter", "_point_goal", "_reset_count", "_reset_rng_dev")


def _bits(t):
    return t.contiguous().view(torch.int32).clone()


def _snapshot(task):
    snap = {k: _bits(getattr(task, k)) for k in WRITTEN}
    cap = task._reset_list.numel() // abi.RESET_SUBLISTS
    counts = task._reset_count[task._reset_slot, :, 0].tolist()
    lists = task._reset_list.view(abi.RESET_SUBLISTS, cap).tolist()
    snap["reset_list"] = [sorted(lists[s][:counts[s]]) for s in range(abi.RESET_SUBLISTS)]
    snap["amp_head"] = task._amp_head
    return snap


def _rollout(over, n, force_generic, steps=STEPS, extra_resets=True, seed=None, snapshots=True):
    """-> (is_plain, [snapshot after the initial reset, after step 0, ...], envs reset during the rollout, steps whose reset launch met finished and unfinished envs)"""
    from phc_amd.env.tasks.vec_task import parse_task
    from phc_amd.utils.flags import flags as gflags
    lib = L.load()
    old = lib.phc_task_force_generic(int(force_generic))
    # the process-global flags decide how a task loads its clips and where its episodes start (`phc_amd.run.main(["test=True", ...])` leaves flags.test set):
    # pinned to their defaults here, so that a seed gives the same rollout whatever ran before in the process
    old_flags = (gflags.test, gflags.im_eval, gflags.no_collision_check)
    gflags.test = gflags.im_eval = gflags.no_collision_check = False
    try:
        torch.manual_seed(SEEDS[n] if seed is None else seed)
        task, env = parse_task(compose([f"env.num_envs={n}", "env.motion_file=synthetic:4:0", *over]))
        plain = task.is_plain()
        env.reset()
        actions = (torch.rand(n, task.num_actions, device=task.device) * 2 - 1) * 0.1
        phase = torch.rand(n, device=task.device)
        snaps, was_reset, mixed = [_snapshot(task)] if snapshots else [], torch.zeros(n, dtype=torch.bool, device=task.device), []
        for k in range(steps):
            flags = task.reset_buf != 0        # the flags of the previous step: what the reset below works on
            was_reset |= flags
            if bool(flags.any()) and not bool(flags.all()):
                mixed.append(k)
            if extra_resets and k == 5:        # phc_im_reset on the list of finished envs with a phase array; the device list stays pending: the next step starts it empty
                task.reset(flags.nonzero().flatten())
            elif extra_resets and k == 8:      # phc_im_reset, masked mode with a phase array, in place of reset_done(); the list stays pending likewise
                buf = task._reset_prologue()
                L.check(lib.phc_im_reset(task._model_struct, task._motion_lib.struct, task._im_params, task._sim_struct, buf, n, None, phase.data_ptr(), 0,
                                         torch.cuda.current_stream().cuda_stream), "phc_im_reset")
            elif extra_resets and k == 10:     # reset_done() as the masked sweep (reset_list cleared): the list counts as consumed, its counter is zeroed by hand
                task._reset_list_pending = False
                task.reset_done()
                task._reset_count[task._reset_slot].zero_()
            else:
                task.reset_done()
            env.step(actions)
            if snapshots:
                snaps.append(_snapshot(task))
        torch.cuda.synchronize()
        return plain, snaps, was_reset.cpu(), mixed
    finally:
        lib.phc_task_force_generic(old)
        gflags.test, gflags.im_eval, gflags.no_collision_check = old_flags


def _assert_equal(a, b, what):
    assert len(a) == len(b)
    for k, (sa, sb) in enumerate(zip(a, b)):
        for name in sa:
            same = torch.equal(sa[name], sb[name]) if isinstance(sa[name], torch.Tensor) else sa[name] == sb[name]
            assert same, f"{what}: {name} differs after step {k - 1} (-1 = the initial reset)"


@pytest.mark.parametrize("n", [3, 9, 130])
def test_plain_kernels_equal_the_generic_ones_bit_for_bit(n):
    plain, shipped, reset_a, mixed_a = _rollout([], n, force_generic=False)
    plain_g, generic, reset_b, mixed_b = _rollout([], n, force_generic=True)
    assert plain and plain_g, "the default task must satisfy phc_im_is_plain (the predicate does not look at the switch)"
    _assert_equal(shipped, generic, f"N={n}")
    for r, mixed in ((reset_a, mixed_a), (reset_b, mixed_b)):
        print(f"N={n}: {int(r.sum())} of {n} envs reset during the rollout; reset launches with finished and unfinished envs before steps {mixed}")
        assert r.any() and not r.all(), "no env, or every env, was reset during the rollout: the run does not compare a reset next to a step"
        assert {5, 8, 10} <= set(mixed), "a list, masked or sweep launch had no finished env, or only finished envs, in front of it"
    progress = torch.stack([s["progress_buf"].view(torch.int64) for s in shipped[1:]])
    assert int(progress.min()) <= 3 < int(progress.max()) and {s["amp_head"] for s in shipped} >= {0, 10}   # both sides of `progress <= 3`; the window wrapped


def test_plain_reset_without_the_amp_table_equals_the_generic_one():
    """`env.amp_ref_table=False` leaves the task plain (the table pointer is not in the list) and sends the AMP history of a reset through the full builds."""
    over = ["+env.amp_ref_table=False"]
    plain_a, a, reset_a, _ = _rollout(over, 9, force_generic=False, steps=6, extra_resets=False)
    plain_b, b, _, _ = _rollout(over, 9, force_generic=True, steps=6, extra_resets=False)
    assert plain_a and plain_b and reset_a.any()
    _assert_equal(a, b, "no AMP table")


@pytest.mark.parametrize("over,plain_field", [(["env.zero_out_far=True"], "zero_out_far"), (["env.obs_v=7"], "obs_v"),
                                              (["env.fut_tracks=True", "env.numTrajSamples=3"], "num_traj_samples"), (["env.occl_training=True"], "occl_mask")],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_tasks_outside_the_plain_set_do_not_move_under_the_switch(over, plain_field):
    plain_a, a, _, _ = _rollout(over, 9, force_generic=False, steps=4, extra_resets=False)
    plain_b, b, _, _ = _rollout(over, 9, force_generic=True, steps=4, extra_resets=False)
    assert not plain_a and not plain_b, f"{over}: {plain_field} is outside the plain set"
    _assert_equal(a, b, str(over))


def test_rebuilding_the_parameter_struct_rechooses_the_kernel():
    """The choice follows `_im_params` and the buffers struct, both rebuilt under keys `launch_generation()` covers: a captured launch cannot outlive it."""
    from phc_amd.env.tasks.vec_task import parse_task
    torch.manual_seed(SEEDS[9])
    task, env = parse_task(compose(["env.num_envs=9", "env.motion_file=synthetic:4:0"]))
    env.reset()
    gen = task.launch_generation()
    assert task.is_plain()
    task._full_body_reward = False      # -> track_body_reward
    task._rebuild_im_params()
    assert not task.is_plain() and task.launch_generation() != gen
    task._full_body_reward = True
    task._rebuild_im_params()
    gen = task.launch_generation()
    assert task.is_plain()
    task._sampled_motion_ids[0] = 1     # the clip-id table is no longer the identity: buf.sampled_motion_ids is passed
    assert task.launch_generation() != gen and not task.is_plain()
    env.step(torch.zeros(9, task.num_actions, device=task.device))   # ... and the generic kernels serve it
    torch.cuda.synchronize()
    assert torch.isfinite(task.obs_buf).all()
