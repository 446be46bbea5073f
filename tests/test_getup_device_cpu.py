"""`+env.task_rng=device` on a machine without a GPU: phc_amd/csrc/phc_getup.h built for the host with g++ (tests/getup_shim.cpp, tests/getup_util.py).

  1. the rules: the host build under explicit uniforms and an explicit permutation against a numpy restatement of HumanoidImGetup._reset_envs
  2. the slot permutation: a bijection for every launch count, uniform over keys
  3. the draws: the FALL share, env_offset, the per-env counters
  4. the bindings: struct size, argument checks, the option in the task's host phases
  5. the stand-alone sanitizer program (tests/getup_asan_main.cpp)"""
import ctypes as C
import itertools

import numpy as np
import pytest

import getup_util as gu
import host_build

PROBS = (0.0, 0.5, 1.0)


def _check_against_oracle(s, u, pg, what):
    before = s.clone()
    want, kind = gu.oracle(s, u, pg)
    s.run_host(u, pg)
    assert s.guards_intact(), what
    assert np.array_equal(s["kind"], kind), what
    for name in ("avail", "assign", "recovery_counter"):
        assert np.array_equal(s[name], want[name]), (what, name)
    for name in ("root_states", "dof_state"):   # bit-equal copies
        assert np.array_equal(s[name].view(np.uint32), want[name].view(np.uint32)), (what, name)
    # what the launch publishes for the launches behind it, and what it must leave alone
    falls = np.flatnonzero(kind == 3)
    assert np.array_equal(s["normal_flag"], (kind == 1).astype(np.int64)), what
    assert np.array_equal(s["fall_list"][:len(falls)], falls) and (s["fall_list"][len(falls):] == s.n).all(), what
    assert s["launch_count"][0] == before["launch_count"][0] + 1 and np.array_equal(s["k"], before["k"]), what   # (given uniforms: no draw was counted)
    for name in ("prob", "reset_buf", "terminate_buf", "fall_root", "fall_dof_pos"):
        assert np.array_equal(s[name], before[name]), (what, name)
    return kind


# ---- 1. the rules ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("done", gu.DONE_SETS)
@pytest.mark.parametrize("n", gu.SIZES)
def test_rules_equal_the_numpy_restatement_of_reset_envs(n, done):
    """Every N of getup_util.SIZES (1, 2, around the wavefront and the scan tile, three tiles) x every done set x (p_recovery, p_fall) in {0, 0.5, 1}^2 x
    terminate_buf all 0 / all 1 / mixed, half of the envs holding a slot: kind, avail, assign, recovery_counter exact, teleported rows bit-equal."""
    rng = np.random.default_rng(n * 31 + len(done))
    seen = set()
    for (pr, pf), term in itertools.product(itertools.product(PROBS, PROBS), ("zeros", "ones", "mixed")):
        s = gu.GetupState(n, seed=n, prob=(pr, pf), done=done, terminate=term)
        u = rng.random((n, 2), dtype=np.float32)
        pg = rng.permutation(len(s.free_after_release()))
        seen |= set(_check_against_oracle(s, u, pg, f"n={n} done={done} p=({pr},{pf}) terminate={term}: ").tolist())
    mask = gu.done_mask(n, done)
    assert seen == ({1, 2, 3} if mask.any() else set()) | (set() if mask.all() else {0}), seen


def test_block_constants_are_the_headers():
    assert gu.shim().getup_block() == gu.BLOCK and gu.SIZES[-1] > 2 * gu.BLOCK
    from phc_amd import abi
    assert (abi.GETUP_BLOCK, abi.GETUP_MAX_ENVS) == (gu.shim().getup_block(), gu.shim().getup_max_envs()) and abi.GETUP_MAX_ENVS >= 65536


@pytest.mark.parametrize("n", (2, 65, 1025))
def test_tight_pool_every_faller_receives_exactly_a_released_slot(n):
    """Every env holds a slot, every other env is done and falls (p_fall = 1): F == n_f, and the fallers' new slots are the released ones as a set, whatever
    the permutation -- the explicit one and the launch's own."""
    for own in (False, True):
        s = gu.GetupState(n, seed=3, prob=(0.0, 1.0), holders=2.0, done="alternate")
        assert (s["avail"] == 1).all()
        done = np.flatnonzero(s["reset_buf"])
        released = np.sort(s["assign"][done])
        free = s.free_after_release()
        assert np.array_equal(free, released)
        if own:
            s.run_host()
        else:
            pg = np.random.default_rng(n).permutation(len(free))
            _check_against_oracle(s, np.full((n, 2), 0.5, np.float32), pg, f"tight n={n}: ")
        assert (s["kind"][done] == 3).all() and np.array_equal(np.sort(s["assign"][done]), released) and (s["avail"] == 1).all() and s.guards_intact()
        assert len(set(s["assign"].tolist())) == n   # the held slots stay distinct


def test_an_env_that_never_held_a_slot_releases_slot_0():
    """assign starts as zeros and is never cleared (reference, torch path): env 5 never held a slot, is done and becomes NORMAL -- slot 0, held by env 2, is
    free afterwards.  Kept on purpose."""
    s = gu.GetupState(8, seed=1, prob=(0.0, 0.0), holders=0.0, done=np.arange(8) == 5)
    s["assign"][2], s["avail"][0] = 0, 1
    _check_against_oracle(s, np.full((8, 2), 0.5, np.float32), np.arange(8), "slot 0: ")
    assert s["kind"][5] == 1 and s["avail"][0] == 0 and s["assign"][2] == 0


@pytest.mark.parametrize("bad", (-1, 65, 1 << 40, -(1 << 40)))
def test_an_assign_entry_outside_the_pool_releases_nothing(bad):
    """N = 65; the done envs' assign entries lie outside [0, N): nothing is released, nothing outside the arrays is touched (guard words behind every array)."""
    s = gu.GetupState(65, seed=2, prob=(0.5, 0.5), done="alternate")
    s["assign"][s["reset_buf"] != 0] = bad
    avail = s["avail"].copy()
    u = np.random.default_rng(9).random((65, 2), dtype=np.float32)
    kind = _check_against_oracle(s, u, np.random.default_rng(9).permutation(len(s.free_after_release())), f"assign={bad}: ")
    assert (s["avail"][avail == 1] == 1).all() and int(s["avail"].sum()) == int(avail.sum()) + int((kind == 3).sum())


def test_a_pool_that_cannot_serve_every_faller_demotes_the_rest():
    """Arrays no run produces (a restored state): all slots marked held, the done envs' assign out of range, so F = 0 < n_f.  The FALL envs become NORMAL,
    nothing is teleported, nothing out of range is touched."""
    s = gu.GetupState(65, seed=4, prob=(0.0, 1.0), done="alternate")
    s["avail"][:] = 1
    s["assign"][:] = -1
    before = s.clone()
    s.run_host()
    done = s["reset_buf"] != 0
    assert s.guards_intact() and (s["kind"][done] == 1).all() and (s["normal_flag"][done] == 1).all() and (s["fall_list"] == 65).all()
    assert np.array_equal(s["root_states"], before["root_states"]) and np.array_equal(s["dof_state"], before["dof_state"]) and (s["avail"] == 1).all()


# ---- 2. the permutation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", (1, 2, 3, 8, 1000))
def test_permutation_is_a_bijection_for_64_consecutive_launch_counts(F):
    perms = [gu.perm(gu.KEY, count, F) for count in range(64)]
    for p in perms:
        assert np.array_equal(np.sort(p), np.arange(F))
    if F >= 8:
        assert all(not np.array_equal(a, b) for a, b in zip(perms, perms[1:]))


def test_permutation_is_uniform_over_keys():
    """F = 8, n_f = 1 (rank 0) over 4096 keys: every slot is taken 512 +- 106 times -- 5 sigma of the binomial, sqrt(4096 * 1/8 * 7/8) = 21.2."""
    took = np.bincount([int(gu.perm(gu.KEY + 0x9E3779B97F4A7C15 * i & (1 << 64) - 1, 0, 8)[0]) for i in range(4096)], minlength=8)
    print("slot counts:", took)
    assert took.sum() == 4096 and (np.abs(took - 512) <= 106).all(), took


# ---- 3. the draws ------------------------------------------------------------------------------------------------------------------------------------
def test_fall_share_of_the_non_recovery_envs():
    """4096 envs, all done, p = (0.5, 0.5): the FALL share of the non-recovery envs is 0.5 +- 0.039 (5 sigma of sqrt(0.25 / 4096)), and so is the RECOVERY
    share of 4096 terminated envs."""
    s = gu.GetupState(4096, seed=5, prob=(0.5, 0.5), holders=0.0, done="all", terminate="zeros")   # nobody terminated: all 4096 are non-recovery envs
    s.run_host()
    assert (s["kind"] != 2).all()
    share = float((s["kind"] == 3).mean())
    s = gu.GetupState(4096, seed=5, prob=(0.5, 0.5), holders=0.0, done="all", terminate="ones")
    s.run_host()
    rec = float((s["kind"] == 2).mean())
    print(f"FALL share of 4096 non-recovery envs: {share:.4f}; RECOVERY share of 4096 terminated envs: {rec:.4f}")
    assert abs(share - 0.5) <= 0.039 and abs(rec - 0.5) <= 0.039
    u = gu.draws(gu.KEY, 0, 4096, 0, 4)
    assert (u >= 0).all() and (u < 1).all() and len(np.unique(u)) > 0.99 * u.size


def test_env_offset_continues_the_stream_of_a_larger_run():
    """Envs 96 .. 127 of a 128-env run and a 32-env run with env_offset 96 draw the same numbers -- the draws, and the kinds of a launch."""
    assert np.array_equal(gu.draws(gu.KEY, 0, 128, 3, 5)[:, 96:], gu.draws(gu.KEY, 96, 32, 3, 5))
    big = gu.GetupState(128, seed=6, holders=0.0, done="all", terminate="ones")
    small = gu.GetupState(32, seed=6, holders=0.0, done="all", terminate="ones", env_offset=96)
    big["k"][:], small["k"][:] = 7, 7
    big.run_host(), small.run_host()
    assert np.array_equal(big["kind"][96:], small["kind"]) and len(set(big["kind"].tolist())) == 3
    # phc_task_draws likewise
    outs = []
    for n, off in ((128, 0), (32, 96)):
        k, phase, offs = np.full(n, 2, np.int32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
        gu.shim().task_draws_host(n, gu.KEY, off, k.ctypes.data, phase.ctypes.data, offs.ctypes.data)
        outs.append((phase[-32:], offs[-32:]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_counters_advance_for_done_envs_only_in_assign_and_for_every_env_in_task_draws():
    s = gu.GetupState(65, seed=7, done="alternate")
    k0, done = s["k"].copy(), s["reset_buf"] != 0
    s.run_host()
    first = s["kind"].copy()
    assert np.array_equal(s["k"], k0 + done) and s["launch_count"][0] == 42
    s["reset_buf"][:] = done   # (the same envs are done again: other draws, another permutation)
    s.run_host()
    assert np.array_equal(s["k"], k0 + 2 * done) and s["launch_count"][0] == 43 and not np.array_equal(s["kind"], first)
    n = 65
    k, phase, offs = np.arange(n, dtype=np.int32), np.full(n, -1, np.float32), np.full((n, 2), -1, np.float32)
    gu.shim().task_draws_host(n, gu.KEY, 0, k.ctypes.data, phase.ctypes.data, offs.ctypes.data)
    p1, o1 = phase.copy(), offs.copy()
    assert np.array_equal(k, np.arange(n) + 1) and (p1 >= 0).all() and (p1 < 1).all() and (o1 >= 0).all() and (o1 < 1).all()
    gu.shim().task_draws_host(n, gu.KEY, 0, k.ctypes.data, None, offs.ctypes.data)   # nullable outputs; the counter still moves
    assert np.array_equal(k, np.arange(n) + 2) and np.array_equal(phase, p1) and not np.array_equal(offs, o1)
    gu.shim().task_draws_host(n, gu.KEY, 0, k.ctypes.data, phase.ctypes.data, None)
    assert np.array_equal(k, np.arange(n) + 3) and not np.array_equal(phase, p1)


# ---- 4. the bindings ---------------------------------------------------------------------------------------------------------------------------------
def test_struct_size_and_symbols():
    from phc_amd import _lib as L
    assert C.sizeof(L.GetupArgs) == gu.shim().getup_sizeof_args()
    assert {"phc_getup_assign", "phc_task_draws", "phc_im_reset_from_state_masked", "phc_refresh_body_state_masked"} <= set(L.EXPORTED_SYMBOLS)
    lib = L.load()
    assert all(hasattr(lib, n) for n in ("phc_getup_assign", "phc_task_draws", "phc_im_reset_from_state_masked", "phc_refresh_body_state_masked"))


def _refused(s):
    """(field, value, code) phc_getup_assign must refuse for the state `s`."""
    from phc_amd import abi
    out = [(name, None, -1) for name in abi.GETUP_ARRAYS]
    out += [("num_envs", -1, -1), ("num_dof", 0, -1), ("recovery_steps", -1, -1), ("env_offset", -1, -1), ("env_offset", (1 << 32) - s.n + 1, -1),
            ("num_envs", abi.GETUP_MAX_ENVS + 1, -2)]
    return out


def test_argument_checks_return_their_codes_without_a_device():
    """The library's entry point on host pointers: every refusal comes back before any device work (this machine has no device to do any on), and the host
    build's check function agrees.  Accepted arguments are only asked of the check function -- they would launch."""
    from phc_amd import _lib as L
    lib, s = L.load(), gu.GetupState(4)
    assert gu.shim().getup_args_check_of(s.args()) == 0
    edge = s.args()
    edge.env_offset = (1 << 32) - s.n
    assert gu.shim().getup_args_check_of(edge) == 0
    assert lib.phc_getup_assign(None, None) == -1
    for field, value, code in _refused(s):
        a = s.args()
        setattr(a, field, value)
        assert gu.shim().getup_args_check_of(a) == code, (field, value)
        assert lib.phc_getup_assign(a, None) == code, (field, value)
    empty = s.args()
    empty.num_envs = 0
    assert lib.phc_getup_assign(empty, None) == 0   # N = 0: no launch
    k = np.zeros(4, np.int32)
    assert lib.phc_task_draws(0, 1, 0, k.ctypes.data, None, None, None) == 0
    for n, off, kp in ((-1, 0, k.ctypes.data), (4, 0, None), (4, -1, k.ctypes.data), (4, (1 << 32) - 3, k.ctypes.data)):
        assert lib.phc_task_draws(n, 1, off, kp, None, None, None) == -1 and gu.shim().task_draws_check_of(n, off, kp) == -1
    assert lib.phc_im_reset_from_state_masked(None, None, None, None, None, None, None) == -1
    assert lib.phc_refresh_body_state_masked(None, None, None, None) == -1


def test_the_option_in_the_host_phases():
    from test_task_config_cpu import GETUP, host_task
    t = host_task(*GETUP)
    assert t.task_rng == "torch" and type(t)._use_reset_list is False and t._use_reset_list is False
    assert host_task().task_rng == "torch"
    d = host_task(*GETUP, "+env.task_rng=device")
    assert d.task_rng == "device" and type(d)._use_reset_list is False and d._use_reset_list is False
    with pytest.raises(ValueError, match="task_rng"):
        host_task("+env.task_rng=nonsense")


def test_stream_keys_of_one_seed_are_apart():
    from phc_amd.env.tasks.humanoid_im import GETUP_DRAWS_TAG, TASK_DRAWS_TAG
    from phc_amd.perturb import stream_key
    keys = {stream_key(3), stream_key(3, TASK_DRAWS_TAG), stream_key(3, GETUP_DRAWS_TAG), stream_key(4, GETUP_DRAWS_TAG)}
    assert len(keys) == 4 and stream_key(3) == stream_key(3, 0x7075736873636864)


# ---- 5. the sanitizer program ------------------------------------------------------------------------------------------------------------------------
def test_host_build_runs_clean_under_the_address_and_undefined_sanitizers():
    """tests/getup_asan_main.cpp (its own main; nothing is loaded into Python): the tight pool and the out-of-range assign at N = 65 and 1025."""
    returncode, stdout, stderr = host_build.run_sanitized("getup_asan_main.cpp")
    print(stdout, stderr)
    assert returncode == 0 and stdout.strip().endswith("ok"), stdout + stderr
