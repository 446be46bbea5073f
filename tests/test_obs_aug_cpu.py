"""`+env.task_rng=device` with add_obs_noise / fut_tracks_dropout / occl_training on a machine without a GPU: phc_amd/csrc/phc_obs_aug.h built for the host with
g++ (tests/obs_aug_shim.cpp, tests/obs_aug_util.py).

  1. the rules: the host build against a numpy restatement of _fut_dropout + _add_obs_noise and of _update_occl_training, and within the error bound of an
     fp64 Box-Muller
  2. the draws: determinism, counters, env_offset, stream keys
  3. statistics of 65 536 draws from a fixed key (deterministic: a failure is a defect)
  4. the bindings: struct size, argument checks, the options in the task's host phases
  5. the stand-alone sanitizer program (tests/obs_aug_asan_main.cpp)

Measured on the host build (glibc logf / sinf / cosf): the largest error of a noised element over every case below is 0.46 of its bound E (obs_aug_util.noise_bound)."""
import ctypes as C

import numpy as np
import pytest

import obs_aug_util as ou
import host_build


def _id_lists(n):
    """A permuted list (the even envs, shuffled), a one-element list, an empty list."""
    return (np.random.default_rng(n).permutation(np.arange(0, n, 2)), np.array([n - 1]), np.array([], dtype=np.int64))


def _selections(n):
    yield "all", None
    for done in ou.DONE_SETS:
        yield "flag", done
    for ids in _id_lists(n):
        yield "ids", ids


# ---- 1. the rules ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ou.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_host_build_equals_the_numpy_restatement_and_the_fp64_box_muller(case):
    """Every shape of obs_aug_util.CASES x every selection form (all rows; row_flag over the done sets none / all / first / last / alternate; env_ids permuted /
    one element / empty): counters, dropout decisions, zeroed blocks, untouched rows and guards exact, noised elements equal to the restatement (same libm) and
    within E = 2^-23 |o'| + noise_std r 2^-19 of the fp64 oracle.  Then a second call on the result: it draws anew and obeys the same rules."""
    worst = 0.0
    for form, select in _selections(case[0]):
        s = ou.AugState(*case, form=form, select=select, seed=case[1])
        before = s.clone()
        s.run_host()
        worst = max(worst, ou.check_call(before, s, f"{case} {form} {select}: ", same_library=True))
        again = s.clone()
        s.run_host()
        worst = max(worst, ou.check_call(again, s, f"{case} {form} {select} (second call): ", same_library=True))
    print(f"{case}: largest error / bound of the host build = {worst:.3f}")


def test_dropout_comes_before_the_noise_and_the_noise_lands_on_the_zeroed_blocks():
    """p = 1: every reference sample is dropped, so every column behind `so` is exactly noise_std * z (0.0f + x == x), and the columns in front are obs + noise."""
    s = ou.AugState(65, 256, 1, 3, 1.0, 0.1, seed=3)
    before = s.clone()
    s.run_host()
    z = ou.normals(s.key, np.arange(65), before["k"], 256)
    assert np.array_equal(s["obs"][:, 1:], np.float32(0.1) * z[:, 1:]) and np.array_equal(s["obs"][:, :1], before["obs"][:, :1] + np.float32(0.1) * z[:, :1])
    assert (np.abs(s["obs"][:, 1:]) > 0).mean() > 0.99
    # p = 0.1: a share of the blocks is zeroed, whole blocks only
    s = ou.AugState(257, 7, 1, 3, 0.1, 0.0, seed=4)
    s.run_host()
    blocks = (s["obs"][:, 1:].reshape(257, 3, 2) == 0)
    assert np.array_equal(blocks[:, :, 0], blocks[:, :, 1]) and 0 < blocks[:, :, 0].mean() < 0.3 and (s["obs"][:, 0] != 0).all()


def test_counters_move_for_selected_rows_only():
    for form, select in (("flag", "alternate"), ("ids", np.array([5, 1, 64]))):
        s = ou.AugState(65, 7, 1, 3, 0.1, 0.1, form=form, select=select, seed=5)
        k0, rows = s["k"].copy(), s.rows()
        s.run_host(), s.run_host()
        want = k0.copy()
        want[rows] += 2
        assert np.array_equal(s["k"], want) and len(rows) < 65


@pytest.mark.parametrize("n", ou.OCCL_N)
@pytest.mark.parametrize("J", ou.OCCL_J)
def test_occlusion_schedule_equals_the_numpy_restatement(n, J):
    """count and mask follow _update_occl_training over 4 calls: body 0 never starts a span, spans lie in [30, 59], running spans count down to 0, and the
    mask is the reference's overwrite (bodies 9 .. 23 visible, every other occluded) whatever the counts say."""
    s = ou.OcclState(n, J, seed=n + J)
    s["count"][:, 0] = 0
    for call in range(4):
        before = s.clone()
        uv = ou.uniforms(s.key, np.arange(n), before["k"], 0, J)
        want, start, spans = ou.oracle_occl(before, uv[:, :, 0], uv[:, :, 1])
        s.run_host()
        assert s.guards_intact()
        ou.assert_bytes_equal(s, want, ("k", "count", "mask"), f"n={n} J={J} call {call}: ")
        assert not start[:, 0].any() and (s["count"][:, 0] == 0).all() and spans.min() >= 30 and spans.max() <= 59
        assert (s["count"][start] == spans[start] - 1).all() and (s["count"][start] >= 29).all() and (s["count"][start] <= 58).all()
        assert np.array_equal(s["count"][~start], np.maximum(before["count"][~start] - 1, 0))
        assert np.array_equal(s["mask"], np.broadcast_to(~((np.arange(J) >= 9) & (np.arange(J) < 24)), (n, J)).astype(np.uint8))


def test_every_span_length_is_drawn_and_none_reaches_span_hi():
    """prob = 1: every body but the root starts a span in every env; the 16 191 spans take each of the 30 values 30 .. 59 (count = span - 1) and no other."""
    s = ou.OcclState(257, 64, prob=1.0, seed=1)
    s.run_host()
    assert np.array_equal(np.unique(s["count"][:, 1:]), np.arange(29, 59)) and (s["count"][:, 0] <= 58).all()


# ---- 2. the draws ------------------------------------------------------------------------------------------------------------------------------------
def test_same_key_env_and_count_give_the_same_bits_and_a_second_call_draws_anew():
    fresh = lambda: ou.AugState(65, 257, 1, 1, 0.0, 0.1, seed=6)
    a, b = fresh(), fresh()
    a.run_host(), b.run_host()
    ou.assert_bytes_equal(a, b, ("obs", "k"))
    first = a["obs"].copy()
    a["obs"][...] = fresh()["obs"]
    a.run_host()   # the same rows again, the counters moved on
    assert not np.array_equal(a["obs"], first) and np.abs(a["obs"] - first).max() > 0.1
    a["obs"][...] = fresh()["obs"]
    a["k"][:] -= 2   # restored counters: the first call's bits again
    a.run_host()
    assert np.array_equal(a["obs"].view(np.uint32), first.view(np.uint32))


def test_env_offset_continues_the_stream_of_a_larger_run():
    """Rows 64 .. 127 of a 128-env call equal a 64-env call with offset 64 -- the noise, the dropout and the occlusion schedule."""
    big, small = ou.AugState(128, 7, 1, 3, 0.1, 0.1, seed=7), ou.AugState(64, 7, 1, 3, 0.1, 0.1, seed=7, env_offset=64)
    small["obs"][...], small["k"][:] = big["obs"][64:], big["k"][64:]
    big.run_host(), small.run_host()
    assert np.array_equal(big["obs"][64:].view(np.uint32), small["obs"].view(np.uint32))
    ob, os_ = ou.OcclState(128, 24, seed=8), ou.OcclState(64, 24, seed=8, env_offset=64)
    os_["count"][...], os_["k"][:] = ob["count"][64:], ob["k"][64:]
    ob.run_host(), os_.run_host()
    assert np.array_equal(ob["count"][64:], os_["count"]) and (ob["count"] >= 29).any()


def test_stream_keys_of_one_seed_are_apart():
    from phc_amd.env.tasks.humanoid_im import GETUP_DRAWS_TAG, OBS_AUG_TAG, OCCL_TAG, TASK_DRAWS_TAG
    from phc_amd.perturb import stream_key
    keys = {stream_key(3), stream_key(3, TASK_DRAWS_TAG), stream_key(3, GETUP_DRAWS_TAG), stream_key(3, OBS_AUG_TAG), stream_key(3, OCCL_TAG), stream_key(4, OBS_AUG_TAG),
            stream_key(4, OCCL_TAG)}
    assert len(keys) == 7


def test_no_two_draws_of_a_call_share_a_counter():
    """Pairs and dropout samples of one row, both uniforms of each, and the next count: all distinct draws (distinct counters under one key)."""
    u = ou.uniforms(ou.KEY, [3, 3], [10, 11], 0, 513 + 3).reshape(-1)
    assert len(np.unique(u)) > 0.999 * u.size


# ---- 3. statistics -----------------------------------------------------------------------------------------------------------------------------------
def _corr(a, b):
    a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


def test_statistics_of_65536_normals():
    """256 envs x 256 columns at count 0 (65 536 normals, 5-sigma bounds): |mean| < 5/256, |var - 1| < 5 sqrt(2/65536), the correlations between neighbouring
    columns, neighbouring envs and consecutive counts each below 5/256, max |z| <= 5.77."""
    z0 = ou.normals(ou.KEY, np.arange(256), np.zeros(256), 256)
    z1 = ou.normals(ou.KEY, np.arange(256), np.ones(256), 256)
    stats = dict(mean=float(z0.mean()), var=float(z0.astype(np.float64).var()), cols=_corr(z0[:, :-1], z0[:, 1:]), envs=_corr(z0[:-1], z0[1:]), counts=_corr(z0, z1),
                 largest=float(np.abs(z0).max()))
    print(stats)
    assert abs(stats["mean"]) < 5 / 256 and abs(stats["var"] - 1) < 5 * np.sqrt(2 / 65536)
    assert all(abs(stats[k]) < 5 / 256 for k in ("cols", "envs", "counts")) and stats["largest"] <= ou.R_MAX


def test_dropout_and_span_start_shares():
    """65 536 dropout uniforms (256 envs x 256 samples) and 65 536 span starts (4096 envs x bodies 1 .. 16) at p = 0.1: |p_hat - 0.1| < 5 sqrt(0.09 / 65536)."""
    u = ou.uniforms(ou.KEY, np.arange(256), np.zeros(256), 128, 256)[:, :, 0]
    s = ou.OcclState(4096, 17, prob=0.1, seed=2)
    s["count"][...] = 0
    s.run_host()
    shares = float((u < np.float32(0.1)).mean()), float((s["count"][:, 1:] > 0).mean())
    print("dropout share, span start share:", shares)
    assert all(abs(p - 0.1) < 5 * np.sqrt(0.09 / 65536) for p in shares) and (s["count"][:, 0] == 0).all()


def test_box_muller_is_finite_at_the_ends_of_u1():
    """u1 = 2^-24 (a = 1 - 2^-24): r = 5.768 <= 5.77; u1 = 1 (a = 0): r = 0; every b."""
    for b in (0.0, 0.25, 0.5, 0.75, 1 - 2.0 ** -24, 2.0 ** -24):
        far, zero = ou.box_muller(1 - 2.0 ** -24, b), ou.box_muller(0.0, b)
        assert np.isfinite(far).all() and np.abs(far).max() <= ou.R_MAX and abs(float(np.hypot(*far.astype(np.float64))) - 5.768) < 1e-3
        assert np.isfinite(zero).all() and (zero == 0).all()


# ---- 4. the bindings ---------------------------------------------------------------------------------------------------------------------------------
def test_struct_size_constants_and_symbols():
    from phc_amd import _lib as L, abi
    sh = ou.shim()
    assert C.sizeof(L.ObsAugArgs) == sh.obs_aug_sizeof_args() and sh.obs_aug_block() == ou.BLOCK
    assert (abi.OBS_AUG_MAX_OBS, abi.OBS_AUG_MAX_SAMPLES, abi.OCCL_MAX_BODIES) == (sh.obs_aug_max_obs(), sh.obs_aug_max_samples(), sh.occl_max_bodies()) == (65536, 1024, 64)
    assert {"phc_obs_augment", "phc_occl_advance"} <= set(L.EXPORTED_SYMBOLS)
    lib = L.load()
    assert hasattr(lib, "phc_obs_augment") and hasattr(lib, "phc_occl_advance")
    # one pair more than a workgroup pass, and more than two passes, are in the cases
    assert {2 * ou.BLOCK + 1, 4 * ou.BLOCK + 1} <= {c[1] for c in ou.CASES}


def test_argument_checks_return_their_codes_without_a_device():
    """The library's entry points on host pointers: every refusal comes back before any device work, and the host build's check functions agree.  Accepted
    arguments are only asked of the check functions -- they would launch."""
    from phc_amd import _lib as L
    lib, sh = L.load(), ou.shim()
    s = ou.AugState(4, 7, 1, 3, 0.1, 0.1, form="flag", select="all")
    assert sh.obs_augment_check_of(s.args()) == 0
    edge = s.args()
    edge.env_offset = (1 << 32) - 4
    assert sh.obs_augment_check_of(edge) == 0
    assert lib.phc_obs_augment(None, None) == -1 and sh.obs_augment_check_of(None) == -1
    ids = np.zeros(4, np.int64)
    refused = [("obs", None, -1), ("k", None, -1), ("num_envs", -1, -1), ("num_obs", -1, -1), ("num_samples", -1, -1), ("self_obs_size", -1, -1),
               ("self_obs_size", 8, -1), ("num_samples", 4, -1), ("env_ids", ids.ctypes.data, -1), ("n_ids", -1, -1), ("n_ids", 2, -1), ("env_offset", -1, -1),
               ("env_offset", (1 << 32) - 3, -1), ("dropout_p", -0.1, -1), ("dropout_p", 1.5, -1), ("dropout_p", float("nan"), -1), ("noise_std", -0.1, -1),
               ("noise_std", float("nan"), -1), ("num_obs", 65536 + 1 + 2, -2)]
    for field, value, code in refused:
        a = s.args()
        setattr(a, field, value)
        assert sh.obs_augment_check_of(a) == code, (field, value)
        assert lib.phc_obs_augment(a, None) == code, (field, value)
    a = s.args()   # above the limits with a tail that divides
    a.num_obs, a.self_obs_size, a.num_samples = 1 + 2050, 1, 2050
    assert sh.obs_augment_check_of(a) == -2 and lib.phc_obs_augment(a, None) == -2
    a = s.args()
    a.row_flag, a.env_ids, a.n_ids = None, ids.ctypes.data, 5    # more ids than envs cannot be distinct
    assert sh.obs_augment_check_of(a) == -1 and lib.phc_obs_augment(a, None) == -1
    a.n_ids = 0                                                   # an empty list: accepted, no launch
    assert lib.phc_obs_augment(a, None) == 0
    empty = s.args()
    empty.num_envs = 0
    assert lib.phc_obs_augment(empty, None) == 0
    o = ou.OcclState(4, 24)
    p = o.pointers()
    assert sh.occl_advance_check_of(4, 24, (1 << 32) - 4, p["k"], 1.0, 30, 31, p["count"], p["mask"]) == 0
    good = dict(n=4, J=24, off=0, k=p["k"], prob=0.1, lo=30, hi=60, count=p["count"], mask=p["mask"])
    for change, code in (({"k": None}, -1), ({"count": None}, -1), ({"mask": None}, -1), ({"n": -1}, -1), ({"J": -1}, -1), ({"off": -1}, -1), ({"off": (1 << 32) - 3}, -1),
                         ({"prob": -0.1}, -1), ({"prob": 1.1}, -1), ({"prob": float("nan")}, -1), ({"hi": 30}, -1), ({"hi": 29}, -1), ({"J": 65}, -2)):
        g = dict(good, **change)
        assert sh.occl_advance_check_of(g["n"], g["J"], g["off"], g["k"], g["prob"], g["lo"], g["hi"], g["count"], g["mask"]) == code, change
        assert lib.phc_occl_advance(g["n"], g["J"], 1, g["off"], g["k"], g["prob"], g["lo"], g["hi"], g["count"], g["mask"], None) == code, change
    assert lib.phc_occl_advance(0, 24, 1, 0, p["k"], 0.1, 30, 60, p["count"], p["mask"], None) == 0


SWITCHES = {"noise": ["env.add_obs_noise=True"], "dropout": ["env.fut_tracks=True", "env.numTrajSamples=3", "env.obs_v=6", "+env.fut_tracks_dropout=True"],
            "occl": ["+env.occl_training=True"]}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_the_options_in_the_host_phases(switch):
    """Host phases only: whole_step_capturable() follows `+env.task_rng=device` for each of the three switches, the device streams (hence the counters the
    device phase allocates) exist only for the options that draw from them, and torch mode plans none."""
    from test_task_config_cpu import host_task
    from phc_amd.env.tasks.humanoid_im import OBS_AUG_TAG, OCCL_TAG
    want = {"noise": {"_obs_aug_k": OBS_AUG_TAG}, "dropout": {"_obs_aug_k": OBS_AUG_TAG}, "occl": {"_occl_k": OCCL_TAG}}[switch]
    t = host_task(*SWITCHES[switch])
    assert (t.add_obs_noise, t._fut_tracks_dropout, t._occl_training) == (switch == "noise", switch == "dropout", switch == "occl")
    assert t.task_rng == "torch" and t._aug_streams == {} and not t.whole_step_capturable()
    d = host_task(*SWITCHES[switch], "+env.task_rng=device")
    assert d.task_rng == "device" and d._aug_streams == want and d.whole_step_capturable()
    plain = host_task("+env.task_rng=device")
    assert plain._aug_streams == {} and plain.whole_step_capturable() and host_task().whole_step_capturable()
    # every other blocker stays
    assert not host_task(*SWITCHES[switch], "+env.task_rng=device", "+env.enableHistObs=True").whole_step_capturable()


# ---- 5. the sanitizer program ------------------------------------------------------------------------------------------------------------------------
def test_host_build_runs_clean_under_the_address_and_undefined_sanitizers():
    """tests/obs_aug_asan_main.cpp (its own main; nothing is loaded into Python): the cases' shapes in all three selection forms and the occlusion schedule,
    on heap arrays of exact size."""
    returncode, stdout, stderr = host_build.run_sanitized("obs_aug_asan_main.cpp")
    print(stdout[-2000:], stderr)
    assert returncode == 0 and stdout.strip().endswith("ok"), stdout + stderr
