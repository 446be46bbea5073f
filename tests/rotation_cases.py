"""Constructed motion libraries whose frame pairs sit in every regime of the lookup's rotation math (helper of test_lookup_rotation_regimes.py,
not a test).

A mocap clip keeps `slerp` at cos_half_theta just below 1, the joints at moderate angles and the root upright.  The libraries made here are
2-frame clips (motion_dt = motion_length = 1/30 s) whose two frames hold chosen quaternion pairs, so that a lookup at time blend / 30 evaluates
slerp(q0, q1, blend) for a pair of a named regime, plus one 5-frame clip (so that `length_starts` is odd for most clips).

  REGIMES         the angle between the two frames: half_theta = acos|q0 . q1|
  pair_rotations  q1 = q0 * delta(2 half_theta), a random half of the q1 negated (the `c < 0` flip)
  exp_map_members first-frame local rotations for quat_to_exp_map / exp_map_round_trip: angles over [0, 2 pi) and the explicit edge members
  root_rotations  yaw grid x tilt for the heading functions
  make_library    the dict `backends.motion_lib_on` takes
  reference       the numpy oracle in fp32 and in fp64 on the same fp32 data, and per case the regime with s / sin_theta / angle of the fp64 run
  excluded        the cases inside a threshold or discontinuity band
  bin_keys / check_bins   the per-regime tolerance rule

Everything is evaluated on the fp32 data the kernels read: the fp64 oracle is the oracle's dtype-generic code on `lib` cast to float64."""
import numpy as np

import phc_oracle as po

F = np.float32
DT = F(1 / 30)

# half_theta ranges.  No pair has s = sin(half_theta) in [0.7e-3, 1.4e-3]: around the 0.001 threshold a 1-ulp difference in c legitimately changes
# the branch, and the midpoint and the slerp differ by up to ~5e-4 there.  (`identical`: |q0|^2 of an fp32 unit quaternion is within 1.2e-7 of 1, so
# s <= 5.5e-4 -- the midpoint branch, 0.5 q0 + 0.5 q0 = q0 exactly -- or c >= 1, q0 itself.)
REGIMES = ("identical", "tiny", "small", "mid", "large", "near_antipodal")
RANGES = {"identical": (0.0, 0.0), "tiny": (1e-7, 3e-4), "small": (2e-3, 0.1), "mid": (0.1, 0.5), "large": (0.5, np.pi / 2 - 0.05),
          "near_antipodal": (np.pi / 2 - 1e-3, np.pi / 2 + 1e-3)}
LOG_UNIFORM = ("tiny", "small")          # ranges of more than a decade
IDENTICAL, MID = REGIMES.index("identical"), REGIMES.index("mid")
S_BAND = (0.7e-3, 1.4e-3)                # slerp's |s| < 0.001
PI_BAND = 1e-3                           # normalize_angle(2 acos w) returns +pi or -pi at pi
MASK_BAND = (0.5e-5, 2e-5)               # the 1e-5 masks of quat_to_angle_axis / exp_map_to_angle_axis
BASE_ROT = np.array([0.5, 0.5, 0.5, 0.5])   # remove_base_rot strips this factor (humanoid.py:1936-1939)

FRAME_KEYS = ("gts", "grs", "gvs", "gavs", "lrs", "dvs", "dof_pos", "gts_t", "grs_t")


# ---- fp64 quaternion construction (xyzw) ------------------------------------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def axis_angle(axis, angle):
    h = 0.5 * np.asarray(angle, np.float64)[..., None]
    return np.concatenate([unit(axis) * np.sin(h), np.cos(h)], axis=-1)


def random_rotations(rng, shape):
    return unit(rng.standard_normal(tuple(shape) + (4,)))


def draw_half_theta(rng, regime_idx):
    ht = np.zeros(regime_idx.shape)
    for r, name in enumerate(REGIMES):
        m = regime_idx == r
        lo, hi = RANGES[name]
        ht[m] = np.exp(rng.uniform(np.log(lo), np.log(hi), m.sum())) if name in LOG_UNIFORM else rng.uniform(lo, hi, m.sum())
    return ht


def pair_rotations(rng, q0, regime_idx):
    """fp32 (q0, q1) with q1 = q0 * delta(2 half_theta) of the regime about a random axis and a random half of the q1 negated.  `q0`: fp64, or fp32 to be
    kept bit for bit (the explicit exp-map members); `identical` pairs are q1 = +-q0 bit for bit."""
    regime_idx = np.asarray(regime_idx)
    delta = axis_angle(rng.standard_normal(regime_idx.shape + (3,)), 2.0 * draw_half_theta(rng, regime_idx))
    q0_32 = np.asarray(q0).astype(F)
    q1_32 = qmul(q0_32.astype(np.float64), delta).astype(F)
    same = regime_idx == IDENTICAL
    q1_32[same] = q0_32[same]
    neg = rng.random(regime_idx.shape) < 0.5
    q1_32[neg] = -q1_32[neg]
    return q0_32, q1_32


def exp_map_members(rng, n):
    """n fp32 first-frame local rotations for quat_to_exp_map / exp_map_round_trip, the flag of those that must sit in an `identical` pair and the flag
    of those that must not sit in a `tiny` one (|q| = 1 - 3e-7 puts c = |q|^2 cos at 1 - 6e-7, s = 1.1e-3, inside the band).  Pinned: the
    members at |w| = 1 to rounding, where the 1-ulp factor a slerp of another regime applies at blend 0 moves w across |w| = 1 (sin_theta 0 / NaN /
    3.4e-4: fp32 has no w in between) and would make them test something else.
    Every 4th is an explicit member, the rest have angles spread over [0, 2 pi) about random axes.  No angle is within 1e-3 of pi; sin_theta of fp32 data
    is 0, NaN or >= 3.4e-4, outside the mask band [0.5e-5, 2e-5] by the format itself; the members for the SECOND mask (exp_map_to_quat's, on
    |exp-map| ~ 2 |v|) have |v| = 1e-6 and 3e-5."""
    ax = lambda: rng.standard_normal(3)
    one_below = np.nextafter(F(1), F(0))

    def with_w(angle, w):
        q = axis_angle(ax(), angle).astype(F)
        q[3] = w
        return q

    def with_v(vn, w):
        return np.concatenate([unit(ax()) * vn, [w]]).astype(F)

    def scaled(angle, k):
        return (axis_angle(ax(), angle).astype(F) * F(k)).astype(F)

    explicit = [   # (quaternion, True: pin to an identical pair / None: keep out of tiny pairs)
        (lambda: axis_angle(ax(), 0.0).astype(F), True), (lambda: axis_angle(ax(), 1e-6).astype(F), True), (lambda: axis_angle(ax(), 3e-5).astype(F), True),
        (lambda: axis_angle(ax(), np.pi - 0.05).astype(F), False), (lambda: axis_angle(ax(), np.pi + 0.05).astype(F), False),
        (lambda: axis_angle(ax(), 2 * np.pi - 1e-3).astype(F), True),                              # (w two ulp from -1)
        (lambda: with_w(1e-4, 1.0), True), (lambda: with_w(1e-4, -1.0), True),                     # w = +-1 exactly, v != 0
        (lambda: scaled(4e-4, 1 + 3e-7), True), (lambda: scaled(4e-4, 1 - 3e-7), True),            # not quite unit: |w| > 1 by rounding -> NaN -> default axis
        (lambda: scaled(2 * np.pi - 4e-4, 1 + 3e-7), True), (lambda: scaled(2 * np.pi - 4e-4, 1 - 3e-7), True),
        (lambda: scaled(rng.uniform(0.2, 3.0), 1 + 3e-7), False), (lambda: scaled(rng.uniform(3.3, 6.0), 1 - 3e-7), None),
        (lambda: scaled(rng.uniform(0.2, 3.0), 1 + 1e-3), False), (lambda: scaled(rng.uniform(0.2, 3.0), 1 - 1e-3), False),   # the |v| / s factor
        (lambda: scaled(rng.uniform(3.3, 6.0), 1 + 1e-3), False), (lambda: scaled(rng.uniform(3.3, 6.0), 1 - 1e-3), False),
        (lambda: with_v(1e-6, one_below), True), (lambda: with_v(3e-5, one_below), True),          # second mask: |exp-map| 2e-6 (masked) and 6e-5 (kept)
    ]
    q, pin, no_tiny = np.zeros((n, 4), F), np.zeros(n, bool), np.zeros(n, bool)
    for i in range(n):
        if i % 4 == 0:
            make, p = explicit[(i // 4) % len(explicit)]
            q[i], pin[i], no_tiny[i] = make(), p is True, p is None
        else:
            a = rng.uniform(0.0, 2 * np.pi)
            if abs(a - np.pi) < 10 * PI_BAND:
                a = np.pi + 0.5
            q[i] = axis_angle(ax(), a).astype(F)
    return q, pin, no_tiny


# root pairs: the heading atan2 stays well conditioned while the rotated x axis keeps a horizontal length >= 0.5, i.e. an elevation <= 60 deg.  A tilt
# about a horizontal axis lifts x by at most the tilt and the pair's delta by at most its own angle 2 half_theta, so tilt <= 60 deg - 2 half_theta with
# half_theta <= 0.5 (identical ... mid) keeps both frames, and every rotation slerp puts between them, inside.
ROOT_REGIMES = ("identical", "tiny", "small", "mid")
YAW_GRID = np.arange(-7, 8) * (np.pi / 8)      # all four quadrants, 0 and +-pi/2 exactly (to fp64), none within 0.39 of +-pi


def root_rotations(rng, n, base_rot=False):
    """n root pairs: yaw over YAW_GRID (every 5th clip untilted, so the grid's yaw is the pair's heading exactly), tilt about a random horizontal axis.
    `base_rot`: post-multiplied by (0.5, 0.5, 0.5, 0.5), for the remove_base_rot=True runs that strip that factor before they take the heading."""
    regime_idx = np.array([REGIMES.index(ROOT_REGIMES[i % len(ROOT_REGIMES)]) for i in range(n)])
    ht = draw_half_theta(rng, regime_idx)
    yaw = YAW_GRID[np.arange(n) % len(YAW_GRID)]
    tilt = rng.uniform(0.0, 1.0, n) * np.maximum(np.pi / 3 - 2 * ht - 1e-3, 0.0)
    tilt[np.arange(n) % 5 == 0] = 0.0
    phi = rng.uniform(0, 2 * np.pi, n)
    q0 = qmul(axis_angle(np.tile([0.0, 0.0, 1.0], (n, 1)), yaw), axis_angle(np.stack([np.cos(phi), np.sin(phi), np.zeros(n)], -1), tilt))
    delta = axis_angle(rng.standard_normal((n, 3)), 2.0 * ht)
    q1 = qmul(q0, delta)
    if base_rot:
        q0, q1 = qmul(q0, BASE_ROT), qmul(q1, BASE_ROT)
    q0_32, q1_32 = q0.astype(F), q1.astype(F)
    same = regime_idx == IDENTICAL
    q1_32[same] = q0_32[same]
    neg = rng.random(n) < 0.5
    q1_32[neg] = -q1_32[neg]
    return q0_32, q1_32, regime_idx


def make_pairs(rng, num_clips, num_bodies, num_ext=0, spherical=True, regimes=REGIMES, amp_roots=False, base_rot=False):
    """The `pairs` argument of make_library: global pairs for every (clip, slot), local pairs for every (clip, body) of a spherical model.  Regimes are
    drawn uniformly from `regimes`, global and local independently; `amp_roots`: slot 0 holds root_rotations()."""
    pool = np.array([REGIMES.index(r) for r in regimes])
    slots = num_bodies + num_ext
    g_regime = pool[rng.integers(0, len(pool), (num_clips, slots))]
    g0, g1 = pair_rotations(rng, random_rotations(rng, (num_clips, slots)), g_regime)
    if amp_roots:
        g0[:, 0], g1[:, 0], g_regime[:, 0] = root_rotations(rng, num_clips, base_rot)
    pairs = dict(g0=g0, g1=g1, g_regime=g_regime)
    if spherical:
        l_regime = pool[rng.integers(0, len(pool), (num_clips, num_bodies))]
        members, pin, no_tiny = exp_map_members(rng, num_clips * num_bodies)
        l_regime[pin.reshape(num_clips, num_bodies)] = IDENTICAL
        l_regime[no_tiny.reshape(num_clips, num_bodies) & (l_regime == REGIMES.index("tiny"))] = REGIMES.index("small")
        l0, l1 = pair_rotations(rng, members.reshape(num_clips, num_bodies, 4), l_regime)
        pairs.update(l0=l0, l1=l1, l_regime=l_regime)
    return pairs


def make_library(num_bodies, num_ext, dofs_per_joint, pairs, rng):
    """The dict `backends.motion_lib_on` takes (robot layout with `dof_pos`, `gts_t`, `grs_t` for dofs_per_joint == 1): 2-frame clips holding `pairs`, and one
    5-frame clip of `mid` steps as motion 1, so that length_starts is 0, 2, 7, 9, ...  Positions and velocities are unit-scale random numbers.
    Extra keys (not part of the library): `pair_motion_ids` [clips], `long_motion_id`, and per frame f the regime of the pair (f, next frame) in
    `g_regime` [frames, slots] / `l_regime` [frames, bodies]."""
    C, nb, slots = pairs["g0"].shape[0], num_bodies, num_bodies + num_ext
    spherical = dofs_per_joint != 1
    assert pairs["g0"].shape[1] == slots and (not spherical or num_ext == 0)
    LONG = 5
    nf = np.array([2, LONG] + [2] * (C - 1), dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(nf)[:-1]]).astype(np.int64)
    Ftot = int(nf.sum())
    pair_ids = np.array([0] + list(range(2, C + 1)), dtype=np.int64)
    f_pair = starts[pair_ids]

    def long_chain(width):     # 5 frames, consecutive ones a `mid` step apart
        q = [random_rotations(rng, (width,)).astype(F)]
        for _ in range(LONG - 1):
            q.append(pair_rotations(rng, q[-1], np.full(width, MID))[1])
        return np.stack(q)

    def rotations(q0, q1, regime, width):
        rot, reg = np.zeros((Ftot, width, 4), F), np.full((Ftot, width), IDENTICAL)     # (a clip's last frame blends with itself)
        rot[f_pair], rot[f_pair + 1], reg[f_pair] = q0, q1, regime
        rot[starts[1]:starts[1] + LONG] = long_chain(width)
        reg[starts[1]:starts[1] + LONG - 1] = MID
        return rot, reg

    rnd = lambda *shape: rng.standard_normal((Ftot,) + shape).astype(F)
    grs_all, g_regime = rotations(pairs["g0"], pairs["g1"], pairs["g_regime"], slots)
    gts_all = rnd(slots, 3)
    lib = dict(gts=gts_all[:, :nb].copy(), grs=grs_all[:, :nb].copy(), gvs=rnd(nb, 3), gavs=rnd(nb, 3),
               motion_lengths=((nf - 1).astype(F) * DT).astype(F), motion_dt=np.full(C + 1, DT, F), motion_num_frames=nf, length_starts=starts,
               pair_motion_ids=pair_ids, long_motion_id=1, g_regime=g_regime)
    if spherical:
        lib["lrs"], lib["l_regime"] = rotations(pairs["l0"], pairs["l1"], pairs["l_regime"], nb)
        lib["dvs"] = rnd(nb - 1, 3)
    else:
        lib.update(dof_pos=rnd(nb - 1), dvs=rnd(nb - 1), gts_t=gts_all, grs_t=grs_all)
    return lib


# ---- reference and case classification ---------------------------------------------------------------------------------------------------------
def _pair_s(q0, q1):
    c = np.abs((q0 * q1).sum(-1))
    with np.errstate(invalid="ignore"):
        return np.sqrt(1.0 - c * c)          # NaN: c > 1 (not-quite-unit data), the `|c| >= 1` branch


def reference(lib, ids, times, offset=None):
    """(r32, r64, cases): the oracle's lookup (po.get_motion_state, or po.get_motion_state_robot for a robot library) on `lib` as it is and on `lib` cast
    to float64, and per case the fp64 run's classification:
      g_regime, g_s          [n, slots]   regime name index and s = sqrt(1 - c^2) of the global pair the lookup blends
      l_regime, l_s          [n, bodies]  the same for the local pair (spherical libraries)
      w, sin_theta, angle    [n, bodies]  of the slerped local rotation: sqrt(1 - w^2) and 2 acos w (NaN for |w| > 1)
      ang2                   [n, bodies]  |exp-map| the second mask of the AMP round trip sees: |normalize_angle(angle)| |v| / sin_theta"""
    fn = po.get_motion_state_robot if "dof_pos" in lib else po.get_motion_state
    lib64 = {k: (v.astype(np.float64) if k in FRAME_KEYS else v) for k, v in lib.items()}
    r32, r64 = fn(lib, ids, times, offset), fn(lib64, ids, times, offset)
    f0, f1 = r64["f0l"], r64["f1l"]
    assert (f0 == r32["f0l"]).all() and (f1 == r32["f1l"]).all() and (r32["blend"] == r64["blend"]).all()
    same = (f0 == f1)[:, None]
    g = lib64.get("grs_t", lib64["grs"])
    cases = dict(g_regime=np.where(same, IDENTICAL, lib["g_regime"][f0]), g_s=_pair_s(g[f0], g[f1]))
    if "lrs" in lib:
        l0, l1 = lib64["lrs"][f0], lib64["lrs"][f1]
        lr = po.slerp(l0, l1, r64["blend"][:, None, None])
        w = lr[..., 3]
        with np.errstate(invalid="ignore", divide="ignore"):
            sin_theta, angle = np.sqrt(1.0 - w * w), 2.0 * np.arccos(w)
            ang2 = np.abs(po.normalize_angle(angle)) * np.linalg.norm(lr[..., :3], axis=-1) / sin_theta
        cases.update(l_regime=np.where(same, IDENTICAL, lib["l_regime"][f0]), l_s=_pair_s(l0, l1), w=w, sin_theta=sin_theta, angle=angle, ang2=ang2)
    return r32, r64, cases


def _in(x, band):
    with np.errstate(invalid="ignore"):
        return (x >= band[0]) & (x <= band[1])


def excluded(cases, what):
    """Mask of the cases inside a threshold or discontinuity band, on the fp64 values:
      "rb_rot"     [n, slots]   s of the global pair in S_BAND -- unless the pair is `identical` (q1 = +-q0 bit for bit): the midpoint is q0 and the slerp
                                (sin((1 - t) h) + sin(t h)) / sin(h) q0 = q0 (1 + O(h^2)), 2e-7 apart at h = 1.4e-3, so the branch does not matter there
                                (a not-quite-unit q0 of norm 1 - 3e-7 has s = 1.1e-3 with itself)
      "dof_pos"    [n, bodies]  s of the local pair in S_BAND, the slerped rotation's angle within PI_BAND of pi, or its sin_theta in MASK_BAND
      "amp_joint"  [n, bodies]  as dof_pos without the pi band (the round trip maps +pi and -pi to the same rotation) but with |exp-map| in MASK_BAND"""
    if what == "rb_rot":
        return _in(cases["g_s"], S_BAND) & (cases["g_regime"] != IDENTICAL)
    m = (_in(cases["l_s"], S_BAND) & (cases["l_regime"] != IDENTICAL)) | _in(cases["sin_theta"], MASK_BAND)
    if what == "dof_pos":
        with np.errstate(invalid="ignore"):
            return m | (np.abs(cases["angle"] - np.pi) < PI_BAND)
    assert what == "amp_joint"
    return m | _in(cases["ang2"], MASK_BAND)


def _decade(x, lo):
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.floor(np.log10(x))
    return np.where(np.isnan(x), 99, np.clip(np.nan_to_num(d, nan=0.0, neginf=lo), lo, -1)).astype(int)


def bin_keys(cases, what):
    """One bin name per case: the pair's regime split by the decade of s; for the joints further by the sign of w and the decade of sin_theta of the slerped
    rotation.  (`nan`: c > 1 resp. |w| > 1; decades are clipped to 1e-5 and to [0.1, 1].)"""
    reg, s = (cases["g_regime"], cases["g_s"]) if what == "rb_rot" else (cases["l_regime"], cases["l_s"])
    ds = _decade(s, -5)
    name = lambda d: "nan" if d == 99 else f"1e{d}"
    keys = np.empty(reg.shape, dtype=object)
    if what == "rb_rot":
        for idx in np.ndindex(reg.shape):
            keys[idx] = f"{REGIMES[reg[idx]]} s~{name(ds[idx])}"
        return keys
    dt = _decade(cases["sin_theta"], -5)
    neg = cases["w"] < 0
    for idx in np.ndindex(reg.shape):
        keys[idx] = f"{REGIMES[reg[idx]]} s~{name(ds[idx])} w{'-' if neg[idx] else '+'} sin~{name(dt[idx])}"
    return keys


def well_conditioned(cases, what):
    """The cases where the new tests must not be looser than the golden test's 2e-5 against the fp32 oracle: slerp with s >= 0.5 (or an identical pair,
    which is exact); for the joints additionally sin_theta >= 0.1 with w >= 0."""
    reg, s = (cases["g_regime"], cases["g_s"]) if what == "rb_rot" else (cases["l_regime"], cases["l_s"])
    with np.errstate(invalid="ignore"):
        m = (s >= 0.5) | (reg == IDENTICAL)
        return m if what == "rb_rot" else m & (cases["sin_theta"] >= 0.1) & (cases["w"] >= 0)


FACTOR, FLOOR, STRICT, MAX_EXCLUDED = 4.0, 2e-6, 2e-5, 0.02


def check_bins(label, got, r32, r64, keys, excl, strict):
    """The tolerance rule.  `got`, `r32`, `r64`: [cases, components]; `keys`, `excl`, `strict`: [cases].
    E_bin = the largest componentwise |fp32 oracle - fp64 oracle| over the bin's non-excluded cases (the reference formula's own fp32 error, which does not
    involve the code under test); the backend passes the bin if its distance to the fp64 oracle is <= 4 E_bin + 2e-6; `strict` cases are additionally
    within 2e-5 of the fp32 oracle; at most 2 % of the cases are excluded.  Prints one line per bin and returns them."""
    got, r32, r64 = (np.asarray(a, np.float64).reshape(len(keys), -1) for a in (got, r32, r64))
    assert np.isfinite(got).all(), f"{label}: non-finite output"
    assert np.isfinite(r32).all() and np.isfinite(r64).all()
    share = excl.mean()
    print(f"[{label}] cases {len(keys)}, excluded {excl.sum()} ({100 * share:.2f} %)")
    assert share <= MAX_EXCLUDED, f"{label}: {100 * share:.2f} % of the cases excluded"
    e, d = np.abs(r32 - r64).max(-1), np.abs(got - r64).max(-1)
    rows, bad = [], []
    for k in sorted(set(keys[~excl])):
        m = (keys == k) & ~excl
        E, D = e[m].max(), d[m].max()
        rows.append((k, int(m.sum()), E, D))
        print(f"[{label}] {k:<44s} n={m.sum():<6d} E_bin={E:.2e}  dist={D:.2e}  bound={FACTOR * E + FLOOR:.2e}")
        if not D <= FACTOR * E + FLOOR:
            bad.append((k, E, D))
    assert not bad, f"{label}: bins beyond 4 E_bin + 2e-6: {bad}"
    ms = strict & ~excl
    if ms.any():
        ds = np.abs(got - r32).max(-1)[ms].max()
        print(f"[{label}] well-conditioned cases n={ms.sum()}: max distance to the fp32 oracle {ds:.2e}")
        assert ds <= STRICT, f"{label}: well-conditioned cases {ds:.2e} from the fp32 oracle"
    return rows
