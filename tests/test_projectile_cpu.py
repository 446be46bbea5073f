"""Thrown projectiles (`+projectile.*`, phc_proj_advance) on a machine without a GPU: the host build of phc_amd/csrc/phc_proj.h (tests/proj_shim.cpp) against
tests/proj_util.py's fp64 statement of the rules, on constructed cases in every decision regime, each on SMPL (26 shapes, the 32-lane mapping's sizes) and G1 (42
shapes) with 1 and 4 slots; the impulse bookkeeping; the aim of a throw; the draws; the options, the task's refusals, the binding and the argument checks; a
stand-alone sanitizer program; and a random run under the 2 % cap on dropped envs.

Decisions (last_hit, hits, life, countdown, thrown, k) are exact.  Floats are held to proj_util.float_bounds, derived there from fp32 unit round-off u = 2^-24
and the case's magnitudes (reach 4.5 m, speeds up to 12 m/s, K = 64 rounded operations per quantity and env step): with the default 0.1 m sphere,
pos_tol = K u reach = 1.7e-5 m and free-flight vel_tol = 4.6e-5 m/s; a hit at centre distance d of impulse j adds n_err = 2 pos_tol / d to the normal and gives
force_tol = (m (1 + e) (2 vel_free + 2 speed n_err) + |j| (K u + 4 n_err)) / dt -- for m = 3 kg at 5 m/s on the shin's 0.054 m capsule 0.9 N of a 292 N force (vel 1.1e-2 m/s, torque 5.9e-2 N m).  Over a
flight of L env steps the random run takes K L.  Worst measured (printed by every test): constructed cases pos 5.8e-7 m, vel 2.4e-6 m/s, force 2.2e-4 N, torque
4.7e-5 N m; random run (696 hits, no env dropped) pos 3.7e-6 m, vel 8.3e-5 m/s, force 7.8e-3 N, torque 4.9e-4 N m."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import proj_util as pu
import host_build

ROBOTS = ["smpl_humanoid", "g1_humanoid"]
R, G, DT, S = 0.1, -9.81, 1 / 30, 8
H = np.float64(np.float32(DT)) / S
WORST = np.zeros(4)


# ---- building a case -------------------------------------------------------------------------------------------------------------------------------------------
def scene(robot, count, n=3, moving=False, bystander=True, **kw):
    """n envs of posed bodies half a metre above their standing height (the ground stays out of the body cases), at rest unless `moving`, past the schedule's
    first launch, every slot parked -- but for a bystander in free flight far from everything, where there is a slot to spare."""
    m = pu.model(robot)
    rbs = pu.posed_rbs(m, n, seed=5, vel=0.3 if moving else 0.0, ang=0.5 if moving else 0.0, height=1.45)
    h = pu.HostProj(m, n, rbs, capsules=pu.tables(m)["capsules"].copy(), count=count, **kw)
    h.started()
    if count > 1 and bystander:
        h.place(0, n - 1, (3.0, 3.0, 2.0), (1.0, 0.5, 0.0), 2.0)
    return m, h


def only(h, *shapes):
    """Take every other shape out of the collision list (radius 0): the neighbours across a joint overlap the ends of a limb's capsule."""
    h.tab["capsules"][[i for i in range(len(h.tab["capsules"])) if i not in shapes], 6] = 0.0


def capsule(h, env, s, t=0.0):
    """Shape s of env `env` in env axes at time t behind the start of the step (fp64): A, B, radius, unit axis."""
    cap, b = h.tab["capsules"][s].astype(np.float64), int(h.tab["owner"][s])
    row = h.rbs[env, b].astype(np.float64)
    ra, rb = pu.quat_rot(row[3:7], cap[0:3]), pu.quat_rot(row[3:7], cap[3:6])
    A = row[0:3] + ra + (row[7:10] + np.cross(row[10:13], ra)) * t
    B = row[0:3] + rb + (row[7:10] + np.cross(row[10:13], rb)) * t
    ax = (B - A) / max(np.linalg.norm(B - A), 1e-12)
    return A, B, cap[6], ax


def side_dir(ax):
    """A unit vector across the axis, as far up as the axis allows (x^ for a vertical one)."""
    u = np.array([0.0, 0.0, 1.0]) - ax[2] * ax
    if np.linalg.norm(u) < 0.3:
        u = np.array([1.0, 0.0, 0.0]) - ax[0] * ax
    return u / np.linalg.norm(u)


def long_shape(m, h):
    """A long, slim capsule: the left shin."""
    s = m.body_names.index("L_Knee" if "L_Knee" in m.body_names else "left_knee_link")
    A, B, rc, _ = capsule(h, 0, s)
    assert rc > 0 and np.linalg.norm(B - A) > 0.15
    return s


def aim(h, slot, env, x_want, v_pre, sub=1, mass=3.0, life=5):
    """Place a flying projectile so that it stands at x_want after `sub` sub-intervals: x_i = x_pre + h (i v_pre + g h i (i + 1) / 2 z^)."""
    assert x_want[2] > R + 0.02, "the case is about bodies, not the ground"
    v_pre = np.asarray(v_pre, dtype=np.float64)
    x_pre = np.asarray(x_want) - H * (sub * v_pre + np.array([0.0, 0.0, G * H * sub * (sub + 1) / 2]))
    h.place(slot, env, x_pre, v_pre, mass, life=life)


def run(h, what, progress=None, speed=12.0):
    """One step of the host build and of the oracle from the same state; decisions exact, floats in the derived bound."""
    o = pu.Oracle(h)
    h.advance(progress)
    o.step(progress)
    worst = pu.compare(h, o, pu.float_bounds(o, speed), what)
    np.maximum(WORST, worst, out=WORST)
    print(f"{what}: worst |host build - fp64| pos {worst[0]:.2e} m, vel {worst[1]:.2e} m/s, force {worst[2]:.2e} N, torque {worst[3]:.2e} N m; "
          f"over the module so far {WORST}")
    return o


def bookkeeping(h, o, before_vel):
    """For every hit of the step: dt * sum_b force[b] == -m (v_after - v_ballistic), the struck row alone is non-zero, and torque == r x force."""
    for hl in o.hit_log:
        env, slot = hl["env"], hl["slot"]
        alone = sum(1 for x in o.hit_log if x["env"] == env) == 1
        if not alone:
            continue
        f = h.force[env].astype(np.float64)
        row = int(h.tab["owner"][hl["shape"]])
        assert (np.delete(f, row, axis=0) == 0).all() and (np.delete(h.torque[env], row, axis=0) == 0).all(), "the force lands on the owner's row alone"
        ballistic = before_vel[slot, env].astype(np.float64) + np.array([0.0, 0.0, G * H * S])
        dv = h.vel[slot, env].astype(np.float64) - ballistic
        tol = pu.float_bounds(o, 12.0)
        np.testing.assert_allclose(float(h.args.dt) * f.sum(0), -hl["m"] * dv, atol=hl["m"] * tol[1] + float(h.args.dt) * tol[2])
        np.testing.assert_allclose(h.torque[env, row], np.cross(hl["r"], f[row]), atol=tol[3])


CASES = [(r, c) for r in ROBOTS for c in (1, 4)]
case = pytest.mark.parametrize("robot,count", CASES, ids=[f"{r.split('_')[0]}-{c}" for r, c in CASES])


# ---- the regimes ---------------------------------------------------------------------------------------------------------------------------------------------------
@case
@pytest.mark.parametrize("where", ["side", "cap"])
def test_hit_on_a_cylinder_side_and_on_an_end_cap(robot, count, where):
    m, h = scene(robot, count)
    s = long_shape(m, h)
    if where == "cap":
        only(h, s)
    A, B, rc, ax = capsule(h, 0, s, H)
    u = side_dir(ax) if where == "side" else ax
    base = 0.5 * (A + B) if where == "side" else B
    aim(h, count - 1, 0, base + u * (rc + R - 0.01), -5.0 * u)
    before = h.vel.copy()
    o = run(h, f"{robot} {where}")
    assert h.last_hit[count - 1, 0] == s and h.hits[count - 1, 0] == 1 and h.hits.sum() == 1 and h.life[count - 1, 0] == 4
    np.testing.assert_allclose(o.hit_log[0]["n"], u, atol=1e-6)
    assert np.linalg.norm(h.force[0, int(h.tab["owner"][s])]) > 50.0
    assert h.vel[count - 1, 0].astype(np.float64) @ u > -4.5, "the impulse acts along the normal (a light link gives way: the sphere need not turn back)"
    bookkeeping(h, o, before)


@case
def test_hit_on_an_extra_shape_lands_on_the_owner_row(robot, count):
    m, h = scene(robot, count)
    s = m.num_bodies if robot == "smpl_humanoid" else m.num_bodies + 1   # SMPL's second toe capsule, G1's third torso capsule
    owner = int(h.tab["owner"][s])
    assert m.body_names[owner] == ("L_Toe" if robot == "smpl_humanoid" else "torso_link") and owner != s
    only(h, s)
    A, B, rc, ax = capsule(h, 0, s, H)
    u = side_dir(ax)
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R - 0.01), -4.0 * u)
    before = h.vel.copy()
    o = run(h, f"{robot} extra shape")
    assert h.last_hit[count - 1, 0] == s and np.linalg.norm(h.force[0, owner]) > 10.0
    bookkeeping(h, o, before)


@case
@pytest.mark.parametrize("gap_mm", [1, -1])
def test_a_millimetre_decides(robot, count, gap_mm):
    m, h = scene(robot, count)
    s = long_shape(m, h)
    only(h, s)
    A, B, rc, ax = capsule(h, 0, s, H * S)
    u, w = side_dir(ax), np.cross(ax, side_dir(ax))
    # grazing: the sphere moves along the axis-normal tangent w and reaches gap = +-1 mm in the LAST sub-interval, approaching by 0.2 m/s
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R + 1e-3 * gap_mm), 0.5 * w - 0.2 * u + np.array([0, 0, -G * H * S]), sub=S)
    o = run(h, f"{robot} gap {gap_mm:+d} mm")
    assert h.hits.sum() == (1 if gap_mm < 0 else 0) and h.last_hit[count - 1, 0] == (s if gap_mm < 0 else -1)
    if gap_mm > 0:
        assert (h.force == 0).all() and (h.torque == 0).all()


@case
def test_overlapping_but_separating_is_no_hit(robot, count):
    m, h = scene(robot, count)
    s = long_shape(m, h)
    only(h, s)
    A, B, rc, ax = capsule(h, 0, s, H)
    u = side_dir(ax)
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R - 0.03), 6.0 * u)
    o = run(h, f"{robot} separating")
    assert h.hits.sum() == 0 and (h.last_hit == -1).all() and (h.force == 0).all() and not o.hit_log


@case
@pytest.mark.parametrize("kind", ["deepest", "tie"])
def test_two_shapes_entered_in_one_sub_interval(robot, count, kind):
    """Body j is laid onto body i (the same row of rigid_body_state) and given i's capsule: an exact tie, which the lowest index wins; with j's radius 2 cm
    larger, j is the deeper one and wins against the lower index."""
    m, h = scene(robot, count)
    i = long_shape(m, h)
    j = m.num_bodies - 1
    assert j > i
    h.rbs[:, j] = h.rbs[:, i]
    h.tab["capsules"][j] = h.tab["capsules"][i]
    if kind == "deepest":
        h.tab["capsules"][j, 6] += 0.02
    only(h, i, j)
    A, B, rc, ax = capsule(h, 0, i, H)
    u = side_dir(ax)
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R - 0.01), -5.0 * u)
    o = run(h, f"{robot} two shapes, {kind}")
    assert h.last_hit[count - 1, 0] == (i if kind == "tie" else j) and h.hits.sum() == 1
    struck = i if kind == "tie" else j
    assert np.linalg.norm(h.force[0, struck]) > 0 and (h.force[0, j if kind == "tie" else i] == 0).all()


@case
@pytest.mark.parametrize("kind", ["recedes", "catches_up"])
def test_a_spinning_body_flips_the_sign_of_vn(robot, count, kind):
    m, h = scene(robot, count)
    s = long_shape(m, h)
    only(h, s)
    A, B, rc, ax = capsule(h, 0, s)
    u = side_dir(ax)
    ra = 0.5 * (A + B) - h.rbs[0, s, 0:3].astype(np.float64)
    lever = np.cross(ra, u)
    assert np.linalg.norm(lever) > 0.05
    point_speed = -1.0 if kind == "recedes" else 1.0                       # of the capsule's middle along u: (w x ra) . u = w . (ra x u)
    h.rbs[0, s, 10:13] = point_speed * lever / (lever @ lever)
    A, B, rc, ax = capsule(h, 0, s, H)
    v = (-0.5 if kind == "recedes" else 0.5) * u                            # the sphere approaches in env axes (recedes) / leaves (catches up)
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R - 0.02), v)
    o = run(h, f"{robot} spinning, {kind}")
    assert h.hits.sum() == (0 if kind == "recedes" else 1)
    if kind == "catches_up":
        assert o.hit_log[0]["vn"] == pytest.approx(-0.5, abs=0.06)


@case
@pytest.mark.parametrize("sub", [1, S])
def test_hit_in_the_first_and_in_the_last_sub_interval(robot, count, sub):
    m, h = scene(robot, count, moving=True)
    s = long_shape(m, h)
    only(h, s)
    A, B, rc, ax = capsule(h, 0, s, H * sub)
    u = side_dir(ax)
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R - 0.01), -5.0 * u, sub=sub)
    before = h.vel.copy()
    o = run(h, f"{robot} sub-interval {sub}")
    assert h.last_hit[count - 1, 0] == s and h.hits.sum() == 1
    # (the impulse came in sub-interval `sub`: the sphere has moved on with its new velocity for the S - sub intervals behind it)
    bookkeeping(h, o, before)


@case
def test_a_second_overlap_later_in_the_step_is_ignored(robot, count):
    """The struck body chases the sphere at 2 m/s: after the impulse of sub-interval 1 the sphere still overlaps and the capsule still closes in -- a candidate in
    every later sub-interval, and no second hit in this env step; the next step hits again at once."""
    m, h = scene(robot, count)
    s = long_shape(m, h)
    only(h, s)
    u = side_dir(capsule(h, 0, s)[3])
    h.rbs[0, s, 7:10] = 2.0 * u
    A, B, rc, ax = capsule(h, 0, s, H)
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R - 0.03), -1.0 * u, mass=5.0)
    run(h, f"{robot} second overlap")
    assert h.hits[count - 1, 0] == 1
    o = run(h, f"{robot} second overlap, next step")
    assert h.hits[count - 1, 0] == 2 and o.hit_log[0]["shape"] == s


@pytest.mark.parametrize("robot,count", [(r, c) for r in ROBOTS for c in (2, 4)], ids=[f"{r.split('_')[0]}-{c}" for r in ROBOTS for c in (2, 4)])
def test_two_projectiles_on_one_body_add(robot, count):
    m, h = scene(robot, count, bystander=False)
    s = long_shape(m, h)
    only(h, s)
    A, B, rc, ax = capsule(h, 0, s, H)
    u = side_dir(ax)
    aim(h, 0, 0, A + 0.3 * (B - A) + u * (rc + R - 0.01), -5.0 * u, mass=2.0)
    aim(h, count - 1, 0, A + 0.7 * (B - A) - u * (rc + R - 0.01), 3.0 * u, mass=4.0)
    o = run(h, f"{robot} two projectiles")
    assert h.hits[0, 0] == 1 and h.hits[count - 1, 0] == 1 and len(o.hit_log) == 2
    each = [-hl["j"] * hl["n"] / o.dt for hl in o.hit_log]
    np.testing.assert_allclose(h.force[0, s], each[0] + each[1], atol=2 * pu.float_bounds(o, 12.0)[2])
    assert np.linalg.norm(each[0] + each[1]) < max(np.linalg.norm(e) for e in each), "opposite sides: the rows add, they do not overwrite"


@case
@pytest.mark.parametrize("kind", ["sticking", "sliding"])
def test_ground_bounce(robot, count, kind):
    m, h = scene(robot, count, friction=1.0)
    vt = 0.5 if kind == "sticking" else 5.0
    h.place(count - 1, 1, (3.0, -3.0, R + 0.002), (vt, 0.0, -1.0), 2.0)
    o = run(h, f"{robot} ground, {kind}")
    vz_in = -1.0 + G * H
    # (the bounce came in sub-interval 1: restitution on v.z, the Coulomb impulse mu (1 + e) |v.z| against v.x; then 7 sub-intervals of gravity and more bounces)
    first = max(vt - 1.0 * 1.2 * abs(vz_in), 0.0)
    assert (first == 0.0) == (kind == "sticking")
    assert abs(h.vel[count - 1, 1, 0]) <= first + 1e-6 and h.vel[count - 1, 1, 1] == 0 and h.pos[count - 1, 1, 2] >= R
    assert (h.vel[count - 1, 1, 0] == 0) == (kind == "sticking")
    assert h.hits.sum() == 0 and (h.force == 0).all()


@case
def test_expiry_parks_and_a_reset_in_mid_flight_zeroes_the_rows(robot, count):
    m, h = scene(robot, count, n=3)
    s = long_shape(m, h)
    only(h, s)
    A, B, rc, ax = capsule(h, 0, s, H)
    u = side_dir(ax)
    aim(h, count - 1, 0, 0.5 * (A + B) + u * (rc + R - 0.01), -5.0 * u)          # would hit -- but env 0 was reset
    h.place(count - 1, 1, (3.0, 3.0, 1.5), (0.0, 1.0, 0.0), 2.0, life=1)           # expires in this step
    h.force[:] = 7.0                                                               # (stale rows of an earlier step)
    h.torque[:] = 7.0
    k = int(h.k[0])
    o = run(h, f"{robot} expiry and reset", progress=np.array([0, 5, 5]))
    assert (h.force == 0).all() and (h.torque == 0).all() and h.hits.sum() == 0
    for env in (0, 1):
        u0 = pu.draws(h.args.key, env, 1, k, 1, count - 1)[0, 0, 0]
        pause = pu.shim().proj_pause_of(h.args, float(u0))
        assert 3 <= pause <= 6 and h.life[count - 1, env] == 0 and h.pos[count - 1, env, 2] == -1000.0
        assert h.countdown[count - 1, env] == (pause - 1 if env == 0 else pause)   # (a reset slot waits from this step on)
    assert (h.k == k + 1).all()


@case
def test_the_last_body_of_the_last_env(robot, count):
    m, h = scene(robot, count, n=3, bystander=False)
    s = m.num_bodies - 1
    only(h, s)
    A, B, rc, ax = capsule(h, 2, s, H)
    assert rc > 0
    u = side_dir(ax)
    aim(h, count - 1, 2, 0.5 * (A + B) + u * (rc + R - 0.01), -5.0 * u)
    run(h, f"{robot} last body of the last env")
    assert h.last_hit[count - 1, 2] == s and np.linalg.norm(h.force[2, s]) > 0 and (h.force[:2] == 0).all() and h.guards_intact()


# ---- throws ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_a_throw_passes_the_resting_target(robot):
    """Bodies at rest and out of the collision list: the thrown path passes the target's centre of mass at t_f = d / s within the sphere's radius (the flight is
    a first-order integration in sub-intervals of h; the start height clamp moves low throws)."""
    m = pu.model(robot)
    n = 64
    rbs = pu.posed_rbs(m, n, seed=2, vel=0.0, ang=0.0)
    caps = pu.tables(m)["capsules"].copy()
    caps[:, 6] = 0.0
    listed = (0, m.num_bodies // 2)
    h = pu.HostProj(m, n, rbs, capsules=caps, count=1, pause=(1, 1), life_steps=60, listed=listed)
    h.advance()                                   # k = 0: reset, countdown 1 -> 0
    h.advance()                                   # the throw, and its first env step of flight
    assert (h.thrown == 1).all() and (h.life == 59).all()
    o = pu.Oracle(h)
    u = pu.draws(h.args.key, 0, n, 1, 1, 0)[0].astype(np.float64)
    tf = (2.0 + 2.0 * u[:, 4]) / (5.0 + 5.0 * u[:, 3])
    body = np.asarray(listed)[np.minimum((u[:, 1] * 2).astype(int), 1)]
    com = rbs[np.arange(n), body, 0:3].astype(np.float64) + pu.quat_rot(rbs[np.arange(n), body, 3:7].astype(np.float64), o.tab["com"][body])
    closest = np.full(n, np.inf)
    t = DT
    for _ in range(40):
        before, tb = h.pos[0].astype(np.float64).copy(), t
        h.advance()
        t += DT
        now = h.pos[0].astype(np.float64)
        inside = (tb <= tf) & (tf < t)
        lam = ((tf - tb) / DT)[:, None]
        d = np.linalg.norm(before + lam * (now - before) - com, axis=-1)
        closest = np.where(inside, d, closest)
    print(f"{robot}: distance from the target's centre of mass at t_f: max {closest.max():.4f} m, mean {closest.mean():.4f} m")
    assert np.isfinite(closest).all() and closest.max() < R


def test_draws_are_uniform_and_independent():
    key = 0x9E3779B97F4A7C15
    u = np.stack([pu.draws(key, 0, 256, 0, 64, slot) for slot in range(4)])       # [slot, k, env, 8]
    flat = u.reshape(-1, 8)
    assert flat.min() >= 0.0 and flat.max() < 1.0
    for i in range(8):
        hist = np.bincount((flat[:, i] * 16).astype(int), minlength=16)
        expect = len(flat) / 16
        assert np.abs(hist - expect).max() < 6 * math.sqrt(expect), (i, hist)
    c = np.corrcoef(flat.T)
    assert np.abs(c - np.eye(8)).max() < 0.02, "the eight draws of a throw"
    for axis, name in ((0, "slots"), (1, "steps"), (2, "envs")):
        a, b = np.take(u, range(0, u.shape[axis] - 1), axis=axis).ravel(), np.take(u, range(1, u.shape[axis]), axis=axis).ravel()
        assert abs(np.corrcoef(a, b)[0, 1]) < 0.01, name
    np.testing.assert_array_equal(pu.draws(key, 100, 56, 3, 5, 2), u[2, 3:8, 100:156])   # env_offset: rank 1's envs continue rank 0's numbering
    assert not np.array_equal(pu.draws(key + 1, 0, 256, 0, 1, 0), u[0, :1])
    from phc_amd.perturb import stream_key
    from phc_amd.projectile import STREAM_TAG
    assert stream_key(3, STREAM_TAG) != stream_key(3) and stream_key(3, STREAM_TAG) != stream_key(4, STREAM_TAG)


# ---- the host side --------------------------------------------------------------------------------------------------------------------------------------------------
NAMES = ["Pelvis", "Torso", "Head"]
BAD_OPTIONS = [
    (dict(), "mass .* is required"), (dict(mass=[1, 5], colour="red"), "unknown projectile option"), (dict(mass=[5, 1]), "projectile.mass"),
    (dict(mass=0), "projectile.mass"), (dict(mass=1, speed=[0, 5]), "projectile.speed"), (dict(mass=1, distance=-1), "projectile.distance"),
    (dict(mass=1, elevation_deg=[0, 100]), "elevation_deg"), (dict(mass=1, radius=0), "radius"), (dict(mass=1, restitution=1.5), "restitution"),
    (dict(mass=1, count=5), "count"), (dict(mass=1, count=0), "count"), (dict(mass=1, substeps=0), "substeps"), (dict(mass=1, bodies=["Tail"]), "no such body"),
    (dict(mass=1, interval_s=[-1, 2]), "interval_s"), (dict(mass=1, life_s=0), "life_s"),
    (dict(mass=1, speed=[5, 25]), "tunnelling"), (dict(mass=1, radius=0.04), "tunnelling"), (dict(mass=1, substeps=4, speed=[5, 13]), "tunnelling"),
]


@pytest.mark.parametrize("cfg,match", BAD_OPTIONS, ids=[f"{i:02d}" for i in range(len(BAD_OPTIONS))])
def test_options_are_checked(cfg, match):
    from phc_amd.projectile import ProjectileOptions
    with pytest.raises(ValueError, match=match):
        ProjectileOptions(cfg, NAMES, DT)


def test_options_defaults_and_the_missing_device():
    from phc_amd.projectile import ProjectileOptions, ProjectileSchedule
    import torch
    o = ProjectileOptions(dict(mass=[1, 5]), NAMES, DT, default_seed=4)
    assert (o.radius, o.speed, o.distance, o.elevation_deg, o.count, o.substeps, o.restitution) == (0.1, (5.0, 10.0), (2.0, 4.0), (0.0, 30.0), 1, 8, 0.2)
    assert o.pause_steps == (60, 120) and o.life_steps == 60 and o.listed == [0] and o.seed == 4
    assert o.speed[1] * DT / o.substeps == pytest.approx(0.0417, abs=1e-3)      # the defaults: 0.042 m per sub-interval against 0.1 m
    assert ProjectileOptions(dict(mass=2, bodies="Head", interval_s=0.1, seed=9), NAMES, DT).listed == [2]
    m = pu.model("smpl_humanoid")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ProjectileSchedule(dict(mass=[1, 5]), 4, m, torch.zeros(4 * m.num_bodies, 13), DT, "cpu")
    with pytest.raises(ValueError, match="tunnelling"):                          # (the options are checked first)
        ProjectileSchedule(dict(mass=[1, 5], speed=[5, 30]), 4, m, torch.zeros(4 * m.num_bodies, 13), DT, "cpu")


PROJ = ["+projectile.mass=[1,5]"]
TASK_REFUSALS = [
    (PROJ + ["+perturb.force=[50,100]"], ValueError, r"\+perturb.\* together with \+projectile"),
    (["robot.has_shape_variation=True", "robot.has_shape_obs=True", "robot.has_shape_obs_disc=True", "robot.has_weight_obs=True"] + PROJ, NotImplementedError,
     "projectile: external wrenches .*has_shape_variation"),
    (["+solver.lane_mapping=3"] + PROJ, NotImplementedError, "projectile: external wrenches .*lane_mapping=3"),
    (["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control", "domain_rand=h1_dr"] + PROJ, NotImplementedError,
     r"domain_rand with \+projectile"),
    (PROJ + ["+projectile.speed=[5,30]"], ValueError, "tunnelling"),
    (PROJ + ["+projectile.shape=box"], ValueError, "unknown projectile option"),
]


@pytest.mark.parametrize("over,exc,match", TASK_REFUSALS, ids=[f"{i:02d}" for i in range(len(TASK_REFUSALS))])
def test_the_task_refuses_by_name(over, exc, match):
    from test_task_config_cpu import host_task
    with pytest.raises(exc, match=match):
        host_task(*over)


def test_the_task_takes_the_group_and_refuses_a_one_shot_wrench():
    from test_task_config_cpu import host_task
    t = host_task(*PROJ, "+projectile.bodies=[Pelvis,Torso,Head]")
    assert t._proj is None and t._push is None          # (the schedule is made with the task's buffers; the host phases checked its options)
    assert host_task()._proj is None
    t._proj, t._dr = object(), None
    with pytest.raises(ValueError, match="thrown projectiles"):
        t.apply_rigid_body_force_tensors(forces=None, torques=None)


def test_binding_types():
    from phc_amd import _lib as L
    assert "phc_proj_advance" in L._SIGNATURES and L._SIGNATURES["phc_proj_advance"] == ([C.POINTER(L.ProjArgs), C.c_void_p], C.c_int32)
    assert (L.PROJ_MAX_SLOTS, L.PROJ_MAX_SHAPES) == (4, 64)
    names = [f for f, _ in L.ProjArgs._fields_]
    assert names[:9] == ["num_envs", "num_bodies", "num_shapes", "num_listed", "count", "pause_lo", "pause_hi", "life_steps", "substeps"]
    assert L.ProjArgs.key.offset % 8 == 0 and L.ProjArgs.env_offset.offset == L.ProjArgs.key.offset + 8 and L.ProjArgs.bodies.offset == L.ProjArgs.key.offset + 16
    assert C.sizeof(L.ProjArgs) == L.ProjArgs.bodies.offset + 19 * 8
    import re
    header = open(os.path.join(host_build.ROOT, "include", "phc_amd.h")).read()
    body = header[header.index("#define PHC_PROJ_MAX_SLOTS"):header.index("} phc_proj_args_t;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    at = [re.search(rf"[\s*]{n}[,;]", body).start() for n in names]
    assert at == sorted(at), "the struct's fields in the binding's order"


BAD_ARGS = [("num_envs", -1), ("num_bodies", 0), ("num_bodies", 65), ("num_shapes", 65), ("num_shapes", 3), ("num_listed", 0), ("num_listed", 65), ("count", 0),
            ("count", 5), ("pause_lo", -1), ("pause_hi", 2), ("pause_hi", (1 << 24) + 1), ("life_steps", 0), ("substeps", 0), ("substeps", 65), ("dt", 0.0),
            ("dt", float("nan")), ("dt", float("inf")), ("gravity_z", 1.0), ("gravity_z", float("-inf")), ("radius", 0.0), ("radius", float("nan")),
            ("restitution", -0.1), ("restitution", 1.5), ("friction", -1.0), ("friction", float("inf")), ("mass_lo", 0.0), ("mass_hi", 0.5), ("mass_hi", float("inf")),
            ("speed_lo", 0.0), ("speed_hi", 1.0), ("dist_lo", -1.0), ("dist_hi", 1.0), ("elev_lo", -2.0), ("elev_hi", 2.0), ("elev_hi", -0.5), ("env_offset", -1),
            ("env_offset", (1 << 32) - 2)]
POINTERS = ["bodies", "capsules", "owner", "body_com", "body_inv_mass", "body_inv_inertia", "rigid_body_state", "life", "countdown", "thrown", "hits", "last_hit",
            "k", "pos", "vel", "mass", "force", "torque"]


def test_proj_args_check_refuses_every_bad_argument():
    m = pu.model("smpl_humanoid")
    h = pu.HostProj(m, 4, pu.posed_rbs(m, 4), count=2)
    check = pu.shim().proj_args_check_of
    assert check(h.args) == 0 and check(None) == -1
    for f, bad in BAD_ARGS:
        keep = getattr(h.args, f)
        setattr(h.args, f, bad)
        assert check(h.args) == -1, (f, bad)
        setattr(h.args, f, keep)
    for f in POINTERS:
        keep = getattr(h.args, f)
        setattr(h.args, f, None)
        assert check(h.args) == -1, f
        setattr(h.args, f, keep)
    h.args.progress_buf = None
    h.args.num_envs = 0
    assert check(h.args) == 0
    h.args.num_envs, h.args.env_offset = 4, (1 << 32) - 4
    assert check(h.args) == 0


def test_rows_snapshot_and_select_on_the_host():
    """phc_proj_rows' per-env code: the snapshot copies every row, the select takes the shadow's rows of the struck envs and writes nothing else; its checks."""
    from phc_amd import _lib as L
    n, count, widths = 5, 2, (13, 7, 1)
    base, shadow, last_hit, bufs = pu.rows_case(n, count, widths)
    mk = lambda mode: pu.rows_args([b.ctypes.data for b in base], [s.ctypes.data for s in shadow], widths, last_hit.ctypes.data, n, count, mode)
    want = [np.where(np.isin(np.arange(n), (1, n - 1))[:, None], s, b) for b, s in zip(base, shadow)]
    kept = [s.copy() for s in shadow]
    pu.shim().proj_rows_host(mk(L.PROJ_SELECT))
    for b, w, s, k in zip(base, want, shadow, kept):
        assert b.tobytes() == w.tobytes() and s.tobytes() == k.tobytes()
    pu.shim().proj_rows_host(mk(L.PROJ_SNAPSHOT))
    for b, s in zip(base, shadow):
        assert s.tobytes() == b.tobytes()
    assert all((x[-pu.PAD:] == pu.GUARD).all() for x in bufs)
    check = pu.shim().proj_rows_check_of
    assert check(mk(0)) == 0 and check(mk(1)) == 0 and check(None) == -1
    for f, bad in (("num_envs", -1), ("num_sets", 0), ("num_sets", 9), ("mode", 2), ("mode", -1), ("count", 0), ("count", 5), ("last_hit", None)):
        a = mk(L.PROJ_SELECT)
        setattr(a, f, bad)
        assert check(a) == -1, (f, bad)
    for f, bad in (("base", None), ("shadow", None), ("width", 0)):
        a = mk(L.PROJ_SNAPSHOT)
        getattr(a, f)[2] = bad
        assert check(a) == -1, f
    a = mk(L.PROJ_SNAPSHOT)
    a.last_hit, a.count = None, 0          # (the snapshot reads neither)
    assert check(a) == 0
    assert L._SIGNATURES["phc_proj_rows"] == ([C.POINTER(L.ProjRows), C.c_void_p], C.c_int32)
    assert C.sizeof(L.ProjRows) == 16 + 8 + 8 * 8 + 8 * 8 + 4 * 8


# ---- stand-alone sanitizer program ------------------------------------------------------------------------------------------------------------------------------
def test_stand_alone_sanitizer_program():
    """tests/proj_asan_main.cpp (its own main; nothing is loaded into Python): N = 65 envs and the corner cases on heap arrays of exact size, under
    AddressSanitizer and UndefinedBehaviorSanitizer."""
    returncode, stdout, stderr = host_build.run_sanitized("proj_asan_main.cpp")
    print(stdout[-2000:], stderr[-4000:])
    assert returncode == 0 and "proj_asan: ok" in stdout


# ---- random run ------------------------------------------------------------------------------------------------------------------------------------------------------
RUN = dict(n=70, steps=60, key=3, pause=(3, 6), life_steps=8, dist=(1.0, 2.0), speed=(8.0, 10.0))   # interval_s = [0.1, 0.2] at dt = 1/30


def random_run(robot="smpl_humanoid", count=1, on_start=None, on_step=None, **kw):
    """N = 70 posed bodies with small velocities, throws every 3 - 6 env steps from 1 - 2 m at 8 - 10 m/s, 8 env steps of life (a projectile that came to rest
    on the ground or on a limb decides by ever smaller margins: the short life keeps the run about impacts).  The host build against the free-running fp64
    oracle; an env whose decision margin (proj_util.Oracle) falls below 1e-5 is dropped from that step on.  `key` was chosen so that the oracle alone drops no
    env (seeds 1 - 12 drop 0 - 3 of 70; the cap of 2 % admits one).  -> (host, oracle, alive [N], worst floats)."""
    o_ = dict(RUN, **kw)
    m = pu.model(robot)
    listed = tuple(m.body_names.index(b) for b in (("Pelvis", "Torso", "Head") if robot == "smpl_humanoid" else ("pelvis", "torso_link", "left_shoulder_pitch_link")))
    rbs = pu.posed_rbs(m, o_["n"], seed=1, vel=0.3, ang=0.5)
    h = pu.HostProj(m, o_["n"], rbs, count=count, pause=o_["pause"], life_steps=o_["life_steps"], dist=o_["dist"], speed=o_["speed"], listed=listed, key=o_["key"],
                    env_offset=o_.get("env_offset", 0))
    o = pu.Oracle(h)
    if on_start is not None:
        on_start(h, o)
    alive, worst = np.ones(o_["n"], dtype=bool), np.zeros(4)
    rng = np.random.default_rng(7)
    for step in range(o_["steps"]):
        progress = None if step % 7 == 6 else np.where(rng.random(o_["n"]) < 0.02, 0, 5).astype(np.int64)   # (a few resets; None: the nullable pointer)
        h.advance(progress)
        o.step(progress)
        alive &= ~(o.margin < 1e-5)
        for name in pu.INT_NAMES + ("k",):
            np.testing.assert_array_equal(getattr(h, name)[..., alive], getattr(o, name)[..., alive], err_msg=f"step {step}: {name}")
        age = int((o.life_steps - o.life)[o.life > 0].max(initial=0)) + 1
        bounds = pu.float_bounds(o, 12.0, K=64 * age)
        fly = (o.life > 0) & alive[None]
        w = [np.abs(h.pos - o.pos)[fly].max(initial=0.0), np.abs(h.vel - o.vel)[fly].max(initial=0.0), np.abs(h.force - o.force)[alive].max(initial=0.0),
             np.abs(h.torque - o.torque)[alive].max(initial=0.0)]
        for x, b, name in zip(w, bounds, ("pos", "vel", "force", "torque")):
            assert x <= b, f"step {step}: {name} differs by {x:.3e}, bound {b:.3e}"
        worst = np.maximum(worst, w)
        assert h.guards_intact()
        if on_step is not None:
            on_step(step, h, progress, alive)
    return h, o, alive, worst


def test_random_run_under_the_cap():
    h, o, alive, worst = random_run()
    dropped = int((~alive).sum())
    print(f"random run: {int(o.thrown.sum())} thrown, {int(o.hits.sum())} hits, {dropped} of 70 envs dropped; worst |host build - fp64| pos {worst[0]:.2e} m, "
          f"vel {worst[1]:.2e} m/s, force {worst[2]:.2e} N, torque {worst[3]:.2e} N m")
    assert dropped <= 0.02 * 70, "the dropped share may not exceed 2 %"
    assert o.hits.sum() >= 70, "at least one hit per env on average"
    assert (h.k == 60).all()
