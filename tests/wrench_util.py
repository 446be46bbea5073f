"""TEST INFRASTRUCTURE for the external-wrench tests (tests/test_ext_wrench_cpu.py, tests/test_ext_wrench_gpu.py): runs the host statement of phc_sim_step_wrench
-- oracle/hostemu's emu_sim_step_wrench -- at single and at double precision, and holds the cases (states and wrenches) both test files use.

Forces stay at or below 300 N and torques at or below 50 N m, so that body speeds stay at a few m/s and the fp32 recursion stays inside the tolerances the
stepper is held to everywhere else (tests/test_dynamics.py::check_step_against: positions 3e-4, velocities 3e-3 / rtol 1e-3; rigid contact 5e-4 and 1e-2)."""
import numpy as np

import dyn_oracle as do
import hostemu_util as hu
from phc_amd import abi

F = np.float32


def load(name):
    """ArticulationModel as the stepper tests set it up (tests/backends.py model_on)."""
    from backends import get_backend, model_on
    return model_on(get_backend("hostemu"), name=name)[0]


def params(**kw):
    return abi.sim_params_struct(**kw)


def host_step(model, prm, root, dof, target, num_sim_calls=2, force=None, torque=None, wrench_sim_calls=0, f64=False, gravity_z=None, reference=False):
    """One launch on the host.  `reference`: through oracle/hostemu's emu_sim_step (no wrench) instead of its emu_sim_step_wrench.  `gravity_z` (fp64 only):
    overrides the parameter struct's value at full double precision.  -> dict(root, dof, rbs, cf, df) of arrays of the build's precision."""
    return hu.host_sim_step(model, prm, root, dof, target, num_sim_calls, f64=f64, force=force, torque=torque,
                            wrench_sim_calls=None if reference else wrench_sim_calls, gravity_z=gravity_z)


def body_mass(model, f64=True):
    """The masses the build computes with (float table entry 3 of every body)."""
    _, floats = model.pack(1.0, 1.0, float_dtype=np.float64 if f64 else F)
    return np.asarray(floats).reshape(-1)[:model.num_bodies * 56].reshape(model.num_bodies, 56)[:, 3].astype(np.float64)


# ---- states -------------------------------------------------------------------------------------------------------------------------------------------------
def smpl_state(model, n, where, seed=0):
    """`ground`: upright, the lowest contact point 4 mm inside the plane, small pose and joint rates; `air`: 3 m up, moving and turning."""
    rng = np.random.default_rng(seed)
    nd = model.num_dof
    root = np.zeros((n, 13), F)
    root[:, 6] = 1.0
    dof = np.zeros((n, nd, 2), F)
    dof[:, :, 0] = rng.normal(0, 0.08, (n, nd))
    dof[:, :, 1] = rng.normal(0, 0.3, (n, nd))
    target = (dof[:, :, 0] + rng.normal(0, 0.1, (n, nd))).astype(F)
    if where == "ground":
        for e in range(n):
            st = do.State(root[e].astype(np.float64), dof[e].astype(np.float64), model)
            Q, R, p = do.kinematics(model, st)
            low = min(p[i][2] + (R[i] @ model.contact_pos[k])[2] - model.contact_radius[k] for k, i in enumerate(model.contact_body))
            root[e, 2] = -low - 0.004
        root[:, 7:10] = rng.normal(0, 0.05, (n, 3))
    else:
        root[:, 2] = 3.0
        q = rng.normal(0, 1, (n, 4)) * np.array([0.2, 0.2, 0.5, 0]) + np.array([0, 0, 0, 1.0])
        root[:, 3:7] = q / np.linalg.norm(q, axis=-1, keepdims=True)
        root[:, 7:10] = rng.normal(0, 0.5, (n, 3))
        root[:, 10:13] = rng.normal(0, 0.5, (n, 3))
    return root, dof, target


def robot_rest_state(model, n, height):
    """A robot at rest in the air, joint angles at zero clipped into the limits, PD targets at the pose."""
    nd = model.num_dof
    lo, hi = model.dof_limits()
    root = np.zeros((n, 13), F)
    root[:, 2] = height
    root[:, 6] = 1.0
    dof = np.zeros((n, nd, 2), F)
    dof[:, :, 0] = np.clip(0.0, lo + 0.05, hi - 0.05)
    return root, dof, dof[:, :, 0].copy()


def world_frames(model, root, dof):
    """fp64 rotation matrices and origins of the bodies of one env."""
    Q, R, p = do.kinematics(model, do.State(np.asarray(root, np.float64), np.asarray(dof, np.float64), model))
    return np.array(R), np.array(p)


# ---- wrenches of the cases ----------------------------------------------------------------------------------------------------------------------------------
DELTA_G = 3.0   # m/s^2: the heaviest SMPL body then carries < 60 N


def gravity_wrench(model, n, f64=True):
    """F_i = m_i (0, 0, DELTA_G) on every body of every env."""
    f = np.zeros((n, model.num_bodies, 3))
    f[:, :, 2] = body_mass(model, f64)[None] * DELTA_G
    return f


COUPLE_JOINTS = {"h1_humanoid": ("left_hip_pitch_link", "torso_link", "right_elbow_link")}


def couple_case(model, root, dof, target, body, dtau):
    """External torque +dtau a on `body` and -dtau a on its parent (a: the joint's world axis at the pose of env 0) <-> the PD target of the joint raised by dtau / kp."""
    j = model.body_names.index(body)
    d = int(model.dof_start[j])
    R, _ = world_frames(model, root[0], dof[0])
    a = R[j] @ model.dof_axis[d]
    n = root.shape[0]
    torque = np.zeros((n, model.num_bodies, 3))
    torque[:, j] = dtau * a
    torque[:, model.parent[j]] = -dtau * a
    tgt = np.array(target, dtype=np.float64)
    tgt[:, d] += dtau / float(model.dof_kp[d])
    return torque, tgt


def yaw_case(model, n):
    """SMPL on the ground, a horizontal force on the pelvis and a torque on the torso (per env different), and the same scene turned by 90 degrees about z."""
    root, dof, target = smpl_state(model, n, "ground", seed=4)
    nb = model.num_bodies
    force, torque = np.zeros((n, nb, 3)), np.zeros((n, nb, 3))
    for e in range(n):
        force[e, 0] = (150.0 + 40.0 * e, -90.0 + 30.0 * e, 0.0)
        torque[e, model.body_names.index("Torso")] = (20.0, -15.0 + 5.0 * e, 30.0)
    return root, dof, target, force, torque


def yaw90_vec(v):
    v = np.asarray(v)
    out = v.copy()
    out[..., 0], out[..., 1] = -v[..., 1], v[..., 0]
    return out


def yaw90_quat(q):
    """(0, 0, sin 45, cos 45) * q, quaternions xyzw."""
    q = np.asarray(q, np.float64)
    s = np.sqrt(0.5)
    x, y, z, w = (q[..., k] for k in range(4))
    return np.stack([s * x - s * y, s * y + s * x, s * w + s * z, s * w - s * z], -1)


def yaw90_state(a):
    """Root states [.., 13] or body states [.., 13] (position, quaternion, velocity, angular velocity) turned by 90 degrees about z."""
    a = np.asarray(a, np.float64)
    return np.concatenate([yaw90_vec(a[..., 0:3]), yaw90_quat(a[..., 3:7]), yaw90_vec(a[..., 7:10]), yaw90_vec(a[..., 10:13])], -1)


def quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# ---- comparisons --------------------------------------------------------------------------------------------------------------------------------------------
def _quat_close(a, b, tol):
    d = np.abs((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum(-1))
    assert np.all(np.abs(d - 1) < tol), f"rotations differ: 1 - |<a, b>| up to {np.abs(d - 1).max():.2e}"


def assert_exact(out, ref, tag=""):
    """fp64 against fp64: 1e-9 on root, dof and body state."""
    for k in ("root", "dof", "rbs"):
        np.testing.assert_allclose(out[k], ref[k], atol=1e-9, rtol=0, err_msg=f"{k} {tag}")


def assert_standing(out, ref, rigid=False, tag=""):
    """fp32 against fp64 at the tolerances the fp32 stepper is held to (see the module docstring)."""
    pa, va = (5e-4, 1e-2) if rigid else (3e-4, 3e-3)
    o = {k: np.asarray(out[k], np.float64) for k in ("root", "dof", "rbs")}
    np.testing.assert_allclose(o["root"][..., 0:3], ref["root"][..., 0:3], atol=pa, err_msg=f"root position {tag}")
    _quat_close(o["root"][..., 3:7], ref["root"][..., 3:7], 1e-5)
    np.testing.assert_allclose(o["root"][..., 7:13], ref["root"][..., 7:13], atol=va, rtol=1e-3, err_msg=f"root velocity {tag}")
    np.testing.assert_allclose(o["dof"][..., 0], ref["dof"][..., 0], atol=pa, err_msg=f"dof position {tag}")
    np.testing.assert_allclose(o["dof"][..., 1], ref["dof"][..., 1], atol=va, rtol=1e-3, err_msg=f"dof velocity {tag}")
    np.testing.assert_allclose(o["rbs"][..., 0:3], ref["rbs"][..., 0:3], atol=pa, err_msg=f"body position {tag}")
    _quat_close(o["rbs"][..., 3:7], ref["rbs"][..., 3:7], 1e-5)
    np.testing.assert_allclose(o["rbs"][..., 7:13], ref["rbs"][..., 7:13], atol=va, rtol=1e-3, err_msg=f"body velocity {tag}")


def report(name, out, ref):
    """Worst differences of a comparison, printed before it asserts."""
    o = {k: np.asarray(out[k], np.float64) for k in ("root", "dof", "rbs")}
    print(f"{name}: body pos {np.abs(o['rbs'][..., 0:3] - ref['rbs'][..., 0:3]).max():.2e}  body vel {np.abs(o['rbs'][..., 7:13] - ref['rbs'][..., 7:13]).max():.2e}  "
          f"dof pos {np.abs(o['dof'][..., 0] - ref['dof'][..., 0]).max():.2e}  dof vel {np.abs(o['dof'][..., 1] - ref['dof'][..., 1]).max():.2e}")
