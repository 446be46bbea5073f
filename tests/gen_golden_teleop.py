"""TEST INFRASTRUCTURE -- golden for phc_teleop_rewards: HumanoidTeleop's regularisation rewards from the reference's OWN code.

Run where the reference checkout is (oracle/ref_shim.py finds it):  python tests/gen_golden_teleop.py   -> tests/golden/teleop_rewards.npz

The reference's module imports the simulator, open3d and a filter module the shim cannot supply, so nothing of it is imported: the `_reward_*` methods,
`_prepare_reward_function`, the summing loop of `_compute_reward` (humanoid_teleop.py:242-246) and the two `last_*` assignments of `post_physics_step`
(:159-160) are cut out of the file's AST and executed on a stand-in `self`, the way oracle/gen_golden_torques.py cuts the gains statement out.
`quat_rotate_inverse` is the reference's (phc/utils/isaacgym_torch_utils.py through the shim).

Two blocks -- H1's sizes and G1's (DoFs, bodies, the ankle links as feet, joint and torque limits of the shipped models) -- of 16 envs and THREE consecutive
steps of seeded inputs, so that the air-time / last-contact state machine runs.  Recorded: the inputs, the initial state, and per step the terms' raw values,
their columns, the summed reward and the state afterwards.  Every term is zero in some env and non-zero in another; every threshold (1 N, the 5 : 1 ratio,
max_contact_force, 0.25 s air time, 0.1 m/s reference speed, both joint-limit sides, the torque limit) is crossed in both directions, and no compared quantity
lies within 1e-3 (relative) of its threshold -- asserted below -- so that no flag can flip on rounding.  (A foot without any contact force compares 0 > 0 in
the stumble test: exact in every arithmetic, exempt.)  The file holds arrays and names only."""
import ast
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import ref_shim  # noqa: E402

ref_shim.install()
OUT = os.path.join(ROOT, "tests", "golden", "teleop_rewards.npz")
F = np.float32
N, STEPS, DT, MARGIN = 16, 3, 0.02, 1e-3
# column order on purpose not the order of the term bits
SPECS = {"k_pos": 100, "r_feet_ori": -1.0, "r_torques": -1e-5, "r_dof_pos_limits": -10.0, "r_feet_air_time_teleop": 10.0, "r_torque_limits": -5.0,
         "r_dof_vel": -1e-3, "r_stumble": -2.0, "r_dof_acc": -2.5e-7, "r_action_rate": -0.01, "r_slippage": -1.0, "r_feet_contact_forces": -0.01,
         "max_contact_force": 200.0}
BLOCKS = {"h1": ["robot=unitree_h1", "env=env_im_h1_phc", "sim=robot_sim", "control=robot_control"],
          "g1": ["robot=unitree_g1", "env=env_im_g1_phc", "sim=robot_sim", "control=robot_control"]}
# foot force patterns (x, y, z) in newtons: none | below 1 N | |F| > 1 with F_z < 1 | light contact | ordinary | above max_contact_force | stumbling
PATTERNS = np.array([[0, 0, 0], [0.3, 0, 0.5], [0.9, 0.2, 0.9], [0, 0, 2.0], [1, -1, 100], [10, 5, 300], [30, 0, 4], [-3, 4, 1.5], [0.5, 0.5, 250]], dtype=F)


class Specs(dict):
    """cfg.env.reward_specs: a dict with attribute access."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def reference_code():
    path = ref_shim.data_path(os.path.join("phc", "env", "tasks", "humanoid_teleop.py"))
    tree = ast.parse(open(path).read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "HumanoidTeleop")
    fns = {n.name: n for n in cls.body if isinstance(n, ast.FunctionDef)}
    methods = [fns[n] for n in fns if n.startswith("_reward_")] + [fns["_prepare_reward_function"]]
    loop = next(n for n in fns["_compute_reward"].body if isinstance(n, ast.For) and "reward_functions" in ast.unparse(n))
    last = [n for n in fns["post_physics_step"].body if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) in ("self.last_actions[:]", "self.last_dof_vel[:]")]
    assert len(last) == 2
    comp = lambda body, what: compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), f"<humanoid_teleop.py: {what}>", "exec")
    return comp(methods, "reward methods"), comp([loop], "summing loop"), comp(last, "last_* assignments"), [f.name for f in methods]


def sizes(tag):
    from phc_amd.config import compose
    from phc_amd.env.tasks.humanoid_im import HumanoidIm
    t = HumanoidIm.host_only(compose(BLOCKS[tag] + ["env.num_envs=4", "env.motion_file=armswing:4"]))
    lo, hi = (x.astype(F) for x in t.model.dof_limits())
    feet = [t._body_names.index(b) for b in t.cfg["env"]["contact_bodies"]]
    return t.num_dof, t.num_bodies, feet, lo, hi, t.model.dof_effort.astype(F)


def inputs(rng, D, NB, feet, lo, hi, effort):
    nf = len(feet)
    x = {}
    u = rng.uniform(0.05, 0.95, (STEPS, N, D))
    q = lo + u * (hi - lo)
    out_lo, out_hi = rng.random((STEPS, N, D)) < 0.08, rng.random((STEPS, N, D)) < 0.08
    out_lo[:, :N // 2], out_hi[:, :N // 2] = False, False          # the first half stays inside the limits
    q = np.where(out_lo, lo - rng.uniform(0.05, 0.3, q.shape), np.where(out_hi, hi + rng.uniform(0.05, 0.3, q.shape), q))
    x["dof_pos"] = q.astype(F)
    x["dof_vel"] = (rng.standard_normal((STEPS, N, D)) * 3.0).astype(F)
    tau = effort * rng.uniform(-0.9, 0.9, (STEPS, N, D))
    over = rng.random((STEPS, N, D)) < 0.1
    over[:, ::2] = False                                           # every other env stays below the torque limits
    x["torques"] = np.where(over, np.sign(tau) * effort * rng.uniform(1.05, 1.5, tau.shape), tau).astype(F)
    x["actions"] = rng.standard_normal((STEPS, N, D)).astype(F)
    cf = np.zeros((STEPS, N, NB, 3), dtype=F)
    cf[:, :, :3] = rng.standard_normal(cf[:, :, :3].shape) * 50   # (bodies that are no feet must not matter; the rest stays 0 to keep the file small)
    cf[:, :, feet] = PATTERNS[rng.integers(0, len(PATTERNS), (STEPS, N, nf))]
    x["contact_forces"] = cf
    some = sorted(set(feet) | {0, 1})                               # the feet and two more bodies move; the others rest at the identity
    x["body_vel"] = np.zeros((STEPS, N, NB, 3), dtype=F)
    x["body_vel"][:, :, some] = rng.standard_normal((STEPS, N, len(some), 3))
    rot = rng.standard_normal((STEPS, N, len(some), 4))
    x["body_rot"] = np.zeros((STEPS, N, NB, 4), dtype=F)
    x["body_rot"][..., 3] = 1
    x["body_rot"][:, :, some] = rot / np.linalg.norm(rot, axis=-1, keepdims=True)
    speed = np.where(rng.random((STEPS, N)) < 0.5, rng.uniform(0.0, 0.08, (STEPS, N)), rng.uniform(0.15, 1.5, (STEPS, N)))
    ang = rng.uniform(0, 2 * np.pi, (STEPS, N))
    x["ref_root_vel"] = np.stack([speed * np.cos(ang), speed * np.sin(ang), rng.standard_normal((STEPS, N))], axis=-1).astype(F)
    # env 0 is quiet: every term is zero there
    for k in ("dof_vel", "torques", "actions"):
        x[k][:, 0] = 0
    x["dof_pos"][:, 0] = (0.5 * (lo + hi)).astype(F)
    x["contact_forces"][:, 0][:, feet] = 0
    x["body_rot"][:, 0] = np.array([0, 0, 0, 1], dtype=F)
    x["rew_in"] = rng.uniform(0.2, 1.0, (STEPS, N)).astype(F)
    x["reward_im"] = rng.uniform(0.0, 1.0, (STEPS, N, 5)).astype(F)
    air0 = rng.choice(np.array([0.0, 0.1, 0.22, 0.24, 0.3, 0.5], dtype=F), (N, nf))
    air0[0] = 0
    x["feet_air_time0"] = air0.astype(F)
    lc0 = rng.random((N, nf)) < 0.5
    lc0[0] = False
    x["last_contacts0"] = lc0
    return x


def far(a, b, what, exempt_zero=False):
    """No a within MARGIN (relative) of its threshold b."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    near = np.abs(a - b) <= MARGIN * np.maximum(np.abs(a), np.abs(b))
    if exempt_zero:
        near &= ~((a == 0) & (b == 0))
    assert not near.any(), f"{what}: {int(near.sum())} compared values within {MARGIN} of the threshold"
    return a > b


def check_margins(x, feet, lo, hi, effort, air_before):
    Ff = x["contact_forces"][:, :, feet].astype(np.float64)
    crossed = {"1 N (norm)": far(np.linalg.norm(Ff, axis=-1), 1.0, "|F| vs 1 N"), "1 N (z)": far(Ff[..., 2], 1.0, "F_z vs 1 N"),
               "5:1": far(np.linalg.norm(Ff[..., :2], axis=-1), 5 * np.abs(Ff[..., 2]), "5 : 1 ratio", exempt_zero=True),
               "max_contact_force": far(np.linalg.norm(Ff, axis=-1), SPECS["max_contact_force"], "|F| vs max_contact_force"),
               "air time 0.25": far(air_before.astype(np.float64) + DT, 0.25, "air time vs 0.25 s"),
               "air time 0": far(air_before, 0.0, "air time vs 0", exempt_zero=True),
               "ref speed": far(np.linalg.norm(x["ref_root_vel"][..., :2].astype(np.float64), axis=-1), 0.1, "reference speed vs 0.1 m/s"),
               "lower limit": far(lo, x["dof_pos"], "q vs lower limit"), "upper limit": far(x["dof_pos"], hi, "q vs upper limit"),
               "torque limit": far(np.abs(x["torques"]), effort, "|tau| vs limit")}
    for name, c in crossed.items():
        assert c.any() and (~c).any(), f"threshold {name} is not crossed in both directions"


def main():
    methods, loop, last, names = reference_code()
    itu = ref_shim.ref_module("phc.utils.isaacgym_torch_utils")
    space = {"torch": torch, "np": np, "copy": copy, "quat_rotate_inverse": itu.quat_rotate_inverse}
    exec(methods, space)
    out = {"dt": np.array(DT, F), "spec_names": np.array(list(SPECS)), "spec_values": np.array(list(SPECS.values()), np.float64),
           "reference_methods": np.array(names)}
    rng = np.random.default_rng(289)
    for tag in BLOCKS:
        D, NB, feet, lo, hi, effort = sizes(tag)
        x = inputs(rng, D, NB, feet, lo, hi, effort)
        nf = len(feet)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        me = types.SimpleNamespace()
        for n in names:
            setattr(me, n, types.MethodType(space[n], me))
        me.reward_specs, me.dt = Specs(SPECS), DT
        me._prepare_reward_function()
        raw_log = []
        me.reward_functions = [(lambda f: (lambda: raw_log.append(f().clone().float()) or raw_log[-1]))(f) for f in me.reward_functions]
        me.dof_pos_limits, me.torque_limits = tt(np.stack([lo, hi], -1)), tt(effort)
        me.feet_indices = torch.tensor(feet, dtype=torch.long)
        me.gravity_vec = torch.tensor([[0.0, 0.0, -1.0]]).repeat(N, 1)
        me.last_actions, me.last_dof_vel = torch.zeros(N, D), torch.zeros(N, D)
        me.feet_air_time, me.last_contacts = tt(x["feet_air_time0"]).clone(), tt(x["last_contacts0"]).clone()
        rec = {k: [] for k in ("raw", "columns", "rew_out", "reward_raw", "last_actions", "last_dof_vel", "feet_air_time", "last_contacts", "air_before")}
        for s in range(STEPS):
            me._dof_pos, me._dof_vel, me.torques, me.actions = tt(x["dof_pos"][s]), tt(x["dof_vel"][s]), tt(x["torques"][s]), tt(x["actions"][s])
            me._contact_forces, me._rigid_body_vel, me._rigid_body_rot = tt(x["contact_forces"][s]), tt(x["body_vel"][s]), tt(x["body_rot"][s])
            me.ref_body_vel = torch.zeros(N, NB, 3)
            me.ref_body_vel[:, 0] = tt(x["ref_root_vel"][s])
            me.rew_buf, me.reward_raw = tt(x["rew_in"][s]).clone(), tt(x["reward_im"][s]).clone()
            rec["air_before"].append(me.feet_air_time.numpy().copy())
            raw_log.clear()
            exec(loop, space, {"self": me})
            exec(last, space, {"self": me})
            rec["raw"].append(torch.stack(raw_log, -1).numpy().copy())
            rec["columns"].append(me.reward_raw[:, 5:].numpy().copy())
            rec["rew_out"].append(me.rew_buf.numpy().copy())
            rec["reward_raw"].append(me.reward_raw.numpy().copy())
            for k in ("last_actions", "last_dof_vel", "feet_air_time", "last_contacts"):
                rec[k].append(getattr(me, k).numpy().copy())
        check_margins(x, feet, lo, hi, effort, np.stack(rec["air_before"]))
        raw = np.stack(rec["raw"])
        for i, name in enumerate(me.reward_names):
            v = raw[..., i]
            assert (v != 0).any() and (v == 0).any(), f"{tag}: {name} must be zero in some env and non-zero in another"
        out.update({f"{tag}/{k}": v for k, v in x.items()})
        out.update({f"{tag}/{k}": np.stack(v) for k, v in rec.items() if k != "air_before"})
        out.update({f"{tag}/feet": np.array(feet, np.int32), f"{tag}/limits_lower": lo, f"{tag}/limits_upper": hi, f"{tag}/torque_limits": effort,
                    f"{tag}/reward_names": np.array(me.reward_names), f"{tag}/reward_scales": np.array([me.reward_scales[n] for n in me.reward_names], np.float64)})
        print(tag, "D", D, "NB", NB, "feet", feet, "names", me.reward_names)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
