"""TEST INFRASTRUCTURE ONLY -- the stepper's articulated-body recursion in plain numpy, fp64, with the LAGGED scheme (`inertia_lag`).

oracle/dyn_oracle.py states one sub-step as a dense solve M nu_dot = rhs; the lagged scheme has no such form (it mixes quantities of two instants), so its only
numeric reference used to be the lane code of csrc/phc_aba.h compiled at double precision -- the same expressions on both sides of every comparison.  This module states
the recursion independently: 6 x 6 spatial matrices and 6-vectors in WORLD axes, ordered [angular; linear], about each body's solver reference point
o_i = p_i + R_i s_off_i (model.solver_tree(): the origin, or for a REVERSED body of a re-rooted tree the anchor of the joint towards its solver parent).  It compiles
nothing and includes no project header; force laws, drives, limits, integration, rate cap and the published outputs are dyn_oracle's own functions.

One FRESH sub-step (every sub-step with inertia_lag 0; sub-step s with s % substeps == 0 otherwise), leaves to base:
    I^A_i  = rigid-body inertia about o_i + sum over children X^T I^a X + sum over pushing ground points dt J^T C J     (C = diag(c_t, c_t, c_n), J = [-[a]x 1])
    p^A_i  = velocity-product force - gravity - external wrench - body-body wrench - sum J^T (F0 - dt C w x (w x a)) + sum over children X^T p^a
    joint towards the solver parent, world axes S_w (3 x n: R axis, or R for a spherical joint), joint-space diagonal d, torque tau:
    D = S_w^T A S_w + diag(d)  (A = the angular block of I^A),   P = S_w D^-1 S_w^T,   U = I^A [1; 0]  (its first three columns),   u = S_w tau - p^A_top
    I^a = I^A - U P U^T,        p^a = p^A + I^a c + U P u,        c = [w_par x (w_i - w_par); w_par x (w_par x r)],  r = o_i - o_par
    X = [[1, 0], [-[r]x, 1]]  carries the parent's acceleration (alpha, a of its reference point) to o_i.
base: I^A [alpha; a] = -p^A;  base to leaves: a' = X acc_par + c,  beta = P (u - U^T a'),  acc_i = a' + [beta; 0];  joint acceleration S_w^T beta (with the opposite
sign when the joint is solved from its other side by a reversed body).

A LAGGED sub-step is the same code path with two substitutions, both kept as world-axes matrices from the last fresh sub-step of the simulate() call: I^A_j and
P_j (for a revolute joint the rank-1 a a^T / D of THAT sub-step's axis).  Everything else is current: levers, rotations, velocity products, bias force, gravity, drive
torque, body-body forces, external wrench.  I^a is formed from the kept matrices and p^a by the fresh expression above (the lane code's bias-only rearrangement
p^A + I^A c + U P (u - U^T c) is algebraically equal; it is NOT transcribed: that equality is what the tests check).

The rules that go with the substitution (comments of csrc/phc_aba.h aba_body_init):
  * a ground point contributes its explicit force F0 only if it PUSHED in the last fresh sub-step (the kept I^A holds its impedance; the kept set covers the first
    64 points of a body) AND still pushes now (penetrating, fn0 > 0).  F0 is evaluated at the current state -- current depth, velocity, friction regime -- while the
    kept impedance is the old one;
  * a point that arrives later carries nothing until the next fresh sub-step; a point that left keeps its impedance in the kept I^A and loses its F0;
  * a revolute joint limit whose engagement is not in the kept P acts as a spring WITHOUT its damper (no implicit share either); one that is in the kept P and is
    still engaged acts in full; one that released contributes no torque (its implicit share stays in the kept P);
  * the joint-space diagonal (`Dw`, `dimp`) is that of the fresh sub-step -- it is inside the kept P, and it is what S5 (dof_force = tau - (d - armature) qdd) uses;
  * `tau_hold` of control modes 1 / 2 is resampled at fresh sub-steps only (they are the first sub-steps of the simulate() calls).

Only tests import this file."""
import numpy as np

import dyn_oracle as do


def _sym_about(model, i, R, so_i):
    """Rigid-body inertia of body i about its reference point, world axes: (Io 3x3, mc = m (com - ref) 3, m)."""
    m = float(model.mass[i])
    c = R @ model.com[i]
    Ic = R @ model.inertia_origin[i] @ R.T - m * ((c @ c) * np.eye(3) - np.outer(c, c))   # about the centre of mass
    r = c - so_i
    return Ic + m * ((r @ r) * np.eye(3) - np.outer(r, r)), m * r, m


def _spatial_inertia(Io, mc, m):
    M = np.zeros((6, 6))
    M[:3, :3] = Io
    M[:3, 3:] = do.skew(mc)
    M[3:, :3] = -do.skew(mc)
    M[3:, 3:] = m * np.eye(3)
    return M


def _shift(r):
    """X: the acceleration [alpha; a] of a body's reference point -> that of the point r away on the same body."""
    X = np.eye(6)
    X[3:, :3] = -do.skew(r)
    return X


def substep(model, st, target, prm, dt, kp_scale=1.0, kd_scale=1.0, tau_hold=None, kept=None, lagged=False, force=None, torque=None, rec=None):
    """One sub-step on `st` (a dyn_oracle.State).  `kept`: the dict a fresh sub-step fills and a lagged one reads.  Returns (applied joint torques, contact forces)."""
    tree = model.solver_tree()
    nb = model.num_bodies
    spar, slev, jsrc = tree["sparent"], tree["slevel"], tree["jsrc"]
    Q, R, p = do.kinematics(model, st)
    w, v = do.body_velocities(model, st, R, p)
    so = np.array([R[i] @ tree["s_off"][i] for i in range(nb)])
    o = p + so
    g = np.array([0.0, 0.0, prm["gravity_z"]])
    IA = np.zeros((nb, 6, 6))
    pA = np.zeros((nb, 6))
    fcontact = np.zeros((nb, 3))
    if rec is not None:
        rec.update(lagged=bool(lagged), contacts=[], limits=[])
    if not lagged:
        kept.clear()
        kept.update(touch=set(), limit={}, d={}, IA={}, P={})
    Fs = Ns = None
    if prm["self_collision"]:
        Fs, Ns = do.self_collision_wrenches(model, R, p, w, v, prm, dt)
    for i in range(nb):
        Io, mc, m = _sym_about(model, i, R[i], so[i])
        IA[i] = _spatial_inertia(Io, mc, m)
        pA[i, :3] = do.cross3(w[i], Io @ w[i]) - do.cross3(mc, g)
        pA[i, 3:] = do.cross3(w[i], do.cross3(w[i], mc)) - m * g
        if force is not None:      # external force at the centre of mass
            pA[i, 3:] -= force[i]
            pA[i, :3] -= do.cross3(mc / m, force[i])
        if torque is not None:
            pA[i, :3] -= torque[i]
        for ordinal, k in enumerate(np.nonzero(model.contact_body == i)[0]):
            arm0 = R[i] @ model.contact_pos[k]
            rad = model.contact_radius[k]
            in_kept = (int(k) in kept["touch"]) if lagged else None
            r_ = None
            if rec is not None:
                r_ = dict(point=int(k), body=int(i), depth=float(rad - (p[i][2] + arm0[2])), fn0=None, kept=in_kept, pushed=False, active=False)
                rec["contacts"].append(r_)
            pt = do.penalty_point(prm, dt, p[i], w[i], v[i], arm0, rad, r_)
            if pt is None or (lagged and not in_kept):
                continue
            arm, uc, fn0, ct, cn = pt
            if r_ is not None:
                r_["pushed"] = True
            Cm = np.diag([ct, ct, cn])
            F0 = np.array([-ct * uc[0], -ct * uc[1], fn0])
            fcontact[i] += F0 - dt * Cm @ do.cross3(w[i], do.cross3(w[i], arm))
            a = arm - so[i]
            J = np.concatenate([-do.skew(a), np.eye(3)], axis=1)
            pA[i] -= J.T @ (F0 - dt * Cm @ do.cross3(w[i], do.cross3(w[i], a)))
            if not lagged:
                IA[i] += dt * J.T @ Cm @ J
                if ordinal < 64:
                    kept["touch"].add(int(k))
        if Fs is not None:
            fcontact[i] += Fs[i]
            pA[i, 3:] -= Fs[i]
            pA[i, :3] -= Ns[i] - do.cross3(so[i], Fs[i])
    # joint drives, in joint coordinates (body j's own joint)
    tau_all, d_all = [None] * nb, [None] * nb
    lo_hi = model.dof_limits() if not model.all_spherical else None
    for j in range(1, nb):
        held = (not lagged) or kept["limit"].get(j, False)
        tau, d, e = do.joint_drive(model, st, j, target, prm, dt, kp_scale, kd_scale, tau_hold, None, limit_damper=held)
        if not lagged:
            kept["limit"][j] = e != 0.0
            kept["d"][j] = d
        tau_all[j], d_all[j] = tau, kept["d"][j]
        if rec is not None and lo_hi is not None and prm["limit_stiffness"] > 0:
            s = int(model.dof_start[j])
            th = float(st.theta[j - 1])
            rec["limits"].append(dict(dof=s, body=j, e=float(e), kept=bool(kept["limit"][j]), below=float(lo_hi[0][s] - th), above=float(th - lo_hi[1][s])))
    # backward sweep
    order = sorted(range(nb), key=lambda i: -int(slev[i]))
    Sw, P, U, u, c, X = {}, {}, {}, {}, {}, {}
    base = int(tree["base"])
    for i in order:
        if lagged:
            IA[i] = kept["IA"][i]
        else:
            kept["IA"][i] = IA[i].copy()
        if i == base:
            continue
        par = int(spar[i])
        js = int(jsrc[i])
        sign = 1.0 if js == i else -1.0   # (a reversed body sees its solver parent's joint from the other side)
        Sw[i] = R[js] @ st.S(js - 1)
        if lagged:
            P[i] = kept["P"][i]
        else:
            D = Sw[i].T @ IA[i][:3, :3] @ Sw[i] + np.diag(d_all[js])
            P[i] = Sw[i] @ np.linalg.inv(D) @ Sw[i].T
            kept["P"][i] = P[i].copy()
        U[i] = IA[i][:, :3]
        u[i] = sign * (Sw[i] @ tau_all[js]) - pA[i][:3]
        r = o[i] - o[par]
        c[i] = np.concatenate([do.cross3(w[par], w[i] - w[par]), do.cross3(w[par], do.cross3(w[par], r))])
        X[i] = _shift(r)
        Ia = IA[i] - U[i] @ P[i] @ U[i].T
        pa = pA[i] + Ia @ c[i] + U[i] @ (P[i] @ u[i])
        if not lagged:
            IA[par] += X[i].T @ Ia @ X[i]
        pA[par] += X[i].T @ pa
    # base, forward sweep
    acc = np.zeros((nb, 6))
    acc[base] = np.linalg.solve(IA[base], -pA[base])
    offs = np.concatenate([[6], 6 + np.cumsum(st.nd)]).astype(int)
    nud = np.zeros(int(offs[-1]))
    for i in reversed(order):
        if i == base:
            continue
        a1 = X[i] @ acc[int(spar[i])] + c[i]
        beta = P[i] @ (u[i] - U[i].T @ a1)
        acc[i] = a1
        acc[i, :3] += beta
        js = int(jsrc[i])
        nud[offs[js - 1]:offs[js]] = (1.0 if js == i else -1.0) * (Sw[i].T @ beta)
    d0 = -so[0]   # the simulator root's origin from its reference point
    nud[0:3] = acc[0, :3]
    nud[3:6] = acc[0, 3:] + do.cross3(acc[0, :3], d0) + do.cross3(w[0], do.cross3(w[0], d0))
    parts = dict(offs=offs, tau=tau_all, dimp=d_all, fcontact=fcontact)
    return do.integrate(model, st, nud, parts, prm, dt, rec)


def sim_step(model, root_states, dof_state, pd_target, params=None, sim_dt=1 / 60, substeps=2, num_sim_calls=2, inertia_lag=0, force=None, torque=None, trace=None,
             kp_scale=1.0, kd_scale=1.0, wrench_sim_calls=None):
    """dyn_oracle.sim_step by the recursion above; `inertia_lag` 1: sub-step s is lagged when s % substeps != 0.  `force` / `torque` [NB, 3]: external wrench (force at
    the centres of mass), world axes, over the first `wrench_sim_calls` simulate calls (None: all).  Same return values as dyn_oracle.sim_step.

    `trace` (a dict): trace["substeps"][s] = dict(lagged, contacts = [per ground point: point, body, depth, fn0 (None above the plane), kept (in the kept set; None in a
    fresh sub-step), pushed, friction / cone_ratio where it applies], limits = [per revolute DoF: dof, body, e (the limit error), kept (the kept P holds the limit),
    below / above (signed distance past the lower / upper limit)], rate_ratio).  Recording changes no number."""
    prm = dict(do.DEFAULT_PARAMS, **(params or {}))
    assert prm["contact_model"] == 0, "the rigid contact model is never lagged"
    st = do.State(root_states, dof_state, model)
    dt = sim_dt / substeps
    tau = np.zeros(model.num_dof)
    fc = np.zeros((model.num_bodies, 3))
    explicit = prm["control_mode"] in (1, 2)
    hold, kept = None, {}
    nw = num_sim_calls if wrench_sim_calls is None else wrench_sim_calls
    for k in range(num_sim_calls * substeps):
        if explicit and k % substeps == 0:
            hold = do.explicit_torque(model, st, pd_target, kp_scale, kd_scale)
        on = k // substeps < nw
        rec = None if trace is None else {}
        tau, fc = substep(model, st, pd_target, prm, dt, kp_scale, kd_scale, hold, kept, bool(inertia_lag) and k % substeps != 0,
                          None if force is None or not on else np.asarray(force, np.float64), None if torque is None or not on else np.asarray(torque, np.float64), rec)
        if trace is not None:
            trace.setdefault("substeps", []).append(rec)
    Q, R, p = do.kinematics(model, st)
    w, v = do.body_velocities(model, st, R, p)
    return st.root_states(), st.dof_state(), np.concatenate([p, np.array(Q), v, w], axis=-1), tau, fc
