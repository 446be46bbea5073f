// phc_proj.h -- thrown projectiles (phc_proj_advance, csrc/phc_proj.hip; contract: include/phc_amd.h): the draws of a throw, the ballistic flight of a
// sphere in sub-intervals of the env step, its bounce on the ground plane, the collision test against the model's capsules and the impulse of a hit,
// handed to the stepper as a force and a torque on the struck body (phc_sim_step_wrench).  PHC_HD: tests/proj_shim.cpp builds all of it for the CPU.
//
// One function, proj_env, is the whole env step of one env.  It is written over a lane group `Grp`: member `lane`, constant PER (shapes and body rows a
// lane owns: index lane + i, i < PER), `argmin` (the group's least (gap, index) pair, into every lane), `bcast` (a value of the lane that owns a
// shape, into every lane) and `any` (is the flag set in any lane of the WAVEFRONT).  The kernel's group has G lanes with PER = 1; the host build's has one lane that owns everything, so both run the same
// arithmetic in the same order and differ by the elementary functions of the throw (sinf, cosf) alone.  Everything that is not per shape or per row
// (draws, slot state, the projectile's motion, the impulse) is computed redundantly by every lane of the group from the same inputs.
#pragma once
#include <math.h>
#include "phc_rng.h"
#include "../../include/phc_amd.h"

namespace phc {

#define PHC_PROJ_DRAWS 8   // per (env, k, slot): pause, body, mass, speed, distance, azimuth, elevation, spare
#define PHC_PROJ_PARK_Z (-1000.0f)

PHC_HD void proj_draws(uint64_t key, uint32_t global_env, uint32_t k, int slot, float u[PHC_PROJ_DRAWS]) {
    const uint64_t base = ((uint64_t)k * PHC_PROJ_MAX_SLOTS + (uint64_t)slot) * PHC_PROJ_DRAWS;
#pragma unroll
    for (int i = 0; i < PHC_PROJ_DRAWS; ++i) u[i] = hash_u01(splitmix64(key ^ ((base + (uint64_t)i) * 0x9E6C63D0876A9A47ull)), global_env);
}

// whole env steps from [pause_lo, pause_hi], like push_pause (phc_push.h)
PHC_HD int proj_pause(const phc_proj_args_t& a, float u0) {
    const int span = a.pause_hi - a.pause_lo;
    const int d = (int)floorf(u0 * (float)(span + 1));
    return a.pause_lo + (d < span ? d : span);
}

PHC_HD V3 proj_ld3(const float* p) { return v3(p[0], p[1], p[2]); }
PHC_HD float proj_lerp(float lo, float hi, float u) { return lo + u * (hi - lo); }

// A body's row of rigid_body_state (pos3, xyzw quaternion, linear velocity of the body's origin, angular velocity; env axes).
struct ProjBody { V3 x, v, w; Q4 q; };
PHC_HD ProjBody proj_body(const phc_proj_args_t& a, int64_t env, int b) {
    const float* s = a.rigid_body_state + (env * a.num_bodies + b) * 13;
    ProjBody r;
    r.x = proj_ld3(s); r.q = q4(s[3], s[4], s[5], s[6]); r.v = proj_ld3(s + 7); r.w = proj_ld3(s + 10);
    return r;
}

// A collision capsule posed at the start of the env step: its endpoints and their velocities v_b + w x (a - x_b).
struct ProjShape { V3 a, b, va, vb; float rc; int owner; };
PHC_HD ProjShape proj_pose_shape(const phc_proj_args_t& a, int64_t env, int s) {
    ProjShape sh;
    if (s >= a.num_shapes) { sh.a = sh.b = sh.va = sh.vb = v3(0.f, 0.f, 0.f); sh.rc = 0.f; sh.owner = 0; return sh; }   // (a lane without a shape: never a candidate)
    const float* c = a.capsules + s * 7;
    sh.owner = a.owner[s];
    sh.rc = c[6];
    const ProjBody B = proj_body(a, env, sh.owner);
    const V3 ra = quat_rotate(B.q, proj_ld3(c)), rb = quat_rotate(B.q, proj_ld3(c + 3));
    sh.a = B.x + ra; sh.b = B.x + rb;
    sh.va = B.v + cross(B.w, ra); sh.vb = B.v + cross(B.w, rb);
    return sh;
}

// The test of one shape at time t behind the start of the step: gap, and whether the sphere at x with velocity v is a candidate (gap < 0 and approaching).
// n: unit vector from the segment's closest point c to the sphere's centre (z^ where they coincide); cp: the contact point c + rc n on the capsule's
// surface; vn: (v - v_point) . n with v_point the velocity of the material point at c.
struct ProjTest { float gap, vn; V3 n, cp; };
PHC_HD bool proj_test_shape(const ProjShape& sh, V3 x, V3 v, float t, float radius, ProjTest& o) {
    const V3 A = sh.a + sh.va * t, B = sh.b + sh.vb * t;
    const V3 ab = B - A;
    const float l2 = dot(ab, ab);
    float s = l2 > 0.f ? dot(x - A, ab) / l2 : 0.f;
    s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
    const V3 c = A + ab * s;
    const V3 d = x - c;
    const float dist = sqrtf(dot(d, d));
    o.n = dist > 0.f ? d * (1.0f / dist) : v3(0.f, 0.f, 1.f);
    o.gap = dist - radius - sh.rc;
    const V3 vp = sh.va + (sh.vb - sh.va) * s;
    o.vn = dot(v - vp, o.n);
    o.cp = c + o.n * sh.rc;
    return sh.rc > 0.f && o.gap < 0.f && o.vn < 0.f;
}

// The impulse of a hit on body `b` at contact point cp (time t behind the start of the step) along n, the struck link taken as a free body:
// j = -(1 + e) vn / (1/m + 1/m_b + n . ((I_w^-1 (r x n)) x r)), r from the link's centre of mass to cp.  The centre of mass is advanced at first order
// like the capsule; I_w^-1 = R I_b^-1 R^T with the rotation at the start of the step.  Returns j; r_out = r.
PHC_HD float proj_impulse(const phc_proj_args_t& a, int64_t env, int b, V3 n, V3 cp, float vn, float t, float m, V3& r_out) {
    const ProjBody B = proj_body(a, env, b);
    const V3 rc = quat_rotate(B.q, proj_ld3(a.body_com + b * 3));
    const V3 com = (B.x + rc) + (B.v + cross(B.w, rc)) * t;
    const V3 r = cp - com;
    const V3 rxn = cross(r, n);
    const V3 l = quat_rotate(quat_conjugate(B.q), rxn);
    const float* I = a.body_inv_inertia + b * 9;
    const V3 Il = v3(I[0] * l.x + I[1] * l.y + I[2] * l.z, I[3] * l.x + I[4] * l.y + I[5] * l.z, I[6] * l.x + I[7] * l.y + I[8] * l.z);
    const V3 Iw = quat_rotate(B.q, Il);
    const float denom = 1.0f / m + a.body_inv_mass[b] + dot(n, cross(Iw, r));
    r_out = r;
    return -(1.0f + a.restitution) * vn / denom;
}

// The throw: target body, mass, start point x0 at distance d from the target's centre of mass x_t (azimuth uniform, elevation from its range), and the
// velocity v0 whose ballistic path meets x_t + v_t t_f at t_f = d / s.
PHC_HD void proj_throw(const phc_proj_args_t& a, int64_t env, const float u[PHC_PROJ_DRAWS], V3& x0, V3& v0, float& m) {
    const int j = (int)floorf(u[1] * (float)a.num_listed);
    const int b = a.bodies[j < a.num_listed - 1 ? j : a.num_listed - 1];
    m = proj_lerp(a.mass_lo, a.mass_hi, u[2]);
    const float s = proj_lerp(a.speed_lo, a.speed_hi, u[3]);
    const float d = proj_lerp(a.dist_lo, a.dist_hi, u[4]);
    const float az = u[5] * 6.283185307179586f;
    const float el = proj_lerp(a.elev_lo, a.elev_hi, u[6]);
    const ProjBody B = proj_body(a, env, b);
    const V3 rc = quat_rotate(B.q, proj_ld3(a.body_com + b * 3));
    const V3 xt = B.x + rc, vt = B.v + cross(B.w, rc);
    const float tf = d / s;
    const float ce = cosf(el);
    x0 = xt + v3(ce * cosf(az), ce * sinf(az), sinf(el)) * d;
    const float zmin = a.radius + 0.01f;
    if (x0.z < zmin) x0.z = zmin;
    v0 = ((xt + vt * tf) - x0) * (1.0f / tf);
    v0.z = v0.z - 0.5f * a.gravity_z * tf;
}

// Host builds only: the least decision margin of an env step -- of the tests whose flip alone would change a decision: |gap| (m) of a shape the sphere
// approaches (vn < 0), |vn| (m/s) of a shape it overlaps (gap < 0); on the ground |x.z - radius| while v.z < 0 and |v.z| while x.z < radius.
PHC_HD void proj_margin(float* margin, float v) { const float x = fabsf(v); if (x < *margin) *margin = x; }

// One env step of env `env` (see the head of this file).  `live` is false for the lanes of a group behind the last env: they run along on env
// num_envs - 1 so that the group operations see every lane, and store nothing.  margin: nullptr on the device.
template <class Grp>
PHC_HD void proj_env(const phc_proj_args_t& a, int64_t env, bool live, const Grp& g, float* margin) {
    const int64_t N = a.num_envs;
    const uint32_t k = (uint32_t)a.k[env];
    const bool reset = k == 0u || (a.progress_buf != nullptr && a.progress_buf[env] == 0);
    const float h = a.dt / (float)a.substeps;
    ProjShape sh[Grp::PER];
    V3 F[Grp::PER], T[Grp::PER];
#pragma unroll
    for (int i = 0; i < Grp::PER; ++i) {
        sh[i] = proj_pose_shape(a, env, g.lane + i);
        F[i] = T[i] = v3(0.f, 0.f, 0.f);
    }
    for (int p = 0; p < a.count; ++p) {
        const int64_t at = (int64_t)p * N + env;
        int life = a.life[at], countdown = a.countdown[at], thrown = a.thrown[at], hits = a.hits[at], last_hit = -1;
        V3 x = proj_ld3(a.pos + at * 3), v = proj_ld3(a.vel + at * 3);
        float m = a.mass[at];
        float u[PHC_PROJ_DRAWS];
        proj_draws(a.key, (uint32_t)(a.env_offset + env), k, p, u);
        const int pause = proj_pause(a, u[0]);
        if (reset) { life = 0; countdown = pause; x = v3(x.x, x.y, PHC_PROJ_PARK_Z); v = v3(0.f, 0.f, 0.f); }
        if (life == 0) {
            if (countdown > 0) countdown -= 1;
            else { proj_throw(a, env, u, x, v, m); life = a.life_steps; thrown += 1; }
        }
        const bool fly = life > 0;
        bool struck = false;
        // (every group of a wavefront runs the sub-intervals when any of its groups has a slot in flight, predicated by `fly`: the branch is uniform over the
        // wavefront, so the group operations below never see a lane switched off; a wavefront of parked slots skips them)
        const int nsub = g.any(fly) ? a.substeps : 0;
        for (int i = 0; i < nsub; ++i) {
            const float t = (float)(i + 1) * h;
            if (fly) {
                v.z = v.z + a.gravity_z * h;
                x = x + v * h;
                if (margin) { if (v.z < 0.f) proj_margin(margin, x.z - a.radius); if (x.z < a.radius) proj_margin(margin, v.z); }
                if (x.z < a.radius && v.z < 0.f) {   // ground: normal impulse with restitution, Coulomb impulse against the tangential velocity
                    const float jn = (1.0f + a.restitution) * -v.z;
                    const float vt = sqrtf(v.x * v.x + v.y * v.y);
                    const float lim = a.friction * jn;
                    const float dv = lim < vt ? lim : vt;
                    if (vt > 0.f) { const float sc = dv / vt; v.x = v.x - v.x * sc; v.y = v.y - v.y * sc; }
                    v.z = -a.restitution * v.z;
                    x.z = a.radius;
                }
            }
            float best = INFINITY;   // the deepest candidate of this lane's shapes; a tie keeps the lowest index
            int win = 0x7fffffff, slot = 0;
            ProjTest bt;
            bt.gap = bt.vn = 0.f; bt.n = bt.cp = v3(0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < Grp::PER; ++q) {
                ProjTest o;
                const bool cand = proj_test_shape(sh[q], x, v, t, a.radius, o);
                if (margin && fly && !struck && sh[q].rc > 0.f) { if (o.vn < 0.f) proj_margin(margin, o.gap); if (o.gap < 0.f) proj_margin(margin, o.vn); }
                if (cand && fly && !struck && o.gap < best) { best = o.gap; win = g.lane + q; slot = q; bt = o; }
            }
            g.argmin(best, win);
            const bool hit = win != 0x7fffffff;
            const int src = hit ? win : 0;
            const V3 n = v3(g.bcast(bt.n.x, src), g.bcast(bt.n.y, src), g.bcast(bt.n.z, src));
            const V3 cp = v3(g.bcast(bt.cp.x, src), g.bcast(bt.cp.y, src), g.bcast(bt.cp.z, src));
            const float vn = g.bcast(bt.vn, src);
            const int owner = g.bcast_i(sh[slot].owner, src);
            if (hit) {
                V3 r;
                const float j = proj_impulse(a, env, owner, n, cp, vn, t, m, r);
                v = v + n * (j / m);
                const V3 f = n * (-j / a.dt);
                const V3 tq = cross(r, f);
#pragma unroll
                for (int q = 0; q < Grp::PER; ++q)
                    if (g.lane + q == owner) { F[q] += f; T[q] += tq; }
                hits += 1; last_hit = win; struck = true;
            }
        }
        if (fly) {
            life -= 1;
            if (life == 0) { countdown = pause; x = v3(x.x, x.y, PHC_PROJ_PARK_Z); v = v3(0.f, 0.f, 0.f); }
        }
        if (live && g.lane == 0) {
            a.life[at] = life; a.countdown[at] = countdown; a.thrown[at] = thrown; a.hits[at] = hits; a.last_hit[at] = last_hit;
            a.pos[at * 3 + 0] = x.x; a.pos[at * 3 + 1] = x.y; a.pos[at * 3 + 2] = x.z;
            a.vel[at * 3 + 0] = v.x; a.vel[at * 3 + 1] = v.y; a.vel[at * 3 + 2] = v.z;
            a.mass[at] = m;
        }
    }
    if (live) {
#pragma unroll
        for (int q = 0; q < Grp::PER; ++q) {
            const int b = g.lane + q;
            if (b < a.num_bodies) {   // every row of the env, once: zero where nothing struck (also at a reset: a parked projectile strikes nothing)
                float* f = a.force + (env * a.num_bodies + b) * 3;
                float* tq = a.torque + (env * a.num_bodies + b) * 3;
                f[0] = F[q].x; f[1] = F[q].y; f[2] = F[q].z;
                tq[0] = T[q].x; tq[1] = T[q].y; tq[2] = T[q].z;
            }
        }
        if (g.lane == 0) a.k[env] = (int32_t)(k + 1u);
    }
}

// The group of the host build: one lane that owns every shape and every row.
struct ProjHostGroup {
    static constexpr int PER = PHC_PROJ_MAX_SHAPES;
    int lane = 0;
    void argmin(float&, int&) const {}
    bool any(bool v) const { return v; }
    float bcast(float v, int) const { return v; }
    int bcast_i(int v, int) const { return v; }
};

// The argument checks of phc_proj_advance (include/phc_amd.h lists them): 0 or PHC_EINVAL.
inline int32_t proj_args_check(const phc_proj_args_t* a) {
    if (!a || !a->bodies || !a->capsules || !a->owner || !a->body_com || !a->body_inv_mass || !a->body_inv_inertia || !a->rigid_body_state) return PHC_EINVAL;
    if (!a->life || !a->countdown || !a->thrown || !a->hits || !a->last_hit || !a->k || !a->pos || !a->vel || !a->mass || !a->force || !a->torque) return PHC_EINVAL;
    if (a->num_envs < 0 || a->num_bodies < 1 || a->num_bodies > PHC_MAX_BODIES || a->num_shapes < 1 || a->num_shapes > PHC_PROJ_MAX_SHAPES) return PHC_EINVAL;
    if (a->num_shapes < a->num_bodies || a->num_listed < 1 || a->num_listed > PHC_MAX_BODIES || a->count < 1 || a->count > PHC_PROJ_MAX_SLOTS) return PHC_EINVAL;
    if (a->pause_lo < 0 || a->pause_hi < a->pause_lo || a->pause_hi > (1 << 24) || a->life_steps < 1 || a->life_steps > (1 << 24)) return PHC_EINVAL;
    if (a->substeps < 1 || a->substeps > 64) return PHC_EINVAL;
    if (!(a->dt > 0.f && a->dt < INFINITY) || !(a->gravity_z <= 0.f && a->gravity_z > -INFINITY) || !(a->radius > 0.f && a->radius < INFINITY)) return PHC_EINVAL;
    if (!(a->restitution >= 0.f && a->restitution <= 1.f) || !(a->friction >= 0.f && a->friction < INFINITY)) return PHC_EINVAL;
    if (!(a->mass_lo > 0.f && a->mass_hi >= a->mass_lo && a->mass_hi < INFINITY) || !(a->speed_lo > 0.f && a->speed_hi >= a->speed_lo && a->speed_hi < INFINITY)) return PHC_EINVAL;
    if (!(a->dist_lo > 0.f && a->dist_hi >= a->dist_lo && a->dist_hi < INFINITY)) return PHC_EINVAL;
    if (!(a->elev_lo >= -1.5707964f && a->elev_hi >= a->elev_lo && a->elev_hi <= 1.5707964f)) return PHC_EINVAL;
    if (a->env_offset < 0 || a->env_offset + (int64_t)a->num_envs > (int64_t)1 << 32) return PHC_EINVAL;
    return 0;
}

// One env's rows of phc_proj_rows (the kernel's block strides over the columns from `first` by `stride`; the host build takes 0, 1).
PHC_HD void proj_rows_env(const phc_proj_rows_t& a, int64_t env, int first, int stride) {
    bool take = a.mode == PHC_PROJ_SNAPSHOT;
    if (!take)
        for (int p = 0; p < a.count; ++p) take = take || a.last_hit[(int64_t)p * a.num_envs + env] >= 0;
    if (!take) return;
    for (int s = 0; s < a.num_sets; ++s) {
        const int w = a.width[s];
        const float* src = (a.mode == PHC_PROJ_SNAPSHOT ? a.base[s] : a.shadow[s]) + env * w;
        float* dst = (a.mode == PHC_PROJ_SNAPSHOT ? a.shadow[s] : a.base[s]) + env * w;
        for (int i = first; i < w; i += stride) dst[i] = src[i];
    }
}

inline int32_t proj_rows_check(const phc_proj_rows_t* a) {
    if (!a || a->num_envs < 0 || a->num_sets < 1 || a->num_sets > PHC_PROJ_MAX_ROWSETS) return PHC_EINVAL;
    if (a->mode != PHC_PROJ_SNAPSHOT && a->mode != PHC_PROJ_SELECT) return PHC_EINVAL;
    if (a->mode == PHC_PROJ_SELECT && (!a->last_hit || a->count < 1 || a->count > PHC_PROJ_MAX_SLOTS)) return PHC_EINVAL;
    for (int s = 0; s < a->num_sets; ++s)
        if (!a->base[s] || !a->shadow[s] || a->width[s] < 1) return PHC_EINVAL;
    return 0;
}

}  // namespace phc
