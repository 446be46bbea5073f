// TEST INFRASTRUCTURE ONLY (built by tests/test_ext_wrench_cpu.py / tests/test_ext_wrench_gpu.py with g++, never loaded by the product).
// The host statement of phc_sim_step_wrench: the phase sequence of oracle/hostemu/hostemu.cpp's emu_sim_step_t -- the very per-lane functions k_sim_step is made
// of -- with the external wrench handed to aba_body_init the way the kernel's WRENCH instantiations hand it over.  oracle/ is a yardstick and stays as it is; this
// driver lives with the tests that need it.
// -DWRENCH_SHIM_F64: every float a double (the preamble of oracle/hostemu/hostemu64.cpp): the exact-arithmetic reference of the same recursion.  The C structs of
// include/phc_amd.h change layout with it; oracle/hostemu_util.py's `*64` mirrors describe them.
#include <math.h>
#include <cmath>
#include <stdint.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include <algorithm>
#ifdef WRENCH_SHIM_F64
#define float double
#define sqrtf sqrt
#define fminf fmin
#define fmaxf fmax
#define expf exp
#define sinf sin
#define cosf cos
#define atan2f atan2
#define acosf acos
#define fabsf fabs
#define rintf rint
#define log1pf log1p
#define logf log
#define floorf floor
#endif
#include "../phc_amd/csrc/phc_aba.h"

using namespace phc;

template <int JT>
static int wrench_sim_step_t(const phc_model_t* model_all, const phc_sim_params_t* prm, const phc_sim_state_t* sim, const float* actions,
                             const float* pd_off, const float* pd_scale, const int32_t* freeze, int num_sim_calls,
                             const float* ext_force, const float* ext_torque, int wrench_nsub) {
    const int nb = model_all->num_bodies, nd = model_all->num_dof;
    const int ndj = JT == PHC_JT_REVOLUTE ? 1 : 3;
    for (int64_t env = 0; env < sim->num_envs; ++env) {
        std::vector<float> xch(PHC_MAX_BODIES * PHC_XCH_STRIDE);
        const phc_model_t model_env = model_for_env(*model_all, *sim, env);
        const phc_model_t* model = &model_env;
        std::vector<AbaLane> L(PHC_MAX_BODIES);
        for (int j = 0; j < PHC_MAX_BODIES; ++j) L[j].level = L[j].slevel = -1;
        for (int j = 0; j < nb; ++j) {
            aba_load_model(L[j], *model, j);
            if (JT == PHC_JT_REVOLUTE) aba_load_model_rev(L[j], *model, j);
            if (actions && j >= 1) {
                for (int k = 0; k < ndj; ++k) {
                    const int d = L[j].dof_start + k;
                    volatile float prod = pd_scale[d] * actions[env * nd + d];
                    float t = pd_off[d] + prod;
                    if (freeze && freeze[d]) t = 0.f;
                    sim->pd_target[env * nd + d] = t;
                }
            }
            aba_load_state<JT>(L[j], *sim, nd, env, j);
        }
        Xch x;
        x.base = xch.data();
        for (int j = 0; j < nb; ++j) aba_fk_jump_begin(L[j], j, x);
        for (int k = 0, ks = model_jump_steps(*model); k < ks; ++k) {
            for (int j = 0; j < nb; ++j) aba_fk_jump_step(L[j], k, x);
            for (int j = 0; j < nb; ++j) aba_write_kin(L[j], xslot(x, j), Xch::es, 6);
        }
        const float dt = prm->sim_dt / (float)prm->substeps;
        const int nsub = num_sim_calls * prm->substeps;
        std::vector<float> caps(PHC_MAX_BODIES * PHC_CAP_STRIDE);
        float favg[PHC_MAX_BODIES * 6];
        const int sd = model_solver_depth(*model, true);
        const bool rerooted = model_tab(*model, 11, 3) != 0;
        for (int s = 0; s < nsub; ++s) {
            if (prm->self_collision) {
                for (int j = 0; j < nb; ++j) aba_publish_shape(L[j], j, x, caps.data());
                for (int e = 0, nx = model_num_extra_shapes(*model); e < nx; ++e) {
                    AbaLane X;
                    aba_load_extra_shape(X, *model, e);
                    aba_publish_shape(X, nb + e, x, caps.data());
                }
                for (int q = 0, np = model_num_pairs(*model); q < np; ++q)
                    aba_collide_pair(*prm, dt, model_pair(*model, q) & 0xff, model_pair(*model, q) >> 8, x, caps.data());
                for (int j = 0; j < nb; ++j) aba_collect_self(L[j], j, caps.data());
            }
            for (int j = 0; j < nb; ++j) aba_velocity_products(L[j], *model, j, x, true);
            const bool rigid = prm->contact_model == 1;
            const int passes = rigid ? (prm->contact_iterations < 1 ? 1 : prm->contact_iterations) : 1;
            const bool lag = !rigid && prm->inertia_lag != 0 && (s % prm->substeps) != 0;
            const bool ext_on = s < wrench_nsub;   // the wrench of this sub-step, as the kernel reads it: the body's own entry of each tensor
            for (int pass = 0; pass < passes; ++pass) {
                for (int j = 0; j < nb; ++j) {
                    V3 F = v3(0.f, 0.f, 0.f), T = v3(0.f, 0.f, 0.f);
                    if (ext_on && ext_force) { const float* p = ext_force + (env * nb + j) * 3; F = v3(p[0], p[1], p[2]); }
                    if (ext_on && ext_torque) { const float* p = ext_torque + (env * nb + j) * 3; T = v3(p[0], p[1], p[2]); }
                    if (rigid) aba_body_init<JT, true>(L[j], *model, *prm, dt, j, s % prm->substeps == 0, true, pass, false, ext_on, F, T);
                    else aba_body_init<JT, false>(L[j], *model, *prm, dt, j, s % prm->substeps == 0, true, 0, lag, ext_on, F, T);
                }
                if (JT == PHC_JT_SPHERICAL && rerooted && pass == 0) {
                    for (int j = 0; j < nb; ++j) aba_publish_drive(L[j], j, x);
                    for (int j = 0; j < nb; ++j) aba_fetch_drive(L[j], j, x);
                }
                for (int l = sd; l >= 0; --l) for (int j = 0; j < nb; ++j) aba_backward_level<JT>(L[j], l, j, x, lag);
                for (int l = 0; l <= sd; ++l) for (int j = 0; j < nb; ++j) aba_accel_level<JT>(L[j], l, j, x);
            }
            if (rigid && (s == nsub - 1 || prm->force_average)) for (int j = 0; j < nb; ++j) aba_publish_contact_rigid(L[j], *model, *prm, *sim, dt, env, j, true);
            if (JT == PHC_JT_SPHERICAL && rerooted) for (int j = 0; j < nb; ++j) aba_accel_finish(L[j], *model, j, x);
            for (int j = 0; j < nb; ++j) aba_integrate_joint<JT>(L[j], *prm, dt);
            if (prm->force_average) for (int j = 0; j < nb; ++j) aba_force_accumulate(L[j], s, nsub, favg + 6 * j);
            for (int j = 0; j < nb; ++j) aba_fk_jump_begin(L[j], j, x);
            for (int k = 0, ks = model_jump_steps(*model); k < ks; ++k) {
                for (int j = 0; j < nb; ++j) aba_fk_jump_step(L[j], k, x);
                for (int j = 0; j < nb; ++j) aba_write_kin(L[j], xslot(x, j), Xch::es, 6);
            }
        }
        for (int j = 0; j < nb; ++j) {
            aba_store_state<JT>(L[j], *sim, nd, env, j);
            aba_publish_body(L[j], *sim, nb, env, j, true);
            if (prm->contact_model != 1) aba_publish_sensors(L[j], *model, *prm, *sim, prm->sim_dt / (float)prm->substeps, env, j);
        }
    }
    return 0;
}

extern "C" int wrench_sim_step(const phc_model_t* model, const phc_sim_params_t* prm, const phc_sim_state_t* sim, const float* actions, const float* pd_off,
                               const float* pd_scale, const int32_t* freeze, int num_sim_calls, const float* ext_force, const float* ext_torque,
                               int wrench_sim_calls) {
    const int calls = wrench_sim_calls < 0 ? 0 : (wrench_sim_calls > num_sim_calls ? num_sim_calls : wrench_sim_calls);
    const bool on = (ext_force || ext_torque) && calls > 0;
    // the refusals of phc_sim_step_wrench / phc_sim_step (phc_sim.hip), mirrored
    if (on && (model->num_shapes > 1 || prm->lane_mapping == 3)) return PHC_EUNSUPPORTED;
    if (prm->contact_model == 1 && prm->inertia_lag) return PHC_EUNSUPPORTED;
    if (prm->inertia_lag && prm->lane_mapping == 3) return PHC_EUNSUPPORTED;
    if (prm->contact_model == 1 && model->max_body_contact_pts > 32) return PHC_EUNSUPPORTED;
    if (prm->inertia_lag && model->max_body_contact_pts > PHC_CP_BITS) return PHC_EUNSUPPORTED;
    const int nsub = on ? calls * prm->substeps : 0;
    if (model->num_dof == model->num_bodies - 1 && model->num_bodies > 2)
        return wrench_sim_step_t<PHC_JT_REVOLUTE>(model, prm, sim, actions, pd_off, pd_scale, freeze, num_sim_calls, ext_force, ext_torque, nsub);
    return wrench_sim_step_t<PHC_JT_SPHERICAL>(model, prm, sim, actions, pd_off, pd_scale, freeze, num_sim_calls, ext_force, ext_torque, nsub);
}
