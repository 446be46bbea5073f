// Host build of phc_amd/csrc/phc_dr.h (and of check_sim_step_dr, phc_amd/csrc/phc_sim_check.h) for tests/test_domain_rand_cpu.py and
// tests/test_domain_rand_gpu.py: the torque-noise draws and the target shift, the delay law, the argument checks, and a whole launch of phc_dr_advance as a
// loop over the envs (all pointers are host memory here).
#include "phc_dr.h"
#include "phc_sim_check.h"

extern "C" {

// out [n]: u of (key, k, call) at indices index0 .. index0 + n - 1
void dr_noise_u_batch(uint64_t key, uint32_t k, uint32_t call, uint32_t index0, int n, float* out) {
    for (int i = 0; i < n; ++i) out[i] = phc::dr_noise_u(key, k, call, index0 + (uint32_t)i);
}

float dr_shifted_target(float target, float u, float amp, float kp) { return phc::dr_target_shift(target, u, phc::dr_noise_gain(amp, kp)); }

int dr_delay_law(int lo, int hi, float u) { return phc::dr_delay_of(lo, hi, u); }

int dr_args_check_of(const phc_dr_args_t* a) { return phc::dr_args_check(a); }

int check_sim_step_dr_of(const phc_model_t* model, const phc_sim_params_t* params, const phc_sim_state_t* sim, const float* actions, const float* off,
                         const float* scale, int32_t num_sim_calls, const phc_sim_dr_t* dr) {
    return phc::check_sim_step_dr(model, params, sim, actions, off, scale, num_sim_calls, dr);
}

// phc_dr_advance's kernel on the host: the same per-env function over all envs
void dr_advance_host(const phc_dr_args_t* a) {
    for (int64_t e = 0; e < a->num_envs; ++e) phc::dr_env(*a, e);
}

}
