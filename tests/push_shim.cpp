// Host build of phc_amd/csrc/phc_push.h for tests/test_push_device_cpu.py and tests/test_push_device_gpu.py: the draws, the transition under given
// uniforms, and a whole launch of phc_push_advance as a loop over the envs (all pointers are host memory here).
#include "phc_push.h"

extern "C" {

// out [n_k, n_env, 5]: the draws of envs env0 .. env0 + n_env - 1 at launch counts k0 .. k0 + n_k - 1
void push_draws_batch(uint64_t key, uint32_t env0, int n_env, uint32_t k0, int n_k, float* out) {
    for (int k = 0; k < n_k; ++k)
        for (int e = 0; e < n_env; ++e) phc::push_draws(key, env0 + (uint32_t)e, k0 + (uint32_t)k, out + ((int64_t)k * n_env + e) * 5);
}

// the argument checks of phc_push_advance, without the launch behind them
int push_args_check_of(const phc_push_args_t* a) { return phc::push_args_check(a); }

int push_pause_of(const phc_push_args_t* a, float u0) { return phc::push_pause(phc::push_params(*a), u0); }

// one step of every env with the uniforms given (u [5, N] as torch.rand((5, N)) lays them out; reset [N] bytes); k is left alone
void push_step_given(const phc_push_args_t* a, const float* u, const uint8_t* reset) {
    for (int64_t e = 0; e < a->num_envs; ++e) {
        const float ue[5] = {u[e], u[a->num_envs + e], u[2 * (int64_t)a->num_envs + e], u[3 * (int64_t)a->num_envs + e], u[4 * (int64_t)a->num_envs + e]};
        phc::push_env_given(*a, e, ue, reset[e] != 0);
    }
}

// phc_push_advance's kernel on the host: the same per-env function over all envs
void push_advance_host(const phc_push_args_t* a) {
    for (int64_t e = 0; e < a->num_envs; ++e) phc::push_env(*a, e);
}

}
