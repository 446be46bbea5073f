// Host build of phc_amd/csrc/phc_getup.h for tests/test_getup_device_cpu.py and tests/test_getup_device_gpu.py: the draws, the slot permutation, a whole launch
// of phc_getup_assign as plain loops (with the uniforms / the permutation given or drawn), phc_task_draws, and the argument checks (all pointers are host
// memory here).
#include "phc_getup.h"

extern "C" {

int getup_sizeof_args() { return (int)sizeof(phc_getup_args_t); }
int getup_block() { return phc::GETUP_BLOCK; }
int getup_max_envs() { return phc::GETUP_MAX_ENVS; }

// out [n_k, n_env, 2]: the draws of envs env0 .. env0 + n_env - 1 at counts k0 .. k0 + n_k - 1
void getup_draws_batch(uint64_t key, uint32_t env0, int n_env, uint32_t k0, int n_k, float* out) {
    for (int k = 0; k < n_k; ++k)
        for (int e = 0; e < n_env; ++e) phc::getup_draws(key, env0 + (uint32_t)e, k0 + (uint32_t)k, out + ((int64_t)k * n_env + e) * 2);
}

// out [F]: pi(0 .. F - 1) of the launch with this key and count
void getup_perm_of(uint64_t key, uint64_t count, uint32_t F, int32_t* out) {
    const uint64_t pkey = phc::getup_perm_key(key, count, F);
    for (uint32_t r = 0; r < F; ++r) out[r] = (int32_t)phc::getup_perm(pkey, F, r);
}

int getup_args_check_of(const phc_getup_args_t* a) { return phc::getup_args_check(a); }
int task_draws_check_of(int32_t num_envs, int64_t env_offset, const int32_t* k) { return phc::task_draws_check(num_envs, env_offset, k); }

// phc_getup_assign on the host; u_given [N, 2] and perm_given [>= number of FALL envs], each nullable
void getup_assign_host_of(const phc_getup_args_t* a, const float* u_given, const int32_t* perm_given) { phc::getup_assign_host(*a, u_given, perm_given); }

// phc_task_draws on the host
void task_draws_host(int32_t num_envs, uint64_t key, int64_t env_offset, int32_t* k, float* cycle_phase, float* offset_rand) {
    for (int64_t e = 0; e < num_envs; ++e) phc::task_draws_env(key, env_offset, k, cycle_phase, offset_rand, e);
}

}
