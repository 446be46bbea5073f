// Host build of phc_amd/csrc/phc_proj.h for tests/test_projectile_cpu.py and tests/test_projectile_gpu.py: the draws, the argument checks, and a whole
// launch of phc_proj_advance as a loop over the envs with the one-lane group (all pointers are host memory here).
#include "phc_proj.h"

extern "C" {

// out [n_k, n_env, 8]: the draws of slot `slot` of envs env0 .. env0 + n_env - 1 at launch counts k0 .. k0 + n_k - 1
void proj_draws_batch(uint64_t key, uint32_t env0, int n_env, uint32_t k0, int n_k, int slot, float* out) {
    for (int k = 0; k < n_k; ++k)
        for (int e = 0; e < n_env; ++e) phc::proj_draws(key, env0 + (uint32_t)e, k0 + (uint32_t)k, slot, out + ((int64_t)k * n_env + e) * PHC_PROJ_DRAWS);
}

// the argument checks of phc_proj_advance, without the launch behind them
int proj_args_check_of(const phc_proj_args_t* a) { return phc::proj_args_check(a); }

int proj_rows_check_of(const phc_proj_rows_t* a) { return phc::proj_rows_check(a); }

// phc_proj_rows' kernel on the host
void proj_rows_host(const phc_proj_rows_t* a) {
    for (int64_t e = 0; e < a->num_envs; ++e) phc::proj_rows_env(*a, e, 0, 1);
}

int proj_pause_of(const phc_proj_args_t* a, float u0) { return phc::proj_pause(*a, u0); }

// phc_proj_advance's kernel on the host.  margin [N], nullable: the least decision margin of each env in this step (phc::proj_margin), +inf where none.
void proj_advance_host(const phc_proj_args_t* a, float* margin) {
    phc::ProjHostGroup g;
    for (int64_t e = 0; e < a->num_envs; ++e) {
        if (margin) margin[e] = INFINITY;
        phc::proj_env(*a, e, true, g, margin ? margin + e : nullptr);
    }
}

}
