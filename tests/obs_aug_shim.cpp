// Host build of phc_amd/csrc/phc_obs_aug.h for tests/test_obs_aug_cpu.py and tests/test_obs_aug_gpu.py: the uniforms, the normal pairs, whole launches of
// phc_obs_augment and phc_occl_advance as plain loops, and the argument checks (all pointers are host memory here).
#include "phc_obs_aug.h"

extern "C" {

int obs_aug_sizeof_args() { return (int)sizeof(phc_obs_aug_args_t); }
int obs_aug_block() { return phc::OBS_AUG_BLOCK; }
int obs_aug_max_obs() { return phc::OBS_AUG_MAX_OBS; }
int obs_aug_max_samples() { return phc::OBS_AUG_MAX_SAMPLES; }
int occl_max_bodies() { return phc::OCCL_MAX_BODIES; }

// out [n, n_index, 2]: u(index0 + i, which) of global env genv[r] at count ks[r]
void aug_uniforms_rows(uint64_t key, const int64_t* genv, const int32_t* ks, int n, uint32_t index0, int n_index, float* out) {
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < n_index; ++i)
            for (uint32_t w = 0; w < 2u; ++w)
                out[((int64_t)r * n_index + i) * 2 + w] = phc::aug_u01(key, (uint32_t)genv[r], (uint32_t)ks[r], index0 + (uint32_t)i, w);
}

// out [n, num_obs]: the normals of the columns of one call on global env genv[r] at count ks[r]
void aug_normals_rows(uint64_t key, const int64_t* genv, const int32_t* ks, int n, int num_obs, float* out) {
    for (int r = 0; r < n; ++r)
        for (int j = 0; j < (num_obs + 1) / 2; ++j) {
            float z0, z1;
            phc::aug_normal_pair(key, (uint32_t)genv[r], (uint32_t)ks[r], (uint32_t)j, &z0, &z1);
            out[(int64_t)r * num_obs + 2 * j] = z0;
            if (2 * j + 1 < num_obs) out[(int64_t)r * num_obs + 2 * j + 1] = z1;
        }
}

void aug_box_muller_of(float a, float b, float* out) { phc::aug_box_muller(a, b, out, out + 1); }

int obs_augment_check_of(const phc_obs_aug_args_t* a) { return phc::obs_augment_check(a); }
int occl_advance_check_of(int32_t num_envs, int32_t J, int64_t env_offset, const int32_t* k, float prob, int32_t span_lo, int32_t span_hi, const int64_t* count,
                          const uint8_t* mask) {
    return phc::occl_advance_check(num_envs, J, env_offset, k, prob, span_lo, span_hi, count, mask);
}

void obs_augment_host_of(const phc_obs_aug_args_t* a) { phc::obs_augment_host(*a); }
void occl_advance_host_of(int32_t num_envs, int32_t J, uint64_t key, int64_t env_offset, int32_t* k, float prob, int32_t span_lo, int32_t span_hi, int64_t* count,
                          uint8_t* mask) {
    phc::occl_advance_host(num_envs, J, key, env_offset, k, prob, span_lo, span_hi, count, mask);
}

}
