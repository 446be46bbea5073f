// Host build of phc_amd/csrc/phc_stream.h for tests/test_stream_cpu.py and tests/test_stream_gpu.py: the argument check and a whole launch of
// phc_stream_track as a loop over the envs (all pointers are host memory here).
#include "phc_stream.h"

extern "C" {

int stream_args_check_of(const phc_model_t* model, const phc_im_params_t* prm, const phc_stream_args_t* a) { return phc::stream_args_check(model, prm, a); }

// phc_stream_track on the host: the entry point's check, then the same per-lane functions and the same group sums over all envs
int stream_track_host(const phc_model_t* model, const phc_im_params_t* prm, const phc_stream_args_t* a) {
    const int rc = phc::stream_args_check(model, prm, a);
    if (rc) return rc;
    const phc_im_params_t p = phc::stream_params(*prm, *a);
    for (int64_t e = 0; e < a->num_envs; ++e) phc::stream_env_host(model->num_bodies, p, *a, e);
    return 0;
}

}
