// Host build of the evaluation kernel's 3x3 similarity solve (phc_amd/csrc/phc_eval.h) for tests/test_eval_device_cpu.py.
#include "phc_eval.h"

extern "C" void eval_similarity_batch(int n, const float* H, const float* sumsq_p, float* R, float* scale) {
    for (int i = 0; i < n; ++i) phc::eval_similarity(H + 9 * i, sumsq_p[i], R + 9 * i, scale + i);
}
