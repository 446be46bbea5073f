// phc_distill.h -- per-element code of the distillation kernels (phc_distill.hip): the SiLU of the student MLP, its derivative, one squared-error term and
// the dataset recorder's row rule.  Plain C++ on the host too (a host build of this header states the same fp32 operations).
#ifndef PHC_DISTILL_H
#define PHC_DISTILL_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PHC_DISTILL_FN __host__ __device__ __forceinline__
#else
#define PHC_DISTILL_FN static inline
#endif

// y = z / (1 + exp(-z)) in fp32 (torch's SiLU).  exp(-z) overflows to +inf below z ~ -88.7: z / inf = -0, never NaN for a finite z.
PHC_DISTILL_FN float phc_silu_f(float z) { return z / (1.0f + expf(-z)); }

// d silu / dz = s (1 + z (1 - s)), s = sigmoid(z).  Both s and 1 - s come from e = exp(-|z|) <= 1 (no overflow, and 1 - s keeps its relative
// precision where s rounds to 1): for z >= 0 s = 1 / (1 + e), 1 - s = e / (1 + e); for z < 0 the two swap.
// The caller multiplies (g s) first, then the bracket: at z = -max the product is 0 x finite, not 0 x inf.
PHC_DISTILL_FN float phc_silu_grad_f(float g, float z) {
    const float e = expf(-fabsf(z));
    const float d = 1.0f + e;
    const float a = 1.0f / d, b = e / d;
    const float s = z >= 0.0f ? a : b, t = z >= 0.0f ? b : a;
    return (g * s) * (1.0f + z * t);
}

// Which row of the batch block env `i` writes at env step `step`, or -1: rows[i] rows starting at row_start[i].
PHC_DISTILL_FN int64_t phc_record_row(int64_t rows_i, int64_t row_start_i, int32_t step) { return (int64_t)step < rows_i ? row_start_i + step : (int64_t)-1; }

#endif /* PHC_DISTILL_H */
