// phc_eval.h -- per-lane pieces of the evaluation sweep's metric accumulation (phc_eval_accumulate, csrc/phc_eval.hip): the position-only
// reference lookup and the 3x3 similarity (Procrustes) solve.  PHC_HD: tests/eval_similarity_shim.cpp builds the solve for the CPU.
#pragma once
#include "phc_task.h"

namespace phc {

// The position quarter of ref_body(): the same two loads and the same lerp, so the value is bit-equal to phc_motion_state's rg_pos.
PHC_HD V3 ref_body_pos(const phc_motion_lib_t& lib, const FrameRef& fr, int j) {
    const float* a = lib.frames + fr.f0 * (int64_t)lib.frame_stride;
    const float* b = lib.frames + fr.f1 * (int64_t)lib.frame_stride;
    return lerp3(ld3(a + fr_pos(lib) + 3 * j), ld3(b + fr_pos(lib) + 3 * j), fr.blend);
}

// One Jacobi rotation of the symmetric 4x4 `A` in the (P, Q) plane, accumulated into the eigenvector columns of `V`.  P, Q are template
// arguments so that every index is a constant and the two matrices stay in registers on the device.
template <int P, int Q>
PHC_HD void eval_jacobi_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));   // (theta^2 overflowing gives t = 0: no rotation)
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // A <- A J
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq; A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // A <- J^T A
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk; A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // V <- V J
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq; V[k][Q] = s * vkp + c * vkq;
    }
}

// Similarity alignment of a centred cloud p onto a centred cloud g (im_eval._procrustes): H[3 a + b] = sum_j p_j[a] g_j[b], sumsq_p = sum_j |p_j|^2
// -> the proper rotation R (row-major, g ~ scale R p) that maximises trace(R H) and scale = (s1 + s2 + d s3) / sumsq_p.
// Horn's closed form (J. Opt. Soc. Am. A 4, 1987): the rotation is the unit quaternion of the largest eigenvalue of a symmetric 4x4 built from H, and
// that eigenvalue IS s1 + s2 + d s3 with d = sign(det H) -- the mirrored case (d = -1) and the planar case (s3 = 0, third axis from the other two) need
// no branch, because the search runs over proper rotations only.  The eigenproblem is solved by cyclic Jacobi sweeps in fp64, at most 12 of them.
// The stop test below is under fp64's epsilon, so it fires only once quadratic convergence has taken the off-diagonal to (near) zero: typically after six
// to eight sweeps, in the worst case never, and then all 12 run.  The inputs and outputs are fp32 like the kernel's lane sums.
PHC_HD void eval_similarity(const float H[9], float sumsq_p, float R[9], float* scale) {
    const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
    double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#if defined(__clang__)
#pragma nounroll   // one sweep's code, not twelve copies of it
#endif
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[0][3]) + fabs(A[1][2]) + fabs(A[1][3]) + fabs(A[2][3]);
        const double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]) + fabs(A[3][3]);
        if (off <= 1e-18 * diag) break;
        eval_jacobi_rotate<0, 1>(A, V); eval_jacobi_rotate<0, 2>(A, V); eval_jacobi_rotate<0, 3>(A, V);
        eval_jacobi_rotate<1, 2>(A, V); eval_jacobi_rotate<1, 3>(A, V); eval_jacobi_rotate<2, 3>(A, V);
    }
    // the eigenvector of the largest eigenvalue (first one on a tie, which only an all-zero H produces: identity rotation, as numpy gives)
    int k = 0;
    double lam = A[0][0];
    if (A[1][1] > lam) { lam = A[1][1]; k = 1; }
    if (A[2][2] > lam) { lam = A[2][2]; k = 2; }
    if (A[3][3] > lam) { lam = A[3][3]; k = 3; }
    // column k of V, picked with 0 / 1 weights: V[.][k] would be a run-time index, which puts the matrix into scratch memory on the device
    const double m0 = k == 0 ? 1.0 : 0.0, m1 = k == 1 ? 1.0 : 0.0, m2 = k == 2 ? 1.0 : 0.0, m3 = k == 3 ? 1.0 : 0.0;
    double w = m0 * V[0][0] + m1 * V[0][1] + m2 * V[0][2] + m3 * V[0][3], x = m0 * V[1][0] + m1 * V[1][1] + m2 * V[1][2] + m3 * V[1][3];
    double y = m0 * V[2][0] + m1 * V[2][1] + m2 * V[2][2] + m3 * V[2][3], z = m0 * V[3][0] + m1 * V[3][1] + m2 * V[3][2] + m3 * V[3][3];
    const double n = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    w *= n; x *= n; y *= n; z *= n;
    R[0] = (float)(w * w + x * x - y * y - z * z); R[1] = (float)(2.0 * (x * y - w * z)); R[2] = (float)(2.0 * (x * z + w * y));
    R[3] = (float)(2.0 * (x * y + w * z)); R[4] = (float)(w * w - x * x + y * y - z * z); R[5] = (float)(2.0 * (y * z - w * x));
    R[6] = (float)(2.0 * (x * z - w * y)); R[7] = (float)(2.0 * (y * z + w * x)); R[8] = (float)(w * w - x * x - y * y + z * z);
    const double ss = sumsq_p > 1e-12f ? (double)sumsq_p : 1e-12;   // np.maximum(sum p^2, 1e-12)
    *scale = (float)(lam / ss);
}

}  // namespace phc
