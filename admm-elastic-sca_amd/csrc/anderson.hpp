// anderson.hpp -- the small solve of Anderson acceleration: the regularised normal equations of the residual
// differences and their Cholesky solve, for up to 8 unknowns.  Shared by the host (anderson_host.cpp: admm_hip_acceleration_query)
// and the device (kernels_anderson.hpp: anderson_decide_kernel).  Both sides compile it with -ffp-contract=off and keep the
// operation order below, so they give the same bits.  Extension, no reference counterpart.
//
//   (A + lambda I) theta = b,   A = dF^T W^2 dF (m x m, symmetric: only its lower triangle is read),   b = dF^T W^2 f,
//   lambda = (EPS * tr A) / m,  EPS = 1e-12 (Tikhonov, fixed).
//
// Operation order.  tr A adds the diagonal in ascending order from 0.  Cholesky A + lambda I = L L^T column by column, j ascending:
// d = (A_jj + lambda) - L_j0 L_j0 - ... - L_j,j-1 L_j,j-1 (left to right), L_jj = sqrt(d); below it, i ascending,
// L_ij = (A_ij - L_i0 L_j0 - ... - L_i,j-1 L_j,j-1) / L_jj.  Forward: y_i = (b_i - L_i0 y_0 - ... - L_i,i-1 y_i-1) / L_ii, i ascending.
// Backward: theta_i = (y_i - L_i+1,i theta_i+1 - ... - L_m-1,i theta_m-1) / L_ii, i descending, the subtractions in ascending row
// order.  Every product is rounded.  A pivot d that is not a finite positive number ends the solve: theta = 0 and the return value
// is 1 (the caller then does not extrapolate).
#pragma once

#ifndef ADMM_HD                // (the same definition as local_math.hpp's)
#if defined(__HIPCC__)
#define ADMM_HD __host__ __device__ __forceinline__
#else
#define ADMM_HD inline
#endif
#endif

namespace admm_anderson {

constexpr int MAX_M = 8;
constexpr double EPS = 1e-12;

// A: m x m, row-major with row stride lda; b, theta: m.  1 <= m <= MAX_M.
ADMM_HD int solve(int m, const double *A, int lda, const double *b, double *theta) {
    double L[MAX_M * MAX_M], y[MAX_M];
    for (int i = 0; i < m; ++i) theta[i] = 0.0;
    double tr = 0.0;
    for (int i = 0; i < m; ++i) tr = tr + A[i * lda + i];
    const double lambda = (EPS * tr) / (double)m;
    for (int j = 0; j < m; ++j) {
        double d = A[j * lda + j] + lambda;
        for (int p = 0; p < j; ++p) d = d - L[j * MAX_M + p] * L[j * MAX_M + p];
        if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) return 1;
        const double ljj = __builtin_sqrt(d);
        L[j * MAX_M + j] = ljj;
        for (int i = j + 1; i < m; ++i) {
            double s = A[i * lda + j];
            for (int p = 0; p < j; ++p) s = s - L[i * MAX_M + p] * L[j * MAX_M + p];
            L[i * MAX_M + j] = s / ljj;
        }
    }
    for (int i = 0; i < m; ++i) {
        double s = b[i];
        for (int p = 0; p < i; ++p) s = s - L[i * MAX_M + p] * y[p];
        y[i] = s / L[i * MAX_M + i];
    }
    for (int i = m - 1; i >= 0; --i) {
        double s = y[i];
        for (int p = i + 1; p < m; ++p) s = s - L[p * MAX_M + i] * theta[p];
        theta[i] = s / L[i * MAX_M + i];
    }
    for (int i = 0; i < m; ++i) if (!(theta[i] == theta[i]) || !(theta[i] <= 1.7976931348623157e308 && theta[i] >= -1.7976931348623157e308)) {
        for (int q = 0; q < m; ++q) theta[q] = 0.0;
        return 1;
    }
    return 0;
}

} // namespace admm_anderson
