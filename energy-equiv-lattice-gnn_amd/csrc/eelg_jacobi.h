// Eigenvalues of a symmetric 6x6 fp32 matrix by cyclic Jacobi (the stiffness metrics of
// csrc/eelg_metrics.hip: torch.linalg.eigvalsh of target and prediction in obtain_errors,
// scripts/train_utils.py:166-168).  Plain C++: the same text compiles into the HIP kernel and,
// with EELG_HD empty, into a host program (tests/test_metrics.py builds one with the address and
// undefined-behaviour sanitizers and runs the hostile matrix set through it).
//
// * Only the LOWER triangle of the input is read (eigvalsh's default UPLO = 'L'); it is kept as
//   21 packed entries, every index a compile-time constant once the (p, q, r) loops are unrolled,
//   so on the device the matrix stays in registers (no scratch).
// * A fixed number of sweeps and no data-dependent exit: a NaN input terminates like any other
//   and comes out as NaN; a rotation whose off-diagonal entry is already zero is the identity.
// * The rotation is formed from d = a_qq - a_pp and b = 2 a_pq divided by max(|d|, |b|): the
//   textbook theta = d / b overflows in theta^2 when a_pq is tiny, here every intermediate is
//   <= sqrt(2) in magnitude.  t = sgn(d) b' / (|d'| + sqrt(d'^2 + b'^2)) is the smaller root
//   (|t| <= 1), d = 0 gives the 45 degree rotation, d = b = 0 gives t = 0.
// * Each diagonal entry is a compensated pair (value + the rounding error its updates have
//   dropped, recovered exactly by the two-sum identity): the eigenvalues are what is left on the
//   diagonal after ~60 updates a_pp -= t a_pq, and plain fp32 accumulation of those loses 2e-7
//   of the largest eigenvalue where LAPACK's fp32 eigvalsh loses 4e-8.  Contraction into fma is
//   switched off inside the routine so that the identity holds for the value that was added.
//
// EELG_JACOBI_SWEEPS: fixed by the host run over the hostile set of tests/helpers_metrics.py
// (random SPD, diagonal, isotropic = 5-fold degenerate, rank 1, indefinite, scales 1e-4 and
// 1e5).  Largest |error| / largest |eigenvalue| against numpy fp64 over the set, by sweep count:
//   1: 9.7e-02   2: 1.7e-02   3: 2.1e-05   4: 3.9e-08   5 .. 12: 3.9e-08   (LAPACK fp32: 3.9e-08;
//   without the compensated diagonal: 2.2e-07 from 4 sweeps on)
// Convergence is quadratic and the set is converged to fp32 after 4 sweeps; 6 leaves two spare
// sweeps for matrices harder than the set (a spare sweep on a converged matrix is 15 identity
// rotations: every b is zero).
#ifndef EELG_JACOBI_H
#define EELG_JACOBI_H

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EELG_HD __host__ __device__
#else
#define EELG_HD
#endif

#ifndef EELG_JACOBI_SWEEPS
#define EELG_JACOBI_SWEEPS 6
#endif

// packed index of the lower-triangle entry (i, j), either order
EELG_HD inline constexpr int eelg_tri(int i, int j) {
  return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;
}

// m: [36] row-major, entries (i, j <= i) read.  eig: [6] ascending.
EELG_HD inline void eelg_jacobi6(const float* m, float* eig, int sweeps = EELG_JACOBI_SWEEPS) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  float a[21];
  float lo[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // rounding errors dropped from a[i][i] so far
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) a[eelg_tri(i, j)] = m[6 * i + j];
#pragma unroll 1
  for (int sweep = 0; sweep < sweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < 5; ++p) {
#pragma unroll
      for (int q = p + 1; q < 6; ++q) {
        const float apq = a[eelg_tri(q, p)], app = a[eelg_tri(p, p)], aqq = a[eelg_tri(q, q)];
        const float d = (aqq - app) + (lo[q] - lo[p]), b = apq + apq;
        const float ad = fabsf(d), ab = fabsf(b);
        const float big = ad > ab ? ad : ab;       // a NaN in d or b reaches t through dd / bb
        float t = 0.f;
        if (!(big == 0.f)) {
          const float dd = ad / big, bb = b / big;
          t = (d >= 0.f ? bb : -bb) / (dd + sqrtf(dd * dd + bb * bb));
        }
        const float c = 1.f / sqrtf(t * t + 1.f), s = t * c, tau = s / (1.f + c);
        const float h = t * apq;
        // two-sum: s = x + y rounded, (x - (s - bb)) + (y - bb) with bb = s - x is the error
        const float sp = app - h, bp = sp - app;
        lo[p] += (app - (sp - bp)) + (-h - bp);
        a[eelg_tri(p, p)] = sp;
        const float sq = aqq + h, bq = sq - aqq;
        lo[q] += (aqq - (sq - bq)) + (h - bq);
        a[eelg_tri(q, q)] = sq;
        a[eelg_tri(q, p)] = 0.f;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (r == p || r == q) continue;
          const float arp = a[eelg_tri(r, p)], arq = a[eelg_tri(r, q)];
          a[eelg_tri(r, p)] = arp - s * (arq + tau * arp);
          a[eelg_tri(r, q)] = arq + s * (arp - tau * arq);
        }
      }
    }
  }
  float e[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) e[i] = a[eelg_tri(i, i)] + lo[i];
  // ascending, by compare-and-swap (a NaN compares false and stays where it is)
#pragma unroll
  for (int n = 5; n > 0; --n)
#pragma unroll
    for (int i = 0; i < n; ++i)
      if (e[i] > e[i + 1]) { const float x = e[i]; e[i] = e[i + 1]; e[i + 1] = x; }
#pragma unroll
  for (int i = 0; i < 6; ++i) eig[i] = e[i];
}

#endif  // EELG_JACOBI_H
