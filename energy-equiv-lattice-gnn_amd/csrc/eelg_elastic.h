// Elastic properties of one 6x6 Mandel stiffness matrix and their gradient (csrc/eelg_elastic.hip:
// the Voigt / Reuss / Hill moduli, Poisson's ratio, the universal anisotropy index and the
// directional Young's modulus).  Plain C++: the same text compiles into the HIP kernels and, with
// EELG_HD empty, into a host program (tests/test_elastic.py builds tests/elastic_host_main.cpp
// with the address and undefined-behaviour sanitizers and runs the SPD set through it).
//
// * The function is defined on the symmetric part A = (C + C^T) / 2: both triangles are read.
//   Symmetric matrices are kept as 21 packed entries (eelg_el_tri), every index a compile-time
//   constant once the loops are unrolled, so on the device they stay in registers (no scratch).
// * Inversion: Cholesky A = L L^T, L^-1 by forward substitution, S = L^-T L^-1, all in fp64 inside
//   the routine; inputs and outputs are fp32.  An fp32 Cholesky inverse loses kappa * 6e-8 on the
//   compliance (6e-5 on the Reuss and E columns of the test set, 8x the error of LAPACK's fp32
//   inverse), and one fp32 Newton step does not recover it because the residual I - A S cancels
//   in fp32.  In fp64 the routine's own error is below the rounding of the fp32 results.
// * spd: every pivot is finite and > 0.  A NaN or an infinity anywhere in A reaches a pivot (entry
//   (i, j) of the lower triangle enters pivot i), so such a matrix is flagged like an indefinite
//   one.  No data-dependent exit: the factorisation of a flagged matrix runs to its end on NaN.
// * Mandel order 11, 22, 33, 23, 13, 12 with sqrt(2) on the shear entries (include/eelg.h).
//   a, b, c of a matrix: the sums of its three normal diagonal entries, its three normal
//   off-diagonal entries (one triangle) and its three shear diagonal entries.
#ifndef EELG_ELASTIC_H
#define EELG_ELASTIC_H

#include <math.h>

#ifndef EELG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EELG_HD __host__ __device__
#else
#define EELG_HD
#endif
#endif

#ifndef EELG_ELASTIC_COLS
#define EELG_ELASTIC_COLS 12
#endif
// columns of a property row
#define EELG_EL_KV 0
#define EELG_EL_GV 1
#define EELG_EL_KR 2
#define EELG_EL_GR 3
#define EELG_EL_KH 4
#define EELG_EL_GH 5
#define EELG_EL_EH 6
#define EELG_EL_NUH 7
#define EELG_EL_AU 8
#define EELG_EL_EMIN 9
#define EELG_EL_EMAX 10
#define EELG_EL_SPD 11

// packed index of the symmetric entry (i, j), either order
EELG_HD inline constexpr int eelg_el_tri(int i, int j) {
  return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;
}

// c: [36] row-major fp32.  a: [21] packed (C + C^T) / 2 (exact in fp64).  s: [21] packed A^-1.
// Returns 1 if A is positive definite (then s is its inverse), else 0 (s is not to be used).
EELG_HD inline int eelg_elastic_invert(const float* c, double* a, double* s) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) a[eelg_el_tri(i, j)] = 0.5 * ((double)c[6 * i + j] + (double)c[6 * j + i]);
  double l[21], inv[6];
  int ok = 1;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = a[eelg_el_tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= l[eelg_el_tri(j, k)] * l[eelg_el_tri(j, k)];
    if (!(d > 0.0) || !(d <= 1.7976931348623157e308)) ok = 0;
    const double r = sqrt(d);
    l[eelg_el_tri(j, j)] = r;
    inv[j] = 1.0 / r;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = a[eelg_el_tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= l[eelg_el_tri(i, k)] * l[eelg_el_tri(j, k)];
      l[eelg_el_tri(i, j)] = v * inv[j];
    }
  }
  // m = L^-1 (lower), column by column
  double m[21];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    m[eelg_el_tri(j, j)] = inv[j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) v -= l[eelg_el_tri(i, k)] * m[eelg_el_tri(k, j)];
      m[eelg_el_tri(i, j)] = v * inv[i];
    }
  }
  // S = m^T m
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double v = 0.0;
#pragma unroll
      for (int k = i; k < 6; ++k) v += m[eelg_el_tri(k, i)] * m[eelg_el_tri(k, j)];
      s[eelg_el_tri(i, j)] = v;
    }
  return ok;
}

EELG_HD inline void eelg_elastic_abc(const double* p, double* abc) {
  abc[0] = (p[eelg_el_tri(0, 0)] + p[eelg_el_tri(1, 1)]) + p[eelg_el_tri(2, 2)];
  abc[1] = (p[eelg_el_tri(1, 0)] + p[eelg_el_tri(2, 0)]) + p[eelg_el_tri(2, 1)];
  abc[2] = (p[eelg_el_tri(3, 3)] + p[eelg_el_tri(4, 4)]) + p[eelg_el_tri(5, 5)];
}

// The nine scalar columns K_V .. A_U from A and S (packed).  spd == 0: K_V and G_V only, the
// other seven are NaN.
EELG_HD inline void eelg_elastic_scalars(const double* a, const double* s, int spd, double* out) {
  double ca[3], sa[3];
  eelg_elastic_abc(a, ca);
  eelg_elastic_abc(s, sa);
  const double kv = (ca[0] + 2.0 * ca[1]) / 9.0;
  const double gv = (ca[0] - ca[1] + 1.5 * ca[2]) / 15.0;
  const double kr = 1.0 / (sa[0] + 2.0 * sa[1]);
  const double gr = 15.0 / (4.0 * sa[0] - 4.0 * sa[1] + 6.0 * sa[2]);
  const double kh = 0.5 * (kv + kr), gh = 0.5 * (gv + gr);
  const double den = 3.0 * kh + gh;
  const double nan = NAN;
  out[EELG_EL_KV] = kv;
  out[EELG_EL_GV] = gv;
  out[EELG_EL_KR] = spd ? kr : nan;
  out[EELG_EL_GR] = spd ? gr : nan;
  out[EELG_EL_KH] = spd ? kh : nan;
  out[EELG_EL_GH] = spd ? gh : nan;
  out[EELG_EL_EH] = spd ? 9.0 * kh * gh / den : nan;
  out[EELG_EL_NUH] = spd ? (3.0 * kh - 2.0 * gh) / (2.0 * den) : nan;
  out[EELG_EL_AU] = spd ? 5.0 * gv / gr + kv / kr - 6.0 : nan;
}

// m(d) = (d1^2, d2^2, d3^2, r2 d2 d3, r2 d1 d3, r2 d1 d2)
EELG_HD inline void eelg_elastic_mandel(float d1f, float d2f, float d3f, double* m) {
  const double r2 = 1.41421356237309504880, d1 = d1f, d2 = d2f, d3 = d3f;
  m[0] = d1 * d1;
  m[1] = d2 * d2;
  m[2] = d3 * d3;
  m[3] = r2 * (d2 * d3);
  m[4] = r2 * (d1 * d3);
  m[5] = r2 * (d1 * d2);
}

// m^T S m, rows in index order
EELG_HD inline double eelg_elastic_quad(const double* s, const double* m) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double row = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) row += s[eelg_el_tri(i, j)] * m[j];
    acc += m[i] * row;
  }
  return acc;
}

// E(d) = 1 / (m^T S m) as the fp32 value that is stored
EELG_HD inline float eelg_elastic_young(const double* s, float d1, float d2, float d3) {
  double m[6];
  eelg_elastic_mandel(d1, d2, d3, m);
  return (float)(1.0 / eelg_elastic_quad(s, m));
}

// Should the pair (ov, oi) replace (v, i) as the minimum / maximum?  The smaller index wins a
// tie, so the reduction gives the first extreme in any order of comparisons; a NaN never wins.
EELG_HD inline bool eelg_elastic_min_takes(float v, int i, float ov, int oi) {
  return ov < v || (ov == v && oi < i);
}
EELG_HD inline bool eelg_elastic_max_takes(float v, int i, float ov, int oi) {
  return ov > v || (ov == v && oi < i);
}

// ---- backward ---------------------------------------------------------------------------------
// Cotangents on the nine scalar columns (g[0..8] of a property row's cotangent) taken back to
// the a, b, c sums: gs[3] for those of S (zero if spd == 0: the cotangents of the NaN columns are
// not read), gc[3] for the direct Voigt terms on those of A.
EELG_HD inline void eelg_elastic_scalars_bwd(const float* props, const float* g, int spd, double* gs,
                                             double* gc) {
  double gkv = g[EELG_EL_KV], ggv = g[EELG_EL_GV];
  gs[0] = gs[1] = gs[2] = 0.0;
  if (spd) {
    const double kv = props[EELG_EL_KV], gv = props[EELG_EL_GV], kr = props[EELG_EL_KR], gr = props[EELG_EL_GR];
    const double kh = 0.5 * (kv + kr), gh = 0.5 * (gv + gr), den = 3.0 * kh + gh, id2 = 1.0 / (den * den);
    double gkr = g[EELG_EL_KR], ggr = g[EELG_EL_GR], gkh = g[EELG_EL_KH], ggh = g[EELG_EL_GH];
    const double geh = g[EELG_EL_EH], gnu = g[EELG_EL_NUH], gau = g[EELG_EL_AU];
    gkh += geh * (9.0 * gh * gh * id2) + gnu * (4.5 * gh * id2);
    ggh += geh * (27.0 * kh * kh * id2) - gnu * (4.5 * kh * id2);
    gkv += 0.5 * gkh;
    gkr += 0.5 * gkh;
    ggv += 0.5 * ggh;
    ggr += 0.5 * ggh;
    ggv += gau * (5.0 / gr);
    ggr -= gau * (5.0 * gv / (gr * gr));
    gkv += gau / kr;
    gkr -= gau * (kv / (kr * kr));
    // K_R = 1 / (a + 2 b), G_R = 15 / (4 a - 4 b + 6 c)
    const double wk = -gkr * kr * kr, wg = -ggr * gr * gr / 15.0;
    gs[0] = wk + 4.0 * wg;
    gs[1] = 2.0 * wk - 4.0 * wg;
    gs[2] = 6.0 * wg;
  }
  gc[0] = gkv / 9.0 + ggv / 15.0;
  gc[1] = 2.0 * gkv / 9.0 - ggv / 15.0;
  gc[2] = ggv / 10.0;
}

// acc [21] += w m m^T
EELG_HD inline void eelg_elastic_outer_acc(double* acc, double w, const double* m) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) acc[eelg_el_tri(i, j)] += w * (m[i] * m[j]);
}

// The cotangent of an a, b, c triple spread over the matrix entries: a and c on the diagonal, b
// (the sum over one triangle) as b / 2 on either side, so the packed matrix stays the gradient
// with respect to a full symmetric matrix.
EELG_HD inline void eelg_elastic_abc_spread(double* p, const double* abc) {
  p[eelg_el_tri(0, 0)] += abc[0];
  p[eelg_el_tri(1, 1)] += abc[0];
  p[eelg_el_tri(2, 2)] += abc[0];
  p[eelg_el_tri(1, 0)] += 0.5 * abc[1];
  p[eelg_el_tri(2, 0)] += 0.5 * abc[1];
  p[eelg_el_tri(2, 1)] += 0.5 * abc[1];
  p[eelg_el_tri(3, 3)] += abc[2];
  p[eelg_el_tri(4, 4)] += abc[2];
  p[eelg_el_tri(5, 5)] += abc[2];
}

// g_C [36] = -S G_S S + the direct terms, both triangles written from one packed result (exactly
// symmetric).  s [21]: the compliance, packed fp64.  gsm [21]: the directional part of G_S (the a, b,
// c part is added here; gsm is used up).  spd == 0: the direct terms alone, s and gsm are not read.
EELG_HD inline void eelg_elastic_grad_c_packed(const double* s, double* gsm, const double* gs, const double* gc,
                                               int spd, float* out) {
  double r[21];
#pragma unroll
  for (int i = 0; i < 21; ++i) r[i] = 0.0;
  if (spd) {
    double t[36];
    eelg_elastic_abc_spread(gsm, gs);
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) v += s[eelg_el_tri(i, k)] * gsm[eelg_el_tri(k, j)];
        t[6 * i + j] = v;
      }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) v -= t[6 * i + k] * s[eelg_el_tri(k, j)];
        r[eelg_el_tri(i, j)] = v;
      }
  }
  eelg_elastic_abc_spread(r, gc);
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 6; ++j) out[6 * i + j] = (float)r[eelg_el_tri(i, j)];
}

// The same from the compliance as the forward of csrc/eelg_elastic.hip stored it: s32 [36] fp32,
// lower triangle read (not read with spd == 0).  gsm: sum_p w_p m m^T.
EELG_HD inline void eelg_elastic_grad_c(const float* s32, double* gsm, const double* gs, const double* gc,
                                        int spd, float* out) {
  double s[21];
#pragma unroll
  for (int i = 0; i < 21; ++i) s[i] = 0.0;
  if (spd) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) s[eelg_el_tri(i, j)] = s32[6 * i + j];
  }
  eelg_elastic_grad_c_packed(s, gsm, gs, gc, spd, out);
}

#endif  // EELG_ELASTIC_H
