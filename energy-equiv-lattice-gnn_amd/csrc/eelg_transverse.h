// Transverse elastic surfaces of one 6x6 Mandel stiffness matrix and their gradient
// (csrc/eelg_transverse.hip): for a direction d the extremes over the transverse circle of the shear
// modulus G(d, n) and of Poisson's ratio nu(d, n), and the linear compressibility beta(d).  Plain
// C++ on top of csrc/eelg_elastic.h: the same text compiles into the HIP kernels and, with EELG_HD
// empty, into a host program (tests/test_transverse.py builds tests/transverse_host_main.cpp with
// the address and undefined-behaviour sanitizers).  include/eelg.h states every formula.
//
// * With n = cos(th) t1 + sin(th) t2 both 1 / G = 4 T^T S T, T = M(sym(d (x) n)), and
//   -nu / E = u^T m(n), u = S m(d), are a mean plus one sinusoid in 2 th, so their extremes over
//   the circle are mean -+ amplitude: no angular search.
// * Everything is fp64 on the packed fp64 compliance S of eelg_elastic_invert; the results are
//   rounded to fp32 once.  The backward evaluates the same expressions on the same S.
// * No data-dependent array index (the frame's axis is chosen by selects), so after unrolling every
//   array lives in registers on the device.
#ifndef EELG_TRANSVERSE_H
#define EELG_TRANSVERSE_H

#include "eelg_elastic.h"

#ifndef EELG_TRANSVERSE_COLS
#define EELG_TRANSVERSE_COLS 7
#endif
#ifndef EELG_TRANSVERSE_DIR_COLS
#define EELG_TRANSVERSE_DIR_COLS 5
#endif
// columns of a property row
#define EELG_TV_GMIN 0
#define EELG_TV_GMAX 1
#define EELG_TV_NUMIN 2
#define EELG_TV_NUMAX 3
#define EELG_TV_BMIN 4
#define EELG_TV_BMAX 5
#define EELG_TV_SPD 6
// columns of a direction's row
#define EELG_TV_GLO 0
#define EELG_TV_GHI 1
#define EELG_TV_NULO 2
#define EELG_TV_NUHI 3
#define EELG_TV_BETA 4

// Everything one direction contributes, forward and backward.
struct eelg_tv_dir {
  double t1[3], t2[3];                   // the transverse frame
  double a[6], u[6];                     // m(d), S m(d)
  double T1[6], T2[6], b1[6], b2[6], X[6];
  double q0;                             // a^T S a = 1 / E
  double mg, pg, qg, hg;                 // M_G, A11 - A22, 2 A12, hypot(pg, qg) = R_G / 2
  double mn, pn, qn, rn;                 // M_nu, (B1 - B2) / 2, Bx, R_nu
  double beta;
};

// M(sym(x (x) y)) = (x1 y1, x2 y2, x3 y3, r2 (x2 y3 + x3 y2) / 2, r2 (x1 y3 + x3 y1) / 2, r2 (x1 y2 + x2 y1) / 2)
EELG_HD inline void eelg_tv_mandel_sym(const double* x, const double* y, double* m) {
  const double h = 0.70710678118654752440;
  m[0] = x[0] * y[0];
  m[1] = x[1] * y[1];
  m[2] = x[2] * y[2];
  m[3] = h * (x[1] * y[2] + x[2] * y[1]);
  m[4] = h * (x[0] * y[2] + x[2] * y[0]);
  m[5] = h * (x[0] * y[1] + x[1] * y[0]);
}

// y = S x, rows in index order
EELG_HD inline void eelg_tv_matvec(const double* s, const double* x, double* y) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double row = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) row += s[eelg_el_tri(i, j)] * x[j];
    y[i] = row;
  }
}

EELG_HD inline double eelg_tv_dot(const double* x, const double* y) {
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) acc += x[i] * y[i];
  return acc;
}

// The frame: j the first index of the smallest |d_j|, t1 = normalize(d x e_j), t2 = d x t1.
EELG_HD inline void eelg_tv_frame(double d1, double d2, double d3, double* t1, double* t2) {
  int j = 0;
  double m = fabs(d1);
  if (fabs(d2) < m) { j = 1; m = fabs(d2); }
  if (fabs(d3) < m) j = 2;
  const double x = j == 0 ? 0.0 : (j == 1 ? -d3 : d2);
  const double y = j == 0 ? d3 : (j == 1 ? 0.0 : -d1);
  const double z = j == 0 ? -d2 : (j == 1 ? d1 : 0.0);
  const double inv = 1.0 / sqrt(x * x + y * y + z * z);
  t1[0] = x * inv;
  t1[1] = y * inv;
  t1[2] = z * inv;
  t2[0] = d2 * t1[2] - d3 * t1[1];
  t2[1] = d3 * t1[0] - d1 * t1[2];
  t2[2] = d1 * t1[1] - d2 * t1[0];
}

// The six quadratic forms of direction (d1, d2, d3) in S (packed fp64) and what follows from them.
EELG_HD inline void eelg_tv_direction(const double* s, float d1f, float d2f, float d3f, eelg_tv_dir& q) {
  const double d[3] = {(double)d1f, (double)d2f, (double)d3f};
  eelg_tv_frame(d[0], d[1], d[2], q.t1, q.t2);
  eelg_elastic_mandel(d1f, d2f, d3f, q.a);
  eelg_tv_mandel_sym(d, q.t1, q.T1);
  eelg_tv_mandel_sym(d, q.t2, q.T2);
  eelg_tv_mandel_sym(q.t1, q.t1, q.b1);
  eelg_tv_mandel_sym(q.t2, q.t2, q.b2);
  eelg_tv_mandel_sym(q.t1, q.t2, q.X);
  double w[6];
  eelg_tv_matvec(s, q.T1, w);
  const double a11 = eelg_tv_dot(q.T1, w), a12 = eelg_tv_dot(q.T2, w);
  eelg_tv_matvec(s, q.T2, w);
  const double a22 = eelg_tv_dot(q.T2, w);
  q.mg = 2.0 * (a11 + a22);
  q.pg = a11 - a22;
  q.qg = 2.0 * a12;
  q.hg = hypot(q.pg, q.qg);
  eelg_tv_matvec(s, q.a, q.u);
  q.q0 = eelg_tv_dot(q.a, q.u);
  const double bb1 = eelg_tv_dot(q.u, q.b1), bb2 = eelg_tv_dot(q.u, q.b2);
  q.mn = 0.5 * (bb1 + bb2);
  q.pn = 0.5 * (bb1 - bb2);
  q.qn = eelg_tv_dot(q.u, q.X);
  q.rn = hypot(q.pn, q.qn);
  q.beta = (q.u[0] + q.u[1]) + q.u[2];
}

// G_lo, G_hi, nu_lo, nu_hi, beta of a direction (fp64)
EELG_HD inline void eelg_tv_values(const eelg_tv_dir& q, double* v) {
  const double e = 1.0 / q.q0, rg = 2.0 * q.hg;
  v[EELG_TV_GLO] = 1.0 / (q.mg + rg);
  v[EELG_TV_GHI] = 1.0 / (q.mg - rg);
  v[EELG_TV_NULO] = -e * (q.mn + q.rn);
  v[EELG_TV_NUHI] = -e * (q.mn - q.rn);
  v[EELG_TV_BETA] = q.beta;
}

// The transverse unit vector at which an extreme is taken.  which: 0 G_lo, 1 G_hi, 2 nu_lo,
// 3 nu_hi.  n = cos(th) t1 + sin(th) t2, 2 th the phase of the sinusoid (+ pi for the _hi
// extremes); an amplitude of exactly 0 gives th = 0 resp. pi / 2.
EELG_HD inline void eelg_tv_normal(const eelg_tv_dir& q, int which, float* n) {
  const bool shear = which < 2;
  const double amp = shear ? q.hg : q.rn;
  const double phase = amp == 0.0 ? 0.0 : (shear ? atan2(q.qg, q.pg) : atan2(q.qn, q.pn));
  const double th = 0.5 * phase;
  const double c = cos(th), sn = sin(th);
  const bool hi = (which & 1) != 0;
  const double c1 = hi ? -sn : c, c2 = hi ? c : sn;
#pragma unroll
  for (int i = 0; i < 3; ++i) n[i] = (float)(c1 * q.t1[i] + c2 * q.t2[i]);
}

// acc [21] += sym(x y^T) = (x y^T + y x^T) / 2
EELG_HD inline void eelg_tv_sym_acc(double* acc, const double* x, const double* y) {
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) acc[eelg_el_tri(i, j)] += 0.5 * (x[i] * y[j] + x[j] * y[i]);
}

// acc [21] += the direction's part of G_S for the cotangents g [5] on (G_lo, G_hi, nu_lo, nu_hi,
// beta).  Every term is d(x^T S y) / dS = sym(x y^T); a hypot passes (p dp + q dq) / R, and exactly
// 0 where R == 0.
EELG_HD inline void eelg_tv_direction_bwd(const eelg_tv_dir& q, const double* g, double* acc) {
  double v[EELG_TRANSVERSE_DIR_COLS];
  eelg_tv_values(q, v);
  // shear: G = 1 / (M -+ R), M = 2 (A11 + A22), R = 2 hypot(A11 - A22, 2 A12)
  const double wl = g[EELG_TV_GLO] * (v[EELG_TV_GLO] * v[EELG_TV_GLO]);
  const double wh = g[EELG_TV_GHI] * (v[EELG_TV_GHI] * v[EELG_TV_GHI]);
  const double gm = -(wl + wh), gr = -(wl - wh);
  const double gp = q.hg == 0.0 ? 0.0 : 2.0 * gr * (q.pg / q.hg);
  const double gq = q.hg == 0.0 ? 0.0 : 2.0 * gr * (q.qg / q.hg);
  const double g11 = 2.0 * gm + gp, g22 = 2.0 * gm - gp, g12 = 2.0 * gq;
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = g11 * q.T1[i] + 0.5 * g12 * q.T2[i];
  eelg_tv_sym_acc(acc, q.T1, y);
#pragma unroll
  for (int i = 0; i < 6; ++i) y[i] = g22 * q.T2[i] + 0.5 * g12 * q.T1[i];
  eelg_tv_sym_acc(acc, q.T2, y);
  // Poisson: nu = -E (M -+ R), E = 1 / q0, M = (B1 + B2) / 2, R = hypot((B1 - B2) / 2, Bx); beta = u^T h
  const double e = 1.0 / q.q0;
  const double ge = -(g[EELG_TV_NULO] * (q.mn + q.rn) + g[EELG_TV_NUHI] * (q.mn - q.rn));
  const double gmn = -e * (g[EELG_TV_NULO] + g[EELG_TV_NUHI]);
  const double grn = -e * (g[EELG_TV_NULO] - g[EELG_TV_NUHI]);
  const double gpn = q.rn == 0.0 ? 0.0 : grn * (q.pn / q.rn);
  const double gqn = q.rn == 0.0 ? 0.0 : grn * (q.qn / q.rn);
  const double gq0 = -(e * e) * ge;
  const double gb1 = 0.5 * (gmn + gpn), gb2 = 0.5 * (gmn - gpn);
#pragma unroll
  for (int i = 0; i < 6; ++i)
    y[i] = gq0 * q.a[i] + gb1 * q.b1[i] + gb2 * q.b2[i] + gqn * q.X[i] + (i < 3 ? g[EELG_TV_BETA] : 0.0);
  eelg_tv_sym_acc(acc, q.a, y);
}

// g_C [36] = -S G_S S from the summed G_S (gsm, used up), exactly symmetric
EELG_HD inline void eelg_tv_grad_c(const double* s, double* gsm, float* out) {
  const double zero[3] = {0.0, 0.0, 0.0};
  eelg_elastic_grad_c_packed(s, gsm, zero, zero, 1, out);
}

#endif  // EELG_TRANSVERSE_H
