// The per-element and per-graph arithmetic of the lattice design step (csrc/eelg_design.hip): the
// strut length and volume term, the tied radius gradient, the heavy-ball step in max-norm with its
// box clamps and the volume-keeping rescale.  Plain C++: the same text compiles into the HIP kernels
// and, with EELG_HD empty, into a host program (tests/test_design.py builds
// tests/design_host_main.cpp with the address and undefined-behaviour sanitizers and runs the test
// cases through eelg_design_graph below).
//
// * Everything is fp32, one rounding per written operation (no contraction into fma: the composed
//   torch form rounds every product, and the two agree bitwise wherever no sum is involved), except
//   - the squared length, two explicit fmaf over vx vx (the vector itself is formed as
//     eelg_edge_embed forms it, (pos[recv] - pos[send]) + shift), and
//   - the volume, whose terms r^2 L are formed and summed in fp64 and rounded to fp32 once: the
//     rescale divides V0 by it, so its rounding error goes into every radius of the graph.
// * Division and square root are the correctly rounded ones (hipcc's default for fp32).
// * The step is not Adam: Adam's first step is sign(g), which turns gradient entries at rounding
//   level into full-size moves.  Here a group (the radii, or the positions, of one graph) moves by
//   step * m with m = beta m + g / max|g|: `step` is the largest move of an iteration from rest.
#ifndef EELG_DESIGN_H
#define EELG_DESIGN_H

#include <math.h>

#ifndef EELG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EELG_HD __host__ __device__
#else
#define EELG_HD
#endif
#endif

// flag bits of a graph (eelg_design_step's flag row)
#define EELG_DESIGN_NONFINITE 1   // a gradient entry of the graph is Inf or NaN: nothing was changed
#define EELG_DESIGN_BAD_INDEX 2   // send / recv / partner leaves the graph's own rows: nothing was read

typedef struct {
  float step_r, step_pos, beta, r_min, r_max, move_limit;
  int keep_volume;
} eelg_design_consts;

// neither Inf nor NaN (on the bits: holds under any floating-point compiler mode)
EELG_HD inline int eelg_design_finite(float x) {
  unsigned u;
  __builtin_memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}

// |(pos[recv] - pos[send]) + shift|
EELG_HD inline float eelg_strut_length(const float* ps, const float* pr, const float* shift) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float vx = pr[0] - ps[0] + shift[0];
  const float vy = pr[1] - ps[1] + shift[1];
  const float vz = pr[2] - ps[2] + shift[2];
  return sqrtf(fmaf(vz, vz, fmaf(vy, vy, vx * vx)));
}

// one directed edge's share of V = 1/2 sum r^2 L (the 1/2 is applied to the sum)
EELG_HD inline double eelg_strut_volume_term(float r, float len) { return ((double)r * (double)r) * (double)len; }

// both directions of a strut get the same value: fp32 addition commutes bitwise
EELG_HD inline float eelg_design_tied(const float* g_r, int e, int partner) {
  return partner != e ? g_r[e] + g_r[partner] : g_r[e];
}

EELG_HD inline float eelg_design_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// a group moves when its step size and its largest gradient entry are both non-zero
EELG_HD inline int eelg_design_moves(float step, float gmax) { return step != 0.f && gmax > 0.f; }

// m <- beta m + g / gmax;  x <- clamp(x - step m, lo, hi)
EELG_HD inline void eelg_design_move(float g, float gmax, float beta, float step, float lo, float hi, float* x,
                                     float* m) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float mn = beta * *m + g / gmax;
  *m = mn;
  *x = eelg_design_clamp(*x - step * mn, lo, hi);
}

// the volume-keeping factor sqrt(V0 / V); 1 where either volume is not a positive finite number
EELG_HD inline float eelg_design_scale(float v0, float v) {
  if (!(v0 > 0.f) || !(v > 0.f) || !eelg_design_finite(v0) || !eelg_design_finite(v)) return 1.f;
  return sqrtf(v0 / v);
}

EELG_HD inline float eelg_design_rescaled(float r, float scale, float r_min, float r_max) {
  return eelg_design_clamp(r * scale, r_min, r_max);
}

#ifndef __HIPCC__
// One graph on the host, every loop in index order: what one workgroup of design_step_kernel does.
// Arrays are the graph's own rows (n nodes, e edges) with send / recv / partner local to them.
// Returns the flag; *vol is the graph's volume afterwards (NaN with EELG_DESIGN_BAD_INDEX).
inline float eelg_design_graph_volume(const float* pos, const float* r, const float* shifts, const int* send,
                                      const int* recv, int e) {
  double v = 0.0;
  for (int k = 0; k < e; ++k)
    v += eelg_strut_volume_term(r[k], eelg_strut_length(pos + 3 * send[k], pos + 3 * recv[k], shifts + 3 * k));
  return (float)(0.5 * v);
}

inline int eelg_design_graph(const float* g_pos, const float* g_r, float* pos, float* r, const float* pos0,
                             float* m_pos, float* m_r, const int* partner, const float* shifts, const int* send,
                             const int* recv, int n, int e, float v0, const eelg_design_consts& k, float* vol) {
  for (int i = 0; i < e; ++i)
    if (send[i] < 0 || send[i] >= n || recv[i] < 0 || recv[i] >= n || partner[i] < 0 || partner[i] >= e) {
      *vol = NAN;
      return EELG_DESIGN_BAD_INDEX;
    }
  int bad = 0;
  float gr = 0.f, gp = 0.f;
  for (int i = 0; i < e; ++i) {
    const float t = eelg_design_tied(g_r, i, partner[i]);
    bad |= !eelg_design_finite(t);
    gr = fmaxf(gr, fabsf(t));
  }
  for (int i = 0; i < 3 * n; ++i) {
    bad |= !eelg_design_finite(g_pos[i]);
    gp = fmaxf(gp, fabsf(g_pos[i]));
  }
  if (bad) {
    *vol = eelg_design_graph_volume(pos, r, shifts, send, recv, e);
    return EELG_DESIGN_NONFINITE;
  }
  if (eelg_design_moves(k.step_pos, gp))
    for (int i = 0; i < 3 * n; ++i)
      eelg_design_move(g_pos[i], gp, k.beta, k.step_pos, pos0[i] - k.move_limit, pos0[i] + k.move_limit, pos + i,
                       m_pos + i);
  if (eelg_design_moves(k.step_r, gr))
    for (int i = 0; i < e; ++i)
      eelg_design_move(eelg_design_tied(g_r, i, partner[i]), gr, k.beta, k.step_r, k.r_min, k.r_max, r + i, m_r + i);
  float v = eelg_design_graph_volume(pos, r, shifts, send, recv, e);
  if (k.keep_volume) {
    const float scale = eelg_design_scale(v0, v);
    for (int i = 0; i < e; ++i) r[i] = eelg_design_rescaled(r[i], scale, k.r_min, k.r_max);
    v = eelg_design_graph_volume(pos, r, shifts, send, recv, e);
  }
  *vol = v;
  return 0;
}
#endif  // __HIPCC__

#endif  // EELG_DESIGN_H
