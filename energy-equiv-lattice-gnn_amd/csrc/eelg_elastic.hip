// Elastic properties of a batch of 6x6 Mandel stiffness matrices and their gradient, one launch
// each way: the Voigt / Reuss / Hill moduli, Poisson's ratio, the universal anisotropy index and
// the directional Young's modulus E(d) = 1 / (m(d)^T S m(d)) with its extremes over a set of
// directions.  The arithmetic of one matrix is csrc/eelg_elastic.h (fp64 inside, fp32 in and out).
//
// elastic_props_kernel: one wavefront (a 64-thread workgroup) per graph.
//  * every lane factorises the symmetric part of the graph's matrix (36 values read through
//    wave-uniform addresses), so the factorisation runs once per wave and S stays in registers;
//  * lanes take the directions lane, lane + 64, ...: E_p is stored as fp32 and each lane keeps the
//    (value, index) pair of its smallest and largest E; a fixed xor butterfly over the wave
//    compares pairs, the smaller index winning a tie, so E_min / E_max are the first extremes;
//  * lane 0 stores the property row and S (fp32), which the backward reads instead of factorising
//    again.
// elastic_props_bwd_kernel: one wavefront per graph.
//  * the extremes' indices are found again from the stored E_p by the same butterfly;
//  * each lane sums the 21 entries of sum_p w_p m m^T, w_p = -(g_p + [p = i_min] g_Emin +
//    [p = i_max] g_Emax) E_p^2, over its directions in direction order; the same butterfly adds
//    the lanes;
//  * every lane then holds G_S and forms -S G_S S plus the direct Voigt terms; lane 0 stores.
// No LDS, no scratch (every array index is a compile-time constant after unrolling), no atomics.
// Every sum has a fixed order that depends on n_dirs alone, so a graph's row and gradient are
// bitwise independent of n_graphs, of the graph's position in the batch and of the run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"
#include "eelg_elastic.h"

#define ELASTIC_NO_INDEX 0x7fffffff

// (value, index) pairs of the lanes' smallest and largest E reduced over the wave
__device__ __forceinline__ void elastic_extremes_wave(float& vmin, int& imin, float& vmax, int& imax) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(vmin, off, 64);
    const int oi = __shfl_xor(imin, off, 64);
    if (eelg_elastic_min_takes(vmin, imin, ov, oi)) { vmin = ov; imin = oi; }
    const float pv = __shfl_xor(vmax, off, 64);
    const int pi = __shfl_xor(imax, off, 64);
    if (eelg_elastic_max_takes(vmax, imax, pv, pi)) { vmax = pv; imax = pi; }
  }
}

__global__ __launch_bounds__(64) void elastic_props_kernel(
    const float* __restrict__ c, const float* __restrict__ dirs, int n_dirs, float* __restrict__ props,
    float* __restrict__ e_dir, float* __restrict__ s_out) {
  const size_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const float* __restrict__ cg = c + g * 36;
  float c32[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) c32[i] = cg[i];
  double a[21], s[21], sc[9];
  const int spd = eelg_elastic_invert(c32, a, s);
  eelg_elastic_scalars(a, s, spd, sc);

  float* __restrict__ eg = e_dir + g * (size_t)n_dirs;
  // the extremes are those of the fp32 values that are stored
  float vmin = INFINITY, vmax = -INFINITY;
  int imin = ELASTIC_NO_INDEX, imax = ELASTIC_NO_INDEX;
  for (int k = lane; k < n_dirs; k += 64) {
    const float e = eelg_elastic_young(s, dirs[(size_t)k * 3], dirs[(size_t)k * 3 + 1], dirs[(size_t)k * 3 + 2]);
    eg[k] = spd ? e : NAN;
    if (eelg_elastic_min_takes(vmin, imin, e, k)) { vmin = e; imin = k; }
    if (eelg_elastic_max_takes(vmax, imax, e, k)) { vmax = e; imax = k; }
  }
  elastic_extremes_wave(vmin, imin, vmax, imax);

  if (lane == 0) {
    float* __restrict__ o = props + g * EELG_ELASTIC_COLS;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = (float)sc[i];
    const bool have = spd && n_dirs > 0;
    o[EELG_EL_EMIN] = have ? vmin : NAN;
    o[EELG_EL_EMAX] = have ? vmax : NAN;
    o[EELG_EL_SPD] = spd ? 1.f : 0.f;
    float* __restrict__ so = s_out + g * 36;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j) so[6 * i + j] = spd ? (float)s[eelg_el_tri(i, j)] : NAN;
  }
}

__global__ __launch_bounds__(64) void elastic_props_bwd_kernel(
    const float* __restrict__ s, const float* __restrict__ dirs, const float* __restrict__ e_dir,
    const float* __restrict__ props, const float* __restrict__ g_props, const float* __restrict__ g_e_dir,
    int n_dirs, float* __restrict__ g_c) {
  const size_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const float* __restrict__ pg = props + g * EELG_ELASTIC_COLS;
  const float* __restrict__ gp = g_props + g * EELG_ELASTIC_COLS;
  float p32[EELG_ELASTIC_COLS], g32[EELG_ELASTIC_COLS], s32[36];
#pragma unroll
  for (int i = 0; i < EELG_ELASTIC_COLS; ++i) {
    p32[i] = pg[i];
    g32[i] = gp[i];
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) s32[i] = s[g * 36 + i];
  const int spd = p32[EELG_EL_SPD] == 1.f;

  double acc[21];
#pragma unroll
  for (int i = 0; i < 21; ++i) acc[i] = 0.0;
  if (spd && n_dirs > 0) {            // wave-uniform
    const float* __restrict__ eg = e_dir + g * (size_t)n_dirs;
    float vmin = INFINITY, vmax = -INFINITY;
    int imin = ELASTIC_NO_INDEX, imax = ELASTIC_NO_INDEX;
    for (int k = lane; k < n_dirs; k += 64) {
      const float e = eg[k];
      if (eelg_elastic_min_takes(vmin, imin, e, k)) { vmin = e; imin = k; }
      if (eelg_elastic_max_takes(vmax, imax, e, k)) { vmax = e; imax = k; }
    }
    elastic_extremes_wave(vmin, imin, vmax, imax);
    const double gmin = g32[EELG_EL_EMIN], gmax = g32[EELG_EL_EMAX];
    for (int k = lane; k < n_dirs; k += 64) {
      double w = g_e_dir ? (double)g_e_dir[g * (size_t)n_dirs + k] : 0.0;
      if (k == imin) w += gmin;
      if (k == imax) w += gmax;
      const double e = eg[k];
      double m[6];
      eelg_elastic_mandel(dirs[(size_t)k * 3], dirs[(size_t)k * 3 + 1], dirs[(size_t)k * 3 + 2], m);
      eelg_elastic_outer_acc(acc, -(w * (e * e)), m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < 21; ++i) acc[i] += __shfl_xor(acc[i], off, 64);
  }
  double gs[3], gc[3];
  eelg_elastic_scalars_bwd(p32, g32, spd, gs, gc);
  float out[36];
  eelg_elastic_grad_c(s32, acc, gs, gc, spd, out);
  if (lane == 0) {
    float* __restrict__ o = g_c + g * 36;
#pragma unroll
    for (int i = 0; i < 36; ++i) o[i] = out[i];
  }
}

extern "C" {

int eelg_elastic_props(const float* c, const float* dirs, int n_graphs, int n_dirs, float* props,
                       float* e_dir, float* s, void* stream) {
  if (n_graphs < 0) return eelg_fail(-2, "elastic_props: %d graphs", n_graphs);
  if (n_graphs == 0) return 0;
  if (n_dirs < 0) return eelg_fail(-2, "elastic_props: %d directions (at least 0)", n_dirs);
  if (!c || !props || !s) return eelg_fail(-2, "elastic_props: null pointer (c, props, s)");
  if (n_dirs > 0 && (!dirs || !e_dir))
    return eelg_fail(-2, "elastic_props: null pointer (dirs, e_dir) with %d directions", n_dirs);
  hipLaunchKernelGGL(elastic_props_kernel, dim3((unsigned)n_graphs), dim3(64), 0, (hipStream_t)stream, c, dirs,
                     n_dirs, props, e_dir, s);
  return eelg_check_launch("elastic_props");
}

int eelg_elastic_props_bwd(const float* s, const float* dirs, const float* e_dir, const float* props,
                           const float* g_props, const float* g_e_dir, int n_graphs, int n_dirs, float* g_c,
                           void* stream) {
  if (n_graphs < 0) return eelg_fail(-2, "elastic_props_bwd: %d graphs", n_graphs);
  if (n_graphs == 0) return 0;
  if (n_dirs < 0) return eelg_fail(-2, "elastic_props_bwd: %d directions (at least 0)", n_dirs);
  if (!s || !props || !g_props || !g_c)
    return eelg_fail(-2, "elastic_props_bwd: null pointer (s, props, g_props, g_c)");
  if (n_dirs > 0 && (!dirs || !e_dir))
    return eelg_fail(-2, "elastic_props_bwd: null pointer (dirs, e_dir) with %d directions", n_dirs);
  hipLaunchKernelGGL(elastic_props_bwd_kernel, dim3((unsigned)n_graphs), dim3(64), 0, (hipStream_t)stream, s,
                     dirs, e_dir, props, g_props, g_e_dir, n_dirs, g_c);
  return eelg_check_launch("elastic_props_bwd");
}

}  // extern "C"
