// Shear, Poisson's ratio and compressibility surfaces of a batch of 6x6 Mandel stiffness matrices
// and their gradient, one launch each way: per direction d the extremes over the transverse circle
// of G(d, n) and nu(d, n) in closed form and beta(d), and their extremes over a set of directions.
// The arithmetic of one matrix and one direction is csrc/eelg_transverse.h (fp64 inside, fp32 out).
//
// transverse_props_kernel: one wavefront (a 64-thread workgroup) per graph.
//  * every lane factorises the symmetric part of the graph's matrix (wave-uniform loads), so S stays
//    in registers as 21 packed fp64;
//  * lanes take the directions lane, lane + 64, ...: the five values of a direction are stored as
//    fp32 and each lane keeps the (value, index) pair of its six extremes; a fixed xor butterfly over
//    the wave compares pairs, the smaller index winning a tie, so the extremes are first extremes;
//  * lane 0 stores the property row, the six indices, the transverse vectors of the four G / nu
//    extremes and S (fp64, which the backward reads instead of factorising again).
// transverse_props_bwd_kernel: one wavefront per graph.
//  * each lane sums the 21 entries of G_S over its directions in direction order, the cotangent of
//    an extreme added to the direction the forward named; the butterfly adds the lanes;
//  * every lane then forms -S G_S S; lane 0 stores.  A graph with spd == 0 stores zeros.
// No LDS, no scratch (every array index is a compile-time constant after unrolling), no atomics.
// Every sum has a fixed order that depends on n_dirs alone, so a graph's rows and gradient are
// bitwise independent of n_graphs, of the graph's position in the batch and of the run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"
#include "eelg_transverse.h"

#define TRANSVERSE_NO_INDEX 0x7fffffff

// column of a direction's row whose extreme is column i of a property row
__device__ __forceinline__ constexpr int transverse_source(int i) { return i < 4 ? i : EELG_TV_BETA; }

__global__ __launch_bounds__(64) void transverse_props_kernel(
    const float* __restrict__ c, const float* __restrict__ dirs, int n_dirs, float* __restrict__ props,
    float* __restrict__ t_dir, int* __restrict__ arg, float* __restrict__ n_ext, double* __restrict__ s_out) {
  const size_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const float* __restrict__ cg = c + g * 36;
  float c32[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) c32[i] = cg[i];
  double a[21], s[21];
  const int spd = eelg_elastic_invert(c32, a, s);

  float* __restrict__ tg = t_dir + g * (size_t)n_dirs * EELG_TRANSVERSE_DIR_COLS;
  // the extremes are those of the fp32 values that are stored; even columns minima, odd maxima
  float ext[6];
  int idx[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    ext[i] = (i & 1) ? -INFINITY : INFINITY;
    idx[i] = TRANSVERSE_NO_INDEX;
  }
  for (int k = lane; k < n_dirs; k += 64) {
    eelg_tv_dir q;
    eelg_tv_direction(s, dirs[(size_t)k * 3], dirs[(size_t)k * 3 + 1], dirs[(size_t)k * 3 + 2], q);
    double v64[EELG_TRANSVERSE_DIR_COLS];
    eelg_tv_values(q, v64);
    float v[EELG_TRANSVERSE_DIR_COLS];
#pragma unroll
    for (int i = 0; i < EELG_TRANSVERSE_DIR_COLS; ++i) {
      v[i] = (float)v64[i];
      tg[(size_t)k * EELG_TRANSVERSE_DIR_COLS + i] = spd ? v[i] : NAN;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const float x = v[transverse_source(i)];
      const bool takes = (i & 1) ? eelg_elastic_max_takes(ext[i], idx[i], x, k)
                                 : eelg_elastic_min_takes(ext[i], idx[i], x, k);
      if (takes) { ext[i] = x; idx[i] = k; }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const float ov = __shfl_xor(ext[i], off, 64);
      const int oi = __shfl_xor(idx[i], off, 64);
      const bool takes = (i & 1) ? eelg_elastic_max_takes(ext[i], idx[i], ov, oi)
                                 : eelg_elastic_min_takes(ext[i], idx[i], ov, oi);
      if (takes) { ext[i] = ov; idx[i] = oi; }
    }

  if (lane == 0) {
    float* __restrict__ o = props + g * EELG_TRANSVERSE_COLS;
    int* __restrict__ ao = arg + g * 6;
    float* __restrict__ no = n_ext + g * 12;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      // an index outside [0, n_dirs): no direction, or none whose value is a number
      const bool have = spd && idx[i] >= 0 && idx[i] < n_dirs;
      o[i] = have ? ext[i] : NAN;
      ao[i] = have ? idx[i] : -1;
      if (i < 4) {
        float n[3] = {NAN, NAN, NAN};
        if (have) {
          const size_t k = (size_t)idx[i];
          eelg_tv_dir q;
          eelg_tv_direction(s, dirs[k * 3], dirs[k * 3 + 1], dirs[k * 3 + 2], q);
          eelg_tv_normal(q, i, n);
        }
        no[3 * i] = n[0];
        no[3 * i + 1] = n[1];
        no[3 * i + 2] = n[2];
      }
    }
    o[EELG_TV_SPD] = spd ? 1.f : 0.f;
    double* __restrict__ so = s_out + g * 21;
#pragma unroll
    for (int i = 0; i < 21; ++i) so[i] = spd ? s[i] : (double)NAN;
  }
}

__global__ __launch_bounds__(64) void transverse_props_bwd_kernel(
    const double* __restrict__ s64, const float* __restrict__ dirs, const float* __restrict__ props,
    const int* __restrict__ arg, const float* __restrict__ g_props, const float* __restrict__ g_t_dir, int n_dirs,
    float* __restrict__ g_c) {
  const size_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int spd = props[g * EELG_TRANSVERSE_COLS + EELG_TV_SPD] == 1.f;      // wave-uniform
  float out[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) out[i] = 0.f;
  if (spd) {
    double s[21], acc[21];
#pragma unroll
    for (int i = 0; i < 21; ++i) {
      s[i] = s64[g * 21 + i];
      acc[i] = 0.0;
    }
    int at[6];
    double gx[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      at[i] = arg[g * 6 + i];
      // the cotangent of an extreme that no direction took (NaN) is not read
      gx[i] = at[i] >= 0 ? (double)g_props[g * EELG_TRANSVERSE_COLS + i] : 0.0;
    }
    for (int k = lane; k < n_dirs; k += 64) {
      double w[EELG_TRANSVERSE_DIR_COLS];
#pragma unroll
      for (int i = 0; i < EELG_TRANSVERSE_DIR_COLS; ++i)
        w[i] = g_t_dir ? (double)g_t_dir[(g * (size_t)n_dirs + k) * EELG_TRANSVERSE_DIR_COLS + i] : 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i)
        if (k == at[i]) w[transverse_source(i)] += gx[i];
      eelg_tv_dir q;
      eelg_tv_direction(s, dirs[(size_t)k * 3], dirs[(size_t)k * 3 + 1], dirs[(size_t)k * 3 + 2], q);
      eelg_tv_direction_bwd(q, w, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < 21; ++i) acc[i] += __shfl_xor(acc[i], off, 64);
    eelg_tv_grad_c(s, acc, out);
  }
  if (lane == 0) {
    float* __restrict__ o = g_c + g * 36;
#pragma unroll
    for (int i = 0; i < 36; ++i) o[i] = out[i];
  }
}

extern "C" {

int eelg_transverse_props(const float* c, const float* dirs, int n_graphs, int n_dirs, float* props,
                          float* t_dir, int* arg, float* n_ext, double* s, void* stream) {
  if (n_graphs < 0) return eelg_fail(-2, "transverse_props: %d graphs", n_graphs);
  if (n_graphs == 0) return 0;
  if (n_dirs < 0) return eelg_fail(-2, "transverse_props: %d directions (at least 0)", n_dirs);
  if (!c || !props || !arg || !n_ext || !s)
    return eelg_fail(-2, "transverse_props: null pointer (c, props, arg, n_ext, s)");
  if ((uintptr_t)s % sizeof(double)) return eelg_fail(-2, "transverse_props: s is not aligned to 8 bytes");
  if (n_dirs > 0 && (!dirs || !t_dir))
    return eelg_fail(-2, "transverse_props: null pointer (dirs, t_dir) with %d directions", n_dirs);
  hipLaunchKernelGGL(transverse_props_kernel, dim3((unsigned)n_graphs), dim3(64), 0, (hipStream_t)stream, c, dirs,
                     n_dirs, props, t_dir, arg, n_ext, s);
  return eelg_check_launch("transverse_props");
}

int eelg_transverse_props_bwd(const double* s, const float* dirs, const float* props, const int* arg,
                              const float* g_props, const float* g_t_dir, int n_graphs, int n_dirs, float* g_c,
                              void* stream) {
  if (n_graphs < 0) return eelg_fail(-2, "transverse_props_bwd: %d graphs", n_graphs);
  if (n_graphs == 0) return 0;
  if (n_dirs < 0) return eelg_fail(-2, "transverse_props_bwd: %d directions (at least 0)", n_dirs);
  if (!s || !props || !arg || !g_props || !g_c)
    return eelg_fail(-2, "transverse_props_bwd: null pointer (s, props, arg, g_props, g_c)");
  if ((uintptr_t)s % sizeof(double)) return eelg_fail(-2, "transverse_props_bwd: s is not aligned to 8 bytes");
  if (n_dirs > 0 && !dirs)
    return eelg_fail(-2, "transverse_props_bwd: null pointer (dirs) with %d directions", n_dirs);
  hipLaunchKernelGGL(transverse_props_bwd_kernel, dim3((unsigned)n_graphs), dim3(64), 0, (hipStream_t)stream, s,
                     dirs, props, arg, g_props, g_t_dir, n_dirs, g_c);
  return eelg_check_launch("transverse_props_bwd");
}

}  // extern "C"
