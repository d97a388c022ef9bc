// Validation / test metrics of a batch of predicted stiffness matrices in one launch: what
// LightningWrappedModel.validation_step (scripts/train_utils.py:66-89) and obtain_errors
// (scripts/train_utils.py:149-171) compute per graph with stiffness_Mandel_to_cart_4, two
// einsums over [B, 3, 3, 3, 3] and two torch.linalg.eigvalsh calls.
//
// stiffness_metrics_kernel: one wavefront (a 64-thread workgroup) per graph.
//  * entrywise errors: lane i < 36 takes entry i of both matrices; squared and absolute
//    differences are summed by a fixed xor butterfly over the wave.
//  * directional stiffness: every lane holds both scaled matrices in registers (36 + 36 values
//    read through wave-uniform addresses) and takes directions lane, lane + 64, ...:
//    c = v^T C v with v = (d1^2, d2^2, d3^2, r2 d2 d3, r2 d1 d3, r2 d1 d2), rows contracted in
//    index order with fmaf; the rank-4 tensor is never formed.  |c - c^| and c are summed per
//    lane in direction order, then by the same butterfly.
//  * eigenvalues: eelg_jacobi6 (eelg_jacobi.h) once per wave: even lanes run it on the target,
//    odd lanes on the prediction (a per-entry select, no divergence); lane 0 and lane 1 store.
// No LDS, no scratch (every array index is a compile-time constant after unrolling), no atomics.
// Every sum has a fixed order that depends on n_dirs alone, so a graph's row is bitwise
// independent of n_graphs and of the graph's position in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"
#include "eelg_jacobi.h"

__device__ __forceinline__ float metrics_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// v^T C v, rows in index order
__device__ __forceinline__ float metrics_quad(const float (&c)[36], const float (&v)[6]) {
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    float row = c[6 * a] * v[0];
#pragma unroll
    for (int b = 1; b < 6; ++b) row = fmaf(c[6 * a + b], v[b], row);
    acc = a == 0 ? v[0] * row : fmaf(v[a], row, acc);
  }
  return acc;
}

__global__ __launch_bounds__(64) void stiffness_metrics_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ dirs,
    int n_dirs, float scale, float* __restrict__ out) {
  const size_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const float* __restrict__ pg = pred + g * 36;
  const float* __restrict__ tg = target + g * 36;
  // the products are rounded before anything is subtracted (10 * C as a tensor of its own)
  float p[36], t[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) {
    p[i] = __fmul_rn(pg[i], scale);
    t[i] = __fmul_rn(tg[i], scale);
  }
  float sq = 0.f, ab = 0.f;
  if (lane < 36) {
    const float df = __fsub_rn(__fmul_rn(pg[lane], scale), __fmul_rn(tg[lane], scale));
    sq = df * df;
    ab = fabsf(df);
  }
  float sdir = 0.f, smean = 0.f;
  const float r2 = 1.41421356237309504880f;
  for (int k = lane; k < n_dirs; k += 64) {
    const float d1 = dirs[(size_t)k * 3], d2 = dirs[(size_t)k * 3 + 1], d3 = dirs[(size_t)k * 3 + 2];
    const float v[6] = {d1 * d1, d2 * d2, d3 * d3, r2 * (d2 * d3), r2 * (d1 * d3), r2 * (d1 * d2)};
    const float ct = metrics_quad(t, v), cp = metrics_quad(p, v);
    sdir += fabsf(ct - cp);
    smean += ct;
  }
  sq = metrics_wave_sum(sq);
  ab = metrics_wave_sum(ab);
  sdir = metrics_wave_sum(sdir);
  smean = metrics_wave_sum(smean);

  const bool odd = lane & 1;
  float m[36], e[6];
#pragma unroll
  for (int i = 0; i < 36; ++i) m[i] = odd ? p[i] : t[i];
  eelg_jacobi6(m, e);

  float* __restrict__ o = out + g * EELG_METRICS_COLS;
  if (lane == 0) {
    o[0] = sq / 36.f;
    o[1] = ab / 36.f;
    o[2] = sdir / (float)n_dirs;
    o[3] = smean / (float)n_dirs;
#pragma unroll
    for (int i = 0; i < 6; ++i) o[4 + i] = e[i];
  } else if (lane == 1) {
#pragma unroll
    for (int i = 0; i < 6; ++i) o[10 + i] = e[i];
  }
}

extern "C" {

int eelg_stiffness_metrics(const float* pred, const float* target, const float* dirs, int n_graphs,
                           int n_dirs, float scale, float* out, void* stream) {
  if (n_graphs < 0) return eelg_fail(-2, "stiffness_metrics: %d graphs", n_graphs);
  if (n_graphs == 0) return 0;
  if (n_dirs <= 0) return eelg_fail(-2, "stiffness_metrics: %d directions (at least 1)", n_dirs);
  if (!pred || !target || !dirs || !out)
    return eelg_fail(-2, "stiffness_metrics: null pointer (pred, target, dirs, out)");
  hipLaunchKernelGGL(stiffness_metrics_kernel, dim3((unsigned)n_graphs), dim3(64), 0, (hipStream_t)stream,
                     pred, target, dirs, n_dirs, scale, out);
  return eelg_check_launch("stiffness_metrics");
}

}  // extern "C"
