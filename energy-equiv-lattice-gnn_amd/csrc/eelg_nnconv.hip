// Edge-conditioned convolution of the NNConv benchmark model (PyG NNConv, aggr='add',
// root_weight=False; scripts/benchmark_models/nnconv_models.py:32-44):
//   Z[e,i,o] = sum_k h[e,k] W3[i*D+o, k] + b3[i*D+o]      (the edge MLP's last Linear, viewed [D, D])
//   msg[e,o] = sum_i x[sender(e), i] relu(Z[e,i,o])
// h [E, D] is the edge MLP's second hidden activation.  The [E, D*D] tensor Z (and relu(Z), and
// its gradient) is never formed: per input channel i the D x D block W3_i = W3[i*D:(i+1)*D, :]
// is one operand of a (32 edges) x D x D product on v_mfma_f32_32x32x2_f32 (exact fp32 products)
// whose result lives in the accumulator registers only.
//
// Fragment convention (32x32x2, as eelg_radial.hip): lane l = 32*hf + j supplies A[row j][k] and
// B[k][col j] of the step's k; the two lane halves take different k of the step (a sum over k, so
// any split of K shared by A and B is exact up to rounding order).  C/D: acc[r] is row
// nnc_row(r, hf) = (r&3) + 8*(r>>2) + 4*hf, column j.  A C-layout register therefore is directly
// an A (or B) operand of a following product whose K index is the C row: step r, half hf takes
// k = nnc_row(r, hf).  Both backward kernels use this, so no tile is transposed through LDS.
//
// nnconv_fwd / nnconv_bwd_edge ("lane = edge"): a wave owns 32 edges, a workgroup 4 waves = 128
// edges.  The h rows of the wave's edges are the B operand, held in registers over the whole i
// loop; the W3_i rows are the A operand, streamed from L2 (every wave reads all of W3 once per 32
// edges; the 4 waves of a workgroup walk i together and share the lines in L1):
//   Zt[o, e] = sum_k W3_i[o,k] h[e,k]      C: row o (registers), column e (lane)
// so everything per edge (x[sender, i], the message / gradient rows) is per lane.  x[sender] is
// staged once per tile in LDS, transposed ([i][edge]: one conflict-free read per i).
//   fwd     : m[e,o] += relu(Zt) x_i; stores msg rows as 16-byte pieces.
//   bwd_edge: g = grad_agg[recv(e)] in C layout; gxe[e,i] = sum_o relu(Z) g (register sum + one
//             cross-half add); dZt = [Z>0] x_i g is the B operand (K = o) of
//             grad_h^T[k', e] += sum_o W3_i[o,k'] dZt[o,e], accumulated over i in registers.
// nnconv_bwd_w ("lane = o"): one wave owns the 32 output rows (i, o-tile) of grad W3 / grad b3 over
// a fixed range of edge tiles.  Z[e, o] = h W3_i^T with the W3 rows held in registers; dZ (C
// layout, row e) is the A operand (K = e) of grad W3_i[o, k'] += sum_e dZ[e,o] h[e,k'].  The
// partial of every edge split is written whole; the caller sums them (eelg_sum_rows).
//
// In all three kernels Z is bias + the same MFMA chain over the same k order, so the ReLU mask
// of the backward is the forward's.  No atomics; every sum has a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"

typedef float nnc_f32x16 __attribute__((ext_vector_type(16)));

#define NNC_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int nnc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

__device__ __forceinline__ float4 nnc_ld4(const float* __restrict__ p, size_t idx, bool ok) {
  const float4 v = *reinterpret_cast<const float4*>(p + (ok ? idx : 0));
  return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}

// x[sender(e)] of the wave's 32 edges into xs[c][j] (lane (j, hf) copies the channels of its half)
template <int D>
__device__ __forceinline__ void nnc_stage_x(const float* __restrict__ x, int s, bool ok, int j, int hf,
                                            float (*xs)[32]) {
  constexpr int KH = D / 2;
#pragma unroll
  for (int c = 0; c < KH; c += 4) {
    const float4 v = nnc_ld4(x, (size_t)s * D + hf * KH + c, ok);
    xs[hf * KH + c + 0][j] = v.x;
    xs[hf * KH + c + 1][j] = v.y;
    xs[hf * KH + c + 2][j] = v.z;
    xs[hf * KH + c + 3][j] = v.w;
  }
}

// Zt tile: acc[r] = b3[i*D + ot*32 + row(r)] + sum_k W3[(i*D + ot*32 + row(r)), k] h[e_j, k]
template <int D>
__device__ __forceinline__ nnc_f32x16 nnc_zt(const float* __restrict__ w3, const float* __restrict__ b3,
                                             int i, int ot, int j, int hf, const float* hb) {
  constexpr int KH = D / 2;
  nnc_f32x16 acc;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 b = *reinterpret_cast<const float4*>(b3 + i * D + ot * 32 + 8 * q + 4 * hf);
    acc[4 * q + 0] = b.x;
    acc[4 * q + 1] = b.y;
    acc[4 * q + 2] = b.z;
    acc[4 * q + 3] = b.w;
  }
  const float* __restrict__ wr = w3 + (size_t)(i * D + ot * 32 + j) * D + hf * KH;
#pragma unroll
  for (int st = 0; st < KH; st += 4) {
    const float4 w = *reinterpret_cast<const float4*>(wr + st);
    acc = NNC_MFMA(w.x, hb[st + 0], acc);
    acc = NNC_MFMA(w.y, hb[st + 1], acc);
    acc = NNC_MFMA(w.z, hb[st + 2], acc);
    acc = NNC_MFMA(w.w, hb[st + 3], acc);
  }
  return acc;
}

template <int D>
__global__ __launch_bounds__(256) void nnconv_fwd_kernel(const float* __restrict__ x,
                                                         const float* __restrict__ h,
                                                         const float* __restrict__ w3,
                                                         const float* __restrict__ b3,
                                                         const int* __restrict__ sender, int n_edges,
                                                         float* __restrict__ msg) {
  constexpr int NT = D / 32, KH = D / 2;
  __shared__ float xs[4][D][32];
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 31, hf = l >> 5;
  const int e0 = (blockIdx.x * 4 + wave) * 32, e = e0 + j;
  const bool ok = e < n_edges;
  nnc_stage_x<D>(x, ok ? sender[e] : 0, ok, j, hf, xs[wave]);
  float hb[KH];
#pragma unroll
  for (int st = 0; st < KH; st += 4) {
    const float4 v = nnc_ld4(h, (size_t)e * D + hf * KH + st, ok);
    hb[st] = v.x, hb[st + 1] = v.y, hb[st + 2] = v.z, hb[st + 3] = v.w;
  }
  __syncthreads();
  if (e0 >= n_edges) return;   // wave-uniform, after the only barrier
  nnc_f32x16 m[NT];
#pragma unroll
  for (int ot = 0; ot < NT; ++ot)
#pragma unroll
    for (int r = 0; r < 16; ++r) m[ot][r] = 0.f;
  for (int i = 0; i < D; ++i) {
    const float xi = xs[wave][i][j];
#pragma unroll
    for (int ot = 0; ot < NT; ++ot) {
      const nnc_f32x16 z = nnc_zt<D>(w3, b3, i, ot, j, hf, hb);
#pragma unroll
      for (int r = 0; r < 16; ++r) m[ot][r] = fmaf(fmaxf(z[r], 0.f), xi, m[ot][r]);
    }
  }
  if (ok) {
#pragma unroll
    for (int ot = 0; ot < NT; ++ot)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(msg + (size_t)e * D + ot * 32 + 8 * q + 4 * hf) =
            make_float4(m[ot][4 * q], m[ot][4 * q + 1], m[ot][4 * q + 2], m[ot][4 * q + 3]);
  }
}

template <int D>
__global__ __launch_bounds__(256) void nnconv_bwd_edge_kernel(
    const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ w3,
    const float* __restrict__ b3, const int* __restrict__ sender, const int* __restrict__ receiver,
    int n_edges, const float* __restrict__ grad_agg, float* __restrict__ gxe,
    float* __restrict__ grad_h) {
  constexpr int NT = D / 32, KH = D / 2;
  // x[sender] of the tile; row i is overwritten by gxe[:, i] once iteration i has read it
  __shared__ float xs[4][D][32];
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, j = l & 31, hf = l >> 5;
  const int e0 = (blockIdx.x * 4 + wave) * 32, e = e0 + j;
  const bool ok = e < n_edges;
  nnc_stage_x<D>(x, ok ? sender[e] : 0, ok, j, hf, xs[wave]);
  float hb[KH];
#pragma unroll
  for (int st = 0; st < KH; st += 4) {
    const float4 v = nnc_ld4(h, (size_t)e * D + hf * KH + st, ok);
    hb[st] = v.x, hb[st + 1] = v.y, hb[st + 2] = v.z, hb[st + 3] = v.w;
  }
  // g[e_j, o] in C layout (row o = ot*32 + nnc_row(r, hf)); zero rows for the masked edges
  nnc_f32x16 g[NT];
  {
    const int rc = ok ? receiver[e] : 0;
#pragma unroll
    for (int ot = 0; ot < NT; ++ot)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = nnc_ld4(grad_agg, (size_t)rc * D + ot * 32 + 8 * q + 4 * hf, ok);
        g[ot][4 * q] = v.x, g[ot][4 * q + 1] = v.y, g[ot][4 * q + 2] = v.z, g[ot][4 * q + 3] = v.w;
      }
  }
  __syncthreads();
  if (e0 >= n_edges) return;   // wave-uniform, after the only workgroup barrier
  nnc_f32x16 gh[NT];
#pragma unroll
  for (int c2 = 0; c2 < NT; ++c2)
#pragma unroll
    for (int r = 0; r < 16; ++r) gh[c2][r] = 0.f;
  for (int i = 0; i < D; ++i) {
    const float xi = xs[wave][i][j];
    float p = 0.f;
#pragma unroll
    for (int ot = 0; ot < NT; ++ot) {
      const nnc_f32x16 z = nnc_zt<D>(w3, b3, i, ot, j, hf, hb);
      float dz[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool pos = z[r] > 0.f;
        p = pos ? fmaf(z[r], g[ot][r], p) : p;
        dz[r] = pos ? xi * g[ot][r] : 0.f;
      }
      // grad_h^T[k', e] += sum_o W3_i[o, k'] dZt[o, e]; step r of half hf: o = ot*32 + row(r, hf)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* __restrict__ wr = w3 + (size_t)(i * D + ot * 32 + nnc_row(r, hf)) * D + j;
#pragma unroll
        for (int c2 = 0; c2 < NT; ++c2) gh[c2] = NNC_MFMA(wr[c2 * 32], dz[r], gh[c2]);
      }
    }
    p += __shfl_xor(p, 32);
    // both halves have read xs[i][j] (one LDS instruction, issued before this store)
    if (hf == 0) xs[wave][i][j] = p;
  }
  __builtin_amdgcn_wave_barrier();
  if (ok) {
#pragma unroll
    for (int c = 0; c < KH; c += 4)
      *reinterpret_cast<float4*>(gxe + (size_t)e * D + hf * KH + c) =
          make_float4(xs[wave][hf * KH + c][j], xs[wave][hf * KH + c + 1][j],
                      xs[wave][hf * KH + c + 2][j], xs[wave][hf * KH + c + 3][j]);
#pragma unroll
    for (int c2 = 0; c2 < NT; ++c2)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(grad_h + (size_t)e * D + c2 * 32 + 8 * q + 4 * hf) =
            make_float4(gh[c2][4 * q], gh[c2][4 * q + 1], gh[c2][4 * q + 2], gh[c2][4 * q + 3]);
  }
}

// grid (D * D/32 output row tiles, edge splits), one wave per workgroup
template <int D>
__global__ __launch_bounds__(64) void nnconv_bwd_w_kernel(
    const float* __restrict__ x, const float* __restrict__ h, const float* __restrict__ w3,
    const float* __restrict__ b3, const int* __restrict__ sender, const int* __restrict__ receiver,
    int n_edges, const float* __restrict__ grad_agg, int tiles_per_split, float* __restrict__ part) {
  constexpr int NT = D / 32, KH = D / 2;
  const int l = threadIdx.x & 63, j = l & 31, hf = l >> 5;
  const int i = blockIdx.x / NT, ot = blockIdx.x - i * NT;
  const int n_tiles = (n_edges + 31) >> 5;
  const int t0 = blockIdx.y * tiles_per_split;
  const int t1 = min(t0 + tiles_per_split, n_tiles);
  // B of the Z product: W3[(i*D + ot*32 + j), k], k = hf*KH + st
  float wb[KH];
  {
    const float* __restrict__ wr = w3 + (size_t)(i * D + ot * 32 + j) * D + hf * KH;
#pragma unroll
    for (int st = 0; st < KH; st += 4) {
      const float4 v = *reinterpret_cast<const float4*>(wr + st);
      wb[st] = v.x, wb[st + 1] = v.y, wb[st + 2] = v.z, wb[st + 3] = v.w;
    }
  }
  const float bias = b3[i * D + ot * 32 + j];
  nnc_f32x16 gw[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) gw[kt][r] = 0.f;
  float db = 0.f;
  // the next tile's h rows (A of the Z product) and edge indices are loaded one tile ahead, so the
  // gathers that depend on the indices issue at the top of a tile and overlap its Z product
  float4 hv[KH / 4];
  int sn[16], rc[16];
  auto load_tile = [&](int t) {
    const int e0 = t * 32;
    const bool okj = e0 + j < n_edges;
#pragma unroll
    for (int st = 0; st < KH; st += 4) hv[st / 4] = nnc_ld4(h, (size_t)(e0 + j) * D + hf * KH + st, okj);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int e = e0 + nnc_row(r, hf);
      const int ec = e < n_edges ? e : 0;
      sn[r] = sender[ec];
      rc[r] = receiver[ec];
    }
  };
  if (t0 < t1) load_tile(t0);
  for (int t = t0; t < t1; ++t) {
    const int e0 = t * 32;
    float4 hc[KH / 4];
    float xv[16], gv[16], hr[16][NT];
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) hc[q] = hv[q];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int e = e0 + nnc_row(r, hf);
      const bool ok = e < n_edges;
      const float* __restrict__ hrow = h + (size_t)(ok ? e : 0) * D + j;
      xv[r] = ok ? x[(size_t)sn[r] * D + i] : 0.f;
      gv[r] = grad_agg[(size_t)rc[r] * D + ot * 32 + j];
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) hr[r][kt] = ok ? hrow[kt * 32] : 0.f;
    }
    if (t + 1 < t1) load_tile(t + 1);
    nnc_f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = bias;
#pragma unroll
    for (int q = 0; q < KH / 4; ++q) {
      z = NNC_MFMA(hc[q].x, wb[4 * q + 0], z);
      z = NNC_MFMA(hc[q].y, wb[4 * q + 1], z);
      z = NNC_MFMA(hc[q].z, wb[4 * q + 2], z);
      z = NNC_MFMA(hc[q].w, wb[4 * q + 3], z);
    }
    // dZ[e, o = ot*32 + j] for e = e0 + row(r, hf): the A operand (K = e) of the second product
    // (x = 0 and h = 0 for the rows past the last edge)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float dz = z[r] > 0.f ? xv[r] * gv[r] : 0.f;
      db += dz;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) gw[kt] = NNC_MFMA(dz, hr[r][kt], gw[kt]);
    }
  }
  float* __restrict__ pb = part + (size_t)blockIdx.y * ((size_t)D * D * (D + 1));
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      pb[(size_t)(i * D + ot * 32 + nnc_row(r, hf)) * D + kt * 32 + j] = gw[kt][r];
  db += __shfl_xor(db, 32);
  if (hf == 0) pb[(size_t)D * D * D + i * D + ot * 32 + j] = db;
}

static bool nnc_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// edge tiles of 32 per split of the weight gradient: at least NNC_MIN_TILES, and at most
// NNC_MAX_PARTS splits (eelg.h)
#define NNC_MIN_TILES 32
static int nnc_tiles_per_split(int n_edges, int D) {
  const int n_tiles = (n_edges + 31) / 32;
  const int max_parts = D == 32 ? EELG_NNC_MAXPARTS_32 : EELG_NNC_MAXPARTS_64;
  const int tps = (n_tiles + max_parts - 1) / max_parts;
  return tps > NNC_MIN_TILES ? tps : NNC_MIN_TILES;
}

extern "C" {

int eelg_nnconv_bwd_w_parts(int n_edges, int D) {
  if (D != 32 && D != 64) return eelg_fail(-2, "nnconv_bwd_w_parts: D = %d (built: 32, 64)", D);
  if (n_edges <= 0) return 0;
  const int n_tiles = (n_edges + 31) / 32, tps = nnc_tiles_per_split(n_edges, D);
  return (n_tiles + tps - 1) / tps;
}

int eelg_nnconv_fwd(const float* x, const float* h, const float* w3, const float* b3,
                    const int* sender, int n_edges, int D, float* msg, void* stream) {
  if (D != 32 && D != 64) return eelg_fail(-2, "nnconv_fwd: D = %d (built: 32, 64)", D);
  if (n_edges < 0) return eelg_fail(-2, "nnconv_fwd: n_edges %d", n_edges);
  if (n_edges == 0) return 0;
  if (!nnc_aligned(x) || !nnc_aligned(h) || !nnc_aligned(w3) || !nnc_aligned(b3) || !nnc_aligned(msg))
    return eelg_fail(-2, "nnconv_fwd: x, h, w3, b3 and msg must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((n_edges + 127) / 128), block(256);
  if (D == 32)
    hipLaunchKernelGGL(nnconv_fwd_kernel<32>, grid, block, 0, s, x, h, w3, b3, sender, n_edges, msg);
  else
    hipLaunchKernelGGL(nnconv_fwd_kernel<64>, grid, block, 0, s, x, h, w3, b3, sender, n_edges, msg);
  return eelg_check_launch("nnconv_fwd");
}

int eelg_nnconv_bwd_edge(const float* x, const float* h, const float* w3, const float* b3,
                         const int* sender, const int* receiver, int n_edges, int D,
                         const float* grad_agg, float* gxe, float* grad_h, void* stream) {
  if (D != 32 && D != 64) return eelg_fail(-2, "nnconv_bwd_edge: D = %d (built: 32, 64)", D);
  if (n_edges < 0) return eelg_fail(-2, "nnconv_bwd_edge: n_edges %d", n_edges);
  if (n_edges == 0) return 0;
  if (!nnc_aligned(x) || !nnc_aligned(h) || !nnc_aligned(w3) || !nnc_aligned(b3) ||
      !nnc_aligned(grad_agg) || !nnc_aligned(gxe) || !nnc_aligned(grad_h))
    return eelg_fail(-2, "nnconv_bwd_edge: x, h, w3, b3, grad_agg, gxe and grad_h must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((n_edges + 127) / 128), block(256);
  if (D == 32)
    hipLaunchKernelGGL(nnconv_bwd_edge_kernel<32>, grid, block, 0, s, x, h, w3, b3, sender, receiver,
                       n_edges, grad_agg, gxe, grad_h);
  else
    hipLaunchKernelGGL(nnconv_bwd_edge_kernel<64>, grid, block, 0, s, x, h, w3, b3, sender, receiver,
                       n_edges, grad_agg, gxe, grad_h);
  return eelg_check_launch("nnconv_bwd_edge");
}

int eelg_nnconv_bwd_w(const float* x, const float* h, const float* w3, const float* b3,
                      const int* sender, const int* receiver, int n_edges, int D,
                      const float* grad_agg, float* part, void* stream) {
  if (D != 32 && D != 64) return eelg_fail(-2, "nnconv_bwd_w: D = %d (built: 32, 64)", D);
  if (n_edges < 0) return eelg_fail(-2, "nnconv_bwd_w: n_edges %d", n_edges);
  if (n_edges == 0) return 0;
  if (!nnc_aligned(x) || !nnc_aligned(h) || !nnc_aligned(w3) || !nnc_aligned(b3) ||
      !nnc_aligned(grad_agg) || !nnc_aligned(part))
    return eelg_fail(-2, "nnconv_bwd_w: x, h, w3, b3, grad_agg and part must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int tps = nnc_tiles_per_split(n_edges, D);
  const dim3 grid(D * (D / 32), eelg_nnconv_bwd_w_parts(n_edges, D)), block(64);
  if (D == 32)
    hipLaunchKernelGGL(nnconv_bwd_w_kernel<32>, grid, block, 0, s, x, h, w3, b3, sender, receiver,
                       n_edges, grad_agg, tps, part);
  else
    hipLaunchKernelGGL(nnconv_bwd_w_kernel<64>, grid, block, 0, s, x, h, w3, b3, sender, receiver,
                       n_edges, grad_agg, tps, part);
  return eelg_check_launch("nnconv_bwd_w");
}

}  // extern "C"
