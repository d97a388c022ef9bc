// Principal-neighbourhood aggregation of the per-edge messages over the receiver CSR
// (interaction_reduction = 'pna'): replaces PNASimple.forward (gnn/blocks.py:817-848, with the
// aggregators and scalers of gnn/pna.py:20-31, 59-78) -- six torch_scatter passes into four
// [N, D] aggregates, a 12-fold [N, D, 12] stack of their scaled copies and a Linear(12, 1) --
// with one pass that writes a single [N, D] result:
//   out[n, c] = coef[n, 0] mean + coef[n, 1] min + coef[n, 2] max + coef[n, 3] std
// where coef[n, k] = sum_s W[3k + s] scale_s(deg_n) is formed by the caller (gnn/ops.py): the
// twelve weights and the three degree scalers never enter the kernels.
//
// One wave owns one receiver row and a span of up to PNA_SPAN column groups (a group = a float4
// when width % 4 == 0 and every pointer is 16-byte aligned, one float otherwise); a lane walks
// the groups lane, lane + 64, ... of the span and, for each, the rows of the segment in batches
// of PNA_EB loads.  The segment bounds and the row's coefficients are wave-uniform.
//   mean = sum / max(deg, 1); min / max = the FIRST extreme in CSR order (strict compare, the
//   rule of eelg_segment_order) and its row; std = sqrt(sum (m - mean)^2 / deg + 1e-5).
// The variance is centred (a second sweep over the segment, from registers when deg <= PNA_EB,
// else re-read through the caches): fp32 E[m^2] - E[m]^2 loses the digits the gradient
// (m - mean) / std needs.  It is >= 0, so the reference's relu is the identity, and its
// zero-gradient case (var == 0) is m - mean == 0 for every row of the segment.
// An empty segment gives mean = min = max = 0, std = sqrt(1e-5) and rows -1.
//
// Backward: grad_src[e, c] = g (coef_mean / deg + coef_std (m_e - mean) / (deg std)
//                               + coef_min [e == argmin] + coef_max [e == argmax])
// is written once for every row of every segment (the segments cover the rows: no zero fill),
// and part[span, n, k] = sum over the span's columns of g agg_k in a fixed order (per lane in
// column order, then an xor butterfly over the wave): no atomics, bitwise repeatable.  The
// caller sums the spans (eelg_sum_rows).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"

#define PNA_EB 4        // source rows per batch of loads
#define PNA_SPAN 512    // column groups per wave (8 per lane)
#define PNA_EPS 1e-5f

typedef float pna_f4n __attribute__((ext_vector_type(4)));
typedef int pna_i4n __attribute__((ext_vector_type(4)));

template <int V> struct pna_vec {
  float v[V];
};

template <int V>
__device__ __forceinline__ pna_vec<V> pna_load(const float* __restrict__ p) {
  pna_vec<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}
template <int V>
__device__ __forceinline__ void pna_load_i(const int* __restrict__ p, int* r) {
  if constexpr (V == 4) {
    const int4 t = *reinterpret_cast<const int4*>(p);
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
  } else {
    r[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void pna_store(float* __restrict__ p, const float* v) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}
// saved state and the [E, width] gradient are read back long after any cache could hold them
template <int V>
__device__ __forceinline__ void pna_store_nt(float* __restrict__ p, const float* v) {
  if constexpr (V == 4) {
    pna_f4n t = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(t, reinterpret_cast<pna_f4n*>(p));
  } else {
    __builtin_nontemporal_store(v[0], p);
  }
}
template <int V>
__device__ __forceinline__ void pna_store_nt(int* __restrict__ p, const int* v) {
  if constexpr (V == 4) {
    pna_i4n t = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(t, reinterpret_cast<pna_i4n*>(p));
  } else {
    __builtin_nontemporal_store(v[0], p);
  }
}

template <int V>
__global__ __launch_bounds__(256) void segment_pna_fwd_kernel(
    const float* __restrict__ src, const int* __restrict__ rowptr, const float* __restrict__ coef,
    int n_rows, int width, int nspan, float* __restrict__ out, float* __restrict__ mean_o,
    float* __restrict__ std_o, int* __restrict__ amin_o, int* __restrict__ amax_o) {
  const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (long long)n_rows * nspan) return;
  const int lane = threadIdx.x & 63;
  const int row = (int)(wid / nspan), span = (int)(wid - (long long)row * nspan);
  const int beg = __builtin_amdgcn_readfirstlane(rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
  const int deg = end - beg;
  const float c_mean = coef[4 * row + 0], c_min = coef[4 * row + 1], c_max = coef[4 * row + 2],
              c_std = coef[4 * row + 3];
  const float fdeg = (float)max(deg, 1), inv_deg = 1.0f / fdeg;
  const int wq = width / V;
  const int q1 = min(wq, (span + 1) * PNA_SPAN);
  for (int q = span * PNA_SPAN + lane; q < q1; q += 64) {
    const size_t col = (size_t)q * V;
    float sum[V], mn[V], mx[V], m2[V];
    int amn[V], amx[V];
#pragma unroll
    for (int t = 0; t < V; ++t) { sum[t] = 0.f; mn[t] = 0.f; mx[t] = 0.f; m2[t] = 0.f; amn[t] = -1; amx[t] = -1; }
    pna_vec<V> v[PNA_EB];
    for (int b = beg; b < end; b += PNA_EB) {
#pragma unroll
      for (int u = 0; u < PNA_EB; ++u) v[u] = pna_load<V>(src + (size_t)min(b + u, end - 1) * width + col);
#pragma unroll
      for (int u = 0; u < PNA_EB; ++u) {
        if (b + u < end) {
#pragma unroll
          for (int t = 0; t < V; ++t) {
            const float x = v[u].v[t];
            sum[t] += x;
            if (amn[t] < 0 || x < mn[t]) { mn[t] = x; amn[t] = b + u; }
            if (amx[t] < 0 || x > mx[t]) { mx[t] = x; amx[t] = b + u; }
          }
        }
      }
    }
    float mean[V];
#pragma unroll
    for (int t = 0; t < V; ++t) mean[t] = sum[t] / fdeg;   // a true division: exact when the mean is representable
    if (deg <= PNA_EB) {
      // the whole segment is still in registers
#pragma unroll
      for (int u = 0; u < PNA_EB; ++u) {
        if (u < deg) {
#pragma unroll
          for (int t = 0; t < V; ++t) { const float d = v[u].v[t] - mean[t]; m2[t] = fmaf(d, d, m2[t]); }
        }
      }
    } else {
      for (int b = beg; b < end; b += PNA_EB) {
#pragma unroll
        for (int u = 0; u < PNA_EB; ++u) v[u] = pna_load<V>(src + (size_t)min(b + u, end - 1) * width + col);
#pragma unroll
        for (int u = 0; u < PNA_EB; ++u) {
          if (b + u < end) {
#pragma unroll
            for (int t = 0; t < V; ++t) { const float d = v[u].v[t] - mean[t]; m2[t] = fmaf(d, d, m2[t]); }
          }
        }
      }
    }
    float sd[V], o[V];
#pragma unroll
    for (int t = 0; t < V; ++t) {
      sd[t] = sqrtf(m2[t] * inv_deg + PNA_EPS);
      o[t] = c_mean * mean[t] + c_min * mn[t] + c_max * mx[t] + c_std * sd[t];
    }
    const size_t at = (size_t)row * width + col;
    pna_store<V>(out + at, o);
    pna_store_nt<V>(mean_o + at, mean);
    pna_store_nt<V>(std_o + at, sd);
    pna_store_nt<V>(amin_o + at, amn);
    pna_store_nt<V>(amax_o + at, amx);
  }
}

__device__ __forceinline__ float pna_wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

template <int V>
__global__ __launch_bounds__(256) void segment_pna_bwd_kernel(
    const float* __restrict__ src, const int* __restrict__ rowptr, const float* __restrict__ coef,
    const float* __restrict__ mean_i, const float* __restrict__ std_i, const int* __restrict__ amin_i,
    const int* __restrict__ amax_i, const float* __restrict__ g_i, int n_rows, int width, int nspan,
    float* __restrict__ gsrc, float* __restrict__ part) {
  const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wid >= (long long)n_rows * nspan) return;
  const int lane = threadIdx.x & 63;
  const int row = (int)(wid / nspan), span = (int)(wid - (long long)row * nspan);
  const int beg = __builtin_amdgcn_readfirstlane(rowptr[row]);
  const int end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
  const int deg = end - beg;
  const float c_mean = coef[4 * row + 0], c_min = coef[4 * row + 1], c_max = coef[4 * row + 2],
              c_std = coef[4 * row + 3];
  const float inv_deg = 1.0f / (float)max(deg, 1);
  const float a_mean = c_mean * inv_deg;
  const int wq = width / V;
  const int q1 = min(wq, (span + 1) * PNA_SPAN);
  float p_mean = 0.f, p_min = 0.f, p_max = 0.f, p_std = 0.f;
  for (int q = span * PNA_SPAN + lane; q < q1; q += 64) {
    const size_t col = (size_t)q * V;
    const size_t at = (size_t)row * width + col;
    const pna_vec<V> g = pna_load<V>(g_i + at), mean = pna_load<V>(mean_i + at),
                     sd = pna_load<V>(std_i + at);
    int amn[V], amx[V];
    pna_load_i<V>(amin_i + at, amn);
    pna_load_i<V>(amax_i + at, amx);
    float bs[V], mnv[V], mxv[V];
#pragma unroll
    for (int t = 0; t < V; ++t) { bs[t] = c_std * inv_deg / sd.v[t]; mnv[t] = 0.f; mxv[t] = 0.f; }
    pna_vec<V> v[PNA_EB];
    for (int b = beg; b < end; b += PNA_EB) {
#pragma unroll
      for (int u = 0; u < PNA_EB; ++u) v[u] = pna_load<V>(src + (size_t)min(b + u, end - 1) * width + col);
#pragma unroll
      for (int u = 0; u < PNA_EB; ++u) {
        if (b + u < end) {
          float gs[V];
#pragma unroll
          for (int t = 0; t < V; ++t) {
            const float x = v[u].v[t];
            float w = fmaf(bs[t], x - mean.v[t], a_mean);
            if (b + u == amn[t]) { w += c_min; mnv[t] = x; }
            if (b + u == amx[t]) { w += c_max; mxv[t] = x; }
            gs[t] = g.v[t] * w;
          }
          pna_store_nt<V>(gsrc + (size_t)(b + u) * width + col, gs);
        }
      }
    }
    // the four column sums of this group, components in order
    float s_mean = 0.f, s_min = 0.f, s_max = 0.f, s_std = 0.f;
#pragma unroll
    for (int t = 0; t < V; ++t) {
      s_mean = fmaf(g.v[t], mean.v[t], s_mean);
      s_min = fmaf(g.v[t], mnv[t], s_min);
      s_max = fmaf(g.v[t], mxv[t], s_max);
      s_std = fmaf(g.v[t], sd.v[t], s_std);
    }
    p_mean += s_mean; p_min += s_min; p_max += s_max; p_std += s_std;
  }
  p_mean = pna_wave_sum(p_mean);
  p_min = pna_wave_sum(p_min);
  p_max = pna_wave_sum(p_max);
  p_std = pna_wave_sum(p_std);
  if (lane == 0) {
    float* __restrict__ o = part + ((size_t)span * n_rows + row) * 4;
    o[0] = p_mean; o[1] = p_min; o[2] = p_max; o[3] = p_std;
  }
}

static bool pna_al16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

static int pna_nspan(int width, bool vec) {
  const int wq = vec ? width / 4 : width;
  return (wq + PNA_SPAN - 1) / PNA_SPAN;
}

extern "C" {

int eelg_segment_pna_parts(int width) {
  if (width < 1) return eelg_fail(-2, "segment_pna: width %d", width);
  // width % 4 == 0 always runs the float4 form (misaligned buffers are refused), so the count
  // depends on the width alone
  return pna_nspan(width, width % 4 == 0);
}

int eelg_segment_pna_fwd(const float* src, const int* rowptr, const float* coef, int n_rows, int width,
                         float* out, float* mean, float* std, int* argmin, int* argmax, void* stream) {
  if (n_rows < 0 || width < 1) return eelg_fail(-2, "segment_pna_fwd: n_rows %d, width %d", n_rows, width);
  if (!src || !rowptr || !coef || !out || !mean || !std || !argmin || !argmax)
    return eelg_fail(-2, "segment_pna_fwd: null pointer (src, rowptr, coef, out, mean, std, argmin, argmax)");
  if (n_rows == 0) return 0;
  const bool vec = width % 4 == 0 && pna_al16(src) && pna_al16(out) && pna_al16(mean) && pna_al16(std) &&
                   pna_al16(argmin) && pna_al16(argmax);
  if (width % 4 == 0 && !vec)
    return eelg_fail(-2, "segment_pna_fwd: rows of %d floats need 16-byte aligned buffers", width);
  const int nspan = pna_nspan(width, vec);
  const long long nblk = ((long long)n_rows * nspan + 3) / 4;
  if (nblk > INT32_MAX) return eelg_fail(-2, "segment_pna_fwd: %d rows x %d columns", n_rows, width);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(segment_pna_fwd_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, s, src, rowptr, coef,
                       n_rows, width, nspan, out, mean, std, argmin, argmax);
  else
    hipLaunchKernelGGL(segment_pna_fwd_kernel<1>, dim3((unsigned)nblk), dim3(256), 0, s, src, rowptr, coef,
                       n_rows, width, nspan, out, mean, std, argmin, argmax);
  return eelg_check_launch("segment_pna_fwd");
}

int eelg_segment_pna_bwd(const float* src, const int* rowptr, const float* coef, const float* mean,
                         const float* std, const int* argmin, const int* argmax, const float* grad_out,
                         int n_rows, int width, float* grad_src, float* grad_coef_part, void* stream) {
  if (n_rows < 0 || width < 1) return eelg_fail(-2, "segment_pna_bwd: n_rows %d, width %d", n_rows, width);
  if (!src || !rowptr || !coef || !mean || !std || !argmin || !argmax || !grad_out || !grad_src ||
      !grad_coef_part)
    return eelg_fail(-2, "segment_pna_bwd: null pointer");
  if (n_rows == 0) return 0;
  const bool vec = width % 4 == 0 && pna_al16(src) && pna_al16(mean) && pna_al16(std) && pna_al16(argmin) &&
                   pna_al16(argmax) && pna_al16(grad_out) && pna_al16(grad_src);
  if (width % 4 == 0 && !vec)
    return eelg_fail(-2, "segment_pna_bwd: rows of %d floats need 16-byte aligned buffers", width);
  const int nspan = pna_nspan(width, vec);
  const long long nblk = ((long long)n_rows * nspan + 3) / 4;
  if (nblk > INT32_MAX) return eelg_fail(-2, "segment_pna_bwd: %d rows x %d columns", n_rows, width);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(segment_pna_bwd_kernel<4>, dim3((unsigned)nblk), dim3(256), 0, s, src, rowptr, coef, mean,
                       std, argmin, argmax, grad_out, n_rows, width, nspan, grad_src, grad_coef_part);
  else
    hipLaunchKernelGGL(segment_pna_bwd_kernel<1>, dim3((unsigned)nblk), dim3(256), 0, s, src, rowptr, coef, mean,
                       std, argmin, argmax, grad_out, n_rows, width, nspan, grad_src, grad_coef_part);
  return eelg_check_launch("segment_pna_bwd");
}

}  // extern "C"
