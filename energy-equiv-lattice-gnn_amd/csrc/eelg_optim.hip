// The tail of the training step in three launches: the loss with its gradient, the partial sums
// of squares of the flat gradient, and clip + AdamW + gradient zeroing over flat buffers
// (per-element arithmetic: eelg_adamw.h).  What they replace: LightningWrappedModel.training_step's
// loss (scripts/train_utils.py:52-60, about ten small torch kernels forward and as many backward),
// Trainer(gradient_clip_val=10.0)'s clip_grad_norm_ and torch.optim.AdamW.step over 102 parameter
// tensors, and zero_grad.
//
// stiffness_loss_kernel: ONE workgroup of 16 wavefronts; wavefront w takes graphs w, w + 16, ...
// (one wavefront per graph at a time: lane i < n holds entry i), sums (p - t)^2 and t^2 by a
// fixed xor butterfly, writes the graph's gradient row and keeps the running sums of the two
// per-graph ratios in graph order.  The 16 running sums are combined through LDS in wavefront
// order by one lane.  No atomics, no scratch: the three outputs are bitwise repeatable.
//
// grad_sqnorm_kernel: block b sums the squares of its contiguous chunk of the flat gradient
// (per thread in index order with fmaf, xor butterfly per wave, the four waves in order) and
// stores partial b with a plain store.  The chunking depends on numel alone.
//
// adamw_flat_kernel: every block first combines ALL partials in the same fixed order in fp64
// (wave 0: lane l takes partials l, l + 64, ...; xor butterfly), so every block derives the
// bitwise-same norm, clip coefficient and step constants; then each thread updates four
// consecutive elements and writes zeros over their gradient.  The launch reads state row `in`
// and block 0 writes state row `out` (in != out: the host alternates them), and it never writes
// the partials: no block overwrites anything another block of the same launch reads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"
#include "eelg_adamw.h"

#define OPT_BLOCK 256
#define LOSS_WAVES 16

__device__ __forceinline__ float optim_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ double optim_wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(64 * LOSS_WAVES) void stiffness_loss_kernel(
    const float* __restrict__ pred, const float* __restrict__ target, int n_graphs, int n,
    float grad_scale, float* __restrict__ out, float* __restrict__ grad) {
  __shared__ float s_ratio[LOSS_WAVES], s_mse[LOSS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float ratio = 0.f, mse = 0.f;   // identical in every lane of the wave
  for (int g = wave; g < n_graphs; g += LOSS_WAVES) {
    float d = 0.f, t = 0.f;
    if (lane < n) {
      t = target[(size_t)g * n + lane];
      d = pred[(size_t)g * n + lane] - t;
    }
    const float mean_d2 = optim_wave_sum(d * d) / (float)n;
    const float mean_t2 = optim_wave_sum(t * t) / (float)n;
    ratio += mean_d2 / mean_t2;
    mse += mean_d2;
    if (lane < n) grad[(size_t)g * n + lane] = eelg_loss_grad_coef(mean_t2, n, n_graphs, grad_scale) * d;
  }
  if (lane == 0) {
    s_ratio[wave] = ratio;
    s_mse[wave] = mse;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float r = s_ratio[0], m = s_mse[0];
#pragma unroll
    for (int w = 1; w < LOSS_WAVES; ++w) {
      r += s_ratio[w];
      m += s_mse[w];
    }
    out[0] = 100.f * (r / (float)n_graphs);
    out[1] = m / (float)n_graphs;
  }
}

// elements per partial: a multiple of 4, so that every chunk starts on a 16-byte boundary
__host__ __device__ inline long long sqnorm_chunk(long long numel, int parts) {
  const long long per = (numel + parts - 1) / parts;
  return (per + 3) / 4 * 4;
}

__global__ __launch_bounds__(OPT_BLOCK) void grad_sqnorm_kernel(const float* __restrict__ g, long long numel,
                                                                long long chunk, float* __restrict__ partials) {
  __shared__ float s_w[OPT_BLOCK / 64];
  const long long lo = (long long)blockIdx.x * chunk;
  const long long hi = lo + chunk < numel ? lo + chunk : numel;
  float s = 0.f;
  for (long long i = lo + 4 * (long long)threadIdx.x; i < hi; i += 4 * OPT_BLOCK) {
    if (i + 4 <= hi) {
      const float4 x = *reinterpret_cast<const float4*>(g + i);
      s = fmaf(x.x, x.x, s);
      s = fmaf(x.y, x.y, s);
      s = fmaf(x.z, x.z, s);
      s = fmaf(x.w, x.w, s);
    } else {
      for (long long j = i; j < hi; ++j) s = fmaf(g[j], g[j], s);
    }
  }
  s = optim_wave_sum(s);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

struct adamw_args {
  double lr, beta1, beta2, eps, weight_decay, max_norm;
  int amsgrad;
};

__global__ __launch_bounds__(OPT_BLOCK) void adamw_flat_kernel(
    float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, float* __restrict__ vmax,
    float* __restrict__ g, long long numel, const float* __restrict__ partials, int parts, adamw_args a,
    const int* __restrict__ row_in, int* __restrict__ row_out) {
  __shared__ eelg_adamw_consts s_k;
  __shared__ float s_coef;
  __shared__ int s_ok;
  if (threadIdx.x < 64) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < parts; i += 64) acc += (double)partials[i];
    acc = optim_wave_sum_f64(acc);
    if (threadIdx.x == 0) {
      const double norm64 = sqrt(acc);
      const float norm = (float)norm64;
      const int ok = eelg_finite(norm);
      const float coef = ok ? eelg_clip_coef(norm64, a.max_norm) : 0.f;
      const int t = row_in[0] + 1;
      s_k = eelg_adamw_prepare(a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.amsgrad, t);
      s_coef = coef;
      s_ok = ok;
      if (blockIdx.x == 0) {
        row_out[0] = ok ? t : t - 1;
        row_out[1] = row_in[1] + (ok ? 0 : 1);
        row_out[2] = __float_as_int(norm);
        row_out[3] = __float_as_int(coef);
      }
    }
  }
  __syncthreads();
  const eelg_adamw_consts k = s_k;
  const float coef = s_coef;
  const bool ok = s_ok != 0;
  const long long i = 4 * ((long long)blockIdx.x * OPT_BLOCK + threadIdx.x);
  if (i >= numel) return;
  if (i + 4 <= numel) {
    if (ok) {
      const float4 g4 = *reinterpret_cast<const float4*>(g + i);
      const float4 p4 = *reinterpret_cast<const float4*>(p + i);
      const float4 m4 = *reinterpret_cast<const float4*>(m + i);
      const float4 v4 = *reinterpret_cast<const float4*>(v + i);
      const float4 x4 = k.amsgrad ? *reinterpret_cast<const float4*>(vmax + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float ge[4] = {g4.x * coef, g4.y * coef, g4.z * coef, g4.w * coef};
      float pe[4] = {p4.x, p4.y, p4.z, p4.w}, me[4] = {m4.x, m4.y, m4.z, m4.w};
      float ve[4] = {v4.x, v4.y, v4.z, v4.w}, xe[4] = {x4.x, x4.y, x4.z, x4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) eelg_adamw_update(k, ge[e], pe + e, me + e, ve + e, xe + e);
      *reinterpret_cast<float4*>(p + i) = make_float4(pe[0], pe[1], pe[2], pe[3]);
      *reinterpret_cast<float4*>(m + i) = make_float4(me[0], me[1], me[2], me[3]);
      *reinterpret_cast<float4*>(v + i) = make_float4(ve[0], ve[1], ve[2], ve[3]);
      if (k.amsgrad) *reinterpret_cast<float4*>(vmax + i) = make_float4(xe[0], xe[1], xe[2], xe[3]);
    }
    *reinterpret_cast<float4*>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (long long j = i; j < numel; ++j) {
      if (ok) {
        float x = k.amsgrad ? vmax[j] : 0.f;
        eelg_adamw_update(k, g[j] * coef, p + j, m + j, v + j, &x);
        if (k.amsgrad) vmax[j] = x;
      }
      g[j] = 0.f;
    }
  }
}

extern "C" {

int eelg_stiffness_loss(const float* pred, const float* target, int n_graphs, int n, float grad_scale,
                        float* out, float* grad, void* stream) {
  if (n_graphs <= 0) return eelg_fail(-2, "stiffness_loss: %d graphs (at least 1)", n_graphs);
  if (n != 36 && n != 21) return eelg_fail(-2, "stiffness_loss: %d entries per graph (36 or 21)", n);
  if (!pred || !target || !out || !grad)
    return eelg_fail(-2, "stiffness_loss: null pointer (pred, target, out, grad)");
  hipLaunchKernelGGL(stiffness_loss_kernel, dim3(1), dim3(64 * LOSS_WAVES), 0, (hipStream_t)stream, pred,
                     target, n_graphs, n, grad_scale, out, grad);
  return eelg_check_launch("stiffness_loss");
}

int eelg_sqnorm_parts(long long numel) {
  if (numel <= 0) return 0;
  const long long parts = (numel + EELG_SQNORM_CHUNK - 1) / EELG_SQNORM_CHUNK;
  return (int)(parts < EELG_SQNORM_MAXPARTS ? parts : EELG_SQNORM_MAXPARTS);
}

int eelg_grad_sqnorm(const float* grad, long long numel, float* partials, void* stream) {
  if (numel <= 0) return eelg_fail(-2, "grad_sqnorm: %lld elements (at least 1)", numel);
  if (!grad || !partials) return eelg_fail(-2, "grad_sqnorm: null pointer (grad, partials)");
  if ((uintptr_t)grad % 16) return eelg_fail(-2, "grad_sqnorm: grad is not 16-byte aligned");
  const int parts = eelg_sqnorm_parts(numel);
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)parts), dim3(OPT_BLOCK), 0, (hipStream_t)stream, grad,
                     numel, sqnorm_chunk(numel, parts), partials);
  return eelg_check_launch("grad_sqnorm");
}

int eelg_adamw_flat(float* p, float* m, float* v, float* vmax, float* grad, long long numel,
                    const float* partials, double lr, double beta1, double beta2, double eps,
                    double weight_decay, double max_norm, int amsgrad, const int* state_in, int* state_out,
                    void* stream) {
  if (numel <= 0) return eelg_fail(-2, "adamw_flat: %lld elements (at least 1)", numel);
  if (numel > (1ll << 40)) return eelg_fail(-2, "adamw_flat: %lld elements (at most 2^40)", numel);
  if (!p || !m || !v || !grad || !partials || !state_in || !state_out || (amsgrad && !vmax))
    return eelg_fail(-2, "adamw_flat: null pointer (p, m, v, vmax with amsgrad, grad, partials, state rows)");
  if (state_in == state_out)
    return eelg_fail(-2, "adamw_flat: state_in and state_out must be different rows");
  if ((uintptr_t)p % 16 || (uintptr_t)m % 16 || (uintptr_t)v % 16 || (uintptr_t)grad % 16 ||
      (amsgrad && (uintptr_t)vmax % 16))
    return eelg_fail(-2, "adamw_flat: p, m, v, vmax and grad must be 16-byte aligned");
  adamw_args a{lr, beta1, beta2, eps, weight_decay, max_norm, amsgrad ? 1 : 0};
  const long long quads = (numel + 3) / 4;
  const long long blocks = (quads + OPT_BLOCK - 1) / OPT_BLOCK;
  hipLaunchKernelGGL(adamw_flat_kernel, dim3((unsigned)blocks), dim3(OPT_BLOCK), 0, (hipStream_t)stream, p, m,
                     v, vmax, grad, numel, partials, eelg_sqnorm_parts(numel), a, state_in, state_out);
  return eelg_check_launch("adamw_flat");
}

}  // extern "C"
