// The per-element arithmetic of the training step's tail (csrc/eelg_optim.hip): the coefficient of
// the loss gradient, torch's gradient-clipping coefficient and torch.optim.AdamW's update rule
// (with or without amsgrad).  Plain C++: the same text compiles into the HIP kernels and, with
// EELG_HD empty, into a host program (tests/test_flat_adamw.py builds tests/adamw_host_main.cpp
// with the address and undefined-behaviour sanitizers and runs the hostile gradient set through
// it).
//
// * The hyper-parameters arrive as doubles, as torch holds them (Python floats), and everything
//   that depends on the step count alone is formed in fp64 once per launch and rounded to fp32
//   once (eelg_adamw_prepare): 1 - beta^t in fp32 would carry 5e-7 of relative error into every
//   parameter at t = 1.
// * The per-element rule follows torch's single-tensor path operation by operation
//   (torch/optim/adam.py, _single_tensor_adam with decoupled decay):
//     p *= 1 - lr wd;  m = lerp(m, g, 1 - beta1);  v = beta2 v + (1 - beta2) g g;
//     vmax = max(vmax, v);  denom = sqrt(vmax or v) / sqrt(bc2) + eps;  p -= (lr / bc1) m / denom
//   with g already multiplied by the clip coefficient.  Elements that are all zero (g, p, m, v)
//   stay exactly +0: p = 0 - step_size * (0 / eps).
// * eelg_clip_coef is clip_grad_norm_'s  min(1, max_norm / (norm + 1e-6)), formed in fp64 from the
//   fp64 norm and rounded to fp32 once: m = lerp(m, g, .) amplifies the coefficient's rounding
//   error where a step's gradient cancels most of the running mean (19x on the hostile set), and
//   torch's fp32 chain (norm, + 1e-6, fp32 max_norm, division) rounds four times.  max_norm <= 0
//   switches clipping off (coefficient exactly 1, which leaves g bitwise as it is).
#ifndef EELG_ADAMW_H
#define EELG_ADAMW_H

#include <math.h>

#ifndef EELG_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define EELG_HD __host__ __device__
#else
#define EELG_HD
#endif
#endif

typedef struct {
  float decay;      // 1 - lr wd
  float w1;         // 1 - beta1
  float beta2;
  float omb2;       // 1 - beta2
  float step_size;  // lr / (1 - beta1^t)
  float bc2_sqrt;   // sqrt(1 - beta2^t)
  float eps;
  int amsgrad;
} eelg_adamw_consts;

// t: the step being taken, counted from 1
EELG_HD inline eelg_adamw_consts eelg_adamw_prepare(double lr, double beta1, double beta2, double eps,
                                                    double weight_decay, int amsgrad, int t) {
  eelg_adamw_consts k;
  const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
  k.decay = (float)(1.0 - lr * weight_decay);
  k.w1 = (float)(1.0 - beta1);
  k.beta2 = (float)beta2;
  k.omb2 = (float)(1.0 - beta2);
  k.step_size = (float)(lr / bc1);
  k.bc2_sqrt = (float)sqrt(bc2);
  k.eps = (float)eps;
  k.amsgrad = amsgrad;
  return k;
}

// neither Inf nor NaN (on the bits: holds under any floating-point compiler mode)
EELG_HD inline int eelg_finite(float x) {
  unsigned u;
  __builtin_memcpy(&u, &x, sizeof u);
  return (u & 0x7f800000u) != 0x7f800000u;
}

// norm: the fp64 square root of the fp64 sum of the partials, not yet rounded to fp32
EELG_HD inline float eelg_clip_coef(double norm, double max_norm) {
  if (!(max_norm > 0.0)) return 1.f;
  const double c = max_norm / (norm + 1e-6);
  return c < 1.0 ? (float)c : 1.f;
}

// g: the gradient after clipping.  vmax is read and written only with k.amsgrad.
EELG_HD inline void eelg_adamw_update(const eelg_adamw_consts& k, float g, float* p, float* m, float* v,
                                      float* vmax) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float pd = *p * k.decay;
  // torch's lerp is fma(weight, g - m, m): when g cancels most of m the product must not be
  // rounded on its own (10x the error in m on the hostile set)
  const float mn = fmaf(k.w1, g - *m, *m);
  const float vn = *v * k.beta2 + k.omb2 * (g * g);
  float second = vn;
  if (k.amsgrad) {
    second = *vmax > vn ? *vmax : vn;
    *vmax = second;
  }
  const float denom = sqrtf(second) / k.bc2_sqrt + k.eps;
  *p = pd - k.step_size * (mn / denom);
  *m = mn;
  *v = vn;
}

// d loss / d pred[b][i] = coef_b * (pred[b][i] - target[b][i]) for
// loss = 100 mean_b( mean_i (pred - target)^2 / mean_i target^2 ), times grad_scale
// (1 / accumulate_grad_batches).  mean_t2: the graph's mean_i target^2; n entries, n_graphs graphs.
EELG_HD inline float eelg_loss_grad_coef(float mean_t2, int n, int n_graphs, float grad_scale) {
  return (200.f * grad_scale) / ((float)n * (float)n_graphs * mean_t2);
}

#endif  // EELG_ADAMW_H
