// Geometry gradients (declared in include/eelg.h): the interaction's gradient w.r.t. the
// spherical harmonics (generated tp_bwd_sh_<cfg>, gen_kernels.py emit_tp_bwd_sh) and the backward
// of the edge embedding (sh_bwd_l<L> from emit_sh_bwd + the Gaussian bases).  A translation
// unit of its own: the training path's kernels are compiled exactly as before.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"

// (x, w, sender, receiver, n_edges, grad_agg, inv_norm, grad_sh)
typedef void (*eelg_tp_bwd_sh_fn)(const float*, const float*, const int*, const int*, int,
                                  const float*, float, float*);
struct eelg_tp_sh_cfg {
  const char* name;
  int nshp;
  eelg_tp_bwd_sh_fn fn;
};

#include "generated/eelg_gen_geom.hip"
// the SH gradients of the further hidden l lists' sets (tpB_l4_h024, ...), a table of their own
#include "generated/eelg_gen_geom_hid.hip"

// ---------------------------------------------------------------------------
// backward of edge_embed_kernel: one thread per edge
// ---------------------------------------------------------------------------
// v = pos[recv] - pos[send] + shift, r = |v|, n = v / r:
//   vbar = (nbar - n (n . nbar)) / r   (sh_bwd_l<L>)   +   n rbar,
//   rbar = sum_k fbar_k (-2 d_k / step) f_k,  f_k = exp(-d_k^2) / 1.12,  d_k = (r - v_k) / step,
// and the same sum over the radius basis gives grad_radius.  gvec rows are [x, y, z, 0].
__global__ __launch_bounds__(256) void edge_embed_bwd_kernel(
    const float* __restrict__ pos, const int* __restrict__ sender, const int* __restrict__ receiver,
    const float* __restrict__ shifts, const float* __restrict__ radius, int n_edges, int lmax,
    int nb, float len_end, float rad_end, const float* __restrict__ gsh, int gsh_ld,
    const float* __restrict__ gfeats, float* __restrict__ gvec, float* __restrict__ grad) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  const int s = sender[e], r = receiver[e];
  const float vx = pos[3 * r + 0] - pos[3 * s + 0] + shifts[3 * e + 0];
  const float vy = pos[3 * r + 1] - pos[3 * s + 1] + shifts[3 * e + 1];
  const float vz = pos[3 * r + 2] - pos[3 * s + 2] + shifts[3 * e + 2];
  const float len = sqrtf(vx * vx + vy * vy + vz * vz);
  const float* __restrict__ ge = gsh + (size_t)e * gsh_ld;
  float gv[3];
  switch (lmax) {
    case 1: sh_bwd_l1(vx, vy, vz, ge, gv); break;
    case 2: sh_bwd_l2(vx, vy, vz, ge, gv); break;
    case 3: sh_bwd_l3(vx, vy, vz, ge, gv); break;
    default: sh_bwd_l4(vx, vy, vz, ge, gv); break;
  }
  const float rad = radius[e];
  const float lstep = len_end / (float)(nb - 1);
  const float rstep = rad_end / (float)(nb - 1);
  const float* __restrict__ gf = gfeats + (size_t)e * 2 * nb;
  float lbar = 0.0f, rbar = 0.0f;
  for (int k = 0; k < nb; ++k) {
    const float vl = (k == nb - 1) ? len_end : lstep * (float)k;
    const float vr = (k == nb - 1) ? rad_end : rstep * (float)k;
    const float dl = (len - vl) / lstep;
    const float dr = (rad - vr) / rstep;
    lbar = fmaf(gf[k] * (-2.0f * dl / lstep), expf(-dl * dl) / 1.12f, lbar);
    rbar = fmaf(gf[nb + k] * (-2.0f * dr / rstep), expf(-dr * dr) / 1.12f, rbar);
  }
  const float inv = 1.0f / fmaxf(len, 1e-12f);
  // d len / d v = v / len (0 at len = 0, where sqrt has no finite slope)
  const float li = len > 0.0f ? lbar * inv : 0.0f;
  reinterpret_cast<float4*>(gvec)[e] =
      make_float4(fmaf(vx, li, gv[0]), fmaf(vy, li, gv[1]), fmaf(vz, li, gv[2]), 0.0f);
  grad[e] = rbar;
}

static const eelg_tp_sh_cfg* tp_sh_cfg(const char* name) {
  for (const eelg_tp_sh_cfg& c : kTpShConfigs)
    if (strcmp(c.name, name) == 0) return &c;
  for (const eelg_tp_sh_cfg& c : kTpShHidConfigs)
    if (strcmp(c.name, name) == 0) return &c;
  return nullptr;
}

extern "C" {

int eelg_tp_bwd_sh(int cfg, const float* x, const float* sh, const float* w, const int* sender,
                   const int* receiver, int n_edges, const float* grad_agg, float inv_norm,
                   float* grad_sh, void* stream) {
  (void)sh;   // the TP is linear in the SH: its SH gradient does not read them
  int n = 0;
  const eelg_tp_cfg* t = eelg_tp_table(&n);
  if (cfg < 0 || cfg >= n) return eelg_fail(-1, "bad tp config %d", cfg);
  const eelg_tp_sh_cfg* c = tp_sh_cfg(t[cfg].name);
  if (!c) return eelg_fail(-2, "tp_bwd_sh: no SH-gradient kernel for config %s", t[cfg].name);
  if (n_edges <= 0) return 0;
  hipLaunchKernelGGL(c->fn, dim3((n_edges + 7) / 8), dim3(256), 0, (hipStream_t)stream, x, w, sender,
                     receiver, n_edges, grad_agg, inv_norm, grad_sh);
  return eelg_check_launch("tp_bwd_sh");
}

int eelg_edge_embed_bwd(const float* pos, const int* sender, const int* receiver,
                        const float* shifts, const float* radius, int n_edges, int lmax, int nb,
                        float len_end, float rad_end, const float* grad_sh, int grad_sh_ld,
                        const float* grad_feats, float* grad_vec, float* grad_radius,
                        void* stream) {
  if (lmax < 1 || lmax > 4) return eelg_fail(-2, "edge_embed_bwd: lmax %d not built (1..4)", lmax);
  if (nb < 2) return eelg_fail(-2, "edge_embed_bwd: need >= 2 bases, got %d", nb);
  if (grad_sh_ld < (lmax + 1) * (lmax + 1))
    return eelg_fail(-2, "edge_embed_bwd: grad_sh row stride %d below %d components", grad_sh_ld,
                     (lmax + 1) * (lmax + 1));
  if (reinterpret_cast<uintptr_t>(grad_vec) & 15)
    return eelg_fail(-2, "edge_embed_bwd: grad_vec must be 16-byte aligned");
  if (n_edges <= 0) return 0;
  hipLaunchKernelGGL(edge_embed_bwd_kernel, dim3((n_edges + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, pos, sender, receiver, shifts, radius, n_edges, lmax, nb,
                     len_end, rad_end, grad_sh, grad_sh_ld, grad_feats, grad_vec, grad_radius);
  return eelg_check_launch("edge_embed_bwd");
}

}  // extern "C"
