// Gradient-based lattice design: the strut volume of every graph of a batch, and the tail of one
// design iteration (tie the two directions of a strut, check, normalise, heavy-ball step with box
// clamps, keep the volume) in one launch.  The arithmetic is csrc/eelg_design.h.
//
// Both kernels: one workgroup of EELG_DESIGN_THREADS threads per graph.  Thread t takes the
// graph's edges e0 + t, e0 + t + T, ... and the node components likewise, so which thread holds an
// element depends on its offset inside the graph alone.  Reductions: an xor butterfly over the wave,
// one LDS slot per wave, and every thread adds the slots in wave order.  The maxima and the flag are
// exact in any order; the volume is summed in fp64 in that fixed order and rounded to fp32 once.  So
// a graph's outputs are bitwise independent of the other graphs, of its position and of the run.
// No atomics, no scratch, LDS for the reduction slots only.
//
// design_step_kernel updates pos, r, m_pos, m_r in place.  A thread re-reads only the elements it
// wrote itself, except for the positions the strut lengths gather: those are read after a
// workgroup barrier, and send / recv are checked to stay inside the graph's own node rows first
// (EELG_DESIGN_BAD_INDEX otherwise: nothing of the graph is read or written), so no workgroup reads
// what another one writes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"
#include "eelg_design.h"

#define DESIGN_T EELG_DESIGN_THREADS
#define DESIGN_WAVES (DESIGN_T / 64)

struct design_scratch {
  double sum[DESIGN_WAVES];
  float gr[DESIGN_WAVES], gp[DESIGN_WAVES];
  int bad[DESIGN_WAVES];
};

// the graph's row ranges, cut to the arrays (a device ptr row that disagrees with the checked host
// mirror cannot lead outside them)
struct design_range {
  int n0, n1, e0, e1;
};

__device__ __forceinline__ design_range design_rows(const int* __restrict__ node_ptr,
                                                    const int* __restrict__ edge_ptr, int g, int n_nodes,
                                                    int n_edges) {
  design_range q;
  q.n0 = min(max(node_ptr[g], 0), n_nodes);
  q.n1 = min(max(node_ptr[g + 1], q.n0), n_nodes);
  q.e0 = min(max(edge_ptr[g], 0), n_edges);
  q.e1 = min(max(edge_ptr[g + 1], q.e0), n_edges);
  return q;
}

// every thread returns the sum over the workgroup, added in one fixed order
__device__ __forceinline__ double design_block_sum(double v, double* slots) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = slots[0];
#pragma unroll
  for (int w = 1; w < DESIGN_WAVES; ++w) t += slots[w];
  __syncthreads();   // the slots are free again
  return t;
}

// 1 where a send / recv / partner of the graph leaves its own rows (workgroup-uniform)
__device__ __forceinline__ int design_bad_index(const design_range& q, const int* __restrict__ send,
                                                const int* __restrict__ recv, const int* __restrict__ partner,
                                                int* slots) {
  int bad = 0;
  for (int e = q.e0 + (int)threadIdx.x; e < q.e1; e += DESIGN_T) {
    const int s = send[e], r = recv[e];
    bad |= s < q.n0 || s >= q.n1 || r < q.n0 || r >= q.n1;
    if (partner) {
      const int p = partner[e];
      bad |= p < q.e0 || p >= q.e1;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = bad;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < DESIGN_WAVES; ++w) t |= slots[w];
  __syncthreads();
  return t;
}

// V = 1/2 sum over the graph's edges of r^2 L, rounded to fp32 once.  pos is read as it is in
// memory now (no __restrict__: design_step_kernel writes it before the call).
__device__ __forceinline__ float design_volume(const design_range& q, const float* pos, const float* r,
                                               const float* __restrict__ shifts, const int* __restrict__ send,
                                               const int* __restrict__ recv, double* slots) {
  double v = 0.0;
  for (int e = q.e0 + (int)threadIdx.x; e < q.e1; e += DESIGN_T)
    v += eelg_strut_volume_term(
        r[e], eelg_strut_length(pos + 3 * (size_t)send[e], pos + 3 * (size_t)recv[e], shifts + 3 * (size_t)e));
  return (float)(0.5 * design_block_sum(v, slots));
}

__global__ __launch_bounds__(DESIGN_T) void strut_volume_kernel(
    const float* __restrict__ pos, const float* __restrict__ r, const float* __restrict__ shifts,
    const int* __restrict__ send, const int* __restrict__ recv, const int* __restrict__ node_ptr,
    const int* __restrict__ edge_ptr, int n_nodes, int n_edges, float* __restrict__ vol) {
  __shared__ design_scratch sc;
  const int g = blockIdx.x;
  const design_range q = design_rows(node_ptr, edge_ptr, g, n_nodes, n_edges);
  if (design_bad_index(q, send, recv, nullptr, sc.bad)) {   // workgroup-uniform
    if (threadIdx.x == 0) vol[g] = NAN;
    return;
  }
  const float v = design_volume(q, pos, r, shifts, send, recv, sc.sum);
  if (threadIdx.x == 0) vol[g] = v;
}

__global__ __launch_bounds__(DESIGN_T) void design_step_kernel(
    const float* __restrict__ g_pos, const float* __restrict__ g_r, float* pos, float* r,
    const float* __restrict__ pos0, float* m_pos, float* m_r, const int* __restrict__ partner,
    const int* __restrict__ node_ptr, const int* __restrict__ edge_ptr, const float* __restrict__ shifts,
    const int* __restrict__ send, const int* __restrict__ recv, const float* __restrict__ v0, int n_nodes,
    int n_edges, eelg_design_consts k, float* __restrict__ vol, int* __restrict__ flag) {
  __shared__ design_scratch sc;
  const int g = blockIdx.x;
  const int tid = threadIdx.x;
  const design_range q = design_rows(node_ptr, edge_ptr, g, n_nodes, n_edges);
  if (design_bad_index(q, send, recv, partner, sc.bad)) {   // every branch below is workgroup-uniform
    if (tid == 0) {
      vol[g] = NAN;
      flag[g] = EELG_DESIGN_BAD_INDEX;
    }
    return;
  }
  const size_t c0 = 3 * (size_t)q.n0, c1 = 3 * (size_t)q.n1;

  // the finite check and the two maxima, over the tied radius gradient and the position gradient
  int bad = 0;
  float gr = 0.f, gp = 0.f;
  for (int e = q.e0 + tid; e < q.e1; e += DESIGN_T) {
    const float t = eelg_design_tied(g_r, e, partner[e]);
    bad |= !eelg_design_finite(t);
    gr = fmaxf(gr, fabsf(t));
  }
  for (size_t c = c0 + tid; c < c1; c += DESIGN_T) {
    const float t = g_pos[c];
    bad |= !eelg_design_finite(t);
    gp = fmaxf(gp, fabsf(t));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bad |= __shfl_xor(bad, off, 64);
    gr = fmaxf(gr, __shfl_xor(gr, off, 64));
    gp = fmaxf(gp, __shfl_xor(gp, off, 64));
  }
  if ((tid & 63) == 0) {
    sc.bad[tid >> 6] = bad;
    sc.gr[tid >> 6] = gr;
    sc.gp[tid >> 6] = gp;
  }
  __syncthreads();
  bad = 0;
  gr = gp = 0.f;
#pragma unroll
  for (int w = 0; w < DESIGN_WAVES; ++w) {
    bad |= sc.bad[w];
    gr = fmaxf(gr, sc.gr[w]);
    gp = fmaxf(gp, sc.gp[w]);
  }
  __syncthreads();

  if (bad) {   // nothing of the graph changes; its current volume is reported
    const float v = design_volume(q, pos, r, shifts, send, recv, sc.sum);
    if (tid == 0) {
      vol[g] = v;
      flag[g] = EELG_DESIGN_NONFINITE;
    }
    return;
  }

  if (eelg_design_moves(k.step_pos, gp))
    for (size_t c = c0 + tid; c < c1; c += DESIGN_T) {
      float x = pos[c], m = m_pos[c];
      const float p0 = pos0[c];
      eelg_design_move(g_pos[c], gp, k.beta, k.step_pos, p0 - k.move_limit, p0 + k.move_limit, &x, &m);
      pos[c] = x;
      m_pos[c] = m;
    }
  if (eelg_design_moves(k.step_r, gr))
    for (int e = q.e0 + tid; e < q.e1; e += DESIGN_T) {
      float x = r[e], m = m_r[e];
      eelg_design_move(eelg_design_tied(g_r, e, partner[e]), gr, k.beta, k.step_r, k.r_min, k.r_max, &x, &m);
      r[e] = x;
      m_r[e] = m;
    }
  __syncthreads();   // the new positions of the whole graph, before the lengths gather them

  float v = design_volume(q, pos, r, shifts, send, recv, sc.sum);
  if (k.keep_volume) {
    const float scale = eelg_design_scale(v0[g], v);
    double acc = 0.0;
    for (int e = q.e0 + tid; e < q.e1; e += DESIGN_T) {
      const float x = eelg_design_rescaled(r[e], scale, k.r_min, k.r_max);
      r[e] = x;
      acc += eelg_strut_volume_term(
          x, eelg_strut_length(pos + 3 * (size_t)send[e], pos + 3 * (size_t)recv[e], shifts + 3 * (size_t)e));
    }
    v = (float)(0.5 * design_block_sum(acc, sc.sum));
  }
  if (tid == 0) {
    vol[g] = v;
    flag[g] = 0;
  }
}

// ptr [n_graphs + 1] on the host: starts at 0, never decreases, ends at n
static int design_ptr_ok(const int* ptr, int n_graphs, int n) {
  if (ptr[0] != 0 || ptr[n_graphs] != n) return 0;
  for (int g = 0; g < n_graphs; ++g)
    if (ptr[g + 1] < ptr[g]) return 0;
  return 1;
}

extern "C" {

int eelg_strut_volume(const float* pos, const float* r, const float* shifts, const int* send, const int* recv,
                      const int* node_ptr, const int* edge_ptr, const int* node_ptr_host,
                      const int* edge_ptr_host, int n_graphs, int n_nodes, int n_edges, float* vol,
                      void* stream) {
  if (n_graphs < 1 || n_nodes < 0 || n_edges < 0)
    return eelg_fail(-2, "strut_volume: %d graphs (at least 1), %d nodes, %d edges", n_graphs, n_nodes, n_edges);
  if (!node_ptr || !edge_ptr || !node_ptr_host || !edge_ptr_host || !vol)
    return eelg_fail(-2, "strut_volume: null pointer (node_ptr, edge_ptr, their host mirrors, vol)");
  if (!design_ptr_ok(node_ptr_host, n_graphs, n_nodes) || !design_ptr_ok(edge_ptr_host, n_graphs, n_edges))
    return eelg_fail(-2, "strut_volume: node_ptr / edge_ptr must start at 0, never decrease and end at %d / %d",
                     n_nodes, n_edges);
  if (n_edges > 0 && (!pos || !r || !shifts || !send || !recv))
    return eelg_fail(-2, "strut_volume: null pointer (pos, r, shifts, send, recv) with %d edges", n_edges);
  hipLaunchKernelGGL(strut_volume_kernel, dim3((unsigned)n_graphs), dim3(DESIGN_T), 0, (hipStream_t)stream, pos, r,
                     shifts, send, recv, node_ptr, edge_ptr, n_nodes, n_edges, vol);
  return eelg_check_launch("strut_volume");
}

int eelg_design_step(const float* g_pos, const float* g_r, float* pos, float* r, const float* pos0, float* m_pos,
                     float* m_r, const int* partner, const int* node_ptr, const int* edge_ptr,
                     const int* node_ptr_host, const int* edge_ptr_host, const float* shifts, const int* send,
                     const int* recv, const float* v0, int n_graphs, int n_nodes, int n_edges, float step_r,
                     float step_pos, float beta, float r_min, float r_max, float move_limit, int keep_volume,
                     float* vol, int* flag, void* stream) {
  if (n_graphs < 1 || n_nodes < 0 || n_edges < 0)
    return eelg_fail(-2, "design_step: %d graphs (at least 1), %d nodes, %d edges", n_graphs, n_nodes, n_edges);
  if (!node_ptr || !edge_ptr || !node_ptr_host || !edge_ptr_host || !vol || !flag)
    return eelg_fail(-2, "design_step: null pointer (node_ptr, edge_ptr, their host mirrors, vol, flag)");
  if (!design_ptr_ok(node_ptr_host, n_graphs, n_nodes) || !design_ptr_ok(edge_ptr_host, n_graphs, n_edges))
    return eelg_fail(-2, "design_step: node_ptr / edge_ptr must start at 0, never decrease and end at %d / %d",
                     n_nodes, n_edges);
  if (n_edges == 0) return 0;
  if (!g_pos || !g_r || !pos || !r || !pos0 || !m_pos || !m_r || !partner || !shifts || !send || !recv || !v0)
    return eelg_fail(-2, "design_step: null pointer (gradients, geometry, momenta, partner, shifts, send, recv, v0)");
  if (!(r_min < r_max) || !(move_limit >= 0.f))
    return eelg_fail(-2, "design_step: r_min %g must lie below r_max %g, move_limit %g at or above 0", (double)r_min,
                     (double)r_max, (double)move_limit);
  const eelg_design_consts k = {step_r, step_pos, beta, r_min, r_max, move_limit, keep_volume};
  hipLaunchKernelGGL(design_step_kernel, dim3((unsigned)n_graphs), dim3(DESIGN_T), 0, (hipStream_t)stream, g_pos,
                     g_r, pos, r, pos0, m_pos, m_r, partner, node_ptr, edge_ptr, shifts, send, recv, v0, n_nodes,
                     n_edges, k, vol, flag);
  return eelg_check_launch("design_step");
}

}  // extern "C"
