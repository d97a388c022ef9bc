// Batch assembly from a device-resident packed dataset (gnn/device_data.py): replaces, per
// training batch, PyG's collation of the sampled graphs (node / edge tensors concatenated,
// edge_index offset by the running node count, `batch` and `ptr`; field layout
// gnn/datasets.py:256-269), RotateLat's per-sample rotation (scripts/train_utils.py:114-146)
// and the sorts that rebuild the receiver / sender CSR of the collated batch.
//
// The packed dataset keeps every graph's rows in the graph's own order with LOCAL endpoint
// indices and the graph's local CSR.  The CSR of a collated batch is the concatenation of the
// local ones plus the output offsets (a stable sort by receiver never interleaves graphs: graph
// g's receivers are all below graph g + 1's and its edges come first), so a batch is a gather
// with offsets, a 3x3 multiply per row and a binary search over the n_graphs + 1 slot offsets.
//
// batch_assemble_kernel: one launch, workgroups of 256 threads.  The first ceil(n_nodes / 256)
// workgroups take one output node per thread, the others one output edge per thread (the split
// is per workgroup, so no wave diverges on it).  A thread finds its slot by binary search over
// the output offsets (a few hundred int32 at most: they stay in the vector L1), then copies its
// row: consecutive lanes read and write consecutive 12-byte rows, so a wave's accesses to the
// [*, 3] tensors cover one contiguous 768-byte span; the CSR gather (sender / receiver through
// the local perm) stays inside one graph's rows.  fp32 with a fixed operation order, no atomics,
// no LDS: two runs are bitwise equal.  Without rotations nothing is multiplied.
//
// mandel_rotate_kernel: one thread per output entry (g, a, b) of C' = M C M^T; the thread forms
// rows a and b of M(Q_g) from the two rows of Q its Mandel indices name and contracts
// t_c = sum_d C[c][d] M[b][d], out = sum_c M[a][c] t_c in index order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/eelg.h"
#include "eelg_internal.h"

// slot of output row j: the last g in [0, n) with off[g] <= j (off[0] = 0 <= j < off[n]; equal
// neighbours -- graphs without edges -- resolve to the slot that owns the row)
__device__ __forceinline__ int batch_slot(const int* __restrict__ off, int n, int j) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void batch_row3(const float* __restrict__ src, const float* __restrict__ q,
                                           float* __restrict__ dst) {
  const float x = src[0], y = src[1], z = src[2];
  if (q) {
    // Q v: component c = Q[c][0] x + Q[c][1] y + Q[c][2] z
    dst[0] = fmaf(q[2], z, fmaf(q[1], y, q[0] * x));
    dst[1] = fmaf(q[5], z, fmaf(q[4], y, q[3] * x));
    dst[2] = fmaf(q[8], z, fmaf(q[7], y, q[6] * x));
  } else {
    dst[0] = x; dst[1] = y; dst[2] = z;
  }
}

__global__ __launch_bounds__(256) void batch_assemble_kernel(
    const eelg_batch_src s, const int* __restrict__ table, const float* __restrict__ rot, int n_graphs,
    int n_nodes, int n_edges, int node_blocks, const eelg_batch_out o) {
  const int ld = n_graphs + 1;
  const int* __restrict__ onode = table;
  const int* __restrict__ oedge = table + ld;
  const int* __restrict__ snode = table + 2 * ld;
  const int* __restrict__ sedge = table + 3 * ld;
  if ((int)blockIdx.x < node_blocks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_nodes) return;
    if (i == 0) { o.rowptr[0] = 0; o.srowptr[0] = 0; o.ptr[0] = 0; }
    if (i < n_graphs) o.ptr[i + 1] = (int64_t)onode[i + 1];   // n_graphs <= n_nodes
    const int g = batch_slot(onode, n_graphs, i);
    const int src = snode[g] + (i - onode[g]);
    if ((unsigned)src >= (unsigned)s.total_nodes) return;
    const int eoff = oedge[g];
    batch_row3(s.positions + (size_t)src * 3, rot ? rot + (size_t)g * 9 : nullptr, o.positions + (size_t)i * 3);
    for (int c = 0; c < s.node_w; ++c)
      o.node_attrs[(size_t)i * s.node_w + c] = s.node_attrs[(size_t)src * s.node_w + c];
    o.batch[i] = (int64_t)g;
    o.rowptr[i + 1] = s.rowend[src] + eoff;
    o.srowptr[i + 1] = s.srowend[src] + eoff;
  } else {
    const int j = ((int)blockIdx.x - node_blocks) * 256 + threadIdx.x;
    if (j >= n_edges) return;
    const int g = batch_slot(oedge, n_graphs, j);
    const int eoff = oedge[g], noff = onode[g], e0 = sedge[g];
    const int src = e0 + (j - eoff);
    if ((unsigned)src >= (unsigned)s.total_edges) return;
    o.edge_index[j] = (int64_t)(s.sender[src] + noff);
    o.edge_index[(size_t)n_edges + j] = (int64_t)(s.receiver[src] + noff);
    batch_row3(s.shifts + (size_t)src * 3, rot ? rot + (size_t)g * 9 : nullptr, o.shifts + (size_t)j * 3);
    for (int c = 0; c < s.edge_w; ++c)
      o.edge_attr[(size_t)j * s.edge_w + c] = s.edge_attr[(size_t)src * s.edge_w + c];
    const int p = s.perm[src];
    o.perm[j] = (int64_t)(p + eoff);
    o.sperm[j] = s.sperm[src] + eoff;
    const int ps = e0 + p;
    if ((unsigned)ps >= (unsigned)s.total_edges) return;
    o.sender[j] = s.sender[ps] + noff;
    o.receiver[j] = s.receiver[ps] + noff;
  }
}

// row a of M(Q) from rows i(a), j(a) of Q (Mandel a <-> (i, j): 0 11, 1 22, 2 33, 3 23, 4 13, 5 12)
__device__ __forceinline__ void mandel_row(const float* __restrict__ q, int a, float* m) {
  const int i = a < 3 ? a : (a == 3 ? 1 : 0);
  const int j = a < 3 ? a : (a == 5 ? 1 : 2);
  const float i0 = q[3 * i], i1 = q[3 * i + 1], i2 = q[3 * i + 2];
  const float j0 = q[3 * j], j1 = q[3 * j + 1], j2 = q[3 * j + 2];
  const float r2 = 1.41421356237309504880f;
  const float wn = a < 3 ? 1.0f : r2;            // w_a / w_b for b <= 3
  const float ws = a < 3 ? 0.70710678118654752440f : 1.0f;   // and for b > 3
  m[0] = wn * (i0 * j0);
  m[1] = wn * (i1 * j1);
  m[2] = wn * (i2 * j2);
  m[3] = ws * fmaf(i2, j1, i1 * j2);
  m[4] = ws * fmaf(i2, j0, i0 * j2);
  m[5] = ws * fmaf(i1, j0, i0 * j1);
}

__global__ __launch_bounds__(256) void mandel_rotate_kernel(
    const float* __restrict__ src, int n_src, const int* __restrict__ sel, const float* __restrict__ rot,
    int n_graphs, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_graphs * 36) return;
  const int g = t / 36, ab = t - g * 36;
  const int row = sel[g];
  if ((unsigned)row >= (unsigned)n_src) return;
  const float* __restrict__ c = src + (size_t)row * 36;
  if (!rot) { out[t] = c[ab]; return; }
  const int a = ab / 6, b = ab - a * 6;
  float ma[6], mb[6];
  mandel_row(rot + (size_t)g * 9, a, ma);
  mandel_row(rot + (size_t)g * 9, b, mb);
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    float tk = c[6 * k] * mb[0];
#pragma unroll
    for (int d = 1; d < 6; ++d) tk = fmaf(c[6 * k + d], mb[d], tk);
    acc = k == 0 ? ma[0] * tk : fmaf(ma[k], tk, acc);
  }
  out[t] = acc;
}

extern "C" {

int eelg_batch_assemble(const eelg_batch_src* src, const int* table, const float* rot, int n_graphs,
                        int n_nodes, int n_edges, const eelg_batch_out* out, void* stream) {
  if (n_graphs < 0 || n_nodes < 0 || n_edges < 0 || n_graphs > n_nodes)
    return eelg_fail(-2, "batch_assemble: %d graphs, %d nodes, %d edges", n_graphs, n_nodes, n_edges);
  if (!src || !out) return eelg_fail(-2, "batch_assemble: null descriptor");
  if (src->node_w < 1 || src->node_w > EELG_BATCH_MAXW || src->edge_w < 1 || src->edge_w > EELG_BATCH_MAXW)
    return eelg_fail(-2, "batch_assemble: node_attrs width %d, edge_attr width %d (1..%d)", src->node_w,
                     src->edge_w, EELG_BATCH_MAXW);
  if (src->total_nodes < 0 || src->total_edges < 0)
    return eelg_fail(-2, "batch_assemble: packed sizes %d nodes, %d edges", src->total_nodes, src->total_edges);
  if (n_graphs == 0 || n_nodes == 0) return 0;
  if (!table || !src->positions || !src->node_attrs || !src->rowend || !src->srowend || !out->positions ||
      !out->node_attrs || !out->batch || !out->ptr || !out->rowptr || !out->srowptr)
    return eelg_fail(-2, "batch_assemble: null pointer (table or a node tensor)");
  if (n_edges > 0 && (!src->sender || !src->receiver || !src->shifts || !src->edge_attr || !src->perm ||
                      !src->sperm || !out->edge_index || !out->shifts || !out->edge_attr || !out->perm ||
                      !out->sperm || !out->sender || !out->receiver))
    return eelg_fail(-2, "batch_assemble: null pointer (an edge tensor)");
  const int node_blocks = (int)(((long long)n_nodes + 255) / 256);
  const int edge_blocks = (int)(((long long)n_edges + 255) / 256);
  hipLaunchKernelGGL(batch_assemble_kernel, dim3((unsigned)(node_blocks + edge_blocks)), dim3(256), 0,
                     (hipStream_t)stream, *src, table, rot, n_graphs, n_nodes, n_edges, node_blocks, *out);
  return eelg_check_launch("batch_assemble");
}

int eelg_mandel_rotate(const float* src, int n_src, const int* sel, const float* rot, int n_graphs,
                       float* out, void* stream) {
  if (n_graphs < 0 || n_src < 0 || n_graphs > INT32_MAX / 36)
    return eelg_fail(-2, "mandel_rotate: %d graphs from %d", n_graphs, n_src);
  if (n_graphs == 0) return 0;
  if (!src || !sel || !out) return eelg_fail(-2, "mandel_rotate: null pointer (src, sel, out)");
  const int blocks = (n_graphs * 36 + 255) / 256;
  hipLaunchKernelGGL(mandel_rotate_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, src,
                     n_src, sel, rot, n_graphs, out);
  return eelg_check_launch("mandel_rotate");
}

}  // extern "C"
