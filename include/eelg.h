/*
 * eelg.h -- C ABI of the MI355X-native EnergyEquivGNN message-passing hot path.
 *
 * Every entry point takes plain device pointers (fp32 data, int32 indices),
 * sizes and a HIP stream (hipStream_t passed as void*), launches asynchronously
 * on that stream and returns 0 on success or a negative code; the message of
 * the last failure on the calling thread is in eelg_last_error().  Nothing here
 * allocates, frees or synchronises, so every call can be captured in a hipGraph.
 *
 * Layout conventions (reference: gnn/datasets.py:256-269, e3nn mul-major rows):
 *   node features   [N, sum_l mul*(2l+1)]   block (mul, l) laid out [mul][2l+1]
 *   edge SH         [E, (lmax+1)^2] in rows padded to a multiple of 4 floats (row stride
 *                   nshp = round_up((lmax+1)^2, 4): 28 for lmax 4, 16 for lmax 3)
 *   TP weights      [E, npaths*mul]          index = path*mul + channel
 *   edges           receiver-sorted; rowptr[N+1] is the receiver CSR,
 *                   sperm/srowptr the sender CSR over the same edge order.
 *
 * Which reference interface each entry point replaces is given per function.
 */
#ifndef EELG_H
#define EELG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library / error handling ------------------------------------------------ */
const char* eelg_version(void);
const char* eelg_last_error(void);

/* Config discovery: the irreps-specialised kernels are looked up by name
 * ("tpA_l4" = 32x0e node irreps, "tpB_l4" = 32x0e+..+32x4e, "sc_l4_c3" ...).
 * Even-parity hidden irreps have sets of their own, named by their l list: "tpB_l2_h02" and
 * "tpB_l3_h02" (32x0e+32x2e x SH(2) / SH(3)) and "tpB_l4_h024" (32x0e+32x2e+32x4e x SH(4): 24
 * paths, weight_numel 768, dmid 4288 against tpB_l4's 42 / 1344 / 7360), each also as "_m16" /
 * "_m64".  Their config indices follow every earlier set's.  They serve every eelg_tp_* entry
 * point below (bf16 storage at mul 32, as the other sets) and eelg_tp_bwd_sh, except the fused
 * backward: eelg_tp_bwd_fused* and eelg_tp_bwf_slot return -2 for them.
 * info receives {din, dmid, weight_numel, nsh, ngroups, npaths, lmax};
 * sig is a structural hash the host re-derives to detect a stale build. */
int eelg_tp_find(const char* name);
int eelg_tp_info(int cfg, int* info7, uint64_t* sig);
/* info receives {D, x_row, out_row, nterms, n_term_groups, D_out, coef_chunk, coef_ld}
 * (D: coupling components per channel of the input, D_out: of the output; they differ when the
 * product maps the SH-lmax interaction irreps onto wider hidden irreps; coef_chunk: the node
 * chunk of eelg_sc_bwd_coef; coef_ld: the row stride of the coefficient matrix, nterms rounded
 * up to a multiple of 16, so every channel row starts on a 64-byte line) */
int eelg_sc_find(const char* name);
int eelg_sc_info(int cfg, int* info8, uint64_t* sig);
/* The output l of a set, in row order: ls8 receives them, the count is returned (< 0: error).
 * The full sets ("sc_l4_c3") write every l of the coupling, 0 .. lmax.  A live-output set
 * ("sc_l4_c3_o024": l = 0, 2, 4) evaluates only the polynomial terms of the listed outputs,
 * for a consumer that reads nothing else (the last layer in front of the stiffness head,
 * Linear(readout, "2x0e+2x2e+1x4e"), gnn/model.py:82-86).  Its output and output-gradient rows
 * are compact: [N, mul * sum(2l+1)] over the listed l only, mul-major per l block (l = 0, 2, 4
 * at mul 32: 480 floats against the full set's 800); x, grad_x and the coefficient layout
 * (its own nterms / coef_ld) are as for any set.  The config indices of the live-output sets
 * follow the full sets'. */
int eelg_sc_outputs(int cfg, int* ls8);
/* The set with cfg's coupling and correlation whose outputs are exactly ls[0 .. n_ls)
 * (its index; < 0: none was generated). */
int eelg_sc_find_outputs(int cfg, const int* ls, int n_ls);

/* Edge geometry + embeddings.
 * Replaces get_edge_vectors_and_lengths (gnn/mace.py:338-352),
 * soft_one_hot_linspace x2 + cat (gnn/model.py:146-156) and
 * o3.SphericalHarmonics(lmax, normalize=True, 'component') (gnn/model.py:126-129,157).
 * sh[E, nshp] (padded rows, pad zeroed), feats[E, 2*nb] =
 * [gauss(len; 0..len_end) | gauss(radius; 0..rad_end)]. */
int eelg_edge_embed(const float* pos, const int* sender, const int* receiver, const float* shifts,
                    const float* radius, int n_edges, int lmax, int nb, float len_end,
                    float rad_end, float* sh, float* feats, void* stream);

/* Fused interaction: agg[n] = inv_norm * sum_{e: recv(e)=n} TP_uvu(x[sender(e)], sh[e], w[e]).
 * Replaces conv_tp(node_feats[sender], edge_attrs, tp_weights) followed by
 * scatter(..., reduce='sum') / agg_norm_const (gnn/blocks.py:591-597).
 * x, sh and w must be 16-byte aligned (the rows travel by LDS-DMA in 16-B pieces); -2 otherwise. */
int eelg_tp_fwd(int cfg, const float* x, const float* sh, const float* w, const int* sender,
                const int* rowptr, int n_nodes, float inv_norm, float* agg, void* stream);

/* Backward of eelg_tp_fwd: grad_w[E, weight_numel] and per-edge grad of
 * x[sender] gxe[E, din] (to be summed per sender with eelg_segment_sum_csr). */
int eelg_tp_bwd(int cfg, const float* x, const float* sh, const float* w, const int* sender,
                const int* receiver, int n_edges, const float* grad_agg, float inv_norm,
                float* grad_w, float* gxe, void* stream);

/* BASELINE config 5 (bf16 storage, fp32 arithmetic): eelg_tp_fwd / eelg_tp_bwd with the
 * edge-sized tensors w, grad_w [E, weight_numel] and gxe [E, din] held as bf16 bit patterns
 * (uint16, round-to-nearest-even on store).  Same reference call sites
 * (gnn/blocks.py:590-597).  eelg_tp_fwd_bf16 moves rows by LDS-DMA like eelg_tp_fwd: x, sh
 * and w must be 16-byte aligned; -2 otherwise. */
int eelg_tp_fwd_bf16(int cfg, const float* x, const float* sh, const void* w, const int* sender,
                     const int* rowptr, int n_nodes, float inv_norm, float* agg, void* stream);
int eelg_tp_bwd_bf16(int cfg, const float* x, const float* sh, const void* w, const int* sender,
                     const int* receiver, int n_edges, const float* grad_agg, float inv_norm,
                     void* grad_w, void* gxe, void* stream);

/* eelg_tp_bwd / eelg_tp_bwd_bf16 with gxe written in sender order: the gxe row of edge e
 * is spos[e] (spos = inverse of the sender-CSR permutation sperm), so the sender sum
 * (eelg_segment_sum_csr with idx = NULL over srowptr) reads gxe contiguously.  Same
 * reference call sites (gnn/blocks.py:591-597). */
int eelg_tp_bwd_sorted(int cfg, const float* x, const float* sh, const float* w, const int* sender,
                       const int* receiver, const int* spos, int n_edges, const float* grad_agg,
                       float inv_norm, float* grad_w, float* gxe, void* stream);
int eelg_tp_bwd_sorted_bf16(int cfg, const float* x, const float* sh, const void* w,
                            const int* sender, const int* receiver, const int* spos, int n_edges,
                            const float* grad_agg, float inv_norm, void* grad_w, void* gxe,
                            void* stream);

/* eelg_tp_fwd / eelg_tp_bwd_sorted (and their _bf16 forms) over SHARED weight rows: the two
 * directions of a strut have equal edge features, hence equal rows of conv_tp_weights
 * (gnn/blocks.py:590), so w holds S <= E rows and wrow[E] (int32) names each edge's row in
 * [0, S).  Forward and backward read w[wrow[e]]; grad_w stays [E, weight_numel], one row per
 * edge in edge order, bitwise what the plain entry points give for the expanded w[wrow].
 * wrow == NULL: every edge its own row, exactly eelg_tp_fwd / eelg_tp_bwd_sorted.
 * Indices are not range-checked: 0 <= wrow[e] < S is the caller's contract. */
int eelg_tp_fwd_rows(int cfg, const float* x, const float* sh, const float* w, const int* wrow,
                     const int* sender, const int* rowptr, int n_nodes, float inv_norm, float* agg,
                     void* stream);
int eelg_tp_fwd_rows_bf16(int cfg, const float* x, const float* sh, const void* w, const int* wrow,
                          const int* sender, const int* rowptr, int n_nodes, float inv_norm,
                          float* agg, void* stream);
int eelg_tp_bwd_rows(int cfg, const float* x, const float* sh, const float* w, const int* wrow,
                     const int* sender, const int* receiver, const int* spos, int n_edges,
                     const float* grad_agg, float inv_norm, float* grad_w, float* gxe, void* stream);
int eelg_tp_bwd_rows_bf16(int cfg, const float* x, const float* sh, const void* w, const int* wrow,
                          const int* sender, const int* receiver, const int* spos, int n_edges,
                          const float* grad_agg, float inv_norm, void* grad_w, void* gxe,
                          void* stream);

/* Backward of eelg_tp_fwd in sender order: one pass over the sender CSR (srowptr [N+1],
 * sperm [E] = edge ids sorted by sender) that writes grad_w[E, weight_numel] at each edge's
 * row and grad_x[N, din] summed per sender in registers -- eelg_tp_bwd + the sender
 * eelg_segment_sum_csr in one launch, without the gxe [E, din] intermediate.  Same
 * reference call sites (gnn/blocks.py:591-597, the autograd of conv_tp + scatter).
 * _bf16: w / grad_w as bf16 bit patterns; grad_x is fp32 either way. */
int eelg_tp_bwd_sender(int cfg, const float* x, const float* sh, const float* w, const int* sperm,
                       const int* srowptr, const int* receiver, int n_nodes,
                       const float* grad_agg, float inv_norm, float* grad_w, float* grad_x,
                       void* stream);
int eelg_tp_bwd_sender_bf16(int cfg, const float* x, const float* sh, const void* w,
                            const int* sperm, const int* srowptr, const int* receiver,
                            int n_nodes, const float* grad_agg, float inv_norm, void* grad_w,
                            float* grad_x, void* stream);

/* Fused backward of linear(tp_interaction(x, sh, w)) -- the interaction's output o3.Linear
 * (7360 -> 800 at lmax 4) and the fused TP + scatter -- w.r.t. x and w, from the linear's output
 * gradient gy [n_nodes, target dim] and its flat weight lin_w (16-B aligned).  Replaces the
 * linear's grad-x followed by eelg_tp_bwd (gnn/blocks.py:591-604 autograd): grad_agg is computed
 * per receiver tile into LDS and never written to HBM.  Writes grad_w [E, wn] and the per-edge
 * grad_x rows gxe [E, din] in receiver-sorted edge order, as eelg_tp_bwd; rowptr is the receiver
 * CSR (int32 [n_nodes + 1]) and receiver the sorted edges' receivers (int32 [E]).  Generated for mul 32 (tpA_l*, tpB_l* only, not the "_h" sets); returns -2 for other configs.  The linear
 * is o3.Linear(irreps_mid.simplify(), target): eelg_tp_bwf_slot returns, per TP slot, the
 * weight offset of its 32 x 32 block, its alpha and its gy offset, for the caller to check
 * against its own linear before using this path. */
int eelg_tp_bwd_fused(int cfg, const float* x, const float* sh, const float* w, const int* sender,
                      const int* receiver,
                      const int* rowptr, int n_nodes, const float* gy, const float* lin_w,
                      float inv_norm, float* grad_w, float* gxe, void* stream);
int eelg_tp_bwd_fused_bf16(int cfg, const float* x, const float* sh, const void* w,
                           const int* sender, const int* receiver, const int* rowptr,
                           int n_nodes, const float* gy,
                           const float* lin_w, float inv_norm, void* grad_w, void* gxe,
                           void* stream);
int eelg_tp_bwf_slot(int cfg, int slot, int* w_off, float* alpha, int* gy_off);

/* CSR segmented sum (deterministic, no atomics):
 * out[r, :] = scale * row_scale[r] * sum_{j in [rowptr[r], rowptr[r+1])} src[idx ? idx[j] : j, :].
 * Replaces torch_scatter.scatter(..., reduce='sum'|'mean') (gnn/blocks.py:595-597,
 * gnn/model.py:100-106) on sorted segments; row_scale may be NULL. */
int eelg_segment_sum_csr(const float* src, const int* rowptr, const int* idx,
                         const float* row_scale, float scale, int n_rows, int width, float* out,
                         void* stream);

/* eelg_segment_sum_csr over bf16 source rows (bit patterns), fp32 accumulation and output:
 * the sender sums of the bf16 per-edge gradient gxe (config 5). */
int eelg_segment_sum_csr_bf16(const void* src, const int* rowptr, const int* idx,
                              const float* row_scale, float scale, int n_rows, int width,
                              float* out, void* stream);

/* Few long segments (per-graph pooling): each segment is cut into n_split pieces summed
 * separately into work[n_rows, n_split, width], then combined in a fixed order:
 * out[r, :] = scale * row_scale[r] * sum_pieces.  Same result contract as
 * eelg_segment_sum_csr (gnn/model.py:100-106 global mean pool), without the
 * one-wave-per-segment serialisation. */
/* Gate nonlinearity of the readout (e3nn nn.Gate, gnn/blocks.py:268-273): rows
 * x = [scalars | gates | gated blocks], y = [cst*silu(scalars) | gated block b channel u
 * times cst*silu(gate of (b, u))], cst = normalize2mom(silu).  blk_mul / blk_dim: the gated
 * blocks (mul copies of a (2l+1)-dim irrep, in row order); n_gates = sum of blk_mul.
 * eelg_gate_bwd writes grad_x for grad_y (one fused pass instead of the split / mul / cat and
 * their backward in torch). */
#define EELG_GATE_MAXBLK 8
#define EELG_GATE_MAXGATED 2048   /* gated elements per row (the kernels' LDS lookup tables) */
#define EELG_GATE_MAXGATES 512
typedef struct { int n_scal, n_gates, n_blk, pad; int blk_mul[EELG_GATE_MAXBLK]; int blk_dim[EELG_GATE_MAXBLK]; } eelg_gate_desc;
int eelg_gate_fwd(const float* x, int n_nodes, const eelg_gate_desc* desc, float cst, float* y,
                  void* stream);
int eelg_gate_bwd(const float* x, const float* grad_y, int n_nodes, const eelg_gate_desc* desc,
                  float cst, float* grad_x, void* stream);

int eelg_segment_sum_split(const float* src, const int* rowptr, const int* idx,
                           const float* row_scale, float scale, int n_rows, int width, int n_split,
                           float* work, float* out, void* stream);

/* torch_scatter's order reductions over CSR segments of src rows (rows rowptr[r]..rowptr[r+1]):
 * op 0 = max, 1 = min, 2 = mul.  Replaces scatter(..., reduce='max'|'min'|'mul') for
 * interaction_reduction (gnn/blocks.py:595-597, on the per-edge messages in receiver order)
 * and global_reduction (gnn/model.py:100-106, on the readout rows in graph order).
 * out[r, c]: the segment's first maximum / minimum (strict compare, so ties keep the earliest
 * row, torch_scatter's CPU arg) or its product; an empty segment gives 0 (max / min) or 1 (mul).
 * arg[r, c] (max / min only, required): the row of the kept element, -1 for an empty segment. */
int eelg_segment_order(const float* src, const int* rowptr, int n_rows, int width, int op,
                       float* out, int* arg, void* stream);
/* Backward: grad_src for every row of every segment (rows outside all segments are not
 * written): max / min -> grad_out at arg, 0 elsewhere (the whole gradient to one element, as
 * torch_scatter's scatter_max / scatter_min); mul -> grad_out times the product of the
 * segment's other entries (prefix x suffix products, exact at zeros).
 * Deliberate differences from torch_scatter on CUDA (parity unpinned, the oracle's torch.prod /
 * torch.max agree with these kernels): scatter_mul's backward divides the product by src, so
 * an entry that is exactly 0 gives NaN/inf there and a finite gradient here; scatter_max /
 * scatter_min on CUDA pick the arg of a tie by an atomic race, here it is always the first. */
int eelg_segment_order_bwd(const float* src, const int* rowptr, const int* arg, const float* grad_out,
                           int n_rows, int width, int op, float* grad_src, void* stream);

/* Principal-neighbourhood aggregation over CSR segments of src rows (interaction_reduction =
 * 'pna'): replaces PNASimple.forward (gnn/blocks.py:817-848; aggregators and scalers of
 * gnn/pna.py:20-31, 59-78), i.e. six torch_scatter passes, the [N, D, 12] stack of scaled
 * aggregates and Linear(12, 1), by one pass:
 *   out[r, c] = coef[r, 0] mean + coef[r, 1] min + coef[r, 2] max + coef[r, 3] std
 * over the rows rowptr[r]..rowptr[r+1] of src [E, width], with
 *   mean = sum / max(deg, 1), min / max = the first extreme in row order (as eelg_segment_order),
 *   std = sqrt(sum (m - mean)^2 / deg + 1e-5)   (centred: >= 0, the reference's relu is a no-op).
 * coef [n_rows, 4] = sum_s W[3k + s] scale_s(deg) is the caller's (the scalers identity,
 * log(deg + 1) / avg_log and its inverse, 1 at deg 0).  Saved for the backward: mean, std
 * [n_rows, width] and argmin, argmax [n_rows, width] (rows of src, -1 for an empty segment, which
 * gives mean = min = max = 0 and std = sqrt(1e-5)).  Any width >= 1: float4 columns when
 * width % 4 == 0 (all [., width] buffers 16-byte aligned, -2 otherwise), scalar columns else. */
int eelg_segment_pna_fwd(const float* src, const int* rowptr, const float* coef, int n_rows, int width,
                         float* out, float* mean, float* std, int* argmin, int* argmax, void* stream);
/* Backward: grad_src [E, width], every row of every segment written once (no zero fill when the
 * segments cover the rows):
 *   grad_src[e, c] = g (coef_mean / deg + coef_std (m_e - mean) / (deg std)
 *                       + coef_min [e == argmin] + coef_max [e == argmax]),  g = grad_out[r, c];
 * and grad_coef_part [eelg_segment_pna_parts(width), n_rows, 4]: the sums of g * (mean, min, max,
 * std) over each span of columns, in a fixed order (no atomics); grad_coef is their sum over the
 * leading dimension (eelg_sum_rows). */
int eelg_segment_pna_parts(int width);
int eelg_segment_pna_bwd(const float* src, const int* rowptr, const float* coef, const float* mean,
                         const float* std, const int* argmin, const int* argmax, const float* grad_out,
                         int n_rows, int width, float* grad_src, float* grad_coef_part, void* stream);

/* Crystal-graph edge convolution (CGC/mCGC benchmark models): replaces
 *   c = cat([x[sender], x[receiver], edge_ft]); msg = softplus(fc_values(c)) * sigmoid(fc_multip(c));
 *   scatter(msg, receiver, reduce)          (scripts/benchmark_models/cgc_modified.py:20-25,
 *                                            cgc_vanilla.py:20-25, gnn/blocks.py:960-966)
 * with the linear split by input block: ps = x W_s^T, pr = x W_r^T + b ([N, 2D], values
 * then multipliers), ep = edge_ft W_e^T ([E, 2D], receiver-sorted edge order).
 * agg[n] = row_scale[n] * sum_e softplus(zv) sigmoid(zm)  (row_scale NULL -> 'sum').
 * Built for D <= EELG_CGC_MAXD (the benchmark models use 128 and 64); -2 otherwise. */
#define EELG_CGC_MAXD 256   /* node_dim of the built CGC kernels (one lane per 64 channels, <= 4) */
int eelg_cgc_fwd(const float* ps, const float* pr, const float* ep, const int* sender,
                 const int* rowptr, const float* row_scale, int n_nodes, int D, float* agg,
                 void* stream);
/* Backward: dz[E, 2D] = d agg / d z per edge and grad_pr[N, 2D] = receiver sums of dz;
 * the sender sums are eelg_segment_sum_csr(dz, srowptr, sperm).  D <= EELG_CGC_MAXD as the forward. */
int eelg_cgc_bwd(const float* ps, const float* pr, const float* ep, const int* sender,
                 const int* rowptr, const float* row_scale, int n_nodes, int D,
                 const float* grad_agg, float* dz, float* grad_pr, void* stream);
/* The same edge convolution with factored edge features (both reference models embed the 5
 * per-edge inputs with one Linear, cgc_modified.py:71-74 / cgc_vanilla.py:60-63, so
 * Ep = [e5 | 1] A): ef[E, 8] = [e5 | 1 | 0 | 0] in CSR edge order and ea[8, 2D] (rows 0..5:
 * A = [W5^T W_e^T ; b5 W_e^T], rows 6..7 unused) replace ep[E, 2D]; the kernels form Ep in
 * registers.  Same outputs as eelg_cgc_fwd / eelg_cgc_bwd on Ep = ef[:, :6] @ ea[:6].
 * receiver[E] (the CSR's receiver of each sorted edge; may be NULL) enables the receiver-
 * streaming kernels: a wave walks the edges of 8 consecutive receivers in batches of 8, the
 * next batch's loads in flight (EELG_CGC_STREAM bit 0 forward, bit 1 backward; default 2). */
int eelg_cgc_fwd_ef(const float* ps, const float* pr, const float* ef, const float* ea,
                    const int* sender, const int* receiver, const int* rowptr,
                    const float* row_scale, int n_nodes, int D, float* agg, void* stream);
/* The factored forward with the layer residual added in the store (round 5):
 * agg[n] = row_scale[n] sum_e msg_e + res[n] (res [N, D], the layer input h of
 * h + conv(h), cgc_modified.py:77 / cgc_vanilla.py:69; NULL: no residual). */
int eelg_cgc_fwd_ef_res(const float* ps, const float* pr, const float* ef, const float* ea,
                        const int* sender, const int* rowptr, const float* row_scale, int n_nodes,
                        int D, const float* res, float* agg, void* stream);
int eelg_cgc_bwd_ef(const float* ps, const float* pr, const float* ef, const float* ea,
                    const int* sender, const int* receiver, const int* rowptr,
                    const float* row_scale, int n_nodes, int D, const float* grad_agg, float* dz,
                    float* grad_pr, float* dea_part, void* stream);
/* dea_part (may be NULL; needs receiver): per-workgroup partials [eelg_cgc_bwd_ef_parts(n), 6, 2D]
 * of d ea[0..5] = ef[:, :6]^T dz, summed by the caller (deterministic); a workgroup covers
 * 4 * EELG_CGC_RPW receivers. */
#define EELG_CGC_RPW 8
int eelg_cgc_bwd_ef_parts(int n_nodes);

/* Edge-conditioned convolution (NNConv benchmark model): replaces PyG's
 *   weight = nn(edge_attr).view(-1, D, D); msg = matmul(x_j.unsqueeze(1), weight).squeeze(1)
 *   (torch_geometric NNConv.message, as built by scripts/benchmark_models/nnconv_models.py:32-44
 *   and called at :73) with nn's last Linear + ReLU folded in:
 *   msg[e, o] = sum_i x[sender[e], i] relu(sum_k h[e, k] w3[i*D + o, k] + b3[i*D + o])
 * h [E, D]: the output of nn's first two Linear + ReLU; w3 [D*D, D], b3 [D*D]: nn's last Linear.
 * The [E, D*D] per-edge matrices exist only in MFMA accumulators (v_mfma_f32_32x32x2_f32, exact
 * fp32 products).  Edges in the receiver-sorted order of the CSR; the aggr='add' receiver sum is
 * eelg_segment_sum_csr(msg, rowptr).  Built for D in {32, 64}; -2 for another D or for a float
 * pointer that is not 16-byte aligned (rows are read as float4).  n_edges == 0 launches nothing. */
#define EELG_NNC_MAXD 64
int eelg_nnconv_fwd(const float* x, const float* h, const float* w3, const float* b3,
                    const int* sender, int n_edges, int D, float* msg, void* stream);
/* Backward w.r.t. the per-edge operands, Z recomputed per tile, g = grad_agg[receiver[e]] ([N, D],
 * the gradient of the receiver sums):
 *   gxe[e, i]    = sum_o relu(Z)[e, i, o] g[e, o]       (grad x = eelg_segment_sum_csr(gxe, srowptr, sperm))
 *   grad_h[e, k] = sum_{i, o} [Z > 0] x[sender[e], i] g[e, o] w3[i*D + o, k]
 * (autograd's backward of the matmul, the view and nn's last ReLU + Linear in the reference). */
int eelg_nnconv_bwd_edge(const float* x, const float* h, const float* w3, const float* b3,
                         const int* sender, const int* receiver, int n_edges, int D,
                         const float* grad_agg, float* gxe, float* grad_h, void* stream);
/* Backward w.r.t. nn's last Linear: part [eelg_nnconv_bwd_w_parts(n_edges, D), D*D*(D+1)], each
 * row = [grad w3 (D*D x D) | grad b3 (D*D)] over one contiguous range of edges,
 *   grad w3[i*D + o, k] = sum_e dZ[e, i, o] h[e, k],  grad b3[i*D + o] = sum_e dZ[e, i, o],
 *   dZ = [Z > 0] x[sender[e], i] g[e, o];
 * the caller sums the rows (eelg_sum_rows).  Partial-sum rule: the edges are cut into tiles of 32;
 * a part covers max(32, ceil(tiles / MAXPARTS)) tiles, MAXPARTS = 256 (D = 32) or 64 (D = 64).  So
 * every part but the last stands for at least 1024 edges (from a few thousand edges on the
 * partials are about (D+1)/1024 of the [E, D*D] tensor they replace, or less) and they never
 * exceed 33 MiB (D = 32) / 65 MiB (D = 64) in total (the [E, D*D] tensor at the benchmark's
 * 1 M edges: 4 GiB / 16 GiB).  The cap is what fills the device: D*D/32 * MAXPARTS one-wave workgroups. */
#define EELG_NNC_MAXPARTS_32 256
#define EELG_NNC_MAXPARTS_64 64
int eelg_nnconv_bwd_w_parts(int n_edges, int D);
int eelg_nnconv_bwd_w(const float* x, const float* h, const float* w3, const float* b3,
                      const int* sender, const int* receiver, int n_edges, int D,
                      const float* grad_agg, float* part, void* stream);

/* Sparse (CSR) x dense with strided operands:
 * out[r*ldo_r + c*ldo_c] = sum_{j in row r} val[j] * B[col[j]*ldb_r + c*ldb_c].
 * Builds the symmetric-contraction coefficients coef = U_sym . W and their weight
 * gradient U_sym^T . g (U_sym 1.6 % dense; replaces the dense U.W contraction of
 * gnn/mace.py:242-277 at the weight level). */
int eelg_csr_spmm(const int* rowptr, const int* col, const float* val, int n_rows, const float* B,
                  int ldb_r, int ldb_c, int n_cols, float* out, int ldo_r, int ldo_c, void* stream);

/* Symmetric contraction (correlation 3) as a sparse polynomial per (node, channel).
 * Replaces SymmetricContraction.forward (gnn/mace.py:173-177, 242-277).
 * x, out: [N, mul*D] mul-major rows; coef: [mul, coef_ld] (info[7]; entries past nterms are
 * read but unused), 16-byte aligned: each wave streams its channel's row into LDS by LDS-DMA in
 * 16-B pieces.  The row tensors (x, out, grad_out, grad_x) must be 16-byte aligned (float4 row
 * access); a misaligned pointer returns -2. */
int eelg_sc_fwd(int cfg, const float* x, const float* coef, int n_nodes, int mul, float* out,
                void* stream);
/* eelg_sc_fwd with the caller's row widths stated: x_row must be mul * D and out_row
 * mul * D_out of the set (a live-output set's rows are narrower than the full set's), else the
 * call fails with -2 and launches nothing. */
int eelg_sc_fwd_rows(int cfg, const float* x, int x_row, const float* coef, int n_nodes, int mul,
                     float* out, int out_row, void* stream);
int eelg_sc_bwd_x(int cfg, const float* x, const float* coef, const float* grad_out, int n_nodes,
                  int mul, float* grad_x, void* stream);
/* eelg_sc_bwd_x that also writes the channel-major copies xt[(c*D + a)*N + n] of x and
 * gt[(c*D_out + q)*N + n] of grad_out (the operands of eelg_sc_bwd_coef) from the tiles it
 * stages anyway, replacing two eelg_sc_cmajor passes; xt / gt may be NULL. */
int eelg_sc_bwd_x_cm(int cfg, const float* x, const float* coef, const float* grad_out,
                     int n_nodes, int mul, float* grad_x, float* xt, float* gt, void* stream);
/* eelg_sc_bwd_x_cm with the row widths of x / grad_x (x_row) and grad_out (grad_row) checked
 * against the set as in eelg_sc_fwd_rows. */
int eelg_sc_bwd_x_rows(int cfg, const float* x, int x_row, const float* coef, const float* grad_out,
                       int grad_row, int n_nodes, int mul, float* grad_x, float* xt, float* gt,
                       void* stream);
/* Channel-major copy xt[(c*D + a)*N + n] of a mul-major row tensor (feeds sc_bwd_coef);
 * which = 0: input (coupling) layout, 1: output layout. */
int eelg_sc_cmajor(int cfg, int which, const float* x, int n_nodes, int mul, float* xt,
                   void* stream);
/* Coefficient gradient (replaces the weight gradient through the U.W contraction of
 * gnn/mace.py:242-277) from the channel-major copies xt[(c*D + a)*N + n] / gt of x and
 * grad_out (eelg_sc_bwd_x_cm or eelg_sc_cmajor).  partial[n_parts, mul, coef_ld] (the
 * entries past nterms of each row are not written), n_parts = eelg_sc_bwd_coef_parts(cfg,
 * n_nodes, mul): one partial per node range (streaming kernel: ranges of whole coef_chunk-node
 * chunks, about 1024 / (mul x term-group sets) of them and at least 2048 nodes each; round-5
 * chunk kernel: one per coef_chunk nodes).  chunk must be the
 * config's coef_chunk (info[6]).  The caller sums over the partials (deterministic).
 * Non-overlapping xt / gt; 16-byte aligned rows (n_nodes % 4 == 0) take the LDS-DMA path. */
int eelg_sc_bwd_coef(int cfg, const float* xt, const float* gt, int n_nodes,
                     int mul, int chunk, float* partial, void* stream);
/* The number of partial rows eelg_sc_bwd_coef writes for n_nodes (-1: unknown config). */
int eelg_sc_bwd_coef_parts(int cfg, int n_nodes, int mul);

/* Symmetric contraction from a term table (correlation 4: U_matrix_real with filter_ir_mid,
 * gnn/mace.py:435-477; the contraction itself gnn/mace.py:242-277).  Replaces
 * SymmetricContraction.forward for the structures without generated kernels.
 * terms[t]: four 8-bit component indices (slot k at bits 8k; an unused slot = D, a constant 1),
 * sorted by output component, desc.orow[q] .. orow[q+1]-1 the terms of output q.  Component a of
 * channel c of node n: x[n*ldx + xb[a] + c*xs[a]]; outputs likewise (ob, os, ldo).
 * coef [mul, ldc], ldc a multiple of 64 >= nterms.  eelg_scg_bwd_coef writes deterministic
 * partials [ceil(n_nodes / EELG_SCG_CHUNK), mul, ldc] (term_out[t]: output of term t; padding
 * terms t >= nterms need indices D and output Dout: they produce 0); the caller sums them. */
#define EELG_SCG_MAXD 25
#define EELG_SCG_CHUNK 256
typedef struct {
  int D, Dout, mul, nterms;
  int xb[EELG_SCG_MAXD], xs[EELG_SCG_MAXD];
  int ob[EELG_SCG_MAXD], os[EELG_SCG_MAXD];
  int orow[EELG_SCG_MAXD + 1];
} eelg_scg_desc;
int eelg_scg_fwd(const eelg_scg_desc* d, const unsigned* terms, const float* x, int ldx, const float* coef,
                 int ldc, int n_nodes, float* out, int ldo, void* stream);
int eelg_scg_bwd_x(const eelg_scg_desc* d, const unsigned* terms, const float* x, int ldx, const float* coef,
                   int ldc, const float* grad_out, int ldg, int n_nodes, float* grad_x, void* stream);
int eelg_scg_bwd_coef(const eelg_scg_desc* d, const unsigned* terms, const int* term_out, int ldc, const float* x,
                      int ldx, const float* grad_out, int ldg, int n_nodes, float* partial, void* stream);

/* Channel-mixing linear on mul-major irreps rows (o3.Linear, gnn/blocks.py:516-521,
 * 553-559,471-476; gnn/model.py:82-86), fp32 MFMA.  A descriptor lists output
 * slots; each slot sums alpha * x_block @ W over its sources, W element
 * B[k][j] = w[w_off + k*ldk + j*ldj] (ldk = n_out, ldj = 1 forward; swapped for
 * grad-x), plus bias[bias_off + j] on scalar slots (bias_off < 0: none). */
#define EELG_LIN_MAXSRC 4
#define EELG_LIN_MAXSLOT 8
typedef struct { int x_off, k, w_off, ldk, ldj; float alpha; } eelg_lin_src;
typedef struct { int y_off, n_out, d, bias_off, n_src; eelg_lin_src src[EELG_LIN_MAXSRC]; int r_off; } eelg_lin_slot;
/* res_row / r_off: the layout of the residual operand of eelg_linear_fwd_res / _pk.  res_row = 0:
 * y's own (row stride y_row, slot offset y_off; r_off is ignored).  res_row > 0: rows of res_row
 * floats in which the slot's block starts at r_off, or r_off < 0: this slot adds no residual
 * (a compact y over some irreps of a wider residual row, or the reverse).  eelg_linear_fwd_pk
 * takes res_row = 0 only. */
typedef struct { int n_slots, max_jt, max_rows, res_row; eelg_lin_slot slot[EELG_LIN_MAXSLOT]; } eelg_lin_desc;
int eelg_linear_fwd(const float* x, int x_row, const float* w, const float* bias, int n_nodes,
                    float* y, int y_row, const eelg_lin_desc* desc, void* stream);
/* eelg_linear_fwd plus a residual res (y's layout, or desc->res_row / r_off; may be NULL)
 * added in the epilogue:
 * y = linear(x) + res, the layer residual h + layer_i(h) of gnn/model.py:92-96 with the
 * product block's o3.Linear (gnn/blocks.py:486) producing layer_i(h). */
int eelg_linear_fwd_res(const float* x, int x_row, const float* w, const float* bias,
                        const float* res, int n_nodes, float* y, int y_row,
                        const eelg_lin_desc* desc, void* stream);

/* The same linear on bf16 MFMA with fp32-accurate split operands (three exact bf16 parts of
 * every fp32 operand, six part products accumulated in fp32).  The weights come
 * pre-split by eelg_linear_pack for this descriptor: pack = bf16 [3][P], P =
 * eelg_linear_pack_size(desc) = sum over slots of n_out * (summed source K), entry
 * [p][off_slot + j*K_slot + k] = part p of alpha * W[k][j] (ldk / ldj of the descriptor, so a
 * grad-x descriptor packs W^T).  The packed path needs every slot to have whole 32-wide K
 * chunks and column tiles, d in {1,3,5,7,9} and 16-byte aligned rows / pack / res; else -2.
 * Replaces the same o3.Linear calls as eelg_linear_fwd_res. */
long long eelg_linear_pack_size(const eelg_lin_desc* desc);
int eelg_linear_pack(const float* w, const eelg_lin_desc* desc, void* pack, void* stream);
int eelg_linear_fwd_pk(const float* x, int x_row, const void* pack, const float* bias,
                       const float* res, int n_nodes, float* y, int y_row,
                       const eelg_lin_desc* desc, void* stream);

/* grad of the weights: partial[p, w_off + u*n_out + j] over node slices p of
 * nodes_per_slice nodes (sum over p on the caller side; deterministic).
 * n_partial must be >= ceil(n_nodes / nodes_per_slice). */
#define EELG_LINW_MAXINS 8
/* ldw: the row stride of the instruction's weight block in w, 0 = n_out (a dense [k, n_out]
 * block).  ldw > n_out addresses n_out columns of a wider block (w_off = the first column):
 * the live columns of a partly read output slot; the other entries of partial are not written. */
typedef struct { int x_off, k, g_off, n_out, d, w_off; float alpha; int ldw; } eelg_linw_ins;
typedef struct { int n_ins, max_jt, max_ut, max_rows; eelg_linw_ins ins[EELG_LINW_MAXINS]; } eelg_linw_desc;
int eelg_linear_bwd_w(const float* x, int x_row, const float* g, int g_row, int n_nodes,
                      int nodes_per_slice, float* partial, int n_partial, int w_total,
                      const eelg_linw_desc* desc, void* stream);
/* Dense weight gradient (a Linear y = x W^T, x [n_rows, k] row stride ldx, g = dL/dy [n_rows,
 * n_out] row stride ldg) on bf16 MFMA with fp32-accurate split operands (round 5; the weight
 * gradients of the CGC models' Linear layers, cgc_modified.py:11-25):
 * partial[s, j, kk] = sum over the rows r of split s (tiles_per_split 32-row tiles) of
 * g[r, j] x[r, kk], s < ceil(ceil(n_rows / 32) / tiles_per_split); the caller sums over s
 * (eelg_sum_rows) to grad W [n_out, k] in torch layout.  k in {32, 64, 96, 128}; -2 otherwise. */
int eelg_linear_bwd_w_x6(const float* g, int ldg, const float* x, int ldx, int n_rows, int n_out,
                         int k, int tiles_per_split, float* partial, void* stream);

/* Radial MLP of the interaction block, fused (gnn/blocks.py:537-549, applied at :590):
 *   [Linear(n_feat -> hidden) + SiLU] + ([Linear(hidden -> hidden) + SiLU]) * (n_hidden - 1)
 *   + Linear(hidden -> n_out, no bias)
 * on edge features feats[E, n_feat].  The hidden layers run on fp32 MFMA; the output layer and
 * its gradients on bf16 MFMA with fp32-accurate operand splitting (each fp32 operand = three
 * bf16 parts exactly, six part products accumulated in fp32; eelg_split_bf16x3).  Built for
 * hidden 32 / 64, n_hidden 1..3, n_feat <= 32, n_out a multiple of 8 (the reference default is
 * 12 -> 64 -> 64 -> weight_numel).  w / b: the hidden Linear weights [hidden, in] and biases
 * [hidden] in torch layout.  Forward: out[E, n_out] (fp32, or bf16 bit patterns when out_bf16)
 * and the pre-activations zsave[n_hidden, E, hidden] (the backward's operand); wo_parts =
 * eelg_split_bf16x3 of W_o [n_out, hidden] (bf16 [3][n_out][hidden], 16-byte aligned). */
#define EELG_RADIAL_MAXH 3
typedef struct {
  int n_feat, hidden, n_hidden, n_out;
  const float* w[EELG_RADIAL_MAXH];
  const float* b[EELG_RADIAL_MAXH];
} eelg_radial_desc;
int eelg_radial_fwd(const float* feats, int n_edges, const eelg_radial_desc* d, const void* wo_parts,
                    int out_bf16, float* zsave, void* out, void* stream);
/* parts[p*n + i] (bf16 bit patterns, p = 0..2): src[i] = parts[i] + parts[n+i] + parts[2n+i]
 * exactly (truncation split: the top 8 significant bits, the next 8, the rest). */
int eelg_split_bf16x3(const float* src, long long n, void* parts, void* stream);
/* Partial-buffer sizes of eelg_radial_bwd for E edges: part_h has n_part rows of
 * hidden*n_feat + hidden + (n_hidden-1)*(hidden^2 + hidden) floats (grad W_0, grad b_0, grad W_1,
 * ... in torch layout); part_wo is [n_split, n_out, hidden]. */
int eelg_radial_plan(int n_edges, int n_out, int* n_part, int* n_split);
/* Backward from grad_w[E, n_out] (fp32, or bf16 when grad_bf16; 16-byte aligned); wot_parts =
 * eelg_split_bf16x3 of W_o^T [hidden, n_out] (bf16 [3][hidden][n_out]):
 * per-wave / per-split partials of every weight and bias gradient; the caller sums part_h
 * and part_wo over their first axis (deterministic).  grad_h[E, hidden] is workspace (it
 * receives grad_w W_o).  No gradient w.r.t. feats (the reference's edge features carry
 * none). */
int eelg_radial_bwd(const void* grad_w, int grad_bf16, int n_edges, const eelg_radial_desc* d,
                    const void* wot_parts, const float* zsave, const float* feats, float* grad_h,
                    float* part_h, float* part_wo, void* stream);
/* The same backward with the hidden-layer weight and bias gradients left to the caller (hidden
 * 64): grad_h as above; gz[n_hidden, E, 64] = grad of the pre-activations z_n; hin[n_hidden - 1,
 * E, 64] = the inputs SiLU(z_{n-1}) of the hidden layers n >= 1; part_wo as above.  The caller
 * forms grad W_n = gz_n^T hin_n (n >= 1), grad W_0 = gz_0^T feats and grad b_n = column sums of
 * gz_n (eelg_linear_bwd_w / eelg_sum_rows). */
int eelg_radial_bwd_chain(const void* grad_w, int grad_bf16, int n_edges, const eelg_radial_desc* d,
                          const void* wot_parts, const float* zsave, float* grad_h, float* gz,
                          float* hin, float* part_wo, void* stream);
/* eelg_radial_bwd_chain for an MLP that ran on n_rows <= E shared rows (eelg_radial_fwd over
 * the representative feature rows; zsave [n_hidden, n_rows, 64]): zrow[E] (int32, 0 <= zrow[e] <
 * n_rows, not range-checked) names the row of edge e.  grad_w, grad_h, gz and hin are per edge,
 * in edge order, as in eelg_radial_bwd_chain, and every result is bitwise what that entry
 * gives for the expanded zsave[:, zrow].  zlast [E, 64] is workspace: the chain kernel leaves the
 * last layer's pre-activations there per edge for the W_o gradient to stream.  No [E, n_out]
 * tensor is expanded or summed per pair, and grad_w is read twice as there. */
int eelg_radial_bwd_chain_rows(const void* grad_w, int grad_bf16, int n_edges, const int* zrow,
                               int n_rows, const eelg_radial_desc* d, const void* wot_parts,
                               const float* zsave, float* grad_h, float* gz, float* hin,
                               float* zlast, float* part_wo, void* stream);

/* ---- Geometry gradients: d stiffness / d (positions, shifts, strut radii) -------------------
 * The reference model is plain differentiable torch, so autograd through its embedding
 * (gnn/model.py:139-157), conv_tp_weights (gnn/blocks.py:590) and conv_tp + scatter
 * (gnn/blocks.py:591-597) gives these; here they are three launches, all deterministic (no
 * atomics), used only when the geometry requires grad. */

/* SH gradient of eelg_tp_fwd (the reference call site gnn/blocks.py:591-597, differentiated
 * w.r.t. edge_attrs):
 *   grad_sh[e, l2^2 + j] = inv_norm * sum_{p with that l2} coef_p * sum_u w[e, p, u] *
 *       sum_{i,k} C_p[i,j,k] * x[sender(e), l1, u, i] * grad_agg[receiver(e), p, u, k].
 * grad_sh is [E, nshp] (rows padded to 16 bytes as the SH rows; the pad is written as 0);
 * sender / receiver are the receiver-sorted edges' ends; w is fp32.  sh is not read (the TP is
 * linear in it) and may be NULL.  -2 for a config without the kernel; no-op for n_edges == 0. */
int eelg_tp_bwd_sh(int cfg, const float* x, const float* sh, const float* w, const int* sender,
                   const int* receiver, int n_edges, const float* grad_agg, float inv_norm,
                   float* grad_sh /* [E, nshp] */, void* stream);

/* Input gradient of the radial MLP (conv_tp_weights, gnn/blocks.py:590): from grad_h[E, hidden]
 * (= grad_w W_o, as eelg_radial_bwd / eelg_radial_bwd_chain / eelg_radial_bwd_gh leave it) and
 * the saved pre-activations zsave[n_hidden, E, hidden], gz_n = grad_h_n SiLU'(z_n),
 * grad_h_{n-1} = gz_n W_n, grad_feats[E, n_feat] = gz_0 W_0.  Same shapes as the forward. */
int eelg_radial_bwd_x(const float* grad_h, int n_edges, const eelg_radial_desc* d,
                      const float* zsave, float* grad_feats, void* stream);
/* grad_h[E, hidden] = grad_w W_o alone (the first kernel of eelg_radial_bwd): what
 * eelg_radial_bwd_x needs when no weight of the MLP requires a gradient. */
int eelg_radial_bwd_gh(const void* grad_w, int grad_bf16, int n_edges, const eelg_radial_desc* d,
                       const void* wot_parts, float* grad_h, void* stream);

/* Backward of eelg_edge_embed (gnn/model.py:139-157 differentiated w.r.t. the edge vector and
 * the radius): from grad_sh[E, grad_sh_ld] (row stride >= (lmax+1)^2) and grad_feats[E, 2*nb],
 * grad_vec[E, 4] = [d/d vx, d/d vy, d/d vz, 0] (16-byte aligned) with v = pos[recv] - pos[send] +
 * shift, and grad_radius[E].  The caller sums grad_vec per receiver minus per sender
 * (eelg_segment_sum_csr) for the node gradient; grad_vec itself is the shifts' gradient. */
int eelg_edge_embed_bwd(const float* pos, const int* sender, const int* receiver,
                        const float* shifts, const float* radius, int n_edges, int lmax, int nb,
                        float len_end, float rad_end, const float* grad_sh, int grad_sh_ld,
                        const float* grad_feats, float* grad_vec, float* grad_radius,
                        void* stream);

/* Deterministic sum over the leading dimension of partial results (the partial buffers of
 * eelg_linear_bwd_w, eelg_radial_bwd and eelg_sc_bwd_coef, and the bias gradients = column
 * sums of grad_out; replaces the reference's implicit autograd reductions, gnn/blocks.py and
 * e3nn o3.Linear biases): out[c] = scale * sum_{r < rows} part[r*ld + c] for c < cols, rows
 * summed in a fixed order.  rows > 256 needs a workspace of eelg_sum_rows_work(rows, cols)
 * floats (0 otherwise).  16-byte aligned part / out with ld, cols multiples of 4 take the
 * float4 path.  -2 on bad sizes. */
long long eelg_sum_rows_work(int rows, long long cols);
int eelg_sum_rows(const float* part, long long ld, int rows, long long cols, float scale, float* out,
                  float* work, long long work_len, void* stream);

/* ---- Batch assembly from a device-resident packed dataset ---------------------------------
 * Replaces, per training batch, PyG's collation of the sampled graphs (concatenated node / edge
 * tensors, edge_index offset by the running node count, the sorted `batch` vector and `ptr`;
 * field layout gnn/datasets.py:256-269), the rotation augmentation RotateLat applies to every
 * sample (scripts/train_utils.py:114-146: positions and shifts times Q^T, the rank-4 targets by
 * four factors of Q) and the two stable sorts + two searches that rebuild the receiver / sender
 * CSR of the collated batch.  The packed dataset holds every graph once: node and edge rows in
 * the graph's own order, LOCAL sender / receiver indices, and the graph's local CSR (perm, sperm
 * and the row ends rowptr[1:], srowptr[1:]).  A stable sort by receiver (or sender) of a collated
 * batch never interleaves graphs, so the batch's CSR is the concatenation of the local ones plus
 * the output offsets: nothing is sorted here.
 *
 * table [4, n_graphs + 1] int32, per slot g of the batch (a graph may fill several slots):
 *   row 0: first output node (row 0 is strictly increasing: every graph has >= 1 node; entry
 *          n_graphs = n_nodes),  row 1: first output edge (entry n_graphs = n_edges),
 *   row 2: first node of the slot's graph in the packed tensors,  row 3: its first edge
 *   (entry n_graphs of rows 2 and 3 is not read).
 * rot [n_graphs, 3, 3] (may be NULL): positions and shifts of slot g become Q_g v (row form
 * v Q_g^T, three fmaf in the order k = 0, 1, 2); NULL copies them unmultiplied.
 * Outputs, per output node i of slot g (source row s): positions, node_attrs, batch[i] = g
 * (int64), rowptr[i + 1] = rowend[s] + edge offset (likewise srowptr; entry 0 = 0), and
 * ptr[g + 1] = the slot's node end (int64 [n_graphs + 1]).  Per output edge j of slot g (source
 * row s): edge_index[0 / 1][j] = local sender / receiver + node offset (int64 [2, n_edges], the
 * graph's own edge order), shifts, edge_attr, perm[j] = local perm + edge offset (int64),
 * sperm[j] likewise (int32), sender[j] / receiver[j] = the endpoints of the graph's edge perm[s]
 * + node offset (int32, receiver-sorted order).
 * One launch, one thread per output node and per output edge; everything fp32 / integer copies,
 * no atomics: bitwise repeatable.  Rows are 12 bytes, so there is no float4 path.  A source row
 * outside [0, total_nodes) / [0, total_edges) (a corrupt table) is skipped, not read.
 * -2: negative sizes, node_w / edge_w outside 1..EELG_BATCH_MAXW, null pointers.  n_graphs == 0
 * (or n_nodes == 0): nothing is launched, 0 is returned.  n_edges == 0: the edge outputs may be
 * NULL. */
#define EELG_BATCH_MAXW 64
typedef struct {
  const float* positions;   /* [total_nodes, 3] */
  const float* node_attrs;  /* [total_nodes, node_w] */
  const int* rowend;        /* [total_nodes] local rowptr[1:] of each graph */
  const int* srowend;       /* [total_nodes] local srowptr[1:] */
  const int* sender;        /* [total_edges] local, the graph's own edge order */
  const int* receiver;
  const float* shifts;      /* [total_edges, 3] */
  const float* edge_attr;   /* [total_edges, edge_w] */
  const int* perm;          /* [total_edges] local receiver-sorted order */
  const int* sperm;         /* [total_edges] local sender order over it */
  int node_w, edge_w, total_nodes, total_edges;
} eelg_batch_src;
typedef struct {
  float* positions; float* node_attrs; int64_t* batch; int64_t* ptr; int* rowptr; int* srowptr;
  int64_t* edge_index; float* shifts; float* edge_attr; int64_t* perm; int* sperm; int* sender;
  int* receiver;
} eelg_batch_out;
int eelg_batch_assemble(const eelg_batch_src* src, const int* table, const float* rot, int n_graphs,
                        int n_nodes, int n_edges, const eelg_batch_out* out, void* stream);

/* Per-graph Mandel 6x6 targets of a batch: out[g] = M(Q_g) src[sel[g]] M(Q_g)^T, the Mandel form
 * of RotateLat's rank-4 rotation einsum('ijkl,ai,bj,ck,dl->abcd') (scripts/train_utils.py:
 * 131-136) followed by the cartesian -> Mandel conversion.  Mandel order 11, 22, 33, 23, 13, 12,
 * weights w = (1, 1, 1, r2, r2, r2), r2 = sqrt(2); for a <-> (i, j), b <-> (k, l):
 *   M_ab = (w_a / w_b) Q_ik Q_jk (b <= 3),  (w_a / w_b) (Q_ik Q_jl + Q_il Q_jk) (b > 3).
 * src [n_src, 6, 6], sel [n_graphs] int32 rows of src, rot [n_graphs, 3, 3] or NULL (out[g] =
 * src[sel[g]], copied), out [n_graphs, 6, 6].  One thread per output entry; fixed order.
 * A sel entry outside [0, n_src) is skipped.  -2: negative sizes, null pointers. */
int eelg_mandel_rotate(const float* src, int n_src, const int* sel, const float* rot, int n_graphs,
                       float* out, void* stream);

/* ---- Validation / test metrics of predicted stiffness matrices -----------------------------
 * One launch for what LightningWrappedModel.validation_step (scripts/train_utils.py:66-89) and
 * obtain_errors (scripts/train_utils.py:149-171) compute per graph: stiffness_Mandel_to_cart_4,
 * einsum('...ijkl,pi,pj,pk,pl->...p') of target and prediction over [B, 3, 3, 3, 3], and two
 * torch.linalg.eigvalsh calls on [B, 6, 6].
 * pred, target [n_graphs, 6, 6] fp32 Mandel (order 11, 22, 33, 23, 13, 12, as eelg_mandel_rotate),
 * dirs [n_dirs, 3] unit vectors, out [n_graphs, EELG_METRICS_COLS].  Both matrices are multiplied
 * by `scale` first (obtain_errors: 10, validation: 1; the products are rounded to fp32 before any
 * difference is taken).  Row of graph g:
 *   0 mseloss         mean_ij (C^ - C)^2
 *   1 loss            mean_ij |C^ - C|
 *   2 dir_loss        mean_p |c_p - c^_p|,  c_p = v_p^T C v_p,
 *                     v = (d1^2, d2^2, d3^2, r2 d2 d3, r2 d1 d3, r2 d1 d2), r2 = sqrt(2): the
 *                     reference's einsum over the cartesian tensor, also for a C that is not
 *                     exactly symmetric; no rank-4 tensor is formed
 *   3 mean_stiffness  mean_p c_p of the target
 *   4..9   target_eig     eigenvalues of the target, ascending
 *   10..15 predicted_eig  eigenvalues of the prediction, ascending
 * Eigenvalues: cyclic Jacobi in fp32 (csrc/eelg_jacobi.h) on the symmetric matrix taken from the
 * LOWER triangle (eigvalsh's UPLO = 'L': the upper triangle is never read), a fixed number of
 * sweeps (EELG_JACOBI_SWEEPS), so any input terminates; a NaN input gives NaN in the columns that
 * depend on it and in no other graph's row.
 * One wavefront per graph, directions strided over the lanes, fixed xor-butterfly sums; no LDS,
 * scratch or atomics.  A graph's row depends on (its two matrices, dirs, n_dirs, scale) alone:
 * bitwise equal in any batch, at any position, on every run.
 * n_graphs == 0: nothing is launched, 0 is returned whatever the pointers.  -2: n_graphs < 0,
 * n_dirs <= 0, a null pointer. */
#define EELG_METRICS_COLS 16
int eelg_stiffness_metrics(const float* pred, const float* target, const float* dirs, int n_graphs,
                           int n_dirs, float scale, float* out, void* stream);

/* ---- Elastic properties of predicted stiffness matrices and their gradient ------------------
 * (csrc/eelg_elastic.hip; the arithmetic of one matrix in csrc/eelg_elastic.h)
 * c [n_graphs, 6, 6] fp32 Mandel, dirs [n_dirs, 3] unit vectors (NULL with n_dirs == 0).  The
 * function is defined on the symmetric part A = (C + C^T) / 2 (both triangles are read), S = A^-1
 * by a Cholesky factorisation in fp64 inside the kernel.  a, b, c of a matrix: the sums of its
 * three normal diagonal entries, its three normal off-diagonal entries (one triangle) and its three
 * shear diagonal entries.  Row of graph g in props [n_graphs, EELG_ELASTIC_COLS]:
 *   0 K_V   (a_A + 2 b_A) / 9                    1 G_V   (a_A - b_A + 1.5 c_A) / 15
 *   2 K_R   1 / (a_S + 2 b_S)                    3 G_R   15 / (4 a_S - 4 b_S + 6 c_S)
 *   4 K_H   (K_V + K_R) / 2                      5 G_H   (G_V + G_R) / 2
 *   6 E_H   9 K_H G_H / (3 K_H + G_H)            7 nu_H  (3 K_H - 2 G_H) / (2 (3 K_H + G_H))
 *   8 A_U   5 G_V / G_R + K_V / K_R - 6
 *   9 E_min, 10 E_max   the extremes of e_dir's row (NaN with n_dirs == 0); on a tie the first
 *                       direction is the extreme, also for the gradient
 *   11 spd  1.0 if every pivot of the factorisation is finite and > 0, else 0.0
 * e_dir [n_graphs, n_dirs]: E_p = 1 / (m_p^T S m_p), m = (d1^2, d2^2, d3^2, r2 d2 d3, r2 d1 d3,
 * r2 d1 d2).  s [n_graphs, 6, 6]: the compliance, kept for the backward.  A graph with spd == 0 has
 * K_V and G_V only: its other columns, its e_dir row and its s are NaN.
 *
 * eelg_elastic_props_bwd: g_c [n_graphs, 6, 6] (exactly symmetric) from the cotangents g_props
 * [n_graphs, EELG_ELASTIC_COLS] and g_e_dir [n_graphs, n_dirs] (NULL: zero) and the forward's s,
 * e_dir and props: the direct terms of K_V and G_V plus -S G_S S, G_S collecting the a, b, c terms
 * of the Reuss / Hill / A_U columns and -E_p^2 m m^T per direction (E_min / E_max on their first
 * extreme).  The spd column has no gradient.  A graph with spd == 0 gets the Voigt terms alone: the
 * cotangents of its NaN columns are not read, so they contribute exactly zero.
 *
 * One wavefront per graph, directions strided over the lanes, fixed xor butterflies (sums, and
 * (value, index) pairs for the extremes); no LDS, scratch or atomics.  A graph's row and gradient
 * depend on (its matrix, dirs, n_dirs, its cotangents) alone: bitwise equal in any batch, at any
 * position, on every run.
 * n_graphs == 0: nothing is launched, 0 is returned whatever the pointers.  -2: n_graphs < 0,
 * n_dirs < 0, a null pointer (dirs, e_dir: only with n_dirs > 0). */
#define EELG_ELASTIC_COLS 12
int eelg_elastic_props(const float* c, const float* dirs, int n_graphs, int n_dirs, float* props,
                       float* e_dir, float* s, void* stream);
int eelg_elastic_props_bwd(const float* s, const float* dirs, const float* e_dir, const float* props,
                           const float* g_props, const float* g_e_dir, int n_graphs, int n_dirs,
                           float* g_c, void* stream);

/* ---- Shear, Poisson's ratio and compressibility surfaces and their gradient --------------------
 * (csrc/eelg_transverse.hip; the arithmetic of one matrix and one direction in
 * csrc/eelg_transverse.h)
 * c, dirs, A and S = A^-1 (fp64) as above.  For a unit direction d and a unit n orthogonal to d
 *   G(d, n)  = 1 / (4 S'_1212)        nu(d, n) = -S'_1122 / S'_1111        beta(d) = S_ijkk d_i d_j
 * with S' the compliance in a frame whose first two axes are d and n.  Both 1 / G and nu are a mean
 * plus one sinusoid in twice the transverse angle, so their extremes over n are closed forms:
 *   frame   j = the first index of the smallest |d_j|, t1 = normalize(d x e_j), t2 = d x t1
 *   M(T)    = (T11, T22, T33, r2 T23, r2 T13, r2 T12),  sym(u (x) v) = (u v^T + v u^T) / 2
 *   a = m(d), T1 = M(sym(d (x) t1)), T2 = M(sym(d (x) t2)), b1 = m(t1), b2 = m(t2),
 *   X = M(sym(t1 (x) t2)), u = S a, E = 1 / (a^T u)
 *   shear   A11 = T1^T S T1, A22 = T2^T S T2, A12 = T1^T S T2
 *           M_G = 2 (A11 + A22), R_G = 2 hypot(A11 - A22, 2 A12)
 *           G_lo = 1 / (M_G + R_G), G_hi = 1 / (M_G - R_G)
 *   Poisson B1 = u^T b1, B2 = u^T b2, Bx = u^T X
 *           M_nu = (B1 + B2) / 2, R_nu = hypot((B1 - B2) / 2, Bx)
 *           nu_lo = -E (M_nu + R_nu), nu_hi = -E (M_nu - R_nu)
 *   beta    = u_1 + u_2 + u_3
 * t_dir [n_graphs, n_dirs, EELG_TRANSVERSE_DIR_COLS]: 0 G_lo, 1 G_hi, 2 nu_lo, 3 nu_hi, 4 beta.
 * props [n_graphs, EELG_TRANSVERSE_COLS]:
 *   0 G_min = min_p G_lo, 1 G_max = max_p G_hi, 2 nu_min = min_p nu_lo, 3 nu_max = max_p nu_hi,
 *   4 beta_min, 5 beta_max: first extremes of the stored fp32 values (the smaller index wins a tie,
 *   a NaN never wins; NaN with n_dirs == 0);  6 spd as in eelg_elastic_props.
 * arg [n_graphs, 6] int32: the direction index of each extreme (-1 where the extreme is NaN).
 * n_ext [n_graphs, 4, 3]: the transverse unit vector n = cos(th) t1 + sin(th) t2 at which G_min,
 * G_max, nu_min, nu_max are taken in their direction: 2 th = atan2(2 A12, A11 - A22) resp.
 * atan2(Bx, (B1 - B2) / 2), plus pi for G_max / nu_max; an amplitude of exactly 0 gives th = 0 resp.
 * pi / 2.  s [n_graphs, 21] fp64: the packed lower triangle of S (entry (i, j), i >= j, at
 * i (i + 1) / 2 + j), kept for the backward: the unit vector (p, q) / R of a hypot amplifies the
 * rounding of S by M / R, so an fp32 copy is not enough.  A graph with spd == 0: spd 0, NaN in every
 * other entry of props, t_dir, n_ext and s, arg -1.
 *
 * eelg_transverse_props_bwd: g_c [n_graphs, 6, 6] (exactly symmetric) = -S G_S S from the
 * cotangents g_props [n_graphs, EELG_TRANSVERSE_COLS] and g_t_dir [n_graphs, n_dirs,
 * EELG_TRANSVERSE_DIR_COLS] (NULL: zero) and the forward's s, props (the spd column) and arg.  Every
 * term of G_S is d(x^T S y) / dS = sym(x y^T); a hypot passes (p dp + q dq) / R and exactly 0 where
 * R == 0; the cotangent of an extreme goes to the direction arg names, alone.  A graph with spd == 0
 * gets exactly zero: none of its cotangents is read.
 *
 * One wavefront per graph, directions strided over the lanes, fixed xor butterflies; no LDS, scratch
 * or atomics.  A graph's rows and gradient depend on (its matrix, dirs, n_dirs, its cotangents)
 * alone: bitwise equal in any batch, at any position, on every run.
 * n_graphs == 0: nothing is launched, 0 is returned whatever the pointers.  -2: n_graphs < 0,
 * n_dirs < 0, a null pointer (dirs, t_dir: only with n_dirs > 0), s not aligned to 8 bytes. */
#define EELG_TRANSVERSE_COLS 7
#define EELG_TRANSVERSE_DIR_COLS 5
int eelg_transverse_props(const float* c, const float* dirs, int n_graphs, int n_dirs, float* props,
                          float* t_dir, int* arg, float* n_ext, double* s, void* stream);
int eelg_transverse_props_bwd(const double* s, const float* dirs, const float* props, const int* arg,
                              const float* g_props, const float* g_t_dir, int n_graphs, int n_dirs,
                              float* g_c, void* stream);

/* ---- The tail of the training step: loss, gradient norm, clip + AdamW --------------------------
 * (csrc/eelg_optim.hip; per-element arithmetic in csrc/eelg_adamw.h)
 *
 * eelg_stiffness_loss: LightningWrappedModel.training_step's loss (scripts/train_utils.py:52-60)
 * and its gradient in one launch.  pred, target [n_graphs, n] fp32 with n = 36 (a [B, 6, 6]
 * stiffness) or 21 (the vanilla CGC benchmark's upper triangle).
 *   out[0] = 100 * mean_b( mean_i (pred - target)^2 / mean_i target^2 )   the loss
 *   out[1] = mean_b( mean_i (pred - target)^2 )                           logged as 'stiffness_loss'
 *   grad [n_graphs, n] = grad_scale * d out[0] / d pred   (grad_scale: 1 / accumulate_grad_batches)
 * One workgroup, one wavefront per graph at a time, every sum in a fixed order that depends on
 * (n_graphs, n) alone: no atomics, no scratch, bitwise repeatable.  A target row of zeros gives
 * Inf / NaN as the reference's division does.  -2: n_graphs < 1, n not 36 or 21, a null pointer.
 *
 * eelg_sqnorm_parts / eelg_grad_sqnorm: partials[0 .. parts) = sums of squares of contiguous
 * chunks of grad [numel] (fp32, 16-byte aligned), parts = min(EELG_SQNORM_MAXPARTS,
 * ceil(numel / EELG_SQNORM_CHUNK)): a function of numel alone, never of the device.  Plain stores,
 * every partial overwritten on every call, fixed summation order.  A square that overflows fp32
 * (|g| > 1.8e19) makes the norm Inf.
 *
 * eelg_adamw_flat: one launch over flat fp32 buffers of numel elements (16-byte aligned):
 *   norm  = sqrt(sum of the partials), combined in fp64 in the same order by every block
 *   coef  = min(1, max_norm / (norm + 1e-6))  (clip_grad_norm_); 1 when max_norm <= 0
 *   torch.optim.AdamW's rule on (p, m = exp_avg, v = exp_avg_sq, vmax = max_exp_avg_sq; vmax may
 *   be NULL without amsgrad) with the gradient coef * grad, decoupled decay p *= 1 - lr wd, bias
 *   corrections from the step count state_in[0] + 1, denom = sqrt(vmax or v) / sqrt(bc2) + eps
 *   grad  = 0 everywhere
 * State rows are 4 x int32: {steps taken, launches skipped, bits of the last norm, bits of the
 * last coefficient}.  The launch reads state_in and writes state_out, which must be two different
 * rows (the caller alternates them by its own call count), and it does not write the partials:
 * no block overwrites what another block of the same launch reads.  A norm that is not finite
 * leaves p, m, v, vmax untouched and the step count as it was, adds one to `skipped`, stores coef
 * 0, and still zeroes grad.  Hyper-parameters come by value (doubles, as torch holds them).
 * Vector stores only; no atomics.  -2: numel < 1, a null or misaligned pointer, state_in ==
 * state_out. */
#define EELG_SQNORM_CHUNK 8192
#define EELG_SQNORM_MAXPARTS 1024
#define EELG_OPTIM_STATE_COLS 4
int eelg_stiffness_loss(const float* pred, const float* target, int n_graphs, int n, float grad_scale,
                        float* out, float* grad, void* stream);
int eelg_sqnorm_parts(long long numel);
int eelg_grad_sqnorm(const float* grad, long long numel, float* partials, void* stream);
int eelg_adamw_flat(float* p, float* m, float* v, float* vmax, float* grad, long long numel,
                    const float* partials, double lr, double beta1, double beta2, double eps,
                    double weight_decay, double max_norm, int amsgrad, const int* state_in, int* state_out,
                    void* stream);

/* ---- Gradient-based lattice design: strut volume and the design step ----------------------------
 * (csrc/eelg_design.hip; per-element arithmetic in csrc/eelg_design.h)
 * A batch of n_graphs lattices in the caller's node / edge order: pos [n_nodes, 3], r [n_edges]
 * (strut radii, every strut listed in both directions), shifts [n_edges, 3], send / recv [n_edges]
 * int32 (batch-global node rows), node_ptr / edge_ptr [n_graphs + 1] int32 on the device: graph g
 * owns the nodes node_ptr[g] .. node_ptr[g + 1] and the edges edge_ptr[g] .. edge_ptr[g + 1] (a
 * graph's edges are contiguous).  node_ptr_host / edge_ptr_host: the same two rows in host memory;
 * a launch cannot read device memory without waiting for the device, so these are what it checks
 * (-2 unless each starts at 0, never decreases and ends at n_nodes / n_edges).  The kernels cut
 * the device rows to the arrays and refuse a graph whose send / recv (or partner) leave its own
 * rows, so a device row that disagrees with its mirror gives that graph NaN (and
 * EELG_DESIGN_BAD_INDEX), never an access outside the arrays.
 *
 * eelg_strut_volume: vol[g] = 1/2 sum over the directed edges e of g of r_e^2 L_e, L_e =
 * |(pos[recv] - pos[send]) + shift_e| with the vector formed in fp32 as eelg_edge_embed forms it;
 * pi and the cell volume are constant for a fixed cell, so this is the relative density up to a
 * factor.  Terms and sum in fp64 in a fixed order, rounded to fp32 once.  Forward only.
 *
 * eelg_design_step: the tail of one design iteration, in place on pos, r and the momenta m_pos
 * [n_nodes, 3], m_r [n_edges], from the gradients g_pos, g_r of the objective to minimise.
 * partner [n_edges] int32, caller order: the edge that is the other direction of the same strut,
 * or the edge itself.  pos0: the initial positions.  v0 [n_graphs]: the volume to keep.  Per graph:
 *   1. g~_r[e] = g_r[e] + g_r[partner[e]] (partner[e] != e), else g_r[e]: bitwise equal in both
 *      directions of a strut.
 *   2. If any g~_r or g_pos of the graph is Inf or NaN: nothing of the graph changes, flag[g] =
 *      EELG_DESIGN_NONFINITE (1), vol[g] = its current volume.
 *   3. G_r = max |g~_r|, G_p = max |g_pos| over the graph.  A group (radii, positions) whose
 *      maximum is 0 or whose step size is 0 is left as it is, momentum included.
 *   4. m_r = beta m_r + g~_r / G_r, r = clamp(r - step_r m_r, r_min, r_max); m_pos = beta m_pos +
 *      g_pos / G_p, pos = clamp(pos - step_pos m_pos, pos0 - move_limit, pos0 + move_limit) per
 *      component.  step_* is the largest move of an iteration from rest, in length units.
 *   5. V of the new geometry; with keep_volume, r = clamp(r sqrt(v0 / V), r_min, r_max) in one
 *      pass and V again.  Where a clamp binds V may miss v0; that is not iterated.  A v0 or V that
 *      is not a positive finite number leaves the radii unscaled.
 *   6. vol[g] = V, flag[g] = 0.
 * Struts that arrive with bitwise-equal radii and momenta in both directions leave that way.
 * One workgroup of EELG_DESIGN_THREADS threads per graph; a graph's outputs depend on its own rows
 * alone: bitwise equal in any batch, at any position, on every run.  No atomics, no scratch, LDS
 * for the reduction slots only.
 * -2: n_graphs < 1, negative sizes, a null pointer, ptr rows that fail the check above, r_min >=
 * r_max, move_limit < 0.  n_edges == 0: eelg_design_step launches nothing (0 is returned, vol and
 * flag are not written); eelg_strut_volume stores zeros. */
#define EELG_DESIGN_THREADS 256
int eelg_strut_volume(const float* pos, const float* r, const float* shifts, const int* send,
                      const int* recv, const int* node_ptr, const int* edge_ptr,
                      const int* node_ptr_host, const int* edge_ptr_host, int n_graphs, int n_nodes,
                      int n_edges, float* vol, void* stream);
int eelg_design_step(const float* g_pos, const float* g_r, float* pos, float* r, const float* pos0,
                     float* m_pos, float* m_r, const int* partner, const int* node_ptr,
                     const int* edge_ptr, const int* node_ptr_host, const int* edge_ptr_host,
                     const float* shifts, const int* send, const int* recv, const float* v0,
                     int n_graphs, int n_nodes, int n_edges, float step_r, float step_pos, float beta,
                     float r_min, float r_max, float move_limit, int keep_volume, float* vol, int* flag,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EELG_H */
