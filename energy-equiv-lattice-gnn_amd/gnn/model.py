"""``GNN_Head`` / ``EnergyEquivGNN`` (reference ``gnn/model.py:26-161``), MI355X-native.

Same constructor (``params`` Namespace), module tree, parameter names and
``forward(batch) -> {'stiffness': [B, 6, 6]}`` as the reference.  Per forward:

1. the batch's receiver-sorted CSR is built once on the device (or taken from
   ``batch.csr`` when the collate already made it) and every edge tensor is
   permuted once into that order;
2. ``eelg_edge_embed`` computes edge vectors, the 2x6 Gaussian edge features
   and the l<=lmax spherical harmonics in one kernel;
3. each ``MACELayer`` runs the fused HIP interaction and the HIP symmetric
   contraction; channel-mixing linears and the readout tail are GEMMs;
4. the per-graph mean pool is ``eelg_segment_sum_csr`` over the sorted
   ``batch`` vector.
"""
from __future__ import annotations

import os
from argparse import Namespace
from typing import Any, Dict

import torch

from . import ops
from .blocks import (Cart_4_to_Mandel, GeneralNonLinearReadoutBlock, MACELayer, PositiveLayer,
                     Spherical_to_Cartesian, as_csr)
from .irreps import Irreps
from .o3 import Linear


def storage_dtype(params: Namespace) -> torch.dtype:
    """Optional ``params.storage_dtype`` ('float32' default, or 'bfloat16'): storage type of
    the edge-sized interaction tensors (BASELINE config 5: bf16 storage, fp32 accumulate).
    Not a reference field; the reference path is all fp32."""
    name = str(getattr(params, "storage_dtype", "float32")).replace("torch.", "")
    table = {"float32": torch.float32, "fp32": torch.float32, "bfloat16": torch.bfloat16,
             "bf16": torch.bfloat16}
    if name not in table:
        raise ValueError(f"storage_dtype {name!r}: expected 'float32' or 'bfloat16'")
    return table[name]


# every layer's radial MLP done before layer 1 starts (they overlap layer 0 only)
RADIAL_AHEAD_OF_LAYER1 = os.environ.get("EELG_RADIAL_BEFORE_L1", "1") != "0"
# every layer's contraction coefficients issued at the start of the forward (GNN_Head._coefficients_ahead)
COEF_AHEAD = os.environ.get("EELG_COEF_AHEAD", "1") != "0"


def _live_inputs(lin: Linear, live_out) -> tuple:
    """the input slots of an ``o3.Linear`` that reach one of its output slots ``live_out``"""
    return tuple(sorted({i for i, o in lin.instructions if o in set(live_out)}))


def _merge_pieces(pieces):
    """adjacent channel ranges of one slot joined"""
    out = []
    for s, c0, cnt in sorted(pieces):
        if out and out[-1][0] == s and out[-1][1] + out[-1][2] == c0:
            out[-1] = (s, out[-1][1], out[-1][2] + cnt)
        else:
            out.append((s, c0, cnt))
    return tuple(out)


def readout_liveness(readout: GeneralNonLinearReadoutBlock, final: Linear) -> Dict[str, tuple]:
    """Which parts of the readout can reach the output of ``final`` (the stiffness linear),
    walked back through the module structure: an ``o3.Linear`` joins equal irreps only
    (its ``instructions``), the Gate passes a scalar slot through and multiplies a gated slot
    by its own gate scalars (so a gate is live exactly when its gated slot is), and the pool
    in between is per column.  Returns the live slots / pieces per module:

    * ``final_in``: slots of ``final.irreps_in`` (= the readout's output irreps);
    * ``gate_scalars`` / ``gate_gated``: slots of the Gate's scalars / gated irreps;
    * ``gate_out``: slots of the Gate's output irreps (= ``linear_2``'s input);
    * ``lin1_out``: pieces (slot, first channel, channels) of ``linear_1.irreps_out``, whose
      first slot merges the scalars and every gate;
    * ``hidden``: slots of ``linear_1.irreps_in``, the last layer's output irreps."""
    gate = readout.equivariant_nonlin
    final_in = _live_inputs(final, range(len(final.irreps_out)))
    gate_out = _live_inputs(readout.linear_2, final_in)
    ns = len(gate.irreps_scalars)
    gate_scalars = tuple(j for j in gate_out if j < ns)
    gate_gated = tuple(j - ns for j in gate_out if j >= ns)
    # the Gate's input row as atoms -- the scalar slots, one run of gates per gated slot (a
    # gate per channel, in slot order), the gated slots -- and each atom's piece of linear_1's
    # output irreps, which are those of the Gate's input with equal neighbours merged
    gate_ir = [ir for mul, ir in gate.irreps_gates for _ in range(mul)]
    atoms, g0 = [("s", j, mul, ir) for j, (mul, ir) in enumerate(gate.irreps_scalars)], 0
    for b, (mul, _) in enumerate(gate.irreps_gated):
        if len(set(gate_ir[g0: g0 + mul])) != 1:
            raise ValueError(f"the gates {gate.irreps_gates} of gated slot {b} are of several irreps")
        atoms.append(("g", b, mul, gate_ir[g0]))
        g0 += mul
    atoms += [("x", b, mul, ir) for b, (mul, ir) in enumerate(gate.irreps_gated)]
    where, s, c0, prev, last = {}, -1, 0, None, 0
    for kind, idx, mul, ir in atoms:
        if ir == prev:
            c0 += last
        else:
            s, c0, prev = s + 1, 0, ir
        where[(kind, idx)] = (s, c0, mul)
        last = mul
    lin1 = readout.linear_1
    if s + 1 != len(lin1.irreps_out) or any(
            sum(cnt for t, _, cnt in where.values() if t == k) != lin1.irreps_out[k].mul
            for k in range(len(lin1.irreps_out))):
        raise ValueError(f"{lin1.irreps_out} is not the simplified Gate input {gate.irreps_in}")
    lin1_out = _merge_pieces([where[("s", j)] for j in gate_scalars]
                             + [where[(k, b)] for k in "gx" for b in gate_gated])
    hidden = _live_inputs(lin1, {p[0] for p in lin1_out})
    return dict(final_in=final_in, gate_out=gate_out, gate_scalars=gate_scalars,
                gate_gated=gate_gated, lin1_out=lin1_out, hidden=hidden)


class GNN_Head(torch.nn.Module):  # noqa: N801
    def __init__(self, params: Namespace) -> None:
        super().__init__()
        self.params = params
        hidden = Irreps(params.hidden_irreps)
        self.number_of_edge_basis = params.num_edge_bases
        node_ft_irreps = Irreps([(hidden.count("0e"), "0e")])
        edge_feats_irreps = Irreps(f"{self.number_of_edge_basis * 2}x0e")
        edge_attr_irreps = Irreps.spherical_harmonics(params.lmax)
        num_features = hidden.count("0e")
        interaction_irreps = (edge_attr_irreps * num_features).sort()[0].simplify()
        readout_irreps = Irreps(params.readout_irreps)
        self.num_interactions = params.message_passes
        storage = storage_dtype(params)

        def layer(inp):
            return MACELayer(inp, edge_attr_irreps, edge_feats_irreps, interaction_irreps, hidden,
                             params.agg_norm_const, params.interaction_reduction, True,
                             params.correlation, MLP_dim=params.inter_MLP_dim,
                             MLP_layers=params.inter_MLP_layers, storage_dtype=storage)

        self.layers = torch.nn.ModuleList([layer(node_ft_irreps)])
        for _ in range(self.num_interactions - 1):
            self.layers.append(layer(hidden))
        self.nonlin_readout = GeneralNonLinearReadoutBlock(hidden, hidden, readout_irreps,
                                                           gate=torch.nn.functional.silu)
        self.global_reduction = params.global_reduction
        self.linear = Linear(readout_irreps, Irreps("2x0e+2x2e+1x4e"), biases=True)
        self.sph_to_cart = Spherical_to_Cartesian()
        self.cart_to_Mandel = Cart_4_to_Mandel()
        self.positive_layer = PositiveLayer(params)
        # forward returns nothing but the stiffness: the irreps of the last layer's output that
        # cannot reach self.linear are not computed (ops.LIVE_OUT, EELG_LIVE_OUT=0: all are)
        live = readout_liveness(self.nonlin_readout, self.linear)
        self.live_irreps = Irreps([hidden[i] for i in live["hidden"]])
        self.live_pruned = bool(ops.LIVE_OUT) and self._prune(live)

    def _prune(self, live) -> bool:
        """Restrict the last layer's contraction and product linear and the readout to the
        live irreps.  False, with nothing changed: everything is live, or the live-output
        contraction set does not exist (correlation 4, a list that was not generated)."""
        ro, prod = self.nonlin_readout, self.layers[-1].product
        lin1, gate, lin2 = ro.linear_1, ro.equivariant_nonlin, ro.linear_2
        if live["hidden"] == tuple(range(len(lin1.irreps_in))):
            return False
        sc_slots = _live_inputs(prod.linear, live["hidden"])
        ls = tuple(prod.linear.irreps_in[i].ir.l for i in sc_slots)
        if [prod.linear.irreps_in[i] for i in sc_slots] != [
                prod.symmetric_contractions.irreps_out[i] for i in sc_slots]:
            return False
        if (not prod.symmetric_contractions.restrict_outputs(ls)
                or prod.symmetric_contractions._live is None):
            return False

        def whole(irreps, slots):
            return tuple((s, 0, irreps[s].mul) for s in slots)

        prod.linear.set_live(whole(prod.linear.irreps_in, sc_slots),
                             whole(prod.linear.irreps_out, live["hidden"]))
        lin1.set_live(whole(lin1.irreps_in, live["hidden"]), live["lin1_out"])
        gate.set_live(live["gate_scalars"], live["gate_gated"])
        lin2.set_live(whole(lin2.irreps_in, live["gate_out"]), whole(lin2.irreps_out, live["final_in"]))
        self.linear.set_live(whole(self.linear.irreps_in, live["final_in"]), None)
        # the Gate's compact input row is linear_1's compact output row, piece by piece
        if lin1.live is None or gate.live is None or lin1.live._out_dim != gate.live.in_dim:
            raise RuntimeError("live readout pieces do not line up")
        return True

    def _radial_weights_ahead(self, edge_feats, csr=None, edge_sh=None):
        """Every layer's radial MLP depends only on the edge features, so all of them run up
        front on a side stream and overlap the VALU-bound interaction / contraction kernels
        of the main stream (their backward runs on that stream too: autograd replays a
        backward op on its forward's stream and inserts the cross-stream waits).  Layer i
        waits for its own weights only."""
        # geometry gradients (the edge features require grad): every layer computes its weights
        # in line, so this path adds no cross-stream lifetimes to the tuned training step
        geom = torch.is_grad_enabled() and edge_feats.requires_grad
        if geom or not (ops.OVERLAP and edge_feats.is_cuda):
            return [None] * self.num_interactions, [None] * self.num_interactions
        main = torch.cuda.current_stream(edge_feats.device)
        side = ops.side_stream(edge_feats.device)
        side.wait_stream(main)
        # edge_feats is made on the main stream and read (and saved for the MLP backward) on
        # the side stream: without this the allocator could hand its block to a main-stream
        # allocation while a side-stream kernel still reads it
        edge_feats.record_stream(side)
        ws, evs = [], []
        with torch.cuda.stream(side):
            for layer in self.layers:
                # one row per strut where the block's predicate allows it (ops.strut_rows)
                smap = layer.interaction.strut_map(csr, edge_feats, edge_sh) if csr is not None else None
                w = layer.interaction.radial_weights(edge_feats, smap)
                ev = torch.cuda.Event()
                ev.record(side)
                ws.append(w)
                evs.append(ev)
        for w in ws:
            # allocator: w is also used on the main stream
            self._main_stream_weight(w).record_stream(main)
        return ws, evs

    @staticmethod
    def _main_stream_weight(w):
        """the tensor of a layer's radial weights that the main stream reads"""
        return w.w if isinstance(w, ops.StrutWeights) else w

    def _coefficients_ahead(self, device) -> None:
        """Every layer's contraction coefficients (``coef = U_sym W``) depend on the weights
        only: issue them all up front on the coefficient side stream (after the main stream's
        last weight update), so no layer waits on a fresh main -> side -> main round trip."""
        if not (ops.OVERLAP and COEF_AHEAD and device.type == "cuda"):
            return
        main = torch.cuda.current_stream(device)
        side = ops.side_stream(device, 1)
        side.wait_stream(main)
        for i, layer in enumerate(self.layers):
            layer.product.symmetric_contractions.coefficients_ahead(
                side, live=self.live_pruned and i == self.num_interactions - 1)

    def forward(self, edge_index, node_ft, edge_sh, edge_feats, batch_idx, num_graphs: int):
        csr, edge_sh, edge_feats = as_csr(edge_index, node_ft.shape[0], edge_sh, edge_feats)
        ws, evs = self._radial_weights_ahead(edge_feats, csr, edge_sh)
        self._coefficients_ahead(node_ft.device)

        def run(i, h, residual=None):
            if evs[i] is not None:
                torch.cuda.current_stream(h.device).wait_event(evs[i])
            # the last layer: only the irreps the readout can pass on to self.linear
            live = self.live_pruned and i == self.num_interactions - 1
            return self.layers[i](h, csr, edge_sh, edge_feats, tp_weights=ws[i], residual=residual,
                                  live=live)

        node_ft = run(0, node_ft)
        if RADIAL_AHEAD_OF_LAYER1 and evs[-1] is not None:
            # the later layers' interaction kernels run without the MLP GEMMs beside them
            torch.cuda.current_stream(node_ft.device).wait_event(evs[-1])
        for i in range(1, self.num_interactions):
            # node_ft + layer_i(node_ft) (gnn/model.py:95), the add fused into the layer's
            # last linear
            node_ft = run(i, node_ft, residual=node_ft)
        out = self.nonlin_readout(node_ft, live=self.live_pruned)
        graph_ft = ops.graph_pool(out, batch_idx, num_graphs, self.global_reduction)
        stiff = self.sph_to_cart(self.linear(graph_ft, live=self.live_pruned))
        return self.positive_layer(self.cart_to_Mandel(stiff))


class _Embed1(torch.autograd.Function):
    """y = b + a w^T for one input feature a [N, 1]: forward torch.addcmul, backward the two
    column sums on ``ops.sum_rows`` (deterministic; torch's reductions were 2 x 33 us per step
    at [32768, 32], r06i).  No gradient w.r.t. the node attributes (data)."""

    @staticmethod
    def forward(ctx, attrs, weight, bias):
        ctx.save_for_backward(attrs)
        ctx.has_bias = bias is not None
        w = weight[:, 0]
        return torch.addcmul(bias, attrs, w) if bias is not None else attrs * w

    @staticmethod
    def backward(ctx, gy):
        from . import ops
        (attrs,) = ctx.saved_tensors
        gy = ops._f32(gy).contiguous()
        gw = ops.sum_rows(gy * attrs).unsqueeze(1) if ctx.needs_input_grad[1] else None
        gb = ops.sum_rows(gy) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return None, gw, gb


def _embed(lin: torch.nn.Linear, attrs: torch.Tensor) -> torch.Tensor:
    """``Linear(1 -> 32)`` of the node attributes (``gnn/model.py:122,142``).  With one input
    feature it is an outer product plus bias: one broadcast multiply-add instead of a K = 1
    library GEMM (0.19 ms per step on MI355X for [32768 x 1] x [1 x 32], r02q), and its weight
    and bias gradients are column sums.  Same values (a single product per output plus the bias)."""
    if lin.in_features != 1:
        return lin(attrs)
    if attrs.is_cuda and not attrs.requires_grad:
        return _Embed1.apply(attrs, lin.weight, lin.bias)
    return torch.addcmul(lin.bias, attrs, lin.weight[:, 0]) if lin.bias is not None \
        else attrs * lin.weight[:, 0]


def _geometry_key(batch, n_edges: int):
    """Identity of the tensors a strut map depends on (storage, version counter, shape, device), or
    None where the batch can have no map: a tensor missing, ``edge_attr`` not one value per edge
    (the ``edge_ft`` forms 'L,r', 'e_vec', 'euler'), or geometry that requires grad (geometry
    gradients compute per-edge weights).  Like the CSR's key this identifies a tensor by address
    and version: a tensor replaced twice between two calls could be freed and its address reused
    by another of the same shape, which would pass for the first; replace the batch instead."""
    ts = [getattr(batch, k, None) for k in ("positions", "shifts", "edge_attr")]
    if not all(torch.is_tensor(t) for t in ts) or any(t.requires_grad for t in ts):
        return None
    pos, shifts, radius = ts
    if radius.numel() != n_edges or tuple(shifts.shape) != (n_edges, 3) or pos.dim() != 2 or pos.shape[1] != 3:
        return None
    return tuple((t.data_ptr(), t._version, tuple(t.shape), str(t.device)) for t in ts)


class EnergyEquivGNN(torch.nn.Module):
    def __init__(self, params: Namespace, *args: Any, **kwargs: Any) -> None:
        super().__init__(*args, **kwargs)
        self.params = params
        hidden = Irreps(params.hidden_irreps)
        self.node_ft_embedding = torch.nn.Linear(1, hidden.count("0e"))
        self.number_of_edge_basis = params.num_edge_bases
        self.max_edge_radius = params.max_edge_radius
        self.lmax = params.lmax
        self.stiffness_head = GNN_Head(params)

    @staticmethod
    def edge_graph(batch, strut: bool = True, build: bool = True) -> ops.EdgeCSR:
        """Receiver-sorted CSR of ``batch.edge_index`` on its device (cached on the batch), with
        the batch's strut map (``ops.StrutMap``: which edges are the two directions of one strut)
        unless ``strut`` is False or EELG_STRUT_WEIGHTS=0.

        Called on a batch ahead of its steps -- collate-time work, as ``bench.py`` does -- this
        builds what the batch does not bring: the CSR, and the map (one sort and a few host
        syncs).  The model's own call inside a step passes ``build=False``: it takes the map an
        earlier call left for these very tensors and otherwise runs on per-edge weights, so a
        fresh batch never pays a sort or a host sync for the map inside a training step."""
        n = batch.node_attrs.shape[0]
        ei = batch.edge_index
        dev = ei.device
        # the cache is valid only for this very edge_index: same storage, no in-place edits
        # since (autograd version counter), same node and edge counts, same device
        key = (ei.data_ptr(), ei._version, tuple(ei.shape), n, str(dev))
        csr = getattr(batch, "_eelg_csr", None)
        if csr is None or getattr(batch, "_eelg_csr_key", None) != key:
            pre = getattr(batch, "csr", None)
            if isinstance(pre, dict) and torch.is_tensor(pre.get("perm")):
                csr = ops.EdgeCSR.from_dict({k: (v.to(dev) if torch.is_tensor(v) else v)
                                             for k, v in pre.items()}, n)
            else:
                csr = ops.EdgeCSR.build(batch.edge_index, n)
            try:
                batch._eelg_csr = csr
                batch._eelg_csr_key = key
            except AttributeError:
                pass
        # the map is kept beside the CSR under a key of its own (the geometry it pairs the edges
        # by), so callers with and without ``strut`` share one CSR
        geo_key = _geometry_key(batch, csr.num_edges) if strut and ops.STRUT_WEIGHTS else None
        if geo_key is None:
            return csr        # (a map left by an earlier call stays; ops.strut_rows decides on its use)
        if csr.strut is not None and getattr(csr, "_strut_key", None) != geo_key:
            csr.strut = None                      # of other tensors
        if csr.strut is None and build:
            csr.strut = ops.build_strut_map(batch.positions, csr.sender, csr.receiver,
                                            batch.shifts[csr.perm], batch.edge_attr[csr.perm].reshape(-1))
            csr._strut_key = geo_key
        return csr

    def forward(self, batch) -> Dict[str, torch.Tensor]:
        dev = batch.positions.device
        if dev.type != "cuda":
            raise RuntimeError("the EnergyEquivGNN hot path runs only on a HIP device "
                               "(got a CPU batch); move the model and batch to 'cuda'")
        with torch.cuda.device(dev):        # kernels launch on the batch's device
            return self._forward(batch)

    def _forward(self, batch) -> Dict[str, torch.Tensor]:
        csr = self.edge_graph(batch, build=False)     # the step builds no strut map
        node_ft = _embed(self.node_ft_embedding, batch.node_attrs)
        geom = torch.is_grad_enabled() and (batch.positions.requires_grad or batch.shifts.requires_grad
                                            or batch.edge_attr.requires_grad)
        if geom and storage_dtype(self.params) != torch.float32:
            raise NotImplementedError(
                "geometry gradients (positions / shifts / edge_attr requiring grad) are built for "
                "fp32 storage only, not storage_dtype='bfloat16'")
        # (with grad: the permutation's backward is a plain scatter, ops.permute_rows)
        shifts = ops.permute_rows(batch.shifts, csr.perm)
        radius = ops.permute_rows(batch.edge_attr, csr.perm).reshape(-1)
        edge_sh, edge_feats = ops.edge_embed(batch.positions, csr, shifts, radius, self.lmax,
                                             self.number_of_edge_basis, 0.6, self.max_edge_radius)
        c = self.stiffness_head(csr, node_ft, edge_sh, edge_feats, batch.batch, batch.num_graphs)
        return {"stiffness": c}
