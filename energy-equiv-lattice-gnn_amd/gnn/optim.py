"""``FlatAdamW``: gradient clipping, ``torch.optim.AdamW`` (with or without amsgrad) and
``zero_grad`` over one flat fp32 buffer, in two HIP launches per optimizer step
(``eelg_grad_sqnorm`` + ``eelg_adamw_flat``, ``csrc/eelg_optim.hip``) after one ``torch.cat`` that
packs the gradients.

What it replaces in the reference's step: ``Trainer(gradient_clip_val=10.0)``'s
``clip_grad_norm_``, ``torch.optim.AdamW.step`` (``scripts/train_utils.py:38-43``) and
``zero_grad``, each a multi-tensor launch chain over the model's 102 parameter tensors.

* On construction the parameters move into one flat buffer (each ``p.data`` becomes a view of its
  slice; slices start on 512-byte boundaries, the alignment torch's allocator gives a tensor of
  its own, and the padding between them stays exactly zero in every buffer).  Do not move the
  module (``.to(...)``) afterwards: that would detach the parameters from the buffer.
* The step count, the count of skipped steps, the last gradient norm and the last clip
  coefficient live on the device (``read_state()`` reads them; nothing else synchronises).
* A gradient norm that is not finite skips the update: parameters, moments and step count stay
  bitwise as they were, the gradient is dropped and ``skipped`` goes up by one.  (torch would
  write NaN into every parameter.)
* With a process group the one all-reduce and the division by the world size act on the packed
  buffer itself.
* ``state_dict`` / ``load_state_dict`` speak ``torch.optim.AdamW``'s format in both directions.
* CPU tensors, or ``EELG_OPTIM_FUSED=0``, take a fallback composed from torch ops with the same
  semantics (the second implementation, the timing baseline and the CPU path).
"""
from __future__ import annotations

import os
from typing import Dict, Iterable, List, Optional

import torch
import torch.distributed as dist

from . import _lib

# the two HIP launches on a HIP device (1), or the composed torch form everywhere (0)
FUSED = os.environ.get("EELG_OPTIM_FUSED", "1") != "0"
ALIGN = 128          # floats: every slice starts on a 512-byte boundary


def _bump_versions(params: List[torch.Tensor]) -> None:
    """The kernels write through raw pointers; caches keyed on a parameter's version (the packed
    split-bf16 weights of ``o3.Linear``) must see a new one.  A host call, no launch."""
    torch.autograd.graph.increment_version(params)


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, max_norm: Optional[float] = None,
                 group=None, fused: Optional[bool] = None):
        """``max_norm``: ``clip_grad_norm_``'s bound on the total gradient norm (None or <= 0: no
        clipping).  ``group``: a process group to average the gradients over (None: the default
        group if ``torch.distributed`` is initialised; False: never all-reduce, for a single
        replica inside a distributed job).  ``fused``: None follows
        ``EELG_OPTIM_FUSED`` on a HIP device; False forces the composed torch form."""
        # every key torch.optim.AdamW's groups carry, so that state dicts pass in both directions
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad),
                        maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=True)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdamW: one parameter group (per-group hyper-parameters are not supported)")
        self.max_norm = float(max_norm) if max_norm else 0.0
        self.group = group
        ps = [p for p in self.param_groups[0]["params"] if p.requires_grad]
        self.param_groups[0]["params"] = ps
        if not ps:
            raise ValueError("FlatAdamW: no parameter requires a gradient")
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or p.device != dev or p.is_sparse:
                raise ValueError("FlatAdamW: dense fp32 parameters on one device")
        self._params = ps
        self.fused = (FUSED if fused is None else bool(fused)) and dev.type == "cuda"
        self._offsets, off = [], 0
        for p in ps:
            self._offsets.append(off)
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.numel = off
        self.flat_p = torch.zeros(off, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros_like(self.flat_p)
        self.flat_v = torch.zeros_like(self.flat_p)
        self.flat_vmax = torch.zeros_like(self.flat_p)
        self.flat_g = torch.zeros_like(self.flat_p)
        with torch.no_grad():
            for p, o in zip(ps, self._offsets):
                view = self.flat_p[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                p.data = view
        # the zero pieces torch.cat puts between the slices (and in place of a missing gradient)
        self._zeros = torch.zeros(max(max(p.numel() for p in ps), ALIGN), dtype=torch.float32, device=dev)
        self._pads = [self._zeros[:(-p.numel()) % ALIGN] for p in ps]
        # device-side state: two rows {steps taken, skipped, bits of norm, bits of coef}; call c
        # reads row c & 1 and writes row (c + 1) & 1
        self._rows = torch.zeros(2, _lib.OPTIM_STATE_COLS, dtype=torch.int32, device=dev)
        self._calls = 0
        if self.fused:
            self._nparts = int(_lib.load().eelg_sqnorm_parts(self.numel))
            self._partials = torch.zeros(self._nparts, dtype=torch.float32, device=dev)
        self._refresh_state_views()
        _bump_versions(ps)

    # -- construction from torch's optimizer ------------------------------------------------
    @classmethod
    def from_torch(cls, opt: torch.optim.Optimizer, max_norm: Optional[float] = None, group=None,
                   fused: Optional[bool] = None) -> "FlatAdamW":
        """Adopt the ``torch.optim.AdamW`` that ``configure_optimizers()`` returns: the same
        parameters and hyper-parameters, and its state if it has stepped already."""
        if len(opt.param_groups) != 1:
            raise ValueError("FlatAdamW.from_torch: one parameter group")
        g = opt.param_groups[0]
        if g.get("maximize") or g.get("differentiable") or g.get("capturable"):
            raise ValueError("FlatAdamW.from_torch: maximize / differentiable / capturable are not supported")
        new = cls(g["params"], lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"],
                  amsgrad=g["amsgrad"], max_norm=max_norm, group=group, fused=fused)
        if len(opt.state):
            new.load_state_dict(opt.state_dict())
        return new

    # -- device-side state --------------------------------------------------------------------
    def _row(self) -> torch.Tensor:
        return self._rows[self._calls & 1]

    def read_state(self) -> Dict[str, float]:
        """``{'step', 'skipped', 'grad_norm', 'clip_coef'}`` read from the device (synchronises)."""
        row = self._row().cpu()
        f = row.view(torch.float32)
        return {"step": int(row[0]), "skipped": int(row[1]), "grad_norm": float(f[2]), "clip_coef": float(f[3])}

    def _refresh_state_views(self) -> None:
        """``self.state[p]`` in torch's layout, as views of the flat buffers.  The step count lives
        on the device, so ``self.state[p]['step']`` is a placeholder between calls and is right only
        in what ``state_dict()`` returns (which reads the device: one synchronisation); schedulers
        and loggers take the count from ``read_state()``."""
        amsgrad = self.param_groups[0]["amsgrad"]
        for p, o in zip(self._params, self._offsets):
            st = {"step": torch.tensor(0.0), "exp_avg": self.flat_m[o:o + p.numel()].view(p.shape),
                  "exp_avg_sq": self.flat_v[o:o + p.numel()].view(p.shape)}
            if amsgrad:
                st["max_exp_avg_sq"] = self.flat_vmax[o:o + p.numel()].view(p.shape)
            self.state[p] = st

    def state_dict(self):
        """``torch.optim.AdamW``'s format (per-parameter ``step``, ``exp_avg``, ``exp_avg_sq``,
        ``max_exp_avg_sq`` with amsgrad; ``param_groups``); tensors are copies.  Empty state before
        the first step, as torch's."""
        now = self.read_state()
        step, skipped = now["step"], now["skipped"]
        self._refresh_state_views()
        for p in self._params:
            self.state[p]["step"] = torch.tensor(float(step))
        sd = super().state_dict()
        if step == 0:
            sd["state"] = {}
        else:
            sd["state"] = {k: {n: t.detach().clone() for n, t in st.items()} for k, st in sd["state"].items()}
        sd["flat_adamw"] = {"skipped": skipped}      # an extra key: torch.optim.AdamW ignores it
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        g = self.param_groups[0]
        if g.get("maximize") or g.get("differentiable"):
            raise ValueError("FlatAdamW.load_state_dict: maximize / differentiable are not supported")
        steps = set()
        with torch.no_grad():
            for buf in (self.flat_m, self.flat_v, self.flat_vmax):
                buf.zero_()
            for p, o in zip(self._params, self._offsets):
                st = self.state.get(p, {})
                if not st:
                    steps.add(0)
                    continue
                steps.add(int(float(st["step"])))
                n = p.numel()
                self.flat_m[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self.flat_v[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                if g["amsgrad"] and "max_exp_avg_sq" in st:
                    self.flat_vmax[o:o + n].copy_(st["max_exp_avg_sq"].reshape(-1))
        if len(steps) != 1:
            raise ValueError(f"FlatAdamW.load_state_dict: one step count for all parameters, got {sorted(steps)}")
        row = torch.zeros(_lib.OPTIM_STATE_COLS, dtype=torch.int32)
        row[0] = steps.pop()
        row[1] = int((state_dict.get("flat_adamw") or {}).get("skipped", 0))   # absent in torch's own dicts
        self._rows[self._calls & 1].copy_(row)
        self._refresh_state_views()

    # -- the step -------------------------------------------------------------------------------
    def _pack(self) -> None:
        """One ``torch.cat`` of the gradients (zeros for a parameter without one and between the
        slices) into the flat gradient buffer."""
        parts = []
        for p, pad in zip(self._params, self._pads):
            if p.grad is not None:
                parts.append(p.grad.reshape(-1))
            else:
                parts.append(self._zeros[:p.numel()])
            if pad.numel():
                parts.append(pad)
        torch.cat(parts, out=self.flat_g)

    def _all_reduce(self) -> None:
        if self.group is False or not (dist.is_available() and dist.is_initialized()):
            return
        world = dist.get_world_size(self.group)
        if world > 1:
            dist.all_reduce(self.flat_g, group=self.group)
            self.flat_g.div_(world)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._pack()
        self._all_reduce()
        g = self.param_groups[0]
        src, dst = self._rows[self._calls & 1], self._rows[(self._calls + 1) & 1]
        if self.fused:
            lib = _lib.load()
            with torch.cuda.device(self.flat_p.device):
                _lib.launch("grad_sqnorm", lib.eelg_grad_sqnorm, self.flat_g, self.numel, self._partials,
                            on=self.flat_p)
                _lib.launch("adamw_flat", lib.eelg_adamw_flat, self.flat_p, self.flat_m, self.flat_v,
                            self.flat_vmax, self.flat_g, self.numel, self._partials, float(g["lr"]),
                            float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                            float(g["weight_decay"]), self.max_norm, int(g["amsgrad"]), src, dst,
                            on=self.flat_p)
        else:
            self._step_composed(g, src, dst)
        self._calls += 1
        for p in self._params:
            p.grad = None
        _bump_versions(self._params)
        return loss

    def _step_composed(self, g, src: torch.Tensor, dst: torch.Tensor) -> None:
        """The same step from torch ops, without a host synchronisation: every new value is
        selected against the old one by the norm's finiteness."""
        lr, (beta1, beta2), eps, wd = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        grad = self.flat_g
        norm = torch.linalg.vector_norm(grad)
        ok = torch.isfinite(norm)
        if self.max_norm > 0:
            coef = torch.clamp(self.max_norm / (norm + 1e-6), max=1.0)
        else:
            coef = torch.ones_like(norm)
        coef = torch.where(ok, coef, torch.zeros_like(coef))
        t = (src[0] + 1).to(torch.float64)
        step_size = (lr / (1.0 - beta1 ** t)).to(torch.float32)
        bc2_sqrt = (1.0 - beta2 ** t).sqrt().to(torch.float32)
        grad = grad * coef
        p = self.flat_p * (1.0 - lr * wd)
        m = self.flat_m.lerp(grad, 1.0 - beta1)
        v = (self.flat_v * beta2).addcmul_(grad, grad, value=1.0 - beta2)
        second = torch.maximum(self.flat_vmax, v) if g["amsgrad"] else v
        denom = (second.sqrt() / bc2_sqrt).add_(eps)
        p = p - step_size * (m / denom)
        self.flat_p.copy_(torch.where(ok, p, self.flat_p))
        self.flat_m.copy_(torch.where(ok, m, self.flat_m))
        self.flat_v.copy_(torch.where(ok, v, self.flat_v))
        if g["amsgrad"]:
            self.flat_vmax.copy_(torch.where(ok, second, self.flat_vmax))
        self.flat_g.zero_()
        oki = ok.to(torch.int32)
        dst[0] = src[0] + oki
        dst[1] = src[1] + (1 - oki)
        dst[2:4] = torch.stack([norm.to(torch.float32), coef.to(torch.float32)]).view(torch.int32)
