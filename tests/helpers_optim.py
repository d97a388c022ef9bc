"""Shared pieces of the optimizer tests: the hostile gradient set, the fp64 restatement of
clip + AdamW over one flat vector, torch's own AdamW as the fp32 baseline and the error measures.

Error measures (against fp64 values computed from the same fp32 gradients):
  p       max |p - p64| / lr        (the update is O(lr) per step whatever the gradient's scale)
  m, v    max |x - x64| / max(|x64|, 2^-126)   elementwise relative; values below the smallest
          normal fp32 number cannot be held to a relative bound and are measured against it
Bound: 4x the error of torch.optim.AdamW in fp32 on the same inputs (the margin for a second fp32
order of operations, as for csrc/eelg_jacobi.h), floored at 2^-23 of the compared value (half an
ulp: p's floor is 2^-23 max|p64| / lr, the relative ones' 2^-23)."""
from __future__ import annotations

import math

import numpy as np
import torch

HOSTILE = (0.0, 1e-30, -1e-30, 1e-8, -1e-8, 1.0, -1.0, 1e4, -1e4)
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
TINY = 2.0 ** -126
ULP = 2.0 ** -23


def hostile_grads(steps: int, n: int, seed: int = 0, scale: float = 1.0) -> torch.Tensor:
    """[steps, n] fp32: the hostile values, each step in another order, times ``scale`` in fp32."""
    rng = np.random.default_rng(seed)
    base = np.resize(np.array(HOSTILE, dtype=np.float32), n)
    rows = [base[rng.permutation(n)] if s else base for s in range(steps)]
    return torch.from_numpy(np.stack(rows)) * torch.tensor(scale, dtype=torch.float32)


def clip_settings(first: torch.Tensor):
    """clip off, inactive, active, and a bound just under / just over the norm of ``first`` (a step's
    gradient)"""
    norm = float(first.double().pow(2).sum().sqrt())
    return {"off": 0.0, "inactive": 1e9, "active": 10.0, "just_under": norm * (1 - 1e-6) - 1e-6,
            "just_over": norm * (1 + 1e-6) + 1e-6}


def start_values(n: int, seed: int = 1) -> torch.Tensor:
    return torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def reference64(p0: torch.Tensor, grads: torch.Tensor, amsgrad: bool, max_norm: float, lr, betas, eps,
                weight_decay):
    """The flat rule in fp64: per step (p, m, v, vmax, norm, coef); a norm that is not finite
    skips the step."""
    p = p0.double().clone()
    m, v, vmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    out, t = [], 0
    for g in grads.double():
        norm = float(g.pow(2).sum().sqrt())
        if math.isfinite(norm):
            t += 1
            coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
            g = g * coef
            p = p * (1 - lr * weight_decay)
            m = m + (1 - betas[0]) * (g - m)
            v = betas[1] * v + (1 - betas[1]) * g * g
            vmax = torch.maximum(vmax, v) if amsgrad else vmax
            denom = (vmax if amsgrad else v).sqrt() / math.sqrt(1 - betas[1] ** t) + eps
            p = p - lr / (1 - betas[0] ** t) * (m / denom)
        else:
            coef = 0.0
        out.append(dict(p=p.clone(), m=m.clone(), v=v.clone(), vmax=vmax.clone(), norm=norm, coef=coef, t=t))
    return out


def torch_adamw(p0s, grads_per_step, dtype, amsgrad: bool, max_norm: float, device="cpu", **kw):
    """torch.optim.AdamW (+ clip_grad_norm_) over the parameter list ``p0s``; ``grads_per_step``
    is a list (steps) of lists (parameters) of gradients.  Returns per step the flat (p, m, v,
    vmax) and the optimizer."""
    hp = dict(HP, **{k: v for k, v in kw.items() if k in HP})
    extra = {k: v for k, v in kw.items() if k not in HP}
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype).clone()) for p in p0s]
    opt = torch.optim.AdamW(ps, amsgrad=amsgrad, **hp, **extra)
    out = []
    for gs in grads_per_step:
        for p, g in zip(ps, gs):
            p.grad = g.to(device=device, dtype=dtype).clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        opt.zero_grad(set_to_none=True)
        out.append(flat_state(opt, ps, amsgrad))
    return out, opt


def flat_state(opt, ps, amsgrad: bool):
    cat = lambda ts: torch.cat([t.detach().reshape(-1).cpu() for t in ts])   # noqa: E731
    d = dict(p=cat(ps), m=cat([opt.state[p]["exp_avg"] for p in ps]),
             v=cat([opt.state[p]["exp_avg_sq"] for p in ps]))
    d["vmax"] = cat([opt.state[p]["max_exp_avg_sq"] for p in ps]) if amsgrad else torch.zeros_like(d["v"])
    return d


def errors(got, ref, lr: float, amsgrad: bool):
    """{'p', 'm', 'v'(, 'vmax')} of one step's values against the fp64 ones"""
    e = {"p": float((got["p"].double() - ref["p"].double()).abs().max()) / lr}
    for k in ("m", "v") + (("vmax",) if amsgrad else ()):
        r = ref[k].double()
        e[k] = float(((got[k].double() - r).abs() / r.abs().clamp_min(TINY)).max())
    return e


def worst(err_list):
    keys = set().union(*err_list)
    return {k: max(e.get(k, 0.0) for e in err_list) for k in sorted(keys)}


def floors(refs, lr: float):
    pf = ULP * max(float(r["p"].abs().max()) for r in refs) / lr
    return {"p": pf, "m": ULP, "v": ULP, "vmax": ULP}


def assert_bounded(mine, base, floor, what=""):
    """every measure of ``mine`` within max(4 x ``base``, ``floor``)"""
    print(f"{what}: this {mine}  torch fp32 {base}")
    for k, v in mine.items():
        assert v <= max(4 * base[k], floor[k]), (what, k, v, base[k], floor[k])
