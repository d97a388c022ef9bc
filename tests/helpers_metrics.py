"""fp64 restatement of the stiffness metrics (``scripts/train_utils.py:149-171``) and the hostile
matrix set of the metrics tests.  The restatement forms the cartesian rank-4 tensor with
``helpers_mandel.mandel_to_cart4`` and contracts it with four copies of the directions, as the
reference does; none of the code under test is used."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from helpers_mandel import mandel_to_cart4

GROUPS = {"mseloss": slice(0, 1), "loss": slice(1, 2), "dir_loss": slice(2, 3),
          "mean_stiffness": slice(3, 4), "target_eig": slice(4, 10), "predicted_eig": slice(10, 16)}


def isotropic(lam: float, mu: float) -> np.ndarray:
    """Mandel matrix of C_ijkl = lam d_ij d_kl + mu (d_ik d_jl + d_il d_jk)."""
    c = np.zeros((6, 6))
    c[:3, :3] = lam
    c[np.arange(3), np.arange(3)] += 2 * mu
    c[np.arange(3, 6), np.arange(3, 6)] = 2 * mu
    return c


def hostile_set() -> torch.Tensor:
    """[10, 6, 6] fp32, all symmetric: 4 random SPD, a diagonal matrix, the isotropic matrix (a
    5-fold degenerate eigenvalue), a rank-1 matrix, a symmetric indefinite matrix, an SPD matrix
    scaled by 1e-4 and one scaled by 1e5."""
    rng = np.random.default_rng(2024)

    def spd():
        a = rng.normal(size=(6, 6))
        return a @ a.T / 6 + 0.5 * np.eye(6)
    mats = [spd() for _ in range(4)]
    mats.append(np.diag([3.0, 0.5, 7.0, 1.0, 2.0, 0.25]))
    mats.append(isotropic(1.5, 0.7))
    u = rng.normal(size=6)
    mats.append(np.outer(u, u))
    s = rng.normal(size=(6, 6))
    mats.append((s + s.T) / 2)
    mats.append(spd() * 1e-4)
    mats.append(spd() * 1e5)
    return torch.from_numpy(np.stack(mats)).float()


def hostile_pairs():
    """(pred, target), each [90, 6, 6]: every matrix of the set as target against every other
    one as prediction."""
    h = hostile_set()
    n = h.shape[0]
    target = torch.cat([h for _ in range(1, n)])
    pred = torch.cat([torch.roll(h, k, 0) for k in range(1, n)])
    return pred.contiguous(), target.contiguous()


def directions(p: int, seed: int = 3) -> torch.Tensor:
    d = torch.randn(p, 3, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (d / d.norm(dim=-1, keepdim=True)).float()


def reference64(pred: torch.Tensor, target: torch.Tensor, dirs: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """[B, 16] fp64 rows (the layout of ``gnn.metrics.METRIC_COLUMNS``) from fp32 inputs taken to
    fp64; eigenvalues of the symmetric matrix of the lower triangle."""
    p, t, d = scale * pred.double().cpu(), scale * target.double().cpu(), dirs.double().cpu()
    mse = (p - t).pow(2).mean(dim=(1, 2))
    l1 = (p - t).abs().mean(dim=(1, 2))
    c = torch.einsum("...ijkl,pi,pj,pk,pl->...p", mandel_to_cart4(t), d, d, d, d)
    cp = torch.einsum("...ijkl,pi,pj,pk,pl->...p", mandel_to_cart4(p), d, d, d, d)
    cols = [mse[:, None], l1[:, None], (c - cp).abs().mean(dim=1)[:, None], c.mean(dim=1)[:, None],
            torch.linalg.eigvalsh(t, UPLO="L"), torch.linalg.eigvalsh(p, UPLO="L")]
    return torch.cat(cols, dim=1)


def normalised_errors(rows: torch.Tensor, ref: torch.Tensor) -> Dict[str, float]:
    """Largest error over the graphs of every column group: scalar columns relative to the
    graph's fp64 value, eigenvalues relative to that matrix's largest |eigenvalue|."""
    rows = rows.detach().double().cpu()
    out = {}
    for name, sl in GROUPS.items():
        mag = ref[:, sl].abs().max(dim=1, keepdim=True).values
        out[name] = float(((rows[:, sl] - ref[:, sl]).abs() / mag).max())
    return out
