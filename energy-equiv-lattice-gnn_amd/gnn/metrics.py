"""Validation and test metrics of predicted stiffness matrices: the evaluation half of
``scripts/train_main.py`` (``validation_step``, ``scripts/train_utils.py:66-89``; ``predict`` ->
``obtain_errors`` -> ``aggr_errors`` -> CSV, ``scripts/train_utils.py:149-202``,
``scripts/train_main.py:111-120``).

``stiffness_metrics`` gives, per graph, the row ``METRIC_COLUMNS``: MSE and L1 over the 36 Mandel
entries, the L1 error and the target's mean of the directional stiffness over a set of unit
directions, and the eigenvalues of target and prediction.  On a HIP device it is one launch of
``eelg_stiffness_metrics`` (``csrc/eelg_metrics.hip``): no rank-4 tensor, no solver-library call,
no host synchronisation, bitwise repeatable.  On CPU tensors, or with ``EELG_METRICS_FUSED=0``, it
is the composed torch form written after the reference (cartesian rank-4 tensor, two einsums,
``torch.linalg.eigvalsh``): the second implementation, the timing baseline and the CPU path.
"""
from __future__ import annotations

import csv
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .lattice_data import mandel_to_cart4

METRIC_COLUMNS = (("mseloss", "loss", "dir_loss", "mean_stiffness")
                  + tuple(f"target_eig_{i}" for i in range(6))
                  + tuple(f"predicted_eig_{i}" for i in range(6)))
# one fused launch on a HIP device (1), or the composed torch form everywhere (0)
FUSED = os.environ.get("EELG_METRICS_FUSED", "1") != "0"
TABLE_COLUMNS = ("name", "rel_dens", "mean_stiffness", "loss", "mseloss", "dir_loss", "tag", "target_eig",
                 "predicted_eig")


def metric_directions(p: int = 250, seed: Optional[int] = None, device=None) -> torch.Tensor:
    """``[p, 3]`` unit fp32 directions: ``randn`` rows normalised (``scripts/train_utils.py:67-68``).
    With a ``seed`` they are drawn by a CPU generator, the same on every device, so an
    evaluation can be replayed; without one they are drawn on ``device`` as the reference does."""
    if seed is None:
        d = torch.randn(p, 3, dtype=torch.float32, device=device)
    else:
        d = torch.randn(p, 3, dtype=torch.float32, generator=torch.Generator().manual_seed(int(seed)))
    d = d / d.norm(dim=-1, keepdim=True)
    return d.to(device) if device is not None else d


def _eigvalsh(x: torch.Tensor) -> torch.Tensor:
    """``torch.linalg.eigvalsh`` (lower triangle); where the solver refuses the batch (a NaN
    entry), the graphs it refuses get NaN, as ``obtain_errors``' ``except`` does for the column."""
    try:
        return torch.linalg.eigvalsh(x)
    except RuntimeError:
        out = torch.full(x.shape[:-1], float("nan"), dtype=x.dtype, device=x.device)
        for g in range(x.shape[0]):
            try:
                out[g] = torch.linalg.eigvalsh(x[g])
            except RuntimeError:
                pass
        return out


def stiffness_metrics_composed(pred: torch.Tensor, target: torch.Tensor, directions: torch.Tensor,
                               scale: float = 1.0) -> torch.Tensor:
    """The reference's formulation, line by line (``scripts/train_utils.py:151-168``)."""
    target = scale * target
    prediction = scale * pred
    mse_loss = torch.nn.functional.mse_loss(prediction, target, reduction="none").mean(dim=(1, 2))
    loss = torch.nn.functional.l1_loss(prediction, target, reduction="none").mean(dim=(1, 2))
    target_4 = mandel_to_cart4(target)
    prediction_4 = mandel_to_cart4(prediction)
    d = directions
    c = torch.einsum("...ijkl,pi,pj,pk,pl->...p", target_4, d, d, d, d)
    c_pred = torch.einsum("...ijkl,pi,pj,pk,pl->...p", prediction_4, d, d, d, d)
    dir_loss = (c - c_pred).abs().mean(dim=1)
    mean_stiffness = c.mean(dim=1)
    target_eig = _eigvalsh(target)
    predicted_eig = _eigvalsh(prediction)
    return torch.cat([mse_loss[:, None], loss[:, None], dir_loss[:, None], mean_stiffness[:, None],
                      target_eig, predicted_eig], dim=1)


def stiffness_metrics(pred: torch.Tensor, target: torch.Tensor, directions: torch.Tensor, scale: float = 1.0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[B, 16]`` fp32 rows ``METRIC_COLUMNS`` of ``scale * pred`` against ``scale * target``
    (``[B, 6, 6]`` Mandel) over ``directions`` (``[P, 3]`` unit vectors).  ``out``: a contiguous
    ``[B, 16]`` fp32 tensor to write into (a row slice of a larger buffer).  Detached: there is
    no backward."""
    pred, target, directions = pred.detach(), target.detach(), directions.detach()
    nb = int(target.shape[0])
    if tuple(pred.shape) != (nb, 6, 6) or tuple(target.shape) != (nb, 6, 6):
        raise ValueError(f"stiffness_metrics: pred {tuple(pred.shape)}, target {tuple(target.shape)}; "
                         "both must be [B, 6, 6]")
    if directions.dim() != 2 or directions.shape[1] != 3 or directions.shape[0] < 1:
        raise ValueError(f"stiffness_metrics: directions {tuple(directions.shape)}, expected [P >= 1, 3]")
    if pred.device != target.device or directions.device != target.device:
        raise ValueError("stiffness_metrics: pred, target and directions must share a device")
    if out is not None and (tuple(out.shape) != (nb, len(METRIC_COLUMNS)) or out.dtype != torch.float32
                            or not out.is_contiguous() or out.device != target.device):
        raise ValueError(f"stiffness_metrics: out must be a contiguous fp32 [{nb}, {len(METRIC_COLUMNS)}] "
                         "tensor on the inputs' device")
    if not (FUSED and target.is_cuda):
        rows = stiffness_metrics_composed(pred.float(), target.float(), directions.float(), scale)
        if out is None:
            return rows
        out.copy_(rows)
        return out
    pred = pred.to(torch.float32).contiguous()
    target = target.to(torch.float32).contiguous()
    directions = directions.to(torch.float32).contiguous()
    if out is None:
        out = torch.empty((nb, len(METRIC_COLUMNS)), dtype=torch.float32, device=target.device)
    with torch.cuda.device(target.device):
        _lib.launch("stiffness_metrics", _lib.load().eelg_stiffness_metrics, pred, target, directions, nb,
                     int(directions.shape[0]), float(scale), out, on=target, timed="stiffness_metrics")
    return out


def validation_metrics(pred: torch.Tensor, target: torch.Tensor, directions: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``{'val_loss', 'val_stiff_dir_loss'}`` of ``validation_step`` (``scripts/train_utils.py:
    76-83``) as 0-dim tensors on the inputs' device: the MSE over all entries and the L1 of the
    directional stiffness over all graphs x directions.  Every graph has the same number of
    entries and directions, so both are the means of the per-graph columns.  Nothing is read
    back."""
    rows = stiffness_metrics(pred, target, directions, 1.0)
    return {"val_loss": rows[:, 0].mean(), "val_stiff_dir_loss": rows[:, 2].mean()}


class ErrorTable:
    """The per-graph error table of ``obtain_errors`` as numpy columns (``TABLE_COLUMNS``):
    ``name`` [G] (objects), ``rel_dens`` [G] (or [G, k]), ``mean_stiffness`` / ``loss`` /
    ``mseloss`` / ``dir_loss`` [G] fp32, ``tag`` [G] (str), ``target_eig`` / ``predicted_eig``
    [G, 6] fp32 ascending."""

    def __init__(self, **columns):
        missing = [k for k in TABLE_COLUMNS if k not in columns]
        if missing or len(columns) != len(TABLE_COLUMNS):
            raise ValueError(f"ErrorTable: columns {sorted(columns)}, expected {TABLE_COLUMNS}")
        n = len(columns["loss"])
        for k in TABLE_COLUMNS:
            v = np.asarray(columns[k], dtype=object if k in ("name", "tag") else None)
            if v.shape[0] != n:
                raise ValueError(f"ErrorTable: column {k} has {v.shape[0]} rows, loss has {n}")
            setattr(self, k, v)

    def __len__(self) -> int:
        return int(self.loss.shape[0])

    def __getitem__(self, key: str) -> np.ndarray:
        if key not in TABLE_COLUMNS:
            raise KeyError(key)
        return getattr(self, key)

    @classmethod
    def from_rows(cls, rows: np.ndarray, names, rel_dens, tag: str) -> "ErrorTable":
        """``rows``: host ``[G, 16]`` in ``METRIC_COLUMNS`` order."""
        rows = np.asarray(rows)
        col = {k: i for i, k in enumerate(METRIC_COLUMNS[:4])}
        return cls(name=np.asarray(list(names), dtype=object), rel_dens=np.asarray(rel_dens),
                   mean_stiffness=rows[:, col["mean_stiffness"]].copy(), loss=rows[:, col["loss"]].copy(),
                   mseloss=rows[:, col["mseloss"]].copy(), dir_loss=rows[:, col["dir_loss"]].copy(),
                   tag=np.full(rows.shape[0], tag, dtype=object), target_eig=rows[:, 4:10].copy(),
                   predicted_eig=rows[:, 10:16].copy())

    @classmethod
    def concat(cls, tables: Sequence["ErrorTable"]) -> "ErrorTable":
        tables = list(tables)
        if not tables:
            raise ValueError("ErrorTable.concat: no tables")
        return cls(**{k: np.concatenate([t[k] for t in tables]) for k in TABLE_COLUMNS})

    def to_csv(self, path) -> None:
        """One line per graph, ``TABLE_COLUMNS`` as the header; vector cells (the eigenvalues) are
        written as ``[v0 v1 ...]``.  Floats are written with ``repr``: they read back exactly."""
        def cell(v):
            if isinstance(v, np.ndarray):
                return "[" + " ".join(repr(float(x)) for x in v.reshape(-1)) + "]"
            if isinstance(v, (np.floating, float)):
                return repr(float(v))
            return str(v)
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(TABLE_COLUMNS)
            for i in range(len(self)):
                w.writerow([cell(self[k][i]) for k in TABLE_COLUMNS])

    def to_frame(self):
        """The reference's ``pandas.DataFrame`` (eigenvalue cells hold one array per graph)."""
        import pandas as pd
        cols = {}
        for k in TABLE_COLUMNS:
            v = self[k]
            cols[k] = list(v) if v.ndim > 1 else v
        return pd.DataFrame(cols)


def _names(batch, n: int) -> List:
    if "name" in batch:
        v = batch["name"]
        return [v] if isinstance(v, str) else list(v)
    return [None] * n


def obtain_errors(results, tag: str, directions: Optional[torch.Tensor] = None) -> ErrorTable:
    """``scripts/train_utils.py:149-171``: ``results`` is a list of ``(prediction_dict, batch)`` pairs
    as ``predict_step`` returns them.  Targets and predictions are multiplied by 10 (the dataset
    multiplier the reference takes back here).  ``directions``: ``[P, 3]`` unit vectors; 250 fresh
    random ones by default, as in the reference."""
    target = torch.cat([x[1]["stiffness"] for x in results])
    prediction = torch.cat([x[0]["stiffness"] for x in results]).detach()
    names = np.concatenate([np.asarray(_names(x[1], int(x[1]["stiffness"].shape[0])), dtype=object) for x in results])
    if all("rel_dens" in x[1] for x in results):
        rel_dens = torch.cat([torch.as_tensor(x[1]["rel_dens"]).reshape(x[1]["stiffness"].shape[0], -1)
                              for x in results]).cpu().numpy()
        rel_dens = rel_dens[:, 0] if rel_dens.shape[1] == 1 else rel_dens
    else:
        rel_dens = np.full(target.shape[0], np.nan, dtype=np.float32)
    if directions is None:
        directions = metric_directions(250, device=target.device)
    rows = stiffness_metrics(prediction, target, directions.to(target.device), 10.0)
    return ErrorTable.from_rows(rows.cpu().numpy(), names, rel_dens, tag)


_AGGR_MEAN = ("loss", "rel_loss", "mseloss", "mse_rel_loss", "dir_loss", "rel_dir_loss", "eig_loss", "rel_eig_loss")
_AGGR_MIN = ("min_pred_eig", "min_target_eig")


def aggr_errors(table) -> Dict[str, float]:
    """``scripts/train_utils.py:173-202`` over an ``ErrorTable`` or a DataFrame with its columns:
    per tag the means of ``loss, rel_loss, mseloss, mse_rel_loss, dir_loss, rel_dir_loss, eig_loss,
    rel_eig_loss``, the minima of ``min_pred_eig, min_target_eig`` and ``prop_eig_negative`` (the
    share of predictions with a negative eigenvalue), keyed ``<column>_<tag>``; ``{}`` if any
    ``loss`` is NaN.  The eigenvalue products (volumes) are formed in fp64 on the host.  The
    input is left as it is (the reference adds its working columns to the frame)."""
    def col(k, width=None):
        v = table[k]
        v = v.to_numpy() if hasattr(v, "to_numpy") else np.asarray(v)
        if width is not None and (v.dtype == object or v.ndim == 1):
            v = np.stack([np.asarray(r, dtype=np.float64).reshape(-1) for r in v])
        return v
    loss = col("loss").astype(np.float64)
    if np.isnan(loss).any():
        return {}
    mean_stiffness = col("mean_stiffness").astype(np.float64)
    mseloss, dir_loss = col("mseloss").astype(np.float64), col("dir_loss").astype(np.float64)
    peig, teig = col("predicted_eig", 6).astype(np.float64), col("target_eig", 6).astype(np.float64)
    tags = np.asarray([str(t) for t in col("tag")], dtype=object)
    predicted_volumes, target_volumes = peig.prod(axis=1), teig.prod(axis=1)
    eig_loss = np.abs(predicted_volumes - target_volumes)
    cols = {"loss": loss, "rel_loss": loss / mean_stiffness, "mseloss": mseloss,
            "mse_rel_loss": np.sqrt(mseloss) / mean_stiffness, "dir_loss": dir_loss,
            "rel_dir_loss": dir_loss / mean_stiffness, "eig_loss": eig_loss,
            "rel_eig_loss": eig_loss / target_volumes,
            "min_pred_eig": peig.min(axis=1), "min_target_eig": teig.min(axis=1)}
    params: Dict[str, float] = {}
    uniq = sorted(set(tags.tolist()))
    for tag in uniq:
        sel = tags == tag
        for k in _AGGR_MEAN:
            params[f"{k}_{tag}"] = float(cols[k][sel].mean())
    for tag in uniq:
        sel = tags == tag
        for k in _AGGR_MIN:
            params[f"{k}_{tag}"] = float(cols[k][sel].min())
    for tag in uniq:
        sel = tags == tag
        params[f"prop_eig_negative_{tag}"] = float((cols["min_pred_eig"][sel] < 0).sum() / sel.sum())
    return params


def _loader_total(loader) -> int:
    """The number of graphs one pass over ``loader`` yields, from host data."""
    if hasattr(loader, "order") and hasattr(loader, "epoch"):          # DeviceLoader
        return int(sum(len(ids) for ids in loader.order(loader.epoch)))
    if hasattr(loader, "indices"):                                      # gnn.data.DataLoader
        return len(loader.indices)
    ds = getattr(loader, "dataset", None)
    if ds is not None and hasattr(ds, "__len__") and not getattr(loader, "drop_last", False):
        return len(ds)
    raise TypeError("evaluate: the loader must say how many graphs it yields (a DeviceLoader, a gnn.DataLoader, or "
                    "a loader with a sized .dataset): the result buffer is allocated before the first batch")


def evaluate(model, loader, tag: str, directions: Optional[torch.Tensor] = None, seed: int = 0,
             scale: float = 10.0, group=None) -> ErrorTable:
    """One test pass: ``model`` (any callable returning ``{'stiffness': [B, 6, 6]}``) over every
    batch of ``loader`` under ``no_grad``, the table of ``obtain_errors`` as the result.

    Each batch's rows are written by ``stiffness_metrics`` into its slice of one preallocated
    device buffer (with the batch's ``rel_dens`` behind them); the host reads the buffer back
    once, after the last batch.  ``directions`` default to ``metric_directions(250, seed)``;
    ``scale`` is ``obtain_errors``' 10.  Names and ``rel_dens`` come from the batches (``None`` /
    NaN where the batches have none).  With a process ``group`` every rank evaluates its own loader
    (its shard) and the host tables are exchanged with ``all_gather_object``: every rank returns
    the whole table, rank 0's rows first.  A sharded ``DeviceLoader`` wraps a ragged last global
    batch round, so the wrapped graphs appear twice."""
    ncol = len(METRIC_COLUMNS)
    total = _loader_total(loader)
    buf = None              # flat fp32: [total, 16] metric rows | [total, k] rel_dens
    names: List = []
    k_rel = 0
    done = 0
    with torch.no_grad():
        for batch in loader:
            pred = model(batch)["stiffness"]
            target = batch["stiffness"]
            nb = int(target.shape[0])
            if directions is None:
                directions = metric_directions(250, seed=seed, device=target.device)
            rel = None
            if "rel_dens" in batch and batch["rel_dens"] is not None:
                rel = torch.as_tensor(batch["rel_dens"]).to(device=target.device, dtype=torch.float32).reshape(nb, -1)
            names.extend(_names(batch, nb))
            if buf is None:
                k_rel = int(rel.shape[1]) if rel is not None else 0
                buf = torch.full((total * (ncol + k_rel),), float("nan"), dtype=torch.float32, device=target.device)
            if done + nb > total:
                raise RuntimeError(f"evaluate: the loader yields more than the {total} graphs it announced")
            stiffness_metrics(pred, target, directions, scale, out=buf[done * ncol:(done + nb) * ncol].view(nb, ncol))
            if (rel.shape[1] if rel is not None else 0) != k_rel:
                raise RuntimeError("evaluate: rel_dens must be carried by all batches or by none")
            if k_rel:
                o = total * ncol + done * k_rel
                buf[o:o + nb * k_rel].view(nb, k_rel).copy_(rel)
            done += nb
    if done != total or done == 0:
        raise RuntimeError(f"evaluate: the loader yielded {done} graphs and announced {total}")
    host = buf.cpu().numpy()                      # the one device -> host copy of the pass
    rows = host[:total * ncol].reshape(total, ncol)
    if k_rel:
        rel_dens = host[total * ncol:].reshape(total, k_rel)
        rel_dens = rel_dens[:, 0].copy() if k_rel == 1 else rel_dens.copy()
    else:
        rel_dens = np.full(total, np.nan, dtype=np.float32)
    table = ErrorTable.from_rows(rows, names, rel_dens, tag)
    if group is not None:
        import torch.distributed as dist
        parts: List[Optional[ErrorTable]] = [None] * dist.get_world_size(group)
        dist.all_gather_object(parts, table, group=group)
        table = ErrorTable.concat(parts)
    return table
