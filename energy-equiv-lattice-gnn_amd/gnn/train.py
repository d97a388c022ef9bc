"""Training-step semantics of ``LightningWrappedModel`` (``scripts/train_utils.py:26-64``)
without the Lightning runtime (not installed; the loop around these steps is ``gnn.trainer``).

``training_step`` computes the reference loss
``100 * mean_b( mean_ij (C - C^)^2 / mean_ij C^2 )``; ``configure_optimizers``
builds the same AdamW(amsgrad) (``scripts/train_utils.py:38-43``); ``validation_step``
computes the reference's two validation metrics (``scripts/train_utils.py:66-89``)
through ``gnn.metrics``.
"""
from __future__ import annotations

from argparse import Namespace
from typing import Any

import torch

from .metrics import metric_directions, validation_metrics


def stiffness_loss(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``scripts/train_utils.py:52-60`` (per-graph means over every non-batch dim: [B, 6, 6]
    as the reference, or the 21-vector of the vanilla CGC benchmark)."""
    dims = tuple(range(1, target.dim()))
    mean_stiffness = target.pow(2).mean(dim=dims)
    per_graph = torch.nn.functional.mse_loss(pred, target, reduction="none").mean(dim=dims)
    return 100 * (per_graph / mean_stiffness).mean()


class LightningWrappedModel(torch.nn.Module):
    def __init__(self, model: Any, params: Namespace) -> None:
        super().__init__()
        if isinstance(params, dict):
            params = Namespace(**params)
        self.params = params
        self.model = model(params)

    def configure_optimizers(self):
        p = self.params
        return torch.optim.AdamW(self.model.parameters(), lr=p.lr, betas=(p.beta1, 0.999),
                                 eps=p.epsilon, amsgrad=p.amsgrad, weight_decay=p.weight_decay)

    def training_step(self, batch, batch_idx: int = 0) -> torch.Tensor:
        out = self.model(batch)
        if getattr(self.params, "fused_loss", False):
            # one launch for the loss and its gradient (ops.stiffness_loss_fused); the backward of
            # the returned loss is scaled by self.loss_grad_scale (1 / accumulate_grad_batches,
            # set by the loop; default 1), its value is not.  Both logged values stay on the device.
            from .ops import stiffness_loss_fused
            loss, mean = stiffness_loss_fused(out["stiffness"], batch["stiffness"],
                                              getattr(self, "loss_grad_scale", 1.0))
            self.train_metrics = {"loss": loss.detach(), "stiffness_loss": mean}
            return loss
        return stiffness_loss(out["stiffness"], batch["stiffness"])

    def validation_step(self, batch, batch_idx: int = 0, directions=None) -> torch.Tensor:
        """``val_loss`` (MSE over all entries); both metrics (``val_loss``, ``val_stiff_dir_loss``:
        the L1 of the directional stiffness over ``directions``, 250 fresh random unit vectors by
        default) are left in ``self.val_metrics`` as 0-dim tensors on the batch's device."""
        with torch.no_grad():
            pred = self.model(batch)["stiffness"]
            if directions is None:
                directions = metric_directions(250, device=pred.device)
            self.val_metrics = validation_metrics(pred, batch["stiffness"], directions)
        return self.val_metrics["val_loss"]

    def predict_step(self, batch, batch_idx: int = 0):
        return self.model(batch), batch
