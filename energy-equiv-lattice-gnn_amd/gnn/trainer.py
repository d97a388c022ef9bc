"""The training loop of ``scripts/train_main.py:89-111``: the subset of ``pytorch_lightning``'s
``Trainer`` / ``ModelCheckpoint`` / ``EarlyStopping`` that the reference's four training scripts
use, with the same argument names, on ``FlatAdamW`` (``gnn.optim``) and, with
``params.fused_loss``, the fused loss (``ops.stiffness_loss_fused``).

Semantics as Lightning's: the loss is always scaled by ``1 / accumulate_grad_batches``; the
micro-batches left over at an epoch's end trigger a step; ``val_check_interval`` counts training
batches (over epoch boundaries, ``check_val_every_n_epoch=None`` as the reference sets it; without
an interval validation runs at every epoch's end); ``val_loss`` is the batch-size-weighted mean
over the validation loader, all-reduced across ranks; ``global_step`` counts optimizer steps;
``EarlyStopping`` counts validation rounds.

The loop never waits for the device inside a step.  Losses go into a device buffer; the host reads
it, with the optimizer's ``skipped`` counter and last gradient norm, once per
``log_every_n_steps`` optimizer steps and at validation.  A skipped step (a gradient norm that is
not finite) sets ``should_stop`` with the reference's "Loss is NaN. Stopping training" message.
One difference from the reference: there the NaN step has already gone through AdamW and every
weight is NaN by the time the loop stops; here ``FlatAdamW`` skips that update and the parameters
stay finite (the stop is noticed at the next read of the counter, at most ``log_every_n_steps``
steps later, none of which can damage them either).

A checkpoint file holds the module's ``state_dict`` under Lightning's key names (``state_dict``,
parameters prefixed ``model.``), the optimizer state in ``torch.optim.AdamW``'s format
(``optimizer_states``), ``global_step``, ``epoch``, the position in the epoch, gradients of an
unfinished accumulation window and the callbacks' state; ``fit(ckpt_path=...)`` continues bitwise.
"""
from __future__ import annotations

import datetime
import math
import os
import time
from typing import Any, Dict, List, Optional

import torch
import torch.distributed as dist

from .optim import FlatAdamW
from .parallel import FlatGradAllReduce

NAN_MESSAGE = "Loss is NaN. Stopping training"


def _world(group=None) -> int:
    return dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1


def _rank() -> int:
    return dist.get_rank() if (dist.is_available() and dist.is_initialized()) else 0


def rank_zero_info(msg: str) -> None:
    if _rank() == 0:
        print(msg, flush=True)


class Callback:
    def on_train_batch_end(self, trainer: "Trainer", module, outputs, batch, batch_idx: int) -> None:
        """after the batch's backward and, at a window's end, its optimizer step (``outputs``: the
        loss tensor, still on the device; reading it here waits for the device)"""

    def on_validation_end(self, trainer: "Trainer", module) -> None:
        pass

    def state_dict(self) -> Dict[str, Any]:
        return {}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        pass


def _better(current: float, best: Optional[float], mode: str) -> bool:
    if best is None:
        return True
    return current < best if mode == "min" else current > best


class ModelCheckpoint(Callback):
    """Keeps the checkpoint with the best ``monitor`` (``save_top_k=1``) under
    ``dirpath`` (default ``<default_root_dir>/checkpoints``) and records ``best_model_path`` /
    ``best_model_score``.  ``filename`` is Lightning's template: ``'{epoch}-{step}-{val_loss:.3f}'``
    gives ``epoch=3-step=100-val_loss=0.123.ckpt``."""

    def __init__(self, dirpath: Optional[str] = None, filename: Optional[str] = None,
                 monitor: str = "val_loss", save_top_k: int = 1, mode: str = "min",
                 every_n_epochs: Optional[int] = None, verbose: bool = False):
        if save_top_k != 1:
            raise ValueError("ModelCheckpoint: save_top_k=1 (the reference's setting) is the supported value")
        if mode not in ("min", "max"):
            raise ValueError(f"ModelCheckpoint: mode {mode!r}")
        self.dirpath, self.filename, self.monitor, self.mode = dirpath, filename, monitor, mode
        self.save_top_k, self.verbose = save_top_k, verbose
        self.best_model_path = ""
        self.best_model_score: Optional[float] = None

    def format_name(self, trainer: "Trainer") -> str:
        template = self.filename or "{epoch}-{step}"
        values = dict(trainer.callback_metrics, epoch=trainer.current_epoch, step=trainer.global_step)
        for key in values:
            template = template.replace("{" + key, key + "={" + key)
        return template.format(**values) + ".ckpt"

    def on_validation_end(self, trainer: "Trainer", module) -> None:
        current = trainer.callback_metrics.get(self.monitor)
        if current is None or not _better(current, self.best_model_score, self.mode):
            return
        dirpath = self.dirpath or os.path.join(trainer.default_root_dir, "checkpoints")
        previous = self.best_model_path
        self.best_model_path = os.path.join(dirpath, self.format_name(trainer))
        self.best_model_score = float(current)
        trainer.save_checkpoint(self.best_model_path)
        if previous and previous != self.best_model_path and trainer.is_global_zero and os.path.exists(previous):
            os.remove(previous)
        if self.verbose:
            rank_zero_info(f"{self.monitor} {current:.6g}: saved {self.best_model_path}")

    def state_dict(self):
        return {"best_model_path": self.best_model_path, "best_model_score": self.best_model_score}

    def load_state_dict(self, state):
        self.best_model_path = state.get("best_model_path", "")
        self.best_model_score = state.get("best_model_score")


class EarlyStopping(Callback):
    """Stops when ``monitor`` has not improved in ``patience`` validation rounds (or is not
    finite)."""

    def __init__(self, monitor: str = "val_loss", patience: int = 3, mode: str = "min", min_delta: float = 0.0,
                 verbose: bool = False, strict: bool = True, check_finite: bool = True):
        if mode not in ("min", "max"):
            raise ValueError(f"EarlyStopping: mode {mode!r}")
        self.monitor, self.patience, self.mode, self.min_delta = monitor, int(patience), mode, abs(min_delta)
        self.verbose, self.strict, self.check_finite = verbose, strict, check_finite
        self.wait_count = 0
        self.best_score: Optional[float] = None
        self.stopped_step: Optional[int] = None

    def on_validation_end(self, trainer: "Trainer", module) -> None:
        current = trainer.callback_metrics.get(self.monitor)
        if current is None:
            if self.strict:
                raise RuntimeError(f"EarlyStopping: no metric {self.monitor!r} among "
                                   f"{sorted(trainer.callback_metrics)}")
            return
        if self.check_finite and not math.isfinite(current):
            self._stop(trainer, f"{self.monitor} = {current} is not finite")
            return
        margin = -self.min_delta if self.mode == "min" else self.min_delta
        if _better(current - margin if self.best_score is not None else current, self.best_score, self.mode):
            self.best_score, self.wait_count = float(current), 0
            return
        self.wait_count += 1
        if self.wait_count >= self.patience:
            self._stop(trainer, f"{self.monitor} did not improve in the last {self.wait_count} validation rounds")

    def _stop(self, trainer, why: str) -> None:
        trainer.should_stop = True
        self.stopped_step = trainer.global_step
        if self.verbose:
            rank_zero_info(f"EarlyStopping: {why}")

    def state_dict(self):
        return {"wait_count": self.wait_count, "best_score": self.best_score, "stopped_step": self.stopped_step}

    def load_state_dict(self, state):
        self.wait_count = state.get("wait_count", 0)
        self.best_score = state.get("best_score")
        self.stopped_step = state.get("stopped_step")


def _seconds(max_time) -> Optional[float]:
    """Lightning's ``max_time``: 'DD:HH:MM:SS', a ``timedelta``, a dict of its keywords, or seconds."""
    if max_time is None:
        return None
    if isinstance(max_time, str):
        d, h, m, s = (int(x) for x in max_time.split(":"))
        return float(((d * 24 + h) * 60 + m) * 60 + s)
    if isinstance(max_time, datetime.timedelta):
        return max_time.total_seconds()
    if isinstance(max_time, dict):
        return datetime.timedelta(**max_time).total_seconds()
    return float(max_time)


def _probe(batch) -> Optional[torch.Tensor]:
    try:
        t = batch["stiffness"]
    except (KeyError, TypeError, IndexError, AttributeError):
        return None
    return t if isinstance(t, torch.Tensor) else None


def _batch_size(batch) -> int:
    n = getattr(batch, "num_graphs", None)
    if n is not None:
        return int(n)
    t = _probe(batch)
    if t is None:
        raise TypeError("Trainer: a batch needs .num_graphs or a 'stiffness' tensor to be weighted by its size")
    return int(t.shape[0])


class Trainer:
    def __init__(self, max_steps: int = -1, max_time=None, accumulate_grad_batches: int = 1,
                 gradient_clip_val: Optional[float] = None, val_check_interval: Optional[int] = None,
                 log_every_n_steps: int = 50, callbacks: Optional[List[Callback]] = None,
                 default_root_dir: Optional[str] = None, fused_optimizer: bool = False, group=None,
                 accelerator: str = "auto", check_val_every_n_epoch: Optional[int] = None):
        """``fused_optimizer``: adopt the module's optimizer into ``FlatAdamW`` (False, the default:
        torch's own ``clip_grad_norm_`` + ``optimizer.step()`` + ``zero_grad``, with
        ``FlatGradAllReduce`` between ranks; off by default because at accumulation 4 its gain per
        batch is inside the run-to-run spread, profiles/train_loop_summary.md).  ``group``: the process group of the data-parallel ranks.  ``accelerator`` and
        ``check_val_every_n_epoch`` are accepted for the reference's call and not used."""
        if accumulate_grad_batches < 1 or log_every_n_steps < 1:
            raise ValueError("Trainer: accumulate_grad_batches and log_every_n_steps are at least 1")
        if val_check_interval is not None and int(val_check_interval) < 1:
            raise ValueError("Trainer: val_check_interval counts training batches (an integer >= 1)")
        self.max_steps = -1 if max_steps is None else int(max_steps)
        self.max_time = _seconds(max_time)
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self.gradient_clip_val = gradient_clip_val
        self.val_check_interval = None if val_check_interval is None else int(val_check_interval)
        self.log_every_n_steps = int(log_every_n_steps)
        cbs = list(callbacks or [])
        # Lightning's order: checkpoints are written after the other callbacks have run
        self.callbacks = ([c for c in cbs if not isinstance(c, ModelCheckpoint)]
                          + [c for c in cbs if isinstance(c, ModelCheckpoint)])
        self.default_root_dir = default_root_dir or os.getcwd()
        self.fused_optimizer = bool(fused_optimizer)
        self.group = group
        self.global_step = 0
        self.current_epoch = 0
        self.should_stop = False
        self.callback_metrics: Dict[str, float] = {}
        self.logged: List[Dict[str, float]] = []     # one entry per training batch read back so far
        self.optimizer = None
        self._batch_pos = 0        # batches of the current epoch already consumed
        self._batches_seen = 0     # training batches over all epochs
        self._micro = 0            # micro-batches in the open accumulation window
        self._skipped_seen = 0
        self._buf = None
        self._buf_rows: List[int] = []

    @property
    def is_global_zero(self) -> bool:
        return _rank() == 0

    @property
    def checkpoint_callback(self) -> Optional[ModelCheckpoint]:
        for c in self.callbacks:
            if isinstance(c, ModelCheckpoint):
                return c
        return None

    # -- pieces ---------------------------------------------------------------------------------
    def _move(self, batch):
        t = _probe(batch)
        if t is not None and t.device != self._device and hasattr(batch, "to"):
            return batch.to(self._device)
        return batch

    def _setup(self, module) -> None:
        self.module = module
        params = [p for p in module.parameters() if p.requires_grad]
        self._params = params
        self._device = params[0].device
        module.loss_grad_scale = 1.0 / self.accumulate_grad_batches
        self._fused_loss = bool(getattr(getattr(module, "params", None), "fused_loss", False))
        opt = module.configure_optimizers()
        if self.fused_optimizer:
            opt = FlatAdamW.from_torch(opt, max_norm=self.gradient_clip_val, group=self.group)
        else:
            self._allreduce = FlatGradAllReduce(params, group=self.group)
        self.optimizer = opt
        cap = self.log_every_n_steps * self.accumulate_grad_batches
        if self.val_check_interval:
            cap = max(cap, self.val_check_interval)
        self._buf = torch.full((cap + self.accumulate_grad_batches, 2), float("nan"), device=self._device)
        self._buf_rows = []

    def _record(self, loss: torch.Tensor) -> None:
        """the batch's losses into the next row of the device buffer (one launch, no read)"""
        if len(self._buf_rows) == self._buf.shape[0]:
            self._flush_log()                 # (a loader without validation and a long epoch tail)
        row = self._buf[len(self._buf_rows)]
        tm = getattr(self.module, "train_metrics", None) if self._fused_loss else None
        if tm is not None:
            torch.stack([tm["loss"], tm["stiffness_loss"]], out=row)
        else:
            row[0].copy_(loss.detach())
        self._buf_rows.append(self._batches_seen)

    def _flush_log(self) -> None:
        """Read the buffered losses and the optimizer's device-side state (synchronises), decide
        the NaN stop and the time limit."""
        n = len(self._buf_rows)
        rows = self._buf[:n].cpu() if n else torch.zeros(0, 2)
        state = self.optimizer.read_state() if self.fused_optimizer else {}
        for i, b in enumerate(self._buf_rows):
            entry = {"batch": b, "loss": float(rows[i, 0]), "stiffness_loss": float(rows[i, 1])}
            if i == n - 1:
                entry.update({"global_step": self.global_step, **{f"optimizer_{k}": v for k, v in state.items()}})
            self.logged.append(entry)
        self._buf_rows = []
        nan = bool(torch.isnan(rows[:, 0]).any()) if n else False
        if state:
            nan = nan or state["skipped"] > self._skipped_seen
            self._skipped_seen = state["skipped"]
        if nan:
            self.should_stop = True
            rank_zero_info(NAN_MESSAGE)
        self._check_time(sync=True)

    def _check_time(self, sync: bool) -> None:
        if self.max_time is None:
            return
        over = time.monotonic() - self._t0 >= self.max_time
        if _world(self.group) > 1:
            if not sync:
                return          # ranks decide together, where the loop reads the device anyway
            flag = torch.tensor([1.0 if over else 0.0], device=self._device)
            dist.broadcast(flag, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0,
                           group=self.group)
            over = bool(flag.item())
        if over:
            self.should_stop = True

    def _optimizer_step(self) -> None:
        if self.fused_optimizer:
            self.optimizer.step()             # all-reduce, clip, AdamW and zeroing inside
        else:
            self._allreduce()
            if self.gradient_clip_val:
                torch.nn.utils.clip_grad_norm_(self._params, self.gradient_clip_val)
            self.optimizer.step()
            self.optimizer.zero_grad(set_to_none=True)
        self._micro = 0
        self.global_step += 1
        if self.global_step % self.log_every_n_steps == 0:
            self._flush_log()
        if self.max_steps >= 0 and self.global_step >= self.max_steps:
            self.should_stop = True

    def _train_batch(self, module, batch, batch_idx: int, n_batches: int) -> torch.Tensor:
        """One training batch: forward, backward of loss / accumulate_grad_batches, the loss into
        the device buffer and, at the window's or the epoch's end, the optimizer step.  Nothing in
        here reads the device (except the buffered read every ``log_every_n_steps`` steps)."""
        batch = self._move(batch)
        loss = module.training_step(batch, batch_idx)
        if self._fused_loss:
            loss.backward()                            # scaled by 1 / accumulate_grad_batches inside the launch
        else:
            (loss * (1.0 / self.accumulate_grad_batches)).backward()
        self._batches_seen += 1
        self._batch_pos = batch_idx + 1
        self._micro += 1
        self._record(loss)
        if self._micro == self.accumulate_grad_batches or batch_idx + 1 == n_batches:
            self._optimizer_step()
        return loss

    def validate(self, module, valid_loader) -> Dict[str, float]:
        """``val_loss`` (and every other entry of ``module.val_metrics``) as batch-size-weighted
        means over ``valid_loader``, summed over the ranks; one read at the end."""
        was_training = module.training
        module.eval()
        sums: Dict[str, torch.Tensor] = {}
        count = 0
        with torch.no_grad():
            for i, batch in enumerate(valid_loader):
                batch = self._move(batch)
                loss = module.validation_step(batch, i)
                metrics = dict(getattr(module, "val_metrics", None) or {})
                metrics.setdefault("val_loss", loss)
                bs = _batch_size(batch)
                count += bs
                for k, v in metrics.items():
                    v = v.detach().to(torch.float32) * bs
                    sums[k] = v if k not in sums else sums[k] + v
        module.train(was_training)
        keys = sorted(sums)
        pack = torch.stack([sums[k] for k in keys] + [torch.tensor(float(count), device=self._device)]) \
            if keys else torch.zeros(1, device=self._device)
        if _world(self.group) > 1:
            dist.all_reduce(pack, group=self.group)
        vals = pack.cpu().tolist()
        out = {k: vals[i] / vals[-1] for i, k in enumerate(keys)} if vals[-1] > 0 else {}
        self.callback_metrics.update(out)
        return out

    def _validation_round(self, module, valid_loader) -> None:
        self.validate(module, valid_loader)
        self._flush_log()
        for cb in self.callbacks:
            cb.on_validation_end(self, module)

    # -- checkpoints ------------------------------------------------------------------------------
    def save_checkpoint(self, path: str) -> None:
        ckpt = {
            "state_dict": {k: v.detach().clone() for k, v in self.module.state_dict().items()},
            "optimizer_states": [self.optimizer.state_dict()],
            "global_step": self.global_step,
            "epoch": self.current_epoch,
            "loops": {"batch_pos": self._batch_pos, "batches_seen": self._batches_seen, "micro": self._micro},
            "pending_grads": [None if p.grad is None else p.grad.detach().clone() for p in self._params],
            "callbacks": {f"{type(c).__name__}:{i}": c.state_dict() for i, c in enumerate(self.callbacks)},
        }
        if self.is_global_zero:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            tmp = path + ".part"
            torch.save(ckpt, tmp)
            os.replace(tmp, path)
        if _world(self.group) > 1:
            dist.barrier(group=self.group)

    def _load_weights(self, module, state_dict) -> None:
        module.load_state_dict(state_dict)
        for m in module.modules():            # weight-derived caches (the packed weights of o3.Linear)
            inv = getattr(m, "invalidate_packed", None)
            if inv is not None:
                inv()

    def _load_checkpoint(self, path: str) -> None:
        ckpt = torch.load(path, map_location=self._device, weights_only=False)
        self._load_weights(self.module, ckpt["state_dict"])
        self.optimizer.load_state_dict(ckpt["optimizer_states"][0])
        if self.fused_optimizer:                   # skips counted before the checkpoint are not new ones
            self._skipped_seen = self.optimizer.read_state()["skipped"]
        self.global_step = int(ckpt["global_step"])
        self.current_epoch = int(ckpt["epoch"])
        loops = ckpt.get("loops", {})
        self._batch_pos = int(loops.get("batch_pos", 0))
        self._batches_seen = int(loops.get("batches_seen", 0))
        self._micro = int(loops.get("micro", 0))
        for p, g in zip(self._params, ckpt.get("pending_grads") or [None] * len(self._params)):
            p.grad = None if g is None else g.to(p.device).clone()
        saved = ckpt.get("callbacks", {})
        for i, c in enumerate(self.callbacks):
            st = saved.get(f"{type(c).__name__}:{i}")
            if st is not None:
                c.load_state_dict(st)

    # -- the loop -----------------------------------------------------------------------------------
    def fit(self, module, train_loader, valid_loader=None, ckpt_path: Optional[str] = None) -> None:
        self._setup(module)
        if ckpt_path is not None:
            self._load_checkpoint(ckpt_path)
        self.should_stop = self.max_steps >= 0 and self.global_step >= self.max_steps
        self._t0 = time.monotonic()
        module.train()
        while not self.should_stop:
            if hasattr(train_loader, "epoch"):
                train_loader.epoch = self.current_epoch       # the epoch's order is a function of its number
            n_batches = len(train_loader)
            for batch_idx, batch in enumerate(train_loader):
                if batch_idx < self._batch_pos:
                    continue                                   # consumed before the checkpoint
                loss = self._train_batch(module, batch, batch_idx, n_batches)
                for cb in self.callbacks:
                    hook = getattr(cb, "on_train_batch_end", None)
                    if hook is not None:
                        hook(self, module, loss, batch, batch_idx)
                if (valid_loader is not None and self.val_check_interval
                        and self._batches_seen % self.val_check_interval == 0):
                    self._validation_round(module, valid_loader)
                self._check_time(sync=False)
                if self.should_stop:
                    break
            if self._batch_pos >= n_batches:                   # the epoch is complete (also when it stops here)
                if valid_loader is not None and not self.val_check_interval and not self.should_stop:
                    self._validation_round(module, valid_loader)
                self.current_epoch += 1
                self._batch_pos = 0
            if n_batches == 0:
                break
        self._flush_log()

    def predict(self, module, loader, ckpt_path: Optional[str] = "best", return_predictions: bool = True):
        """``[module.predict_step(batch, i) for batch in loader]`` under ``no_grad``, after loading
        ``ckpt_path`` ('best': the checkpoint callback's ``best_model_path``; None: the weights as
        they are)."""
        if ckpt_path == "best":
            cb = self.checkpoint_callback
            if cb is None or not cb.best_model_path:
                raise RuntimeError("Trainer.predict(ckpt_path='best'): no ModelCheckpoint has saved a checkpoint")
            ckpt_path = cb.best_model_path
        self._device = next(module.parameters()).device
        if ckpt_path is not None:
            ckpt = torch.load(ckpt_path, map_location=self._device, weights_only=False)
            self._load_weights(module, ckpt["state_dict"])
        was_training = module.training
        module.eval()
        with torch.no_grad():
            out = [module.predict_step(self._move(batch), i) for i, batch in enumerate(loader)]
        module.train(was_training)
        return out if return_predictions else None
