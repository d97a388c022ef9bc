"""``gnn.trainer`` on the CPU with a tiny torch module that has the training / validation-step
interface: accumulation, validation interval, the weighted ``val_loss``, checkpoints, early
stopping, the NaN stop, ``max_steps``, ``predict(ckpt_path='best')``, bitwise resume, and one
gradient all-reduce per optimizer step over two gloo ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gnn.train import stiffness_loss


class _Batch(dict):
    @property
    def num_graphs(self):
        return int(self["stiffness"].shape[0])


class _Loader:
    """``n`` graphs in batches of ``bs``; the order of epoch e is a seeded permutation of (seed + e),
    as ``gnn.data.DataLoader``'s."""

    def __init__(self, n=40, bs=4, shuffle=True, seed=0, offset=0):
        g = torch.Generator().manual_seed(100 + offset)
        self.x = torch.randn(n, 5, generator=g)
        w = torch.randn(5, 36, generator=torch.Generator().manual_seed(7))
        self.c = (self.x @ w).view(n, 6, 6) + 0.3 * torch.randn(n, 6, 6, generator=g)
        self.n, self.bs, self.shuffle, self.seed, self.epoch = n, bs, shuffle, seed, 0

    def __len__(self):
        return (self.n + self.bs - 1) // self.bs

    def __iter__(self):
        idx = np.arange(self.n)
        if self.shuffle:
            idx = np.random.default_rng(self.seed + self.epoch).permutation(self.n)
        self.epoch += 1
        for s in range(0, self.n, self.bs):
            i = torch.from_numpy(idx[s:s + self.bs])
            yield _Batch(x=self.x[i], stiffness=self.c[i], ids=i)


class _Tiny(torch.nn.Module):
    def __init__(self, seed=0, nan_at=None, val_script=None):
        super().__init__()
        torch.manual_seed(seed)
        self.model = torch.nn.Sequential(torch.nn.Linear(5, 33), torch.nn.Tanh(), torch.nn.Linear(33, 36))
        self.nan_at, self.val_script = nan_at, val_script
        self.seen, self.val_rounds, self.train_calls = [], 0, 0

    def forward(self, batch):
        return {"stiffness": self.model(batch["x"]).view(-1, 6, 6)}

    def configure_optimizers(self):
        return torch.optim.AdamW(self.model.parameters(), lr=1e-2, amsgrad=True, weight_decay=1e-2)

    def training_step(self, batch, batch_idx=0):
        self.seen.append(batch["ids"].tolist())
        loss = stiffness_loss(self(batch)["stiffness"], batch["stiffness"])
        if self.nan_at is not None and self.train_calls == self.nan_at:
            loss = loss * float("nan")
        self.train_calls += 1
        return loss

    def validation_step(self, batch, batch_idx=0):
        if batch_idx == 0:
            self.val_rounds += 1
        loss = torch.nn.functional.mse_loss(self(batch)["stiffness"], batch["stiffness"])
        if self.val_script is not None:
            loss = loss * 0 + self.val_script[min(self.val_rounds, len(self.val_script)) - 1]
        self.val_metrics = {"val_loss": loss, "val_other": 2 * loss}
        return loss

    def predict_step(self, batch, batch_idx=0):
        return self(batch), batch


class _Recorder:
    """a callback that notes where every validation round happened"""

    def __init__(self):
        self.rounds = []

    def on_validation_end(self, trainer, module):
        self.rounds.append(dict(batches=trainer._batches_seen, step=trainer.global_step,
                                val_loss=trainer.callback_metrics["val_loss"],
                                weights={k: v.detach().clone() for k, v in module.state_dict().items()}))

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        pass


def _trainer(**kw):
    from gnn.trainer import Trainer
    kw.setdefault("log_every_n_steps", 1)
    kw.setdefault("fused_optimizer", True)
    return Trainer(**kw)


@pytest.mark.parametrize("fused_optimizer", [True, False])
def test_accumulation_steps_after_batches_4_8_10_with_the_gradients_of_loss_over_4(monkeypatch, fused_optimizer):
    from gnn.optim import FlatAdamW
    m = _Tiny()
    twin = _Tiny()
    twin.load_state_dict(m.state_dict())
    loader = _Loader()
    assert len(loader) == 10
    stepped, grads = [], []
    cls = FlatAdamW if fused_optimizer else torch.optim.AdamW
    real = cls.step

    def spy(self, *a, **k):
        stepped.append(tr._batches_seen)
        grads.append([p.grad.detach().clone() for p in m.parameters()])
        return real(self, *a, **k)
    monkeypatch.setattr(cls, "step", spy)
    tr = _trainer(max_steps=3, accumulate_grad_batches=4, fused_optimizer=fused_optimizer)
    tr.fit(m, loader)
    assert stepped == [4, 8, 10] and tr.global_step == 3 and tr.current_epoch == 1
    assert all(p.grad is None for p in m.parameters())
    # the first window by hand on the twin (same initial weights): sum_i grad(loss_i / 4)
    ref_loader = _Loader()
    for i, b in enumerate(ref_loader):
        if i == 4:
            break
        (stiffness_loss(twin(b)["stiffness"], b["stiffness"]) * 0.25).backward()
    for g, p in zip(grads[0], twin.parameters()):
        assert torch.equal(g, p.grad)
    assert len(tr.logged) == 10 and [e["batch"] for e in tr.logged] == list(range(1, 11))
    assert all(np.isfinite(e["loss"]) for e in tr.logged)


def test_validation_fires_every_val_check_interval_batches_over_epoch_boundaries():
    rec = _Recorder()
    m = _Tiny()
    tr = _trainer(max_steps=13, accumulate_grad_batches=2, val_check_interval=3, callbacks=[rec])
    tr.fit(m, _Loader(), _Loader(n=11, shuffle=False, offset=1))
    assert [r["batches"] for r in rec.rounds] == [3, 6, 9, 12, 15, 18, 21, 24]
    assert tr.global_step == 13 and m.val_rounds == 8


def test_val_loss_is_the_batch_size_weighted_mean_with_a_ragged_last_batch():
    m = _Tiny()
    valid = _Loader(n=11, bs=4, shuffle=False, offset=1)
    tr = _trainer()
    tr._setup(m)
    got = tr.validate(m, valid)
    sizes, losses = [], []
    with torch.no_grad():
        for b in valid:
            sizes.append(b.num_graphs)
            losses.append(float(torch.nn.functional.mse_loss(m(b)["stiffness"], b["stiffness"])))
    assert sizes == [4, 4, 3]
    want = sum(s * l for s, l in zip(sizes, losses)) / 11
    assert got["val_loss"] == pytest.approx(want, rel=1e-6)
    assert got["val_other"] == pytest.approx(2 * want, rel=1e-6)
    assert abs(want - sum(losses) / 3) > 1e-4 * want          # the plain mean over batches is another number
    assert m.training


def test_best_checkpoint_is_the_lowest_val_loss_and_predict_restores_it(tmp_path):
    from gnn.trainer import ModelCheckpoint
    script = [5.0, 3.0, 4.0, 2.5, 2.75, 6.0]
    rec = _Recorder()
    ck = ModelCheckpoint(filename="{epoch}-{step}-{val_loss:.3f}", monitor="val_loss", save_top_k=1)
    m = _Tiny(val_script=script)
    tr = _trainer(max_steps=12, val_check_interval=2, callbacks=[ck, rec], default_root_dir=str(tmp_path))
    valid = _Loader(n=8, shuffle=False, offset=1)
    tr.fit(m, _Loader(), valid)
    assert [r["val_loss"] for r in rec.rounds] == pytest.approx(script)
    assert ck.best_model_score == pytest.approx(2.5)
    files = os.listdir(tmp_path / "checkpoints")
    assert files == ["epoch=0-step=8-val_loss=2.500.ckpt"] and ck.best_model_path.endswith(files[0])
    saved = torch.load(ck.best_model_path, weights_only=False)
    assert set(saved) >= {"state_dict", "optimizer_states", "global_step", "epoch", "loops", "callbacks"}
    assert saved["global_step"] == 8 and set(saved["state_dict"]) == set(m.state_dict())
    assert set(saved["optimizer_states"][0]["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}
    best = rec.rounds[3]["weights"]
    assert any(not torch.equal(v, best[k]) for k, v in m.state_dict().items())     # training went on
    out = tr.predict(m, valid, ckpt_path="best")
    assert len(out) == 2 and out[0][0]["stiffness"].shape == (4, 6, 6)
    for k, v in m.state_dict().items():
        assert torch.equal(v, best[k]), k
    with torch.no_grad():
        b0 = next(iter(valid))
        assert torch.equal(out[0][0]["stiffness"], m(b0)["stiffness"])


def test_early_stopping_counts_validation_rounds():
    from gnn.trainer import EarlyStopping
    rec = _Recorder()
    es = EarlyStopping(monitor="val_loss", patience=2, mode="min")
    m = _Tiny(val_script=[3.0, 2.0, 2.5, 2.0, 1.0])
    tr = _trainer(max_steps=100, val_check_interval=2, callbacks=[es, rec])
    tr.fit(m, _Loader(), _Loader(n=8, shuffle=False, offset=1))
    # best at round 2; rounds 3 and 4 (2.0 is no improvement) use up the patience
    assert len(rec.rounds) == 4 and tr.should_stop and tr.global_step == 8 and es.stopped_step == 8
    assert es.best_score == 2.0 and es.wait_count == 2


@pytest.mark.parametrize("fused_optimizer", [True, False])
def test_a_nan_loss_stops_the_loop(capsys, fused_optimizer):
    m = _Tiny(nan_at=5)
    tr = _trainer(max_steps=100, accumulate_grad_batches=2, fused_optimizer=fused_optimizer)
    tr.fit(m, _Loader())
    assert tr.should_stop and tr.global_step == 3 and m.train_calls == 6
    assert "Loss is NaN. Stopping training" in capsys.readouterr().out
    finite = all(bool(torch.isfinite(p).all()) for p in m.parameters())
    if fused_optimizer:          # the flat step skipped the update; torch's own wrote NaN everywhere
        assert finite and tr.optimizer.read_state()["skipped"] == 1 and tr.optimizer.read_state()["step"] == 2
    else:
        assert not finite


def test_max_steps_holds_and_global_step_counts_optimizer_steps():
    m = _Tiny()
    tr = _trainer(max_steps=7, accumulate_grad_batches=3)
    tr.fit(m, _Loader())
    # 10 batches per epoch: steps after batches 3, 6, 9, 10 | 13, 16, 19
    assert tr.global_step == 7 and m.train_calls == 19 and tr.current_epoch == 1
    assert tr.optimizer.read_state()["step"] == 7
    tr2 = _trainer(max_steps=0)
    tr2.fit(_Tiny(), _Loader())
    assert tr2.global_step == 0


def test_shipped_defaults():
    """both fused pieces are opt-in (profiles/train_loop_summary.md says why)"""
    from gnn.trainer import Trainer
    from gnn.train import LightningWrappedModel
    assert Trainer().fused_optimizer is False
    assert not getattr(LightningWrappedModel(lambda p: torch.nn.Linear(1, 1), {}).params, "fused_loss", False)


def _opt_tensors(opt):
    sd = opt.state_dict()
    return [t for k in sorted(sd["state"]) for _, t in sorted(sd["state"][k].items())]


@pytest.mark.parametrize("acc", [1, 2])
def test_resume_continues_bitwise(tmp_path, acc):
    """6 steps straight = 3 steps + save + resume + 3 steps: parameters, optimizer state and batch
    order (3 steps at 4 batches per epoch and acc = 1 stop inside the first epoch; with acc = 2
    inside the second)."""
    straight = _Tiny()
    tr = _trainer(max_steps=6, accumulate_grad_batches=acc)
    tr.fit(straight, _Loader(n=16))
    first = _Tiny()
    tr1 = _trainer(max_steps=3, accumulate_grad_batches=acc)
    tr1.fit(first, _Loader(n=16))
    path = str(tmp_path / "mid.ckpt")
    tr1.save_checkpoint(path)
    second = _Tiny(seed=99)                                   # other weights: everything comes from the file
    tr2 = _trainer(max_steps=6, accumulate_grad_batches=acc)
    tr2.fit(second, _Loader(n=16), ckpt_path=path)
    assert tr2.global_step == 6 and tr2.current_epoch == tr.current_epoch
    assert first.seen + second.seen == straight.seen
    for (k, a), b in zip(straight.state_dict().items(), second.state_dict().values()):
        assert torch.equal(a, b), k
    for a, b in zip(_opt_tensors(tr.optimizer), _opt_tensors(tr2.optimizer)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    calls = []
    real = dist.all_reduce

    def counting(t, *a, **k):
        calls.append(t.numel())
        return real(t, *a, **k)
    dist.all_reduce = counting
    from gnn.trainer import Trainer
    m = _Tiny()                                                # the same init on both ranks
    tr = Trainer(max_steps=3, accumulate_grad_batches=4, gradient_clip_val=10.0, log_every_n_steps=1,
                 fused_optimizer=True)
    tr.fit(m, _Loader(offset=rank))                            # each rank its own graphs
    torch.save({"calls": calls, "numel": tr.optimizer.numel, "steps": tr.global_step,
                "weights": [p.detach().clone() for p in m.parameters()]}, f"{out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world_2_one_all_reduce_per_optimizer_step(tmp_path):
    out = str(tmp_path / "ddp")
    mp.spawn(_gloo_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = [torch.load(f"{out}.{r}", weights_only=False) for r in range(2)]
    for g in got:
        # 10 micro-batches, 3 optimizer steps: three all-reduces, each of the one flat buffer
        assert g["steps"] == 3 and g["calls"] == [g["numel"]] * 3
    for a, b in zip(got[0]["weights"], got[1]["weights"]):
        assert torch.equal(a, b)
    single = _Tiny()
    _trainer(max_steps=3, accumulate_grad_batches=4, gradient_clip_val=10.0).fit(single, _Loader(offset=0))
    assert any(not torch.equal(a, p.detach()) for a, p in zip(got[0]["weights"], single.parameters()))
