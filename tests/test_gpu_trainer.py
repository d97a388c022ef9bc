"""The training step's tail on the device: ``eelg_stiffness_loss``, ``eelg_grad_sqnorm`` +
``eelg_adamw_flat`` (``csrc/eelg_optim.hip``), ``FlatAdamW`` and ``Trainer`` on the model.

Bounds: against fp64 values from the same fp32 inputs, 4x the error of the composed fp32 form on
the device (``gnn.train.stiffness_loss`` and its autograd; ``torch.optim.AdamW(fused=True)`` after
``clip_grad_norm_``), floored at 2^-23 of the compared value; set-wide (the largest error over the
cases of one test against 4x the baseline's largest), as in ``test_flat_adamw``.  Every figure is
printed before it is asserted."""
import pytest
import torch

from helpers import batch, params
from helpers_optim import HP, assert_bounded, clip_settings, errors, floors, hostile_grads, reference64, start_values, torch_adamw, worst

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23


# ---------------------------------------------------------------------------------------------
# the loss kernel
def _loss_case(nb, n, seed):
    gen = torch.Generator().manual_seed(seed)
    target = torch.randn(nb, n, generator=gen)
    if nb >= 3:
        target[nb // 2] *= 1e-12                      # a row of tiny norm
    pred = target + 0.1 * torch.randn(nb, n, generator=gen) * target.abs().amax(dim=1, keepdim=True)
    return pred, target


def _shape(t, n):
    return t.view(-1, 6, 6) if n == 36 else t


@pytest.fixture(scope="module")
def loss_runs():
    """every (B, n): fp64 oracle, composed fp32 on the device, and the kernel (twice)"""
    from gnn.ops import stiffness_loss_fused
    from gnn.train import stiffness_loss
    from oracle.train import stiffness_loss as oracle_loss
    runs = {}
    for n in (36, 21):
        for nb in (1, 3, 17, 65):
            pred, target = _loss_case(nb, n, 10 * nb + n)
            p64 = pred.double().requires_grad_(True)
            l64 = oracle_loss(p64.view(nb, n, 1), target.double().view(nb, n, 1))
            l64.backward()
            mean64 = (pred.double() - target.double()).pow(2).mean()
            pc = _shape(pred, n).to(DEV).requires_grad_(True)
            lc = stiffness_loss(pc, _shape(target, n).to(DEV))
            lc.backward()
            mc = float(torch.nn.functional.mse_loss(pc.detach(), _shape(target, n).to(DEV)))
            fused = []
            for _ in range(2):
                pf = _shape(pred, n).to(DEV).requires_grad_(True)
                lf, mf = stiffness_loss_fused(pf, _shape(target, n).to(DEV))
                lf.backward()
                fused.append((lf.detach().cpu(), mf.detach().cpu(), pf.grad.detach().cpu().view(nb, n)))
            runs[(nb, n)] = dict(pred=pred, target=target, l64=l64.item(), g64=p64.grad.detach(), mean64=float(mean64),
                                 lc=lc.item(), mc=mc, gc=pc.grad.detach().cpu().view(nb, n), fused=fused)
    return runs


def test_loss_kernel_against_the_fp64_oracle(loss_runs):
    """Loss, logged mean and gradient for B in {1, 3, 17, 65} x n in {36, 21}, a target row of norm
    1e-12 included, against ``oracle.train.stiffness_loss`` and its autograd in fp64.
    Measured set-wide (kernel | composed fp32 on the device): loss 1.0e-7 | 1.0e-7, gradient (of the
    graph's largest entry) 1.9e-7 | 2.2e-7, logged mean 1.3e-7 | 1.0e-7."""
    mine = {"loss": 0.0, "grad": 0.0, "mean": 0.0}
    base = {"loss": 0.0, "grad": 0.0, "mean": 0.0}
    for (nb, n), r in loss_runs.items():
        lf, mf, gf = r["fused"][0]
        assert lf.dim() == 0 and mf.dim() == 0
        scale = r["g64"].abs().amax(dim=1, keepdim=True)
        e = {"loss": abs(float(lf) - r["l64"]) / abs(r["l64"]),
             "grad": float(((gf.double() - r["g64"]).abs() / scale).max()),
             "mean": abs(float(mf) - r["mean64"]) / r["mean64"]}
        b = {"loss": abs(r["lc"] - r["l64"]) / abs(r["l64"]),
             "grad": float(((r["gc"].double() - r["g64"]).abs() / scale).max()),
             "mean": abs(r["mc"] - r["mean64"]) / r["mean64"]}
        print(f"B={nb} n={n}: kernel {e}  composed fp32 {b}")
        mine = {k: max(v, e[k]) for k, v in mine.items()}
        base = {k: max(v, b[k]) for k, v in base.items()}
    print("set-wide: kernel", mine, "composed fp32", base)
    assert mine["loss"] <= max(4 * base["loss"], ULP)
    assert mine["grad"] <= max(4 * base["grad"], ULP)
    assert mine["mean"] <= max(4 * base["mean"], ULP)


def test_loss_kernel_is_bitwise_repeatable(loss_runs):
    for key, r in loss_runs.items():
        for a, b in zip(*r["fused"]):
            assert torch.equal(a, b), key


def test_loss_kernel_honours_grad_scale_and_the_incoming_gradient(loss_runs):
    from gnn.ops import stiffness_loss_fused
    r = loss_runs[(17, 36)]
    lf, _mf, gf = r["fused"][0]
    p = r["pred"].view(-1, 6, 6).to(DEV).requires_grad_(True)
    loss, mean = stiffness_loss_fused(p, r["target"].view(-1, 6, 6).to(DEV), grad_scale=0.25)
    assert not mean.requires_grad
    (loss * 3.0).backward()
    assert torch.equal(loss.detach().cpu(), lf)                       # the value is not scaled
    assert torch.equal(p.grad.cpu().view(17, 36), gf * 0.25 * 3.0)    # powers of two and one multiply


def test_fused_loss_in_training_step_mirrors_val_metrics():
    from gnn.train import LightningWrappedModel

    class Stub(torch.nn.Module):
        def __init__(self, p):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor(1.1))

        def forward(self, b):
            return {"stiffness": self.w * b["stiffness"] + 0.05}
    pred, target = _loss_case(5, 36, 3)
    b = {"stiffness": target.view(-1, 6, 6).to(DEV)}
    plain = LightningWrappedModel(Stub, {}).to(DEV)
    fused = LightningWrappedModel(Stub, {"fused_loss": True}).to(DEV)
    fused.loss_grad_scale = 0.5
    lp = plain.training_step(b)
    assert not hasattr(plain, "train_metrics")
    lf = fused.training_step(b)
    assert set(fused.train_metrics) == {"loss", "stiffness_loss"}
    assert all(v.dim() == 0 and v.is_cuda and not v.requires_grad for v in fused.train_metrics.values())
    assert float(lf) == pytest.approx(float(lp), rel=1e-5)
    lp.backward()
    lf.backward()
    assert float(fused.model.w.grad) == pytest.approx(0.5 * float(plain.model.w.grad), rel=1e-4)


# ---------------------------------------------------------------------------------------------
# the norm and update kernels on raw flat buffers
def _run_flat(p0, grads, amsgrad, max_norm, poison=None):
    """the two launches per step; returns per step the flat values and the state row"""
    from gnn import _lib
    lib = _lib.load()
    n = p0.numel()
    p = p0.to(DEV).clone()
    m, v, vmax = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    rows = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    partials = torch.full((lib.eelg_sqnorm_parts(n),), float("nan"), device=DEV)
    out = []
    for s, g in enumerate(grads):
        gd = g.to(DEV).clone()
        if poison is not None and s == poison[0]:
            gd[poison[1]] = poison[2]
        st = _lib.stream(p)
        _lib.check(lib.eelg_grad_sqnorm(_lib.ptr(gd), n, _lib.ptr(partials), st), "grad_sqnorm")
        _lib.check(lib.eelg_adamw_flat(_lib.ptr(p), _lib.ptr(m), _lib.ptr(v), _lib.ptr(vmax if amsgrad else None),
                                       _lib.ptr(gd), n, _lib.ptr(partials), HP["lr"], HP["betas"][0],
                                       HP["betas"][1], HP["eps"], HP["weight_decay"], float(max_norm), int(amsgrad),
                                       _lib.ptr(rows[s & 1]), _lib.ptr(rows[(s + 1) & 1]), st), "adamw_flat")
        row = rows[(s + 1) & 1].cpu()
        out.append(dict(p=p.cpu(), m=m.cpu(), v=v.cpu(), vmax=vmax.cpu(), grad_zero=not bool(gd.any()),
                        t=int(row[0]), skipped=int(row[1]), norm=float(row.view(torch.float32)[2]),
                        coef=float(row.view(torch.float32)[3])))
    return out


NUMELS = (1, 63, 64, 65, 1027, 4099, 552210)


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("numel", NUMELS)
def test_flat_kernels_against_fp64(numel, amsgrad):
    """The hostile set: gradients x 1 and x 1/4, 3 steps, clip off / inactive / active / just under /
    just over the first step's norm; ``torch.optim.AdamW(fused=True)`` on the device is the fp32
    baseline.  Measured, largest over the sizes (kernels | torch): p 1.2e-3 lr | 1.2e-3 lr (numel
    552,210, where some |p| reach 5 and one ulp of p is 5e-4 lr), m 9.0e-7 | 4.7e-7, v 2.1e-7 |
    2.1e-7, vmax 2.1e-7 | 2.1e-7."""
    p0 = start_values(numel)
    mine, theirs, refs = [], [], []
    for scale in (1.0, 0.25):
        grads = hostile_grads(3, numel, scale=scale)
        for name, max_norm in clip_settings(grads[0]).items():
            ref = reference64(p0, grads, amsgrad, max_norm, **HP)
            got = _run_flat(p0, grads, amsgrad, max_norm)
            base, _ = torch_adamw([p0], [[g] for g in grads], torch.float32, amsgrad, max_norm, device=DEV, fused=True)
            mine += [errors(g, r, HP["lr"], amsgrad) for g, r in zip(got, ref)]
            theirs += [errors(b, r, HP["lr"], amsgrad) for b, r in zip(base, ref)]
            refs += ref
            print(f"numel={numel} scale={scale} clip={name}: kernels", worst(mine[-3:]), "torch", worst(theirs[-3:]))
            for g, r in zip(got, ref):
                assert g["grad_zero"] and g["t"] == r["t"] and g["skipped"] == 0
                assert abs(g["norm"] - r["norm"]) <= 4 * ULP * r["norm"]
                assert abs(g["coef"] - r["coef"]) <= 4 * ULP * r["coef"]
            if name in ("off", "inactive"):
                assert all(g["coef"] == 1.0 for g in got)
            if numel > 1:
                assert (got[0]["coef"] < 1.0) == (name in ("active", "just_under")), name
            if not amsgrad:
                assert not got[-1]["vmax"].any()       # never touched without amsgrad
    assert_bounded(worst(mine), worst(theirs), floors(refs, HP["lr"]), f"numel={numel} amsgrad={amsgrad}")


@pytest.mark.parametrize("numel", (65, 4099, 552210))
def test_flat_kernels_are_bitwise_repeatable(numel):
    p0, grads = start_values(numel), hostile_grads(3, numel)
    a, b = _run_flat(p0, grads, True, 10.0), _run_flat(p0, grads, True, 10.0)
    for x, y in zip(a, b):
        for k in ("p", "m", "v", "vmax"):
            assert torch.equal(x[k], y[k]), k
        assert (x["norm"], x["coef"]) == (y["norm"], y["coef"])


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("numel", (1, 65, 552210))
def test_a_gradient_that_is_not_finite_skips_the_step(numel, bad):
    p0, grads = start_values(numel), hostile_grads(3, numel)
    got = _run_flat(p0, grads, True, 10.0, poison=(1, numel - 1, bad))
    assert [g["t"] for g in got] == [1, 1, 2] and [g["skipped"] for g in got] == [0, 1, 1]
    assert all(g["grad_zero"] for g in got) and got[1]["coef"] == 0.0
    for k in ("p", "m", "v", "vmax"):
        assert torch.equal(got[0][k], got[1][k]), k
        assert bool(torch.isfinite(got[2][k]).all())
    assert not torch.equal(got[1]["p"], got[2]["p"])


def test_entry_points_reject_bad_arguments():
    from gnn import _lib
    lib = _lib.load()
    x = torch.zeros(8, device=DEV)
    rows = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    st = _lib.stream(x)
    assert lib.eelg_grad_sqnorm(_lib.ptr(x), 0, _lib.ptr(x), st) == -2
    assert lib.eelg_grad_sqnorm(_lib.ptr(x[1:]), 4, _lib.ptr(x), st) == -2            # misaligned
    args = (_lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), 8, _lib.ptr(x), 1e-3, .9, .999, 1e-8, 0., 0., 1)
    assert lib.eelg_adamw_flat(*args, _lib.ptr(rows[0]), _lib.ptr(rows[0]), st) == -2   # one row for both
    assert lib.eelg_stiffness_loss(_lib.ptr(x), _lib.ptr(x), 1, 8, 1.0, _lib.ptr(x), _lib.ptr(x), st) == -2
    torch.cuda.synchronize()


def test_flat_adamw_on_the_device_keeps_its_padding_zero():
    from gnn.optim import ALIGN, FlatAdamW
    sizes = (1, 3, 6, 33, 448)
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen).to(DEV)) for n in sizes]
    opt = FlatAdamW(ps, amsgrad=True, max_norm=10.0, **HP)
    assert opt.fused and opt.numel == 4 * ALIGN + 512
    for s in range(3):
        flat = hostile_grads(1, sum(sizes), seed=s)[0].to(DEV)
        for p, g in zip(ps[:-1] if s == 1 else ps, flat.split(sizes)):     # step 1: the last one has no gradient
            p.grad = g.clone()
        opt.step()
        assert all(p.grad is None for p in ps) and not opt.flat_g.any()
    mask = torch.ones(opt.numel, dtype=torch.bool, device=DEV)
    for p, o in zip(ps, opt._offsets):
        mask[o:o + p.numel()] = False
        assert p.data_ptr() == opt.flat_p.data_ptr() + 4 * o
    for buf in (opt.flat_p, opt.flat_m, opt.flat_v, opt.flat_vmax, opt.flat_g):
        assert not buf[mask].any()
    assert opt.read_state()["step"] == 3 and opt.read_state()["skipped"] == 0


# ---------------------------------------------------------------------------------------------
# model level
@pytest.fixture(scope="module")
def pieces():
    b1, rmax = batch(4, 24, 96, 1234)
    b2, _ = batch(4, 24, 96, 4321)
    p = params(2, lmax=4, max_edge_radius=rmax, lr=1e-3, beta1=0.9, epsilon=1e-8, amsgrad=True, weight_decay=1e-2)
    return p, [b1.to(DEV), b2.to(DEV)]


def _module(p, seed=0, **kw):
    from argparse import Namespace
    from gnn import EnergyEquivGNN
    from gnn.train import LightningWrappedModel
    torch.manual_seed(seed)
    return LightningWrappedModel(EnergyEquivGNN, Namespace(**{**vars(p), **kw})).to(DEV)


def _flat_of(ts):
    return torch.cat([t.detach().reshape(-1).cpu() for t in ts])


def test_one_step_same_gradients_as_torch_and_fresh_forward(pieces):
    """Accumulation 2 and an active clip: FlatAdamW and torch's AdamW receive bitwise-equal gradients;
    both updates against the fp64 update of those gradients; then the stepped model's forward equals
    that of a freshly built model loaded from its state_dict (no stale weight cache)."""
    from gnn.optim import FlatAdamW
    p, bs = pieces
    ma, mb = _module(p), _module(p)
    ps_a, ps_b = list(ma.parameters()), list(mb.parameters())
    assert all(torch.equal(x, y) for x, y in zip(ps_a, ps_b))
    with torch.no_grad():
        warm = ma.model(bs[0])["stiffness"]                             # fills the packed-weight caches
    oa = FlatAdamW.from_torch(ma.configure_optimizers(), max_norm=1.0)
    ob = mb.configure_optimizers()
    assert oa.fused and oa.param_groups[0]["amsgrad"]
    p0 = _flat_of(ps_a)
    for b in bs:
        (ma.training_step(b) * 0.5).backward()
        (mb.training_step(b) * 0.5).backward()
    ga, gb = _flat_of([q.grad for q in ps_a]), _flat_of([q.grad for q in ps_b])
    assert torch.equal(ga, gb)
    norm = float(ga.double().norm())
    max_norm = 0.5 * norm                                                  # the clip is active
    oa.max_norm = max_norm
    oa.step()
    torch.nn.utils.clip_grad_norm_(ps_b, max_norm)
    ob.step()
    hp = dict(lr=p.lr, betas=(p.beta1, 0.999), eps=p.epsilon, weight_decay=p.weight_decay)
    ref = reference64(p0, ga[None], True, max_norm, **hp)[0]
    st = oa.read_state()
    assert st["step"] == 1 and st["skipped"] == 0 and st["clip_coef"] == pytest.approx(0.5, rel=1e-5)
    assert st["grad_norm"] == pytest.approx(norm, rel=1e-6)
    got = dict(p=_flat_of(ps_a), m=_flat_of([oa.state[q]["exp_avg"] for q in ps_a]),
               v=_flat_of([oa.state[q]["exp_avg_sq"] for q in ps_a]),
               vmax=_flat_of([oa.state[q]["max_exp_avg_sq"] for q in ps_a]))
    base = dict(p=_flat_of(ps_b), m=_flat_of([ob.state[q]["exp_avg"] for q in ps_b]),
                v=_flat_of([ob.state[q]["exp_avg_sq"] for q in ps_b]),
                vmax=_flat_of([ob.state[q]["max_exp_avg_sq"] for q in ps_b]))
    assert_bounded(errors(got, ref, p.lr, True), errors(base, ref, p.lr, True), floors([ref], p.lr), "model step")
    # stale-cache test
    from gnn import EnergyEquivGNN
    with torch.no_grad():
        stepped = ma.model(bs[0])["stiffness"]
        torch.manual_seed(77)
        fresh = EnergyEquivGNN(p)
        fresh.load_state_dict({k: v.detach().cpu() for k, v in ma.model.state_dict().items()})
        fresh = fresh.to(DEV)
        assert torch.equal(stepped, fresh(bs[0])["stiffness"])
    assert not torch.equal(stepped, warm)


def _hand_loop(p, bs, steps, acc, clip, fused_loss):
    from gnn.optim import FlatAdamW
    m = _module(p, fused_loss=fused_loss)
    m.loss_grad_scale = 1.0 / acc
    opt = FlatAdamW.from_torch(m.configure_optimizers(), max_norm=clip)
    k = 0
    for _ in range(steps):
        for _ in range(acc):
            loss = m.training_step(bs[k % len(bs)], k % len(bs))
            (loss if fused_loss else loss * (1.0 / acc)).backward()
            k += 1
        opt.step()
    return m, opt


@pytest.mark.parametrize("fused_loss", [False, True])
def test_trainer_schedule_equals_a_hand_written_loop_and_resumes_bitwise(pieces, tmp_path, fused_loss):
    """Four Trainer optimizer steps (accumulation 2, clip 10) = the hand-written loop over the same
    pieces, bitwise; and 2 steps + save + resume + 2 steps = the same."""
    from gnn.trainer import Trainer
    p, bs = pieces
    hand, hopt = _hand_loop(p, bs, 4, 2, 10.0, fused_loss)
    kw = dict(accumulate_grad_batches=2, gradient_clip_val=10.0, log_every_n_steps=50, fused_optimizer=True)
    m = _module(p, fused_loss=fused_loss)
    tr = Trainer(max_steps=4, **kw)
    tr.fit(m, bs)
    assert tr.global_step == 4 and tr.optimizer.read_state()["step"] == 4
    assert len(tr.logged) == 8 and all(e["loss"] == e["loss"] for e in tr.logged)
    if fused_loss:
        assert all(e["stiffness_loss"] == e["stiffness_loss"] for e in tr.logged)
    for (k, a), b in zip(hand.state_dict().items(), m.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(hopt.flat_m, tr.optimizer.flat_m) and torch.equal(hopt.flat_vmax, tr.optimizer.flat_vmax)
    first = _module(p, fused_loss=fused_loss)
    t1 = Trainer(max_steps=2, **kw)
    t1.fit(first, bs)
    path = str(tmp_path / "mid.ckpt")
    t1.save_checkpoint(path)
    second = _module(p, seed=5, fused_loss=fused_loss)
    t2 = Trainer(max_steps=4, **kw)
    t2.fit(second, bs, ckpt_path=path)
    assert t2.global_step == 4
    for (k, a), b in zip(m.state_dict().items(), second.state_dict().values()):
        assert torch.equal(a, b), k
    for name in ("flat_m", "flat_v", "flat_vmax"):
        assert torch.equal(getattr(tr.optimizer, name), getattr(t2.optimizer, name)), name


class _SyncGuard:
    """no synchronising call between the end of batch ``start`` and the end of batch ``stop``"""

    def __init__(self, start, stop):
        self.start, self.stop, self.guarded = start, stop, 0

    def on_train_batch_end(self, trainer, module, outputs, batch, batch_idx):
        if trainer._batches_seen == self.start:
            torch.cuda.set_sync_debug_mode("error")
        elif trainer._batches_seen == self.stop:
            torch.cuda.set_sync_debug_mode(0)
        if self.start < trainer._batches_seen <= self.stop:
            self.guarded += 1

    def on_validation_end(self, trainer, module):
        pass

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        pass


@pytest.mark.parametrize("fused_loss", [False, True])
def test_three_trainer_steps_after_warm_up_do_not_synchronise(pieces, fused_loss):
    from gnn.trainer import Trainer
    p, bs = pieces
    m = _module(p, fused_loss=fused_loss)
    guard = _SyncGuard(4, 10)                     # 2 warm-up steps, then 3 steps of 2 batches
    tr = Trainer(max_steps=5, accumulate_grad_batches=2, gradient_clip_val=10.0, log_every_n_steps=50,
                 callbacks=[guard], fused_optimizer=True)
    try:
        tr.fit(m, bs)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert guard.guarded == 6 and tr.global_step == 5 and len(tr.logged) == 10
