"""Second-order smoothness on the GPU: the two kernels of csrc/kernels/smooth2.hip under the per-element fp64
checks of _smooth2_refs.py, their add-into mode, their builders' host checks, the autograd function with
``smooth_order=2`` (composition, launches, no host synchronisation) and the fused trainer with
``unsup_smooth_order=2``."""
import math

import pytest
import torch

import _smooth2_refs as S
import _unsup_refs as R
from _train_refs import bits_equal
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import smooth2_sums, unsup_loss, unsup_loss_reference
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train.trainer import TrainConfig, Trainer

pytestmark = pytest.mark.gpu


def _d(t):
    return None if t is None else t.cuda()


class Kernels:
    """The ops themselves, outputs pre-filled with NaN so that unwritten elements show."""

    def smooth2_loss(self, pred, img1, prm):
        N, B, H, W, _ = pred.shape
        part = torch.full((nat.smooth2_loss_blocks(B * H * W), N, 4), float("nan"), device="cuda")
        nat.ops().smooth2_loss([_d(pred), _d(img1), torch.tensor(prm, device="cuda"), part], [B, H, W, N])
        return part.cpu()

    def smooth2_loss_bwd(self, pred, img1, prm, scale):
        N, B, H, W, _ = pred.shape
        grad = torch.full(pred.shape, float("nan"), device="cuda")
        nat.ops().smooth2_loss_bwd([_d(pred), _d(img1), torch.tensor(prm, device="cuda"), _d(scale), grad], [B, H, W, N, 0])
        return grad.cpu()


@pytest.mark.parametrize("case", S.CASES, ids=str)
def test_kernels_against_the_fp64_reference(case):
    """Every case: the sums and every gradient element under the derived tolerances, outputs pre-filled with NaN, two
    runs bitwise equal; the NaN case: that iteration's sums and the triples that touch the pixel, nothing else."""
    S.check_partials(Kernels(), case)
    S.check_grad(Kernels(), case)


@pytest.mark.parametrize("case", [(3, 2, 13, 37, False), (12, 2, 40, 72, True)], ids=str)
def test_add_into_equals_write_then_add(case):
    c = S.inputs(case)
    pred, img1, scale = c.pred.cuda(), c.img1.cuda(), c.scale.cuda()
    base = torch.randn(c.pred.shape, generator=torch.Generator().manual_seed(3)).cuda()
    written = nat.smooth2_loss_grad(pred, img1, scale, S.EPS_S, S.KAPPA)
    out = base.clone()
    assert nat.smooth2_loss_grad(pred, img1, scale, S.EPS_S, S.KAPPA, out=out) is out
    assert bits_equal(out, base + written)
    assert bits_equal(written.cpu(), Kernels().smooth2_loss_bwd(c.pred, c.img1, S.PRM, c.scale))
    # the front end's partials are the op's
    assert bits_equal(nat.smooth2_loss_partials(pred, img1, S.EPS_S, S.KAPPA).cpu(), Kernels().smooth2_loss(c.pred, c.img1, S.PRM))


def test_builders_host_checks():
    N, B, H, W = 2, 1, 6, 10
    P = B * H * W
    dev = "cuda"
    pred, img = torch.zeros(N, B, H, W, 2, device=dev), torch.zeros(B, H, W, 3, device=dev)
    prm, scale = torch.tensor(S.PRM, device=dev), torch.ones(N, device=dev)
    part = torch.zeros(nat.smooth2_loss_blocks(P), N, 4, device=dev)
    grad = torch.zeros_like(pred)
    odd = torch.zeros(2 * N * P + 1, device=dev)[1:]                 # 4-byte aligned only
    wide = torch.zeros(N, B, H, 2 * W, 2, device=dev)[:, :, :, :W]   # not contiguous
    for op, good, ints, bad, bad_ints in (
        ("smooth2_loss", [pred, img, prm, part], [B, H, W, N],
         [(0, pred.double()), (0, pred[:1]), (0, odd), (0, wide), (0, pred.cpu()), (0, None), (1, img[:, :5]), (1, img.half()),
          (1, None), (2, prm[:3]), (2, None), (3, part[:, :1]), (3, part.double()), (3, None), (3, pred.view(-1)[:part.numel()])],
         ([B, H, W, 0], [B, H, W, 33], [0, H, W, N], [1 << 12, 1 << 10, 1 << 9, N])),
        ("smooth2_loss_bwd", [pred, img, prm, scale, grad], [B, H, W, N, 0],
         [(0, pred.double()), (0, odd), (1, img[:, :5]), (2, prm[:3]), (3, scale[:1]), (3, scale.double()), (3, None),
          (4, grad[:1]), (4, grad.double()), (4, None), (4, pred), (4, odd)],
         ([B, H, W, 0, 0], [B, H, W, 33, 0], [0, H, W, N, 0], [B, H, W, N, 2], [B, H, W, N, -1])),
    ):
        fn = getattr(nat.ops(), op)
        for k, t in bad:
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good[:k] + [t] + good[k + 1:], ints)
        for b in bad_ints:
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good, list(b))
        fn(good, ints)                                               # and the good call runs
    torch.cuda.synchronize()
    # the front ends refuse before anything is launched
    launched = []
    real = nat.ops
    try:
        nat.ops = lambda: launched.append(1) or real()
        for bad in ((pred.double(), img), (torch.zeros(33, B, H, W, 2, device=dev), img), (odd.view(N, B, H, W, 2), img),
                    (wide, img), (pred, img.double()), (pred, img.cpu()), (pred, img[:, :5]),
                    (pred, torch.zeros(B, H, 2 * W, 3, device=dev)[:, :, :W])):
            with pytest.raises(ValueError, match="smooth2_loss:"):
                nat.smooth2_loss_partials(*bad)
            with pytest.raises(ValueError, match="smooth2_loss_bwd:"):
                nat.smooth2_loss_grad(*bad, scale)
        for kw in (dict(scale=scale[:1]), dict(scale=scale.double()), dict(scale=scale.cpu()),
                   dict(scale=torch.ones(N, 2, device=dev)), dict(scale=scale, out=grad[:1]), dict(scale=scale, out=grad.double()),
                   dict(scale=scale, out=odd.view(N, B, H, W, 2)), dict(scale=scale, prm=prm[:3]),
                   dict(scale=scale, prm=prm.cpu())):
            with pytest.raises(ValueError, match="smooth2_loss_bwd:"):
                nat.smooth2_loss_grad(pred, img, **kw)
        assert not launched
    finally:
        nat.ops = real


def _case():
    c = R.unsup_inputs((3, 2, 13, 37, False), True)
    return c, c.pred.cuda(), c.img1.cuda(), c.img2.cuda(), _d(c.mask)


class _Recorder:
    """``nat.ops()`` with the name of every op that is looked up recorded."""

    def __init__(self, real, names):
        self._real, self._names = real, names

    def __getattr__(self, name):
        self._names.append(name)
        return getattr(self._real, name)


@pytest.mark.parametrize("photo", ["charbonnier", "census"])
def test_autograd_function(photo, monkeypatch):
    c, pred, i1, i2, mask = _case()
    prm = (0.01, 0.001, 10.0, 0.4)
    kw = dict(gamma=0.7, eps=prm[0], eps_s=prm[1], edge_kappa=prm[2], smooth_weight=0.08, out_penalty=prm[3], photo=photo,
              smooth_order=2)
    names = []
    real = nat.ops
    monkeypatch.setattr(nat, "ops", lambda: _Recorder(real(), names))
    f = pred.clone().requires_grad_(True)
    loss, mets = unsup_loss(f, i1, i2, mask, **kw)
    (3.0 * loss).backward()
    monkeypatch.undo()
    # the launches: with the census term the two kernels of unsup.hip would carry nothing and are not issued
    if photo == "census":
        assert names == ["smooth2_loss", "census_gray", "census_loss", "census_loss_bwd", "smooth2_loss_bwd"]
        assert not [n for n in names if n.startswith("unsup_loss")]
    else:
        assert names == ["unsup_loss", "smooth2_loss", "unsup_loss_bwd", "smooth2_loss_bwd"]
    # the loss is the value assembled from the partials, the gradient the ops' with the stated scales
    s2 = nat.smooth2_loss_partials(pred, i1, prm[1], prm[2]).double().sum(0)
    sm = s2[:, 0] + s2[:, 1]
    w = 0.7 ** torch.arange(c.N - 1, -1, -1, dtype=torch.float64, device="cuda")
    zero = torch.zeros_like(w)
    if photo == "census":
        part, coef = nat.census_loss_partials(pred, i1, i2, mask, prm[3])
        col = part.double().sum(0)[:, 0]
    else:
        col = nat.unsup_loss_partials(pred, i1, i2, mask, *prm).double().sum(0)[:, 0]
    want = (w * (col / c.P + 0.08 * (sm / (2.0 * c.P)))).sum().float()
    assert bits_equal(loss.detach(), want)
    # gl w_i / P for the photometric term, a zero first-order scale, gl w_i smooth_weight / (2P) for smooth2; gl = 3
    if photo == "census":
        grad = nat.census_loss_grad(pred, i1, i2, mask, (w / c.P * 3.0).float(), prm[3], coef=coef)
    else:
        grad = nat.unsup_loss_grad(pred, i1, i2, mask, (torch.stack([w / c.P, zero], -1) * 3.0).float(), *prm)
    nat.smooth2_loss_grad(pred, i1, (w * (0.08 / (2.0 * c.P)) * 3.0).float(), prm[1], prm[2], out=grad)
    assert bits_equal(f.grad, grad)
    # ... and the golden op's, loosely (the kernels' own accuracy: test_kernels_against_the_fp64_reference)
    g = c.pred.clone().requires_grad_(True)
    gl, gm = unsup_loss_reference(g, c.img1, c.img2, c.mask, **kw)
    (3.0 * gl).backward()
    assert torch.allclose(loss.cpu(), gl.detach(), rtol=1e-5)
    assert torch.allclose(f.grad.cpu(), g.grad, rtol=1e-2, atol=1e-4 * float(g.grad.abs().max()))
    for k in ("photo", "smooth", "inside"):
        assert torch.allclose(mets[k].cpu(), gm[k], rtol=1e-5), k
    assert set(mets) == {"photo", "smooth", "inside"} and not mets["photo"].requires_grad
    # two identical calls are bitwise equal
    f2 = pred.clone().requires_grad_(True)
    loss2, _ = unsup_loss(f2, i1, i2, mask, **kw)
    (3.0 * loss2).backward()
    assert bits_equal(loss2.detach(), loss.detach()) and bits_equal(f2.grad, f.grad)
    # smooth_order=1 is the call without the argument
    outs = []
    base = {k: v for k, v in kw.items() if k != "smooth_order"}
    for extra in ({}, {"smooth_order": 1}):
        f1 = pred.clone().requires_grad_(True)
        l1, m1 = unsup_loss(f1, i1, i2, mask, **base, **extra)
        l1.backward()
        outs.append((l1.detach(), f1.grad, m1["smooth"]))
    assert all(bits_equal(a, b) for a, b in zip(*outs)) and not torch.equal(outs[0][0], loss.detach())
    # N > 32 runs the golden op on the device; the golden sums on the device agree with the kernel's
    many = torch.zeros(33, 1, 8, 9, 2, device="cuda")
    img = torch.rand(1, 8, 9, 3, device="cuda")
    a, _ = unsup_loss(many, img, img, photo=photo, smooth_order=2)
    b, _ = unsup_loss_reference(many.cpu(), img.cpu(), img.cpu(), photo=photo, smooth_order=2)
    assert torch.allclose(a.cpu(), b, rtol=1e-5)
    assert torch.allclose(smooth2_sums(pred, i1, prm[1], prm[2]).double(), s2[:, :2], rtol=1e-4)


@pytest.mark.parametrize("photo", ["charbonnier", "census"])
def test_no_host_synchronisation_between_forward_and_backward(photo):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    _, pred, i1, i2, mask = _case()
    f = pred.clone().requires_grad_(True)
    kw = dict(photo=photo, smooth_order=2)
    unsup_loss(f, i1, i2, mask, **kw)[0].backward()     # warm: the library, the parameter tensor, allocator blocks
    unsup_loss(f, i1, i2, None, **kw)[0].backward()
    f.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, mets = unsup_loss(f, i1, i2, mask, **kw)
        loss.backward()
        loss2, _ = unsup_loss(f, i1, i2, None, **kw)
        loss2.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and math.isfinite(float(loss2.detach())) and bool(torch.isfinite(f.grad).all())


# ------------------------------------------------------------------ fused trainer
KW = dict(arch="raft_small", steps=2, batch=2, iters=3, size=(128, 160), log_every=100, lr=2e-4)


def _params(tr):
    tr.flush()
    return [p.detach().clone() for p in tr.model.parameters()]


def test_fused_trainer_second_order(monkeypatch):
    seen = []
    real = T.unsup_loss

    def spy(preds, *a, **k):
        loss, mets = real(preds, *a, **k)
        seen.append((preds.detach().clone(), loss.detach().clone(), k))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy)
    tr = Trainer(TrainConfig(loss="unsup", unsup_smooth_order=2, **KW))
    assert tr.device.type == "cuda"
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(2)]
    outs = [tr.train_step(b) for b in batches]
    after = _params(tr)
    assert tr.skipped == 0 and all(math.isfinite(float(o["loss"])) for o in outs)
    assert set(outs[0]) == {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px"}
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # the step-1 loss is the second-order loss of that step's own predictions
    preds, loss, k = seen[0]
    assert k == {"smooth_order": 2}
    cfg = tr.cfg
    again, _ = real(preds, batches[0][0], batches[0][1], None, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s,
                    cfg.unsup_edge_kappa, cfg.unsup_smooth_weight, cfg.unsup_out_penalty, smooth_order=2)
    assert bits_equal(again, loss) and bits_equal(outs[0]["loss"], loss)
    gold, _ = unsup_loss_reference(preds.cpu(), batches[0][0].cpu(), batches[0][1].cpu(), smooth_order=2)
    assert torch.allclose(loss.cpu(), gold, rtol=1e-4)
    first, _ = real(preds, batches[0][0], batches[0][1], None)
    assert not torch.equal(first, loss)
    # the labels take no part in the gradient
    monkeypatch.setattr(T, "unsup_loss", real)
    other = Trainer(TrainConfig(loss="unsup", unsup_smooth_order=2, **KW))
    for i1, i2, flow, valid in batches:
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(a, b) for a, b in zip(after, _params(other)))


def test_fused_trainer_second_order_drops_a_nan_prediction(monkeypatch):
    real = T.unsup_loss
    calls = []

    def poisoned(preds, *a, **k):
        calls.append(1)
        if len(calls) == 2:                             # step 2: one NaN in a middle iteration's prediction
            bad = torch.ones_like(preds)
            bad[1, 0, 40, 50, 0] = float("nan")
            preds = preds * bad
        return real(preds, *a, **k)

    monkeypatch.setattr(T, "unsup_loss", poisoned)
    tr = Trainer(TrainConfig(loss="unsup", unsup_smooth_order=2, **KW))
    tr.train_step(tr.batch_for(0))
    w1 = _params(tr)
    m = tr.train_step(tr.batch_for(1))
    assert not math.isfinite(float(m["loss"])) and not math.isfinite(float(m["grad_norm"]))
    tr.flush()
    assert tr.skipped == 1 and all(torch.equal(a, b) for a, b in zip(w1, _params(tr)))
    assert tr.step == 2 and all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_fused_trainer_first_order_equals_the_run_without_the_field():
    runs = []
    for kw in ({}, {"unsup_smooth_order": 1}):
        tr = Trainer(TrainConfig(loss="unsup", **KW, **kw))
        losses = [tr.train_step(tr.batch_for(s))["loss"] for s in range(2)]
        runs.append((losses, _params(tr)))
    assert all(bits_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
