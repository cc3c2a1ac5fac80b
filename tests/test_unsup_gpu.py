"""Label-free training on the GPU: the two kernels of csrc/kernels/unsup.hip under the per-element
fp64 checks of _unsup_refs.py, their builders' host checks, the autograd function (gradient,
assembled loss, no host synchronisation) and the fused trainer with ``loss="unsup"``."""
import math

import pytest
import torch

import _unsup_refs as R
from _train_refs import bits_equal
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import unsup_loss, unsup_loss_reference
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train.trainer import TrainConfig, Trainer

pytestmark = pytest.mark.gpu


def _d(t):
    return None if t is None else t.cuda()


class Kernels:
    """The ops themselves, outputs pre-filled with NaN so that unwritten elements show."""

    def unsup_loss(self, pred, img1, img2, mask, prm):
        N, B, H, W, _ = pred.shape
        part = torch.full((nat.unsup_loss_blocks(B * H * W), N, 4), float("nan"), device="cuda")
        nat.ops().unsup_loss([_d(pred), _d(img1), _d(img2), _d(mask), torch.tensor(prm, device="cuda"), part], [B, H, W, N])
        return part.cpu()

    def unsup_loss_bwd(self, pred, img1, img2, mask, prm, scale):
        N, B, H, W, _ = pred.shape
        grad = torch.full(pred.shape, float("nan"), device="cuda")
        nat.ops().unsup_loss_bwd([_d(pred), _d(img1), _d(img2), _d(mask), torch.tensor(prm, device="cuda"), _d(scale), grad],
                                 [B, H, W, N])
        return grad.cpu()


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("case", R.UNSUP_CASES, ids=str)
def test_kernels_against_the_fp64_reference(case, with_mask):
    R.check_unsup_loss(Kernels(), case, with_mask)
    R.check_unsup_loss_bwd(Kernels(), case, with_mask)


def test_builders_host_checks():
    N, B, H, W = 2, 1, 6, 10
    P = B * H * W
    dev = "cuda"
    pred, img = torch.zeros(N, B, H, W, 2, device=dev), torch.zeros(B, H, W, 3, device=dev)
    mask, prm, scale = torch.ones(B, H, W, device=dev), torch.tensor(R.PRM, device=dev), torch.ones(N, 2, device=dev)
    part = torch.zeros(nat.unsup_loss_blocks(P), N, 4, device=dev)
    grad = torch.zeros_like(pred)
    ints = [B, H, W, N]
    fwd, bwd = [pred, img, img.clone(), mask, prm, part], [pred, img, img.clone(), mask, prm, scale, grad]
    odd = torch.zeros(2 * N * P + 1, device=dev)[1:]                 # 4-byte aligned only
    wide = torch.zeros(N, B, H, 2 * W, 2, device=dev)[:, :, :, :W]   # not contiguous
    for op, good, bad in (
        ("unsup_loss", fwd, [(0, pred.double()), (0, pred[:1]), (0, odd), (0, wide), (0, pred.cpu()), (1, img[:, :5]),
                             (2, img.half()), (2, None), (3, mask.bool()), (3, mask[:, :5]), (4, prm[:3]), (4, None),
                             (5, part[:, :1]), (5, part.double()), (5, None), (5, pred.view(-1)[:part.numel()])]),
        ("unsup_loss_bwd", bwd, [(0, pred.double()), (1, img[:, :5]), (3, mask.bool()), (4, prm[:3]), (5, scale[:1]),
                                 (5, scale.double()), (5, None), (6, grad[:1]), (6, grad.double()), (6, None), (6, pred)]),
    ):
        fn = getattr(nat.ops(), op)
        for k, t in bad:
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good[:k] + [t] + good[k + 1:], ints)
        for bad_ints in ([B, H, W, 0], [B, H, W, 33], [0, H, W, N], [1 << 12, 1 << 10, 1 << 9, N]):
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good, bad_ints)
        fn(good, ints)                                               # and the good call runs
    torch.cuda.synchronize()
    # the front ends refuse before anything is launched
    with pytest.raises(ValueError, match="unsup_loss"):
        nat.unsup_loss_partials(pred.double(), img, img)
    with pytest.raises(ValueError, match="unsup_loss"):
        nat.unsup_loss_partials(torch.zeros(33, B, H, W, 2, device=dev), img, img)


def _case(with_mask=True):
    c = R.unsup_inputs((3, 2, 13, 37, False), with_mask)
    return c, c.pred.cuda(), c.img1.cuda(), c.img2.cuda(), _d(c.mask)


def test_autograd_function():
    c, pred, i1, i2, mask = _case()
    kw = dict(gamma=0.7, eps=R.PRM[0], eps_s=R.PRM[1], edge_kappa=R.PRM[2], smooth_weight=0.08, out_penalty=R.PRM[3])
    f = pred.clone().requires_grad_(True)
    loss, mets = unsup_loss(f, i1, i2, mask, **kw)
    (3.0 * loss).backward()
    # the loss is the value assembled from the partials, the gradient the op's with the stated scales
    s = nat.unsup_loss_partials(pred, i1, i2, mask, *R.PRM).double().sum(0)
    w = 0.7 ** torch.arange(c.N - 1, -1, -1, dtype=torch.float64, device="cuda")
    want = (w * (s[:, 0] / c.P + 0.08 * (s[:, 1] / (2.0 * c.P)))).sum().float()
    assert bits_equal(loss.detach(), want)
    # gl w_i / P and gl w_i smooth_weight / (2P), gl = 3
    scale = (torch.stack([w / c.P, w * (0.08 / (2.0 * c.P))], -1) * 3.0).float()
    assert bits_equal(f.grad, nat.unsup_loss_grad(pred, i1, i2, mask, scale, *R.PRM))
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
    # N > 32 runs the golden op on the device
    many = torch.zeros(33, 1, 4, 6, 2, device="cuda")
    img = torch.rand(1, 4, 6, 3, device="cuda")
    a, _ = unsup_loss(many, img, img)
    b, _ = unsup_loss_reference(many.cpu(), img.cpu(), img.cpu())
    assert torch.allclose(a.cpu(), b, rtol=1e-5)


def test_no_host_synchronisation_between_forward_and_backward():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    _, pred, i1, i2, mask = _case()
    f = pred.clone().requires_grad_(True)
    unsup_loss(f, i1, i2, mask)[0].backward()          # warm: the library, the parameter tensor, allocator blocks
    unsup_loss(f, i1, i2, None)[0].backward()
    f.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, mets = unsup_loss(f, i1, i2, mask)
        loss.backward()
        loss2, _ = unsup_loss(f, i1, i2, None)
        loss2.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and math.isfinite(float(loss2.detach())) and bool(torch.isfinite(f.grad).all())


# ------------------------------------------------------------------ fused trainer
KW = dict(arch="raft_small", steps=3, batch=2, iters=3, size=(128, 160), log_every=100, lr=2e-4)


def _params(tr):
    tr.flush()
    return [p.detach().clone() for p in tr.model.parameters()]


def test_fused_trainer_unsup(monkeypatch):
    seen = []
    real = T.unsup_loss

    def spy(preds, *a, **k):
        loss, mets = real(preds, *a, **k)
        seen.append((preds.detach().clone(), loss.detach().clone()))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy)
    tr = Trainer(TrainConfig(loss="unsup", **KW))
    assert tr.device.type == "cuda"
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(3)]
    outs = [tr.train_step(b) for b in batches]
    after = _params(tr)
    assert tr.skipped == 0 and all(math.isfinite(float(o["loss"])) for o in outs)
    assert set(outs[0]) == {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px"}
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # the step-1 loss is unsup_loss of that step's own predictions
    preds, loss = seen[0]
    cfg = tr.cfg
    again, _ = real(preds, batches[0][0], batches[0][1], None, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s,
                    cfg.unsup_edge_kappa, cfg.unsup_smooth_weight, cfg.unsup_out_penalty)
    assert bits_equal(again, loss) and bits_equal(outs[0]["loss"], loss)
    gold, _ = unsup_loss_reference(preds.cpu(), batches[0][0].cpu(), batches[0][1].cpu())
    assert torch.allclose(loss.cpu(), gold, rtol=1e-4)
    # the labels take no part in the gradient
    monkeypatch.setattr(T, "unsup_loss", real)
    other = Trainer(TrainConfig(loss="unsup", **KW))
    for i1, i2, flow, valid in batches:
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(a, b) for a, b in zip(after, _params(other)))


def test_fused_trainer_unsup_drops_a_nan_prediction(monkeypatch):
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
    tr = Trainer(TrainConfig(loss="unsup", **KW))
    tr.train_step(tr.batch_for(0))
    w1 = _params(tr)
    m = tr.train_step(tr.batch_for(1))
    assert not math.isfinite(float(m["loss"])) and not math.isfinite(float(m["grad_norm"]))
    tr.flush()
    assert tr.skipped == 1 and all(torch.equal(a, b) for a, b in zip(w1, _params(tr)))
    tr.train_step(tr.batch_for(2))
    tr.flush()
    assert tr.step == 3 and tr.skipped == 1 and all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_fused_trainer_defaults_equal_explicit_sequence():
    runs = []
    for kw in ({}, {"loss": "sequence"}):
        tr = Trainer(TrainConfig(**KW, **kw))
        losses = [tr.train_step(tr.batch_for(s))["loss"] for s in range(3)]
        runs.append((losses, _params(tr)))
    assert all(bits_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
