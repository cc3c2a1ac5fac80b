"""The census photometric term on the GPU: the kernels of csrc/kernels/census.hip under the
per-element fp64 checks of _census_refs.py, their builders' host checks, the autograd function
(gradient, assembled loss, no host synchronisation) and the fused trainer with
``unsup_photo="census"``."""
import math

import pytest
import torch

import _census_refs as CR
from _train_refs import bits_equal
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import census_sums, unsup_loss, unsup_loss_reference
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train.trainer import TrainConfig, Trainer

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _d(t):
    return None if t is None else t.cuda()


def _prm(pen):
    return torch.tensor([0.01, 0.001, 10.0, pen], device="cuda")


class Kernels:
    """The ops themselves, outputs pre-filled with NaN so that unwritten elements show."""

    @staticmethod
    def gray(img1, img2):
        B, H, W, _ = img1.shape
        gray = torch.full((2, B, H, W), NAN, device="cuda")
        nat.ops().census_gray([_d(img1), _d(img2), gray], [B, H, W])
        return gray

    def _forward(self, pred, img1, img2, mask, pen):
        N, B, H, W, _ = pred.shape
        gray = self.gray(img1, img2)
        part = torch.full((nat.census_tiles(B, H, W), N, 4), NAN, device="cuda")
        coef = torch.full((N, B, H, W), NAN, device="cuda")
        nat.ops().census_loss([_d(pred), gray, _d(mask), _prm(pen), part, coef], [B, H, W, N])
        return gray, part, coef

    def census_loss(self, pred, img1, img2, mask, pen):
        gray, part, coef = self._forward(pred, img1, img2, mask, pen)
        assert bool(torch.isfinite(gray).all())
        return part.cpu(), coef.cpu()

    def census_loss_bwd(self, pred, img1, img2, mask, pen, scale):
        N, B, H, W, _ = pred.shape
        gray, _, coef = self._forward(pred, img1, img2, mask, pen)
        grad = torch.full(pred.shape, NAN, device="cuda")
        nat.ops().census_loss_bwd([_d(pred), gray, coef, _d(scale), grad], [B, H, W, N, 0])
        # add = 1 adds exactly that gradient to what the tensor holds
        base = torch.randn(pred.shape, generator=torch.Generator().manual_seed(1)).cuda()
        both = base.clone()
        nat.ops().census_loss_bwd([_d(pred), gray, coef, _d(scale), both], [B, H, W, N, 1])
        assert bits_equal(both, grad + base)
        return grad.cpu()


def test_tile_constants():
    assert (nat.CENSUS_TILE, nat.CENSUS_ITERS) == (CR.CENSUS_TILE, CR.CENSUS_ITERS)
    tx, ty = nat.CENSUS_TILE
    N, B, H, W, _ = CR.TILE_CASE
    assert H // ty >= 3 and H % ty and W // tx >= 3 and W % tx and N > nat.CENSUS_ITERS and N % nat.CENSUS_ITERS


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("case", CR.CENSUS_CASES, ids=str)
def test_kernels_against_the_fp64_reference(case, with_mask):
    ref = CR.census_ref(case, with_mask)
    N, B, H, W, _ = case
    if H > 2 * CR.R and W > 2 * CR.R:                       # the clamp path is exercised (a CPU check)
        assert any(ref.clamp_seen)
    CR.check_census_loss(Kernels(), case, with_mask)
    CR.check_census_loss_bwd(Kernels(), case, with_mask)


def test_gray_planes():
    c = CR.census_inputs((3, 2, 13, 37, False), False)
    gray = Kernels.gray(c.img1, c.img2).cpu().double()
    for k, img in enumerate((c.img1, c.img2)):
        g, gB = CR.gray64(img)
        assert bool(((gray[k] - g).abs() <= CR.U_ACC * gB).all())
    assert bits_equal(nat.census_gray_planes(c.img1.cuda(), c.img2.cuda()).cpu(), gray.float())


def test_builders_host_checks():
    N, B, H, W = 2, 1, 9, 10
    P = B * H * W
    dev = "cuda"
    pred, img = torch.zeros(N, B, H, W, 2, device=dev), torch.zeros(B, H, W, 3, device=dev)
    gray, mask, prm = torch.zeros(2, B, H, W, device=dev), torch.ones(B, H, W, device=dev), _prm(0.5)
    part, coef = torch.zeros(nat.census_tiles(B, H, W), N, 4, device=dev), torch.zeros(N, B, H, W, device=dev)
    scale, grad = torch.ones(N, device=dev), torch.zeros_like(pred)
    odd = torch.zeros(2 * N * P + 1, device=dev)[1:]                 # 4-byte aligned only
    wide = torch.zeros(N, B, H, 2 * W, 2, device=dev)[:, :, :, :W]   # not contiguous
    for op, good, ints, bad, bad_ints in (
        ("census_gray", [img, img.clone(), gray], [B, H, W],
         [(0, img.double()), (0, img[:, :5]), (0, img.cpu()), (1, None), (1, img.half()), (2, gray[:1]), (2, gray.double()),
          (2, None), (2, img.view(-1)[:2 * P])],
         ([0, H, W], [B, 0, W], [1 << 12, 1 << 10, 1 << 9])),
        ("census_loss", [pred, gray, mask, prm, part, coef], [B, H, W, N],
         [(0, pred.double()), (0, pred[:1]), (0, odd), (0, wide), (0, pred.cpu()), (1, gray[:1]), (1, None), (2, mask.bool()),
          (2, mask[:, :5]), (3, prm[:3]), (3, None), (4, part[:, :1]), (4, part.double()), (4, None),
          (4, pred.view(-1)[:part.numel()]), (5, coef[:1]), (5, None), (5, gray.view(-1)[:N * P])],
         ([B, H, W, 0], [B, H, W, 33], [0, H, W, N], [1 << 12, 1 << 10, 1 << 9, N])),
        ("census_loss_bwd", [pred, gray, coef, scale, grad], [B, H, W, N, 0],
         [(0, pred.double()), (0, odd), (1, gray[:1]), (2, coef[:1]), (2, None), (3, scale[:1]), (3, scale.double()), (3, None),
          (4, grad[:1]), (4, grad.double()), (4, None), (4, pred)],
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
    with pytest.raises(ValueError, match="census_gray"):
        nat.census_loss_partials(pred, img.double(), img)
    with pytest.raises(ValueError, match="census_loss"):
        nat.census_loss_partials(pred.double(), img, img)
    with pytest.raises(ValueError, match="census_loss"):
        nat.census_loss_partials(torch.zeros(33, B, H, W, 2, device=dev), img, img)
    with pytest.raises(ValueError, match="census_loss"):
        nat.census_loss_partials(odd.view(N, B, H, W, 2), img, img)
    with pytest.raises(ValueError, match="census_loss"):
        nat.census_loss_partials(wide, img, img)
    with pytest.raises(ValueError, match="census_loss"):
        nat.census_loss_partials(pred, img, img, gray=gray[:1])
    with pytest.raises(ValueError, match="census_gray"):
        nat.census_gray_planes(img.double(), img.double())
    with pytest.raises(ValueError, match="census_gray"):
        nat.census_gray_planes(img, img.cpu())
    for kw in (dict(scale=scale[:1]), dict(scale=scale.double()), dict(scale=scale, coef=coef[:1]), dict(scale=scale, out=grad[:1]),
               dict(scale=scale.cpu())):
        with pytest.raises(ValueError, match="census_loss_bwd"):
            nat.census_loss_grad(pred, img, img, None, **kw)


def _case(with_mask=True):
    c = CR.census_inputs((3, 2, 13, 37, False), with_mask)
    return c, c.pred.cuda(), c.img1.cuda(), c.img2.cuda(), _d(c.mask)


def test_autograd_function():
    c, pred, i1, i2, mask = _case()
    prm = (0.01, 0.001, 10.0, 0.4)
    kw = dict(gamma=0.7, eps=prm[0], eps_s=prm[1], edge_kappa=prm[2], smooth_weight=0.08, out_penalty=prm[3], photo="census")
    f = pred.clone().requires_grad_(True)
    loss, mets = unsup_loss(f, i1, i2, mask, **kw)
    (3.0 * loss).backward()
    # the loss is the value assembled from the partials, the gradient the ops' with the stated scales
    part, coef = nat.census_loss_partials(pred, i1, i2, mask, prm[3])
    s = part.double().sum(0)
    sm = nat.unsup_loss_partials(pred, i1, i2, mask, *prm).double().sum(0)[:, 1]
    w = 0.7 ** torch.arange(c.N - 1, -1, -1, dtype=torch.float64, device="cuda")
    want = (w * (s[:, 0] / c.P + 0.08 * (sm / (2.0 * c.P)))).sum().float()
    assert bits_equal(loss.detach(), want)
    # gl w_i / P for the census term, (0, gl w_i smooth_weight / (2P)) for the existing kernel, gl = 3
    smooth_scale = (torch.stack([torch.zeros_like(w), w * (0.08 / (2.0 * c.P))], -1) * 3.0).float()
    grad = nat.unsup_loss_grad(pred, i1, i2, mask, smooth_scale, *prm)
    nat.census_loss_grad(pred, i1, i2, mask, (w / c.P * 3.0).float(), prm[3], coef=coef, out=grad)
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
    # N > 32 runs the golden op on the device
    many = torch.zeros(33, 1, 8, 9, 2, device="cuda")
    img = torch.rand(1, 8, 9, 3, device="cuda")
    a, _ = unsup_loss(many, img, img, photo="census")
    b, _ = unsup_loss_reference(many.cpu(), img.cpu(), img.cpu(), photo="census")
    assert torch.allclose(a.cpu(), b, rtol=1e-5)
    # the golden sums on the device agree with the kernel's
    assert torch.allclose(census_sums(pred, i1, i2, mask, prm[3]).double(), s, rtol=1e-4)


def test_no_host_synchronisation_between_forward_and_backward():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    _, pred, i1, i2, mask = _case()
    f = pred.clone().requires_grad_(True)
    unsup_loss(f, i1, i2, mask, photo="census")[0].backward()   # warm: the library, the parameter tensor, allocator blocks
    unsup_loss(f, i1, i2, None, photo="census")[0].backward()
    f.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, mets = unsup_loss(f, i1, i2, mask, photo="census")
        loss.backward()
        loss2, _ = unsup_loss(f, i1, i2, None, photo="census")
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


def test_fused_trainer_census(monkeypatch):
    seen = []
    real = T.unsup_loss

    def spy(preds, *a, **k):
        loss, mets = real(preds, *a, **k)
        seen.append((preds.detach().clone(), loss.detach().clone(), k))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy)
    tr = Trainer(TrainConfig(loss="unsup", unsup_photo="census", **KW))
    assert tr.device.type == "cuda"
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(3)]
    outs = [tr.train_step(b) for b in batches]
    after = _params(tr)
    assert tr.skipped == 0 and all(math.isfinite(float(o["loss"])) for o in outs)
    assert set(outs[0]) == {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px"}
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # the step-1 loss is the census loss of that step's own predictions
    preds, loss, k = seen[0]
    assert k == {"photo": "census"}
    cfg = tr.cfg
    again, _ = real(preds, batches[0][0], batches[0][1], None, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s,
                    cfg.unsup_edge_kappa, cfg.unsup_smooth_weight, cfg.unsup_out_penalty, photo="census")
    assert bits_equal(again, loss) and bits_equal(outs[0]["loss"], loss)
    gold, _ = unsup_loss_reference(preds.cpu(), batches[0][0].cpu(), batches[0][1].cpu(), photo="census")
    assert torch.allclose(loss.cpu(), gold, rtol=1e-4)
    # the labels take no part in the gradient
    monkeypatch.setattr(T, "unsup_loss", real)
    other = Trainer(TrainConfig(loss="unsup", unsup_photo="census", **KW))
    for i1, i2, flow, valid in batches:
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(a, b) for a, b in zip(after, _params(other)))


def test_fused_trainer_census_drops_a_nan_prediction(monkeypatch):
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
    tr = Trainer(TrainConfig(loss="unsup", unsup_photo="census", **KW))
    tr.train_step(tr.batch_for(0))
    w1 = _params(tr)
    m = tr.train_step(tr.batch_for(1))
    assert not math.isfinite(float(m["loss"])) and not math.isfinite(float(m["grad_norm"]))
    tr.flush()
    assert tr.skipped == 1 and all(torch.equal(a, b) for a, b in zip(w1, _params(tr)))
    tr.train_step(tr.batch_for(2))
    tr.flush()
    assert tr.step == 3 and tr.skipped == 1 and all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_fused_trainer_charbonnier_equals_the_run_without_the_field():
    runs = []
    for kw in ({}, {"unsup_photo": "charbonnier"}):
        tr = Trainer(TrainConfig(loss="unsup", **KW, **kw))
        losses = [tr.train_step(tr.batch_for(s))["loss"] for s in range(3)]
        runs.append((losses, _params(tr)))
    assert all(bits_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
