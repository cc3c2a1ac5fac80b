"""Self-supervision on the GPU: crop_resize bitwise against the golden op, the two loss kernels of
csrc/kernels/selfsup.hip under the per-element fp64 checks of _selfsup_refs.py, the builders' host checks,
the autograd function (the batch window read in place, no host synchronisation) and the fused trainer."""
import math

import pytest
import torch

import _selfsup_refs as R
from _train_refs import bits_equal
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import crop_resize, lands_inside, selfsup_loss, selfsup_loss_reference
from jax_raft_amd.train import selfsup as S
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train.trainer import TrainConfig, Trainer

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _d(t):
    return None if t is None else t.cuda()


def _off8(t):
    """A contiguous GPU copy of t whose address is 8-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 2, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[2:].view(t.shape)
    v.copy_(t)
    return v


# ------------------------------------------------------------------ crop_resize
@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("case", R.CROP_CASES_GPU, ids=str)
def test_crop_resize_is_the_golden_op(case, C):
    B, H, W, c = case
    x = R.crop_input(case, C)
    scale = {1: (0.75,), 2: S.flow_scale(H, W, c), 3: None}[C]
    want = crop_resize(x, c, scale)
    out = torch.full(x.shape, NAN, device="cuda")
    got = nat.crop_resize(x.cuda(), c, scale, out=out)
    assert got is out and bits_equal(got.cpu(), want)
    assert bits_equal(nat.crop_resize(x.cuda(), c, scale).cpu(), want)          # repeatable, and without out
    # an 8-byte aligned input and output: element stores
    out8 = _off8(torch.full(x.shape, NAN))
    assert out8.data_ptr() % 16 == 8
    assert bits_equal(nat.crop_resize(_off8(x), c, scale, out=out8).cpu(), want)
    # nothing outside the crop is read
    poisoned = torch.full_like(x, NAN)
    poisoned[:, c:H - c, c:W - c] = x[:, c:H - c, c:W - c]
    assert bits_equal(nat.crop_resize(poisoned.cuda(), c, scale).cpu(), want)


def test_crop_resize_vector_stores_and_ones():
    x = R.crop_input((2, 40, 64, 8), 3)                     # W % 4 == 0: the 16-byte stores
    for C in (1, 2, 3):
        xc = x[..., :C].contiguous()
        out = torch.full(xc.shape, NAN, device="cuda")
        assert bits_equal(nat.crop_resize(xc.cuda(), 8, out=out).cpu(), crop_resize(xc, 8))
    assert bool((nat.crop_resize(torch.ones(1, 40, 64, 1, device="cuda"), 3) == 1.0).all())


def test_crop_resize_host_checks():
    x = torch.zeros(1, 8, 12, 3, device="cuda")
    for bad_c in (0, 4, 1.0):
        with pytest.raises(ValueError, match="crop_resize"):
            nat.crop_resize(x, bad_c)
    for bad in (x.double(), x.half(), torch.zeros(1, 8, 12, 4, device="cuda"), torch.zeros(1, 8, 24, 3, device="cuda")[:, :, ::2]):
        with pytest.raises(ValueError, match="crop_resize"):
            nat.crop_resize(bad, 1)
    for out in (torch.zeros(1, 8, 12, 3), torch.zeros(1, 8, 12, 2, device="cuda"), x):
        with pytest.raises(ValueError, match="crop_resize"):
            nat.crop_resize(x, 1, out=out)
    prm, out = torch.ones(6, device="cuda"), torch.zeros_like(x)
    fn = nat.ops().crop_resize
    for t in ([x.cpu(), prm, out], [x, prm[:5], out], [x, prm, out[:, :4]], [x, prm, x], [x, prm.double(), out], [x, None, out]):
        with pytest.raises(RuntimeError, match="crop_resize:"):
            fn(t, [1, 8, 12, 3, 1])
    for ints in ([1, 8, 12, 3, 4], [1, 8, 12, 3, 0], [2, 8, 12, 3, 1], [1, 8, 12, 4, 1]):
        with pytest.raises(RuntimeError, match="crop_resize:"):
            fn([x, prm, out], ints)
    fn([x, prm, out], [1, 8, 12, 3, 1])
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the loss kernels
class Kernels:
    """The ops themselves, outputs pre-filled with NaN so that unwritten elements show."""

    def selfsup_loss(self, stack, target, weight, eps, b0):
        N, Btot, H, W, _ = stack.shape
        B = target.shape[0]
        part = torch.full((nat.selfsup_loss_blocks(B * H * W), N, 4), NAN, device="cuda")
        nat.ops().selfsup_loss([_d(stack), _d(target), _d(weight), torch.tensor([eps], device="cuda"), part], [N, B, H, W, Btot, b0])
        return part.cpu()

    def selfsup_loss_bwd(self, stack, target, weight, eps, scale, b0):
        N, Btot, H, W, _ = stack.shape
        B = target.shape[0]
        grad = torch.full((N, B, H, W, 2), NAN, device="cuda")
        nat.ops().selfsup_loss_bwd([_d(stack), _d(target), _d(weight), torch.tensor([eps], device="cuda"), _d(scale), grad],
                                   [N, B, H, W, Btot, b0])
        return grad.cpu()


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=str)
def test_kernels_against_the_fp64_reference(case):
    assert nat.selfsup_loss_blocks(case[1] * case[2] * case[3]) == R.blocks_expected(case[1] * case[2] * case[3])
    R.check_loss(Kernels(), case)
    R.check_loss_bwd(Kernels(), case)


def test_kernels_nan_cases():
    R.check_loss(Kernels(), R.NAN_CASE, nan=True)
    R.check_loss_bwd(Kernels(), R.NAN_CASE, nan=True)


@pytest.mark.parametrize("case", [R.LOSS_CASES[6], R.LOSS_CASES[7]], ids=str)
def test_batch_window_is_the_call_on_a_copy(case):
    c = R.loss_inputs(case)
    assert c.B0 > 0 and c.Btot > c.B
    k = Kernels()
    copy = c.stack[:, c.B0:c.B0 + c.B].contiguous()
    assert bits_equal(k.selfsup_loss(c.stack, c.target, c.weight, R.EPS, c.B0), k.selfsup_loss(copy, c.target, c.weight, R.EPS, 0))
    assert bits_equal(k.selfsup_loss_bwd(c.stack, c.target, c.weight, R.EPS, c.scale, c.B0),
                      k.selfsup_loss_bwd(copy, c.target, c.weight, R.EPS, c.scale, 0))
    # 8-byte aligned operands run the kernels' other instantiation (8-byte loads and stores): the same pixel of the same
    # thread, so the same partial sums and the same gradient bit for bit
    stack8, target8 = _off8(c.stack), _off8(c.target)
    N, Btot, H, W, _ = c.stack.shape
    prm, scale = torch.tensor([R.EPS], device="cuda"), c.scale.cuda()
    grad = torch.full((N, c.B, H, W, 2), NAN, device="cuda")
    nat.ops().selfsup_loss_bwd([stack8, target8, _d(c.weight), prm, scale, grad], [N, c.B, H, W, Btot, c.B0])
    assert bits_equal(grad.cpu(), k.selfsup_loss_bwd(c.stack, c.target, c.weight, R.EPS, c.scale, c.B0))
    part = torch.full((nat.selfsup_loss_blocks(c.P), N, 4), NAN, device="cuda")
    nat.ops().selfsup_loss([stack8, target8, _d(c.weight), prm, part], [N, c.B, H, W, Btot, c.B0])
    assert bits_equal(part.cpu(), k.selfsup_loss(c.stack, c.target, c.weight, R.EPS, c.B0))


def test_builders_host_checks():
    N, B, H, W, Btot, B0 = 2, 1, 6, 10, 3, 1
    P, dev = B * H * W, "cuda"
    pred, target = torch.zeros(N, Btot, H, W, 2, device=dev), torch.zeros(B, H, W, 2, device=dev)
    weight, prm, scale = torch.ones(B, H, W, device=dev), torch.tensor([R.EPS], device=dev), torch.ones(N, device=dev)
    part, grad = torch.zeros(nat.selfsup_loss_blocks(P), N, 4, device=dev), torch.zeros(N, B, H, W, 2, device=dev)
    ints = [N, B, H, W, Btot, B0]
    fwd, bwd = [pred, target, weight, prm, part], [pred, target, weight, prm, scale, grad]
    odd = torch.zeros(pred.numel() + 1, device=dev)[1:]                 # 4-byte aligned only
    wide = torch.zeros(B, H, 2 * W, 2, device=dev)[:, :, :W]            # not contiguous
    for op, good, bad in (
        ("selfsup_loss", fwd, [(0, pred.double()), (0, pred[:, :1]), (0, odd), (0, pred.cpu()), (0, None), (1, wide),
                               (1, target[:, :5]), (1, target.half()), (2, weight.bool()), (2, weight[:, :5]), (3, prm.repeat(2)),
                               (3, None), (4, part[:, :1]), (4, part.double()), (4, None), (4, pred.view(-1)[:part.numel()])]),
        ("selfsup_loss_bwd", bwd, [(0, pred.double()), (1, target[:, :5]), (2, weight.bool()), (3, prm.repeat(2)),
                                   (4, scale[:1]), (4, None), (5, grad[:1]), (5, grad.double()), (5, None),
                                   (5, pred.view(-1)[:grad.numel()].view(grad.shape))])):
        fn = getattr(nat.ops(), op)
        for k, t in bad:
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good[:k] + [t] + good[k + 1:], ints)
        for bad_ints in ([0, B, H, W, Btot, B0], [33, B, H, W, Btot, B0], [N, B, H, W, Btot, 3], [N, B, H, W, Btot, -1],
                         [N, 4, H, W, Btot, 0], [N, B, 1 << 16, 1 << 16, Btot, 0]):
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good, bad_ints)
        fn(good, ints)                                                   # and the good call runs
        fn(good[:2] + [None] + good[3:], ints)                           # ... without a weight too
    torch.cuda.synchronize()
    # the front ends refuse before anything is launched
    for call in (lambda: nat.selfsup_loss_partials(pred.double(), target.double()),
                 lambda: nat.selfsup_loss_partials(torch.zeros(33, B, H, W, 2, device=dev), target),
                 lambda: nat.selfsup_loss_partials(pred, target, batch0=3),
                 lambda: nat.selfsup_loss_partials(pred[:, :, :, ::2], target[:, :, ::2]),
                 lambda: nat.selfsup_loss_partials(pred, target.cpu()),
                 lambda: nat.selfsup_loss_grad(pred, target, None, scale.double(), batch0=1),
                 lambda: nat.selfsup_loss_grad(pred, target, None, scale[:1], batch0=1)):
        with pytest.raises(ValueError, match="selfsup_loss"):
            call()


# ------------------------------------------------------------------ the autograd function
def _autograd_case():
    c = R.loss_inputs(R.LOSS_CASES[6])
    return c, c.stack.cuda(), c.target.cuda(), c.weight.cuda()


def test_autograd_function_reads_the_window_in_place(monkeypatch):
    c, stack, target, weight = _autograd_case()
    seen = []
    real = nat.selfsup_loss_partials

    def spy(preds, *a, **k):
        seen.append((preds.data_ptr(), k.get("batch0")))
        return real(preds, *a, **k)

    monkeypatch.setattr(nat, "selfsup_loss_partials", spy)
    f = stack.clone().requires_grad_(True)
    loss, mets = selfsup_loss(f[:, c.B0:c.B0 + c.B], target, weight, 0.8, R.EPS)
    loss.backward()
    assert seen == [(f.data_ptr(), c.B0)]                               # the whole stack, no copy of the window
    want, want_m = selfsup_loss_reference(c.stack[:, c.B0:c.B0 + c.B].double(), c.target.double(), c.weight.double(), 0.8, R.EPS)
    assert math.isclose(float(loss.detach()), float(want), rel_tol=1e-5)
    assert math.isclose(float(mets["selfsup"]), float(want_m["selfsup"]), rel_tol=1e-5)
    assert math.isclose(float(mets["selfsup_w"]), float(want_m["selfsup_w"]), rel_tol=1e-6)
    # the gradient: the kernel's inside the window, exactly 0 outside it
    w = (0.8 ** torch.arange(c.N - 1, -1, -1, dtype=torch.float64) / c.P).float()
    _, ref, tol = R.loss_formulas(c.stack[:, c.B0:c.B0 + c.B], c.target, c.weight, R.EPS, w)
    g = f.grad.cpu()
    assert R.ratio(g[:, c.B0:c.B0 + c.B], ref, tol) <= 1.0
    assert bool((g[:, :c.B0] == 0).all()) and bool((g[:, c.B0 + c.B:] == 0).all())
    # N > 32 and fp64 run the golden op on the device
    many = torch.zeros(33, 1, 4, 6, 2, device="cuda")
    a, _ = selfsup_loss(many, torch.ones(1, 4, 6, 2, device="cuda"))
    b, _ = selfsup_loss_reference(many.cpu(), torch.ones(1, 4, 6, 2))
    assert torch.allclose(a.cpu(), b, rtol=1e-5) and len(seen) == 1


def test_no_host_synchronisation_between_forward_and_backward():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    c, stack, target, weight = _autograd_case()
    f = stack.clone().requires_grad_(True)
    x = torch.rand(2, 16, 20, 2, device="cuda")
    selfsup_loss(f[:, c.B0:c.B0 + c.B], target, weight, 0.8, R.EPS)[0].backward()   # warm: the library, the parameter tensors
    selfsup_loss(f[:, :c.B], target, None, 0.8, R.EPS)[0].backward()
    nat.crop_resize(x, 2, (1.5, 2.0))
    f.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss, mets = selfsup_loss(f[:, c.B0:c.B0 + c.B], target, weight, 0.8, R.EPS)
        loss.backward()
        loss2, _ = selfsup_loss(f[:, :c.B], target, None, 0.8, R.EPS)
        loss2.backward()
        y = nat.crop_resize(x, 2, (1.5, 2.0))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and math.isfinite(float(loss2.detach())) and bool(torch.isfinite(f.grad).all())
    assert bool(torch.isfinite(y).all())


# ------------------------------------------------------------------ fused trainer
KW = dict(arch="raft_small", steps=3, batch=1, iters=3, size=(128, 128), log_every=100, lr=2e-4)
ON = dict(loss="unsup", unsup_occlusion="range", unsup_selfsup_weight=0.3, unsup_selfsup_crop=16)
KEYS = {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px", "visible", "selfsup", "selfsup_w"}


def _params(tr):
    tr.flush()
    return [p.detach().clone() for p in tr.model.parameters()]


def _spies(monkeypatch):
    real_u, real_s = T.unsup_loss, S.selfsup_loss
    seen = {"unsup": [], "selfsup": [], "real": real_s}

    def spy_u(preds, a, b, mask, *rest, **k):
        loss, mets = real_u(preds, a, b, mask, *rest, **k)
        seen["unsup"].append((preds.detach().clone(), a, b, None if mask is None else mask.clone(), loss.detach().clone()))
        return loss, mets

    def spy_s(preds, target, weight, *rest):
        loss, mets = real_s(preds, target, weight, *rest)
        seen["selfsup"].append((preds.detach().clone(), target.clone(), weight.clone(), loss.detach().clone()))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy_u)
    monkeypatch.setattr(S, "selfsup_loss", spy_s)
    return seen


@pytest.mark.parametrize("kind", ["range", "fb"])
def test_fused_trainer_selfsup(kind, monkeypatch):
    seen = _spies(monkeypatch)
    windows, real_partials = [], nat.selfsup_loss_partials
    monkeypatch.setattr(nat, "selfsup_loss_partials",
                        lambda preds, *a, **k: windows.append((tuple(preds.shape), k.get("batch0"))) or real_partials(preds, *a, **k))
    kw = {**KW, **ON, "unsup_occlusion": kind}
    tr = Trainer(TrainConfig(**kw))
    assert tr.device.type == "cuda"
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(3)]
    outs = [tr.train_step(b) for b in batches]
    after = _params(tr)
    assert tr.skipped == 0 and all(math.isfinite(float(o["loss"])) for o in outs) and set(outs[0]) == KEYS
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # step 1, from its own predictions through nat.*; the target and the weight bitwise the golden ones
    B, c, cfg = 1, 16, tr.cfg
    full, a, b, mask, unsup = seen["unsup"][0]
    student, target, weight, term = seen["selfsup"][0]
    assert full.shape == student.shape == (3, 2 * B, 128, 128, 2)
    assert windows[0] == ((3, 4 * B, 128, 128, 2), 2 * B)                # the student half of the 4B stack, read in place
    vis = nat.visibility_masks(full[-1, :B].contiguous(), full[-1, B:].contiguous(), kind, cfg.unsup_occ_thr).view(2 * B, 128, 128)
    assert torch.equal(mask, vis)
    Tp = vis * lands_inside(full[-1]).float()
    Sp = nat.visibility_masks(student[-1, :B].contiguous(), student[-1, B:].contiguous(), kind,
                              cfg.unsup_occ_thr).view(2 * B, 128, 128) * lands_inside(student[-1]).float()
    want_t = crop_resize(full[-1].cpu(), c, S.flow_scale(128, 128, c))
    want_w = crop_resize(Tp.cpu().unsqueeze(-1), c).squeeze(-1) * (1.0 - Sp.cpu())
    assert bits_equal(target.cpu(), want_t) and bits_equal(weight.cpu(), want_w)
    again, _ = seen["real"](student, target, weight, cfg.gamma, cfg.unsup_selfsup_eps)     # on a copy of the window
    assert bits_equal(again, term) and bits_equal(outs[0]["loss"], unsup + cfg.unsup_selfsup_weight * term)
    gold, _ = selfsup_loss_reference(student.cpu(), want_t, want_w, cfg.gamma, cfg.unsup_selfsup_eps)
    assert torch.allclose(term.cpu(), gold, rtol=1e-4)
    if kind != "range":
        return
    # the labels take no part in the gradient
    monkeypatch.undo()
    other = Trainer(TrainConfig(**kw))
    for i1, i2, flow, valid in batches:
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(p, q) for p, q in zip(after, _params(other)))


def test_fused_trainer_weight_zero_is_the_run_without_the_fields():
    runs = []
    base = dict(loss="unsup", unsup_occlusion="range")
    for kw in ({}, {"unsup_selfsup_weight": 0.0, "unsup_selfsup_crop": 16, "unsup_selfsup_after": 1}):
        tr = Trainer(TrainConfig(**KW, **base, **kw))
        outs = [tr.train_step(tr.batch_for(s)) for s in range(3)]
        assert all("selfsup" not in o for o in outs)
        runs.append(([o["loss"] for o in outs], _params(tr)))
    assert all(bits_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_fused_trainer_drops_a_nan_student_prediction(monkeypatch):
    real = S.selfsup_loss
    calls = []

    def poisoned(preds, *a, **k):
        calls.append(1)
        if len(calls) == 2:                             # step 2: one NaN in a middle iteration of the student
            bad = torch.ones_like(preds)
            bad[1, 0, 40, 50, 0] = NAN
            preds = preds * bad
        return real(preds, *a, **k)

    monkeypatch.setattr(S, "selfsup_loss", poisoned)
    tr = Trainer(TrainConfig(**KW, **ON))
    tr.train_step(tr.batch_for(0))
    w1 = _params(tr)
    m = tr.train_step(tr.batch_for(1))
    assert not math.isfinite(float(m["grad_norm"]))
    tr.flush()
    assert tr.skipped == 1 and all(torch.equal(a, b) for a, b in zip(w1, _params(tr)))
    tr.train_step(tr.batch_for(2))
    tr.flush()
    assert tr.step == 3 and tr.skipped == 1 and all(torch.isfinite(p).all() for p in tr.model.parameters())
