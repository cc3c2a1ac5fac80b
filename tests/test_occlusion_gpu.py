"""The range-map kernels of csrc/kernels/occlusion.hip on the GPU, bitwise against the golden ops of
train/occlusion.py (computed on the CPU), their builders' host checks, the absence of host
synchronisation, and the fused trainer with ``unsup_occlusion``."""
import math

import pytest
import torch

import _occlusion_refs as OR
from _train_refs import bits_equal
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import range_map, unsup_loss, unsup_loss_reference, visibility_masks
from jax_raft_amd.train import occlusion as O
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train.trainer import TrainConfig, Trainer

pytestmark = pytest.mark.gpu
SENTINEL = 0x7f7f7f7f
MAPS = ((1, 1), (5, 7), (33, 70), (64, 128))     # 33 x 70: several blocks per map, an odd width for the row tail


def _fields(B, H, W):
    """name -> (flow_fw, flow_bw) on the CPU."""
    out = {
        "smooth": (OR.smooth_field(B, H, W, 1), OR.smooth_field(B, H, W, 2)),
        "random": (OR.random_field(B, H, W, 1), OR.random_field(B, H, W, 2)),
        "one_cell": (OR.one_cell_field(B, H, W, H // 3, W - 1), OR.one_cell_field(B, H, W, 0, 0) + 0.5),
        "special": (OR.special_field(B, H, W), -OR.special_field(B, H, W)),
    }
    return out


def _launch(fw, bw, T_):
    """The raw ops on pre-filled outputs: every element of acc is cleared and every mask written."""
    B, H, W, _ = fw.shape
    dfw, dbw = fw.cuda(), bw.cuda()
    acc = torch.full((2, B, H, W), SENTINEL, dtype=torch.int32, device="cuda")
    vis = torch.full((2, B, H, W), float("nan"), device="cuda")
    acc.zero_()
    nat.ops().range_splat([dfw, dbw, acc], [B, H, W])
    nat.ops().range_visible([dfw, dbw, acc, vis], [B, H, W, T_])
    return acc, vis


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", MAPS, ids=lambda v: str(v))
def test_kernels_equal_the_golden_ops(B, H, W):
    for name, (fw, bw) in _fields(B, H, W).items():
        for thr in (0.5, 0.9):
            T_ = O.range_threshold(thr)
            acc, vis = _launch(fw, bw, T_)
            want_acc = torch.stack([range_map(fw), range_map(bw)])
            want_vis = torch.stack(visibility_masks(fw, bw, "range", thr))
            assert torch.equal(acc.cpu(), want_acc), (name, thr)
            assert bits_equal(vis.cpu(), want_vis), (name, thr)
            # the front ends, twice: bitwise repeatable
            for _ in range(2):
                assert torch.equal(nat.range_map(fw.cuda(), bw.cuda()), acc)
                assert bits_equal(nat.visibility_masks(fw.cuda(), bw.cuda(), "range", thr), vis)
        one = nat.range_map(fw.cuda())                          # one direction: half the call
        assert one.shape == (B, H, W) and torch.equal(one, acc[0])
        fb = nat.visibility_masks(fw.cuda(), bw.cuda(), "fb", alpha=0.02, beta=0.25)
        assert bits_equal(fb.cpu(), torch.stack(visibility_masks(fw, bw, "fb", alpha=0.02, beta=0.25))), name
    if (H, W) == (33, 70):                                      # the contention case
        acc = nat.range_map(_fields(B, H, W)["one_cell"][0].cuda())
        assert bool((acc[:, H // 3, W - 1] == 256 * H * W).all()) and int(acc.sum()) == B * 256 * H * W


def test_two_layer_scene():
    fw, bw, want_fw, want_bw, off = OR.two_layer_scene(3)
    for kind in O.KINDS:
        got = nat.visibility_masks(fw.cuda(), bw.cuda(), kind).cpu()
        assert bits_equal(got, torch.stack(visibility_masks(fw, bw, kind)))
        assert torch.equal(got[0][off], want_fw[off]) and torch.equal(got[1][off], want_bw[off])   # off the 1-pixel rim
    # views at offsets that are only 8-byte aligned take the element path: no copy is needed
    H, W = OR.SCENE_HW
    buf = torch.zeros(2 * 3 * H * W * 2 + 2, device="cuda")
    a, b = buf[2:2 + 3 * H * W * 2].view(3, H, W, 2), buf[2 + 3 * H * W * 2:].view(3, H, W, 2)
    a.copy_(fw)
    b.copy_(bw)
    assert a.data_ptr() % 16 == 8
    assert bits_equal(nat.visibility_masks(a, b, "range").cpu(), torch.stack(visibility_masks(fw, bw, "range")))


def test_host_checks():
    B, H, W = 2, 6, 10
    P = B * H * W
    dev = "cuda"
    f, g = torch.zeros(B, H, W, 2, device=dev), torch.zeros(B, H, W, 2, device=dev)
    acc, vis = torch.zeros(2, B, H, W, dtype=torch.int32, device=dev), torch.zeros(2, B, H, W, device=dev)
    odd = torch.zeros(2 * P + 1, device=dev)[1:].view(B, H, W, 2)                  # 4-byte aligned only
    wide = torch.zeros(B, H, 2 * W, 2, device=dev)[:, :, :W]                       # not contiguous
    for op, good, ints, bad, bad_ints in (
        ("range_splat", [f, g, acc], [B, H, W],
         [(0, f.double()), (0, f[:1]), (0, f.cpu()), (0, None), (0, odd), (0, wide), (1, g.half()), (1, g[:1]), (1, wide),
          (2, acc[:1]), (2, acc.float()), (2, None), (2, acc.cpu()), (2, f.view(-1).view(torch.int32)), (1, acc.view(torch.float32).view(-1)[:2 * P])],
         ([0, H, W], [B, 0, W], [B, H, 0], [1, 1 << 12, (1 << 11) + 1], [40000, H, W])),
        ("range_visible", [f, g, acc, vis], [B, H, W, 128],
         [(0, f.double()), (0, odd), (0, wide), (0, None), (1, None), (1, g.cpu()), (1, g[:1]), (2, acc[:1]), (2, acc.long()),
          (2, None), (3, vis[:1]), (3, vis.double()), (3, None), (3, vis.cpu()), (3, acc.view(torch.float32)),
          (3, f.view(2, B, H, W)), (3, g.view(-1))],
         ([0, H, W, 128], [B, H, 0, 128], [1, 1 << 12, (1 << 11) + 1, 128], [B, H, W, 1 << 40])),
    ):
        fn = getattr(nat.ops(), op)
        for k, t in bad:
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good[:k] + [t] + good[k + 1:], ints)
        for b in bad_ints:
            with pytest.raises(RuntimeError, match=op + ":"):
                fn(good, list(b))
        fn(good, ints)                                                             # and the good call runs
    torch.cuda.synchronize()
    # the front ends refuse before anything is launched
    for bad in (f.double(), f[0], f[..., :1], f.cpu(), wide, odd, f[:1]):
        with pytest.raises(ValueError, match="visibility_masks"):
            nat.visibility_masks(f, bad, "range")
        with pytest.raises(ValueError, match="visibility_masks"):
            nat.visibility_masks(bad, f, "fb")
        with pytest.raises(ValueError, match="range_map"):
            nat.range_map(f, bad)
    for bad in (f.double(), f[0], wide, odd):
        with pytest.raises(ValueError, match="range_map"):
            nat.range_map(bad)
    with pytest.raises(ValueError, match="unknown kind"):
        nat.visibility_masks(f, g, "soft")


def test_no_host_synchronisation():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    B, H, W = 2, 33, 70
    fw, bw = OR.smooth_field(B, H, W, 1).cuda(), OR.smooth_field(B, H, W, 2).cuda()
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(2 * B, H, W, 3, generator=g).cuda(), torch.rand(2 * B, H, W, 3, generator=g).cuda()
    preds = torch.stack([torch.cat([fw, bw]) * 0.5, torch.cat([fw, bw])]).requires_grad_(True)

    def step():
        last = preds[-1].detach()
        mask = nat.visibility_masks(last[:B], last[B:], "range").view(2 * B, H, W)
        loss, _ = unsup_loss(preds, a, b, mask)
        loss.backward()
        return mask, loss

    step()                                   # warm: the library, the parameter tensor, allocator blocks
    preds.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        mask, loss = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(preds.grad).all())
    assert bits_equal(mask.cpu(), torch.cat(visibility_masks(fw.cpu(), bw.cpu(), "range")))


# ------------------------------------------------------------------ fused trainer
KW = dict(arch="raft_small", steps=3, batch=2, iters=3, size=(128, 160), log_every=100, lr=2e-4)   # tests/test_census_gpu.py's


def _params(tr):
    tr.flush()
    return [p.detach().clone() for p in tr.model.parameters()]


@pytest.mark.parametrize("kind,photo", [("range", "charbonnier"), ("fb", "charbonnier"), ("range", "census")])
def test_fused_trainer_with_masks(kind, photo, monkeypatch):
    seen = []
    real = T.unsup_loss

    def spy(preds, a, b, mask, *rest, **k):
        loss, mets = real(preds, a, b, mask, *rest, **k)
        seen.append((preds.detach().clone(), a, b, mask.clone(), rest, k, loss.detach().clone()))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy)
    extra = {} if photo == "charbonnier" else {"unsup_photo": photo}
    tr = Trainer(TrainConfig(loss="unsup", unsup_occlusion=kind, **extra, **KW))
    assert tr.device.type == "cuda"
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(3)]
    outs = [tr.train_step(b) for b in batches]
    after = _params(tr)
    assert tr.skipped == 0 and all(math.isfinite(float(o["loss"])) for o in outs)
    assert set(outs[0]) == {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px", "visible"}
    assert all(0.0 < float(o["visible"]) <= 1.0 for o in outs)
    assert not all(torch.equal(p, q) for p, q in zip(before, after))
    # step 1: the loss of its own predictions with the masks of its own final predictions
    preds, a, b, mask, rest, k, loss = seen[0]
    B = KW["batch"]
    H, W = KW["size"]
    assert preds.shape == (KW["iters"], 2 * B, H, W, 2) and k == ({} if photo == "charbonnier" else {"photo": photo})
    last = preds[-1].float()
    masks = nat.visibility_masks(last[:B].contiguous(), last[B:].contiguous(), kind, tr.cfg.unsup_occ_thr).view(2 * B, H, W)
    assert bits_equal(masks, mask) and bits_equal(outs[0]["visible"], masks.mean())
    again, _ = real(preds, a, b, masks, *rest, **k)
    assert bits_equal(again, loss) and bits_equal(outs[0]["loss"], loss)
    # the masks on the GPU are the golden masks of the same predictions, the loss close to the golden loss
    gold_masks = torch.cat(visibility_masks(last[:B].cpu(), last[B:].cpu(), kind, tr.cfg.unsup_occ_thr))
    assert bits_equal(mask.cpu(), gold_masks)
    gold, _ = unsup_loss_reference(preds.float().cpu(), a.cpu(), b.cpu(), gold_masks, *rest, **k)
    assert torch.allclose(loss.cpu(), gold, rtol=1e-4)
    # the labels take no part in the gradient
    monkeypatch.setattr(T, "unsup_loss", real)
    other = Trainer(TrainConfig(loss="unsup", unsup_occlusion=kind, **extra, **KW))
    for i1, i2, flow, valid in batches:
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(p, q) for p, q in zip(after, _params(other)))


def test_fused_trainer_with_masks_drops_a_nan_prediction(monkeypatch):
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
    tr = Trainer(TrainConfig(loss="unsup", unsup_occlusion="range", **KW))
    tr.train_step(tr.batch_for(0))
    w1 = _params(tr)
    m = tr.train_step(tr.batch_for(1))
    assert not math.isfinite(float(m["loss"])) and not math.isfinite(float(m["grad_norm"]))
    tr.flush()
    assert tr.skipped == 1 and all(torch.equal(a, b) for a, b in zip(w1, _params(tr)))
    tr.train_step(tr.batch_for(2))
    tr.flush()
    assert tr.step == 3 and tr.skipped == 1 and all(torch.isfinite(p).all() for p in tr.model.parameters())


def test_fused_trainer_none_equals_the_run_without_the_field():
    runs = []
    for kw in ({}, {"unsup_occlusion": "none"}):
        tr = Trainer(TrainConfig(loss="unsup", **KW, **kw))
        outs = [tr.train_step(tr.batch_for(s)) for s in range(3)]
        assert all("visible" not in o for o in outs)
        runs.append(([o["loss"] for o in outs], _params(tr)))
    assert all(bits_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
