"""Occlusion-aware label-free training on the CPU: the golden ops of train/occlusion.py (the range map
under exact integer checks and an independent fp64 splat, the visibility masks on a scene with known
occlusion), the front ends' host checks, the two op rows and the trainer switch."""
import json
import math

import pytest
import torch

import _occlusion_refs as OR
from _train_refs import bits_equal
from jax_raft_amd import fb_consistency
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import lands_inside, range_map, unsup_loss, visibility_masks
from jax_raft_amd.train import occlusion as O
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train.trainer import UNSUP_FIELDS, TrainConfig, Trainer, config_from_args

CPU = torch.device("cpu")
NAN, INF = OR.NAN, OR.INF


def _translation(B, H, W, dx, dy):
    f = torch.zeros(B, H, W, 2)
    f[..., 0], f[..., 1] = dx, dy
    return f


# ------------------------------------------------------------------ range_map
def test_integer_translation():
    H, W = 9, 13
    acc = range_map(_translation(2, H, W, 3.0, -2.0))
    want = torch.zeros(2, H, W, dtype=torch.int32)
    want[:, :H - 2, 3:] = 256                                  # the covered region; the strip left behind gets nothing
    assert acc.dtype == torch.int32 and torch.equal(acc, want)
    assert torch.equal(range_map(torch.zeros(1, 4, 5, 2)), torch.full((1, 4, 5), 256, dtype=torch.int32))


@pytest.mark.parametrize("dx,dy", [(0.5, 0.25), (-1.3, 2.7), (0.03, -0.49), (7 / 16, 9 / 16)])
def test_fractional_translation_gives_256_in_the_covered_interior(dx, dy):
    H, W = 12, 15
    acc = range_map(_translation(1, H, W, dx, dy))[0]
    # a cell whose four possible sources all exist: the landing points' floors span [lo, hi] per axis
    x_lo, x_hi = math.floor(dx) + 1, W - 1 + math.floor(dx)
    y_lo, y_hi = math.floor(dy) + 1, H - 1 + math.floor(dy)
    inner = acc[max(y_lo, 0):min(y_hi, H - 1) + 1, max(x_lo, 0):min(x_hi, W - 1) + 1]
    assert inner.numel() >= (H - 4) * (W - 3) and bool((inner == 256).all())
    assert torch.equal(acc, OR.range_map_loops(_translation(1, H, W, dx, dy))[0])


def test_nonfinite_and_far_landings_contribute_nothing():
    for bad in (NAN, INF, -INF, 1e30, -1e30):
        for ch in (0, 1):
            f = torch.zeros(1, 5, 6, 2)
            f[0, 2, 3, ch] = bad
            want = torch.full((1, 5, 6), 256, dtype=torch.int32)
            want[0, 2, 3] = 0
            assert torch.equal(range_map(f), want), (bad, ch)
    assert not range_map(torch.full((2, 3, 4, 2), NAN)).any()
    # px = -1 and px = W are outside (strict comparisons)
    f = torch.full((1, 1, 4, 2), NAN)
    f[0, 0, 0] = torch.tensor([-1.0, 0.0])
    f[0, 0, 3] = torch.tensor([1.0, 0.0])
    assert not range_map(f).any()


def test_partial_taps():
    H, W = 4, 6
    f = torch.full((1, H, W, 2), NAN)
    f[0, 1, 0] = torch.tensor([-0.5, 0.0])                     # px = -0.5: taps x = -1 (dropped) and 0
    f[0, 2, W - 1] = torch.tensor([0.25, 0.0])                 # px = W - 0.75: taps W-1 and W (dropped)
    f[0, 0, 3] = torch.tensor([0.0, -0.75])                    # py = -0.75: taps y = -1 (dropped) and 0
    f[0, H - 1, 2] = torch.tensor([0.0, 0.5])                  # py = H - 0.5
    want = torch.zeros(1, H, W, dtype=torch.int32)
    want[0, 1, 0] = 8 * 16
    want[0, 2, W - 1] = 12 * 16
    want[0, 0, 3] = 16 * 4
    want[0, H - 1, 2] = 16 * 8
    assert torch.equal(range_map(f), want)


def test_conservation():
    B, H, W = 2, 11, 14
    f = OR.smooth_field(B, H, W, seed=3, amp=4.0)
    px = torch.arange(W, dtype=torch.float32).view(1, 1, W) + f[..., 0]
    py = torch.arange(H, dtype=torch.float32).view(1, H, 1) + f[..., 1]
    x0, y0 = torch.floor(px), torch.floor(py)
    full = (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)     # the four taps are all in the map
    partial = ~full & (px > -1) & (px < W) & (py > -1) & (py < H)
    assert int(full.sum()) > 100 and int(partial.sum()) > 10
    by_hand = 0
    for b, y, x in partial.nonzero().tolist():
        fx, fy = float(px[b, y, x]), float(py[b, y, x])
        ix, iy = math.floor(fx), math.floor(fy)
        qx, qy = round((fx - ix) * 16), round((fy - iy) * 16)
        for dy in (0, 1):
            for dx in (0, 1):
                if 0 <= ix + dx < W and 0 <= iy + dy < H:
                    by_hand += (qx if dx else 16 - qx) * (qy if dy else 16 - qy)
    assert int(range_map(f).sum()) == 256 * int(full.sum()) + by_hand


def test_tie_rounds_to_even():
    def one(fx, fy):
        f = torch.full((1, 5, 7, 2), NAN)
        f[0, 2, 3] = torch.tensor([fx, fy])
        return range_map(f)[0]

    acc = one(1 / 32, 0.0)                                      # (1/32) * 16 = 0.5 -> 0
    assert int(acc[2, 3]) == 256 and int(acc.sum()) == 256
    acc = one(3 / 32, 0.0)                                      # 1.5 -> 2
    assert (int(acc[2, 3]), int(acc[2, 4])) == (14 * 16, 2 * 16)
    acc = one(0.0, 5 / 32)                                      # 2.5 -> 2
    assert (int(acc[2, 3]), int(acc[3, 3])) == (14 * 16, 2 * 16)
    acc = one(-1 / 32, 0.0)                                     # fraction 31/32: 15.5 -> 16
    assert int(acc[2, 3]) == 256


@pytest.mark.parametrize("seed", [0, 1])
def test_against_an_fp64_splat(seed):
    f = OR.smooth_field(2, 24, 40, seed=seed, amp=3.5)
    acc = range_map(f)
    ref, n = OR.splat_fp64(f)
    # per tap: |q/16 - w| <= 1/32 on each axis, so the product is off by at most 1/32 + 1/32 + 1/1024; the
    # 2^-20 covers the fp64 reference's own rounding with a very wide margin
    bound = n.double() * (1 / 32 + 1 / 32 + 1 / 1024) + n.double() * 2.0 ** -20
    err = (acc.double() / 256.0 - ref).abs()
    print(f"worst error / bound {float((err / bound.clamp_min(1e-30)).max()):.3f}, most taps {int(n.max())}")
    assert bool((err <= bound).all()) and int(n.max()) >= 5
    assert torch.equal(acc, OR.range_map_loops(f))
    assert torch.equal(range_map(OR.special_field(1, 6, 9)), OR.range_map_loops(OR.special_field(1, 6, 9)))
    r = OR.random_field(1, 9, 11, seed)
    assert torch.equal(range_map(r), OR.range_map_loops(r))


def test_overflow_guard_and_checks():
    big = torch.zeros(1, 1, 1, 2).expand(1, 2 ** 12 + 1, 2 ** 11, 2)       # H * W = 2^23 + 2^11, no memory behind it
    for fn in (range_map, nat.range_map):
        with pytest.raises(ValueError, match="2\\^23"):
            fn(big)
    with pytest.raises(ValueError, match="2\\^23"):
        nat.visibility_masks(big, big, "range")
    # every source on one cell: 256 H W, the sum the bound is for
    acc = range_map(OR.one_cell_field(1, 33, 70, 5, 64))
    assert int(acc[0, 5, 64]) == 256 * 33 * 70 and int(acc.sum()) == 256 * 33 * 70
    f = torch.zeros(1, 4, 5, 2)
    for fn in (range_map, lands_inside, nat.range_map):
        for bad in (f[0], f.double(), f[..., :1], torch.zeros(1, 0, 5, 2)):
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (visibility_masks, nat.visibility_masks):
        for kind in ("", "Range", None, "soft"):
            with pytest.raises(ValueError, match="unknown kind"):
                fn(f, f, kind)
        for bad in (f[0], f.double(), f[:, :3]):
            with pytest.raises(ValueError):
                fn(f, bad, "range")
            with pytest.raises(ValueError):
                fn(bad, f, "fb")
    # the CPU front ends are the golden ops
    g = OR.smooth_field(2, 7, 9)
    assert torch.equal(nat.range_map(g), range_map(g))
    assert torch.equal(nat.range_map(g, -g), torch.stack([range_map(g), range_map(-g)]))
    for kind in O.KINDS:
        assert torch.equal(nat.visibility_masks(g, -g, kind, 0.4), torch.stack(visibility_masks(g, -g, kind, 0.4)))
    assert (O.range_threshold(0.5), O.range_threshold(0.501), O.range_threshold(0.0), O.range_threshold(1.0)) == (128, 129, 0, 256)


# ------------------------------------------------------------------ visibility masks
@pytest.mark.parametrize("kind", O.KINDS)
def test_known_occlusion_scene(kind):
    fw, bw, want_fw, want_bw, off = OR.two_layer_scene(2)
    vis_fw, vis_bw = visibility_masks(fw, bw, kind)
    assert vis_fw.dtype == torch.float32 and vis_fw.shape == (2,) + OR.SCENE_HW and not vis_fw.requires_grad
    # compared off a rim of OR.RIM = 1 pixel on either side of the layer boundaries
    assert int((~off).sum()) > 0 and torch.equal(vis_fw[off], want_fw[off]) and torch.equal(vis_bw[off], want_bw[off])
    assert int((want_fw[off] == 0).sum()) >= 2 * (OR.SQ - 2) * (OR.SHIFT - 2)
    # a pixel whose own flow leaves the frame keeps mask 1, on the covered strip too
    y, x = OR.SQ_Y + 4, OR.SQ_X + OR.SQ + 2
    assert float(vis_fw[0, y, x]) == 0.0
    for bad in (100.0, -100.0, NAN, INF):
        f2 = fw.clone()
        f2[0, y, x, 0] = bad
        assert float(visibility_masks(f2, bw, kind)[0][0, y, x]) == 1.0, bad
    # no gradient, whatever the inputs carry
    a, b = fw.clone().requires_grad_(True), bw.clone().requires_grad_(True)
    m = visibility_masks(a, b, kind)
    assert not m[0].requires_grad and not m[1].requires_grad


def test_range_threshold_and_symmetry():
    f = OR.smooth_field(2, 20, 30, seed=4, amp=5.0)
    g = OR.smooth_field(2, 20, 30, seed=5, amp=5.0)
    for thr in (0.25, 0.5, 0.9):
        vis_fw, vis_bw = visibility_masks(f, g, "range", thr)
        T_ = math.ceil(thr * 256)
        assert torch.equal(vis_fw.bool(), ~lands_inside(f) | (range_map(g) >= T_))
        assert torch.equal(vis_bw.bool(), ~lands_inside(g) | (range_map(f) >= T_))
        swapped = visibility_masks(g, f, "range", thr)
        assert torch.equal(swapped[0], vis_bw) and torch.equal(swapped[1], vis_fw)
    assert 0.0 < float(visibility_masks(f, g, "range")[0].mean()) < 1.0


def test_fb_kind_is_the_stated_composition():
    f = OR.smooth_field(2, 20, 30, seed=6, amp=4.0)
    g = -f + 0.4 * OR.smooth_field(2, 20, 30, seed=7, amp=2.0)
    f[0, 3, 4, 0] = NAN
    for alpha, beta in ((0.01, 0.5), (0.05, 0.125)):
        occ_fw, occ_bw = fb_consistency(f, g, alpha, beta)
        vis_fw, vis_bw = visibility_masks(f, g, "fb", alpha=alpha, beta=beta)
        assert bits_equal(vis_fw, (~lands_inside(f) | ~occ_fw).float())
        assert bits_equal(vis_bw, (~lands_inside(g) | ~occ_bw).float())
        assert 0.0 < float(vis_fw.mean()) < 1.0
    assert float(vis_fw[0, 3, 4]) == 1.0                         # a non-finite own flow is "not inside"


# ------------------------------------------------------------------ op rows
@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_op_rows():
    for op, n in (("range_splat", 3), ("range_visible", 4)):
        assert list(torch.ops.jax_raft_amd.op_arity(op)) == [1, n, n]
        for k in (n - 1, n + 1):
            with pytest.raises(RuntimeError, match=rf"{op}: expected {n} ints, got {k}\b"):
                getattr(torch.ops.jax_raft_amd, op)([None], [1] * k)
        assert hasattr(torch.classes.jax_raft_amd.Plan(), "add_" + op)
        for ints in ([0, 4, 4, 128], [1, 2 ** 12 + 1, 2 ** 11, 128], [1, 2 ** 24, 1, 128], [40000, 4, 4, 128]):
            with pytest.raises(RuntimeError, match=op + ":"):      # the builder's own checks name the op
                getattr(torch.ops.jax_raft_amd, op)([None], ints[:n])
        with pytest.raises(RuntimeError, match=op + ":"):
            getattr(torch.ops.jax_raft_amd, op)([torch.zeros(1, 4, 4, 2)] + [None] * 3, [1, 4, 4, 128][:n])   # a CPU tensor


# ------------------------------------------------------------------ trainer
# 128 x 128 is the smallest frame the model takes (four pyramid levels at 1/8 resolution need 16 x 16 features)
KW = dict(arch="raft_small", steps=3, batch=2, iters=2, size=(128, 128), log_every=1, lr=1e-4)
OLD_KEYS = {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px"}


def _params(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


def test_config_and_cli():
    d = TrainConfig()
    assert (d.unsup_occlusion, d.unsup_occ_thr, d.unsup_occ_after) == ("none", 0.5, 0)
    for kw in ({"unsup_occlusion": "range"}, {"unsup_occlusion": "fb"}, {"unsup_occ_thr": 0.25}, {"unsup_occ_after": 5}):
        with pytest.raises(ValueError, match="unsup_occ"):
            TrainConfig(**kw)
        TrainConfig(loss="unsup", **kw)
    for bad in ("soft", "", None, "Range"):
        with pytest.raises(ValueError, match="unsup_occlusion"):
            TrainConfig(loss="unsup", unsup_occlusion=bad)
    with pytest.raises(ValueError, match="graph_step"):
        TrainConfig(loss="unsup", unsup_occlusion="range", graph_step=True)
    assert UNSUP_FIELDS[0] == "loss" and len(UNSUP_FIELDS) == 6   # the tuple is left as it is
    import argparse
    ns = argparse.Namespace(**{**{k: v for k, v in TrainConfig().__dict__.items() if k != "mix_weights"}, "mix": None,
                               "loss": "unsup", "unsup_occlusion": "range", "unsup_occ_thr": 0.75, "unsup_occ_after": 7})
    got = config_from_args(ns)
    assert (got.unsup_occlusion, got.unsup_occ_thr, got.unsup_occ_after) == ("range", 0.75, 7)


def test_trainer_none_is_the_run_without_the_field(tmp_path):
    runs = []
    for k, kw in enumerate(({}, {"unsup_occlusion": "none"})):
        tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / str(k)), loss="unsup", **KW, **kw), device=CPU)
        logs = []
        tr.fit(log=logs.append)
        lines = [json.loads(line) for line in logs]
        assert all(OLD_KEYS <= set(line) and "visible" not in line for line in lines)
        config = json.load(open(tmp_path / str(k) / "latest.json"))["config"]
        assert (config["unsup_occlusion"], config["unsup_occ_thr"], config["unsup_occ_after"]) == ("none", 0.5, 0)
        runs.append((_params(tr), [line["loss"] for line in lines], [sorted(line) for line in lines]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])) and runs[0][1:] == runs[1][1:]
    # a default (supervised) run records the three new keys too
    tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / "s"), **KW), device=CPU)
    tr.save(str(tmp_path / "s"))
    config = json.load(open(tmp_path / "s" / "latest.json"))["config"]
    assert {"unsup_occlusion", "unsup_occ_thr", "unsup_occ_after"} <= set(config) and not set(config) & set(UNSUP_FIELDS)


@pytest.mark.parametrize("kind", O.KINDS)
def test_trainer_with_masks_cpu(kind, monkeypatch):
    seen = []
    real = T.unsup_loss

    def spy(preds, a, b, mask, *rest, **k):
        loss, mets = real(preds, a, b, mask, *rest, **k)
        seen.append((preds.detach().clone(), a, b, None if mask is None else mask.clone(), loss.detach().clone()))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy)
    tr = Trainer(TrainConfig(loss="unsup", unsup_occlusion=kind, **KW), device=CPU)
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(3)]
    outs = [tr.train_step(b) for b in batches]
    after = _params(tr)
    assert tr.skipped == 0 and all(math.isfinite(float(o["loss"])) for o in outs)
    assert all(set(o) == OLD_KEYS | {"visible"} for o in outs)
    assert all(0.0 < float(o["visible"]) <= 1.0 for o in outs)
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # step 1: both directions as one batch of 2B, the masks those of the final prediction
    preds, a, b, mask, loss = seen[0]
    B, cfg = 2, tr.cfg
    i1, i2 = batches[0][:2]
    assert preds.shape == (2, 2 * B, 128, 128, 2) and torch.equal(a, torch.cat([i1, i2])) and torch.equal(b, torch.cat([i2, i1]))
    vis_fw, vis_bw = visibility_masks(preds[-1, :B], preds[-1, B:], kind, cfg.unsup_occ_thr)
    want = torch.cat([vis_fw, vis_bw])
    assert torch.equal(mask, want) and bits_equal(outs[0]["visible"], want.mean())
    again, _ = unsup_loss(preds, a, b, want, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s, cfg.unsup_edge_kappa,
                          cfg.unsup_smooth_weight, cfg.unsup_out_penalty)
    assert bits_equal(again, loss) and bits_equal(outs[0]["loss"], loss)
    # the supervised metrics are the forward direction's
    from jax_raft_amd.train.loss import sequence_loss
    _, sup = sequence_loss(preds[:, :B], batches[0][2], batches[0][3], cfg.gamma, cfg.max_flow)
    assert bits_equal(outs[0]["epe"], sup["epe"])
    # the labels take no part in the gradient
    monkeypatch.setattr(T, "unsup_loss", real)
    other = Trainer(TrainConfig(loss="unsup", unsup_occlusion=kind, **KW), device=CPU)
    for i1, i2, flow, valid in batches:
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(p, q) for p, q in zip(after, _params(other)))


def test_trainer_masks_start_after(monkeypatch):
    seen = []
    real = T.unsup_loss

    def spy(preds, a, b, mask, *rest, **k):
        loss, mets = real(preds, a, b, mask, *rest, **k)
        seen.append((preds.detach().clone(), a, b, mask, rest, loss.detach().clone()))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy)
    tr = Trainer(TrainConfig(loss="unsup", unsup_occlusion="range", unsup_occ_after=2, **KW), device=CPU)
    outs = [tr.train_step(tr.batch_for(s)) for s in range(3)]
    for k in (0, 1):
        preds, a, b, mask, rest, loss = seen[k]
        assert mask is None and preds.shape[1] == 4 and float(outs[k]["visible"]) == 1.0
        assert bits_equal(real(preds, a, b, None, *rest)[0], loss) and bits_equal(outs[k]["loss"], loss)
    assert seen[2][3] is not None and seen[2][3].shape == (4, 128, 128) and 0.0 < float(outs[2]["visible"]) <= 1.0


def test_trainer_census_with_masks_cpu():
    tr = Trainer(TrainConfig(loss="unsup", unsup_photo="census", unsup_occlusion="range", **{**KW, "steps": 1}), device=CPU)
    out = tr.train_step(tr.batch_for(0))
    assert math.isfinite(float(out["loss"])) and set(out) == OLD_KEYS | {"visible"}
