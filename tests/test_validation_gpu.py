"""Validation during training on the GPU: the metrics kernels (csrc/kernels/metrics.hip) against
the golden op (eval/metrics.py) -- every count bitwise, the fp64 sums within the summation-order
bound 2 * N * 2^-53 of test_validation.py -- their repeatability, the front-end without host
synchronisation, its host checks, the streaming ``evaluate`` against the stand-alone validators on
the same model, and the trainer's in-loop validation on the fused path.

The kernel's block is 256 threads of 4 pixels: the shapes below have widths that are no multiple
of 4, pitches that differ between pred and gt, and one sample of five blocks with a partial last."""
import json
import math

import pytest
import torch

from jax_raft_amd import flow_metrics, raft_small
from jax_raft_amd.eval.kitti import validate_kitti
from jax_raft_amd.eval.validate import evaluate
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train.trainer import TrainConfig, Trainer
from test_augment import write_chairs
from test_eval import _make_sintel
from test_sparse import write_kitti
from test_validation import (KITTI_SIZES, SINTEL, _state, assert_rows, boundary_case, close, numpy_rows,
                             sintel_with_fp64_epe)

pytestmark = pytest.mark.gpu

SIZES = [(21, 37), (20, 33), (9, 5)]


def maps(seed=5, B=3, pred_hw=(21, 37), gt_hw=(23, 41)):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(B, *pred_hw, 2, generator=g) * 4
    gt = torch.randn(B, *gt_hw, 2, generator=g) * 30
    gt[0, :4] = 0                                    # |gt| == 0: outliers by epe alone, and 0 / 0
    pred[0, 0, :3] = 0
    valid = (torch.rand(B, *gt_hw, generator=g) < 0.6).to(torch.uint8) * 255
    valid[:, ::2] //= 255                            # bytes 0, 1 and 255
    return pred, gt, valid


def fill_outside(pred, gt, valid, sizes, poison):
    """Everything outside each sample's rectangle: 0, or NaN / 0xFF."""
    p, g, v = pred.clone(), gt.clone(), valid.clone()
    fv, bv = (float("nan"), 255) if poison else (0.0, 0)
    for n, (h, w) in enumerate(sizes):
        p[n, h:], p[n, :, w:], g[n, h:], g[n, :, w:] = fv, fv, fv, fv
        v[n, h:], v[n, :, w:] = bv, bv
    return p, g, v


def gpu(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def check_against_golden(pred, gt, valid, sizes):
    want_rows, want_acc = flow_metrics(pred, gt, valid, sizes)
    rows, acc = nat.flow_metrics(*gpu(pred, gt, valid), sizes)
    assert rows.is_cuda and acc.is_cuda and rows.dtype == acc.dtype == torch.float64
    hw = sizes or [(min(pred.shape[1], gt.shape[1]), min(pred.shape[2], gt.shape[2]))] * pred.shape[0]
    assert_rows(rows, want_rows.numpy(), hw)
    assert_rows(rows, numpy_rows(pred, gt, valid, hw), hw)
    acc, n = acc.cpu(), sum(h * w for h, w in hw)
    assert torch.equal(acc[1:6], want_acc[1:6]) and acc[7] == want_acc[7] == pred.shape[0]
    assert close(acc[0], want_acc[0], n) and close(acc[6], want_acc[6], n)
    return rows.cpu(), acc


@pytest.mark.parametrize("with_valid", (True, False))
def test_kernel_equals_golden_and_reads_nothing_outside(with_valid):
    pred, gt, valid = maps()
    out = []
    for poison in (False, True):
        p, g, v = fill_outside(pred, gt, valid, SIZES, poison)
        out.append(check_against_golden(p, g, v if with_valid else None, SIZES))
    # both fills: identical results (without a plane, a dense sample's valid bytes are never read)
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[1][1]).all()


def test_default_sizes_are_the_smaller_map():
    pred, gt, valid = maps()
    check_against_golden(pred, gt, valid, None)


def test_boundary_pixels():
    pred, gt, valid, _ = boundary_case()
    rows, acc = check_against_golden(pred, gt, valid, None)
    assert rows[0, 1:].tolist() == [13.0, 2.0, 5.0, 10.0, 6.0]                # by hand: test_validation.py
    assert rows[1].tolist() == [0.0] * 6 and math.isnan(float(rows[2, 0])) and acc[7] == 3
    check_against_golden(pred[:2], gt[:2], valid[:2], None)                    # finite: the image mean of an empty sample


def test_several_blocks_with_a_partial_last():
    sizes = [(47, 93), (13, 90)]                      # 47 * 24 = 1128 runs of 4: five blocks of 256, the last with 104
    assert nat.flow_metrics_blocks(*sizes[0]) == 5 and 47 * 24 % nat.METRICS_BLOCK
    pred, gt, valid = maps(seed=9, B=2, pred_hw=(47, 93), gt_hw=(50, 95))
    check_against_golden(pred, gt, valid, sizes)
    check_against_golden(pred, gt, None, sizes)


def test_repeatable_and_accumulates():
    pred, gt, valid = maps(seed=11, B=4, pred_hw=(47, 93), gt_hw=(47, 93))
    dp, dg, dv = gpu(pred, gt, valid)
    r1, a1 = nat.flow_metrics(dp, dg, dv)
    r2, a2 = nat.flow_metrics(dp, dg, dv)
    assert torch.equal(r1, r2) and torch.equal(a1, a2)                         # bitwise, run to run
    _, acc = nat.flow_metrics(dp[:1], dg[:1], dv[:1])
    rows, same = nat.flow_metrics(dp[1:], dg[1:], dv[1:], acc=acc)
    assert same is acc and torch.equal(rows, r1[1:])
    _, want = flow_metrics(pred[:1], gt[:1], valid[:1])
    flow_metrics(pred[1:], gt[1:], valid[1:], acc=want)
    acc = acc.cpu()
    assert torch.equal(acc[1:6], want[1:6]) and acc[7] == want[7] == 4
    assert close(acc[0], want[0], 4 * 47 * 93) and close(acc[6], want[6], 4 * 47 * 93)
    assert torch.equal(acc[1:6], a1.cpu()[1:6]) and close(acc[0], a1.cpu()[0], 4 * 47 * 93)
    held = torch.zeros(9, dtype=torch.float64, device="cuda")                  # an acc that is a view at 8 bytes
    nat.flow_metrics(dp, dg, dv, acc=held[1:])
    assert held[0] == 0 and torch.equal(held[1:], a1)


def test_front_end_does_not_synchronise():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    pred, gt, valid = maps()
    dp, dg, dv = gpu(pred, gt, valid)
    acc = torch.zeros(8, dtype=torch.float64, device="cuda")
    nat.flow_metrics(dp, dg, dv, SIZES, acc)          # warm: the library, allocator blocks
    acc.zero_()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rows, out = nat.flow_metrics(dp, dg, dv, SIZES, acc)
        nat.flow_metrics(dp, dg, None, SIZES, acc)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert out is acc and acc[7] == 6
    assert_rows(rows, flow_metrics(pred, gt, valid, SIZES)[0].numpy(), SIZES)


def test_host_checks_come_before_any_launch():
    pred, gt, valid = gpu(*maps())
    acc = torch.zeros(8, dtype=torch.float64, device="cuda")
    for bad in ([(22, 37)] * 3, [(21, 38)] * 3, [(21, 37)] * 2, [(21, 0)] * 3):
        with pytest.raises(ValueError):
            nat.flow_metrics(pred, gt, valid, bad, acc)
    for args in ((pred.double(), gt, valid), (pred, gt.half(), valid), (pred, gt, valid.bool()), (pred, gt, valid[:, :21]),
                 (pred, gt, valid, None, acc.float()), (pred, gt.cpu(), valid), (pred, gt, valid, None, acc.cpu())):
        with pytest.raises(ValueError):
            nat.flow_metrics(*args)
    torch.cuda.synchronize()
    assert not acc.any()                              # nothing was launched
    # the launch builder's own checks (a direct caller of the op)
    B, nb = 3, nat.flow_metrics_blocks(21, 37)
    sizes = torch.tensor(SIZES, dtype=torch.int32, device="cuda")
    part = torch.empty(B * nb * 2, dtype=torch.float64, device="cuda")
    rows = torch.empty(B, 6, dtype=torch.float64, device="cuda")
    ints = [B, 21, 37, 23, 41, nb]
    good = [pred, gt, valid, sizes, part, rows, acc]
    for k, t in ((0, pred.double()), (1, gt[:2]), (2, valid.int()), (3, sizes.long()), (3, sizes[:2]), (4, part[:-1]),
                 (4, part.float()), (5, rows[:2]), (6, acc[:6]), (6, rows.view(-1)[:8]), (0, None), (3, None)):
        with pytest.raises(RuntimeError, match="flow_metrics"):
            nat.ops().flow_metrics(good[:k] + [t] + good[k + 1:], ints)
    with pytest.raises(RuntimeError, match="flow_metrics"):
        nat.ops().flow_metrics(good, [B, 21, 37, 23, 41, 0])
    torch.cuda.synchronize()
    assert not acc.any()


# ---------------------------------------------------------------- evaluate on generated trees
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("val_trees_gpu")
    sintel, kitti = root / "Sintel", root / "KITTI"
    _make_sintel(str(sintel), scenes=2, frames=4, H=SINTEL[0], W=SINTEL[1])   # 6 pairs a pass
    write_kitti(kitti, KITTI_SIZES)
    return str(sintel), str(kitti)


@pytest.fixture(scope="module")
def model():
    return raft_small(seed=0)[0].cuda().eval()


def test_evaluate_equals_validate_sintel_gpu(trees, model):
    """Batches of 4 + a tail of 2, the final-flow plan on both sides: the engine is bitwise
    repeatable at a given plan, so the flows are the same and every count is equal."""
    dev = torch.device("cuda", torch.cuda.current_device())
    want = sintel_with_fp64_epe(model, trees[0], dev, iters=3, batch_size=4, return_all_iters=False)
    got = evaluate(model, "sintel-clean", trees[0], iters=3, batch=4)
    assert got["pairs"] == want["pairs"] == 6 and got["pixels"] == 6 * SINTEL[0] * SINTEL[1]
    assert all(got[k] == want[k] for k in ("1px", "3px", "5px"))
    assert close(got["epe"], want["epe64"], got["pixels"])
    # the validator's own epe sums each pair's fp32 array in fp32 first: see sintel_with_fp64_epe
    per_pair = SINTEL[0] * SINTEL[1]
    assert abs(got["epe"] - want["epe"]) <= (128 / 8 + math.log2(per_pair / 128)) * 2.0 ** -24 * want["epe"]
    tail = evaluate(model, "sintel-final", trees[0], iters=3, batch=4, max_pairs=5)
    assert tail["pairs"] == 5 and tail["pixels"] == 5 * per_pair and math.isfinite(tail["epe"])


def test_evaluate_equals_validate_kitti_gpu(trees, model):
    want = validate_kitti(model, trees[1], iters=3, verbose=False, return_all_iters=False)
    got = evaluate(model, "kitti", trees[1], iters=3)
    assert got["pairs"] == want["pairs"] == 3 and got["f1"] == want["f1"]
    assert close(got["epe_image_mean"], want["epe"], sum(h * w for h, w in KITTI_SIZES))


# ---------------------------------------------------------------- the trainer, fused path
def test_trainer_validates_without_changing_the_fused_run(tmp_path):
    data, ck = tmp_path / "chairs", tmp_path / "ck"
    data.mkdir()
    h, w = 128, 160
    write_chairs(data, 8, h + 8, w + 8)
    split = data / "FlyingChairs_train_val.txt"
    split.write_text("1\n1\n2\n1\n1\n2\n1\n1\n")
    base = dict(arch="raft_small", data=str(data), size=(h, w), batch=2, iters=2, steps=4, lr=2e-4, log_every=2,
                chairs_split=str(split))
    plain = Trainer(TrainConfig(**base))
    assert plain.device.type == "cuda" and len(plain.loader.ds) == 6
    plain.fit(log=lambda line: None)
    tr = Trainer(TrainConfig(**base, val=(f"chairs-val={data}",), val_every=2, val_iters=3, val_batch=2, ckpt_dir=str(ck)))
    logs = []
    tr.fit(log=logs.append)
    assert [e["step"] for e in tr.val_history] == [2, 4] and tr.skipped == plain.skipped == 0
    a, b = _state(plain), _state(tr)
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k].cpu(), b[k].cpu()
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8) if x.ndim else x, y.view(torch.uint8) if y.ndim else y), k
    logged = [json.loads(l)["val"] for l in logs if '"val":' in l]
    assert logged == [json.loads(l) for l in open(ck / "val.jsonl")] and logged[-1]["step"] == 4
    fresh = raft_small(weights=str(ck / "step_4.msgpack"))[0]
    again = evaluate(fresh, "chairs-val", str(data), iters=3, batch=2)
    last = logged[-1]["chairs-val"]
    assert again["pairs"] == last["pairs"] == 2 and all(again[k] == last[k] for k in ("1px", "3px", "5px", "f1", "pixels"))
    assert close(again["epe"], last["epe"], again["pixels"])
    plain.loader.close()
    tr.loader.close()
