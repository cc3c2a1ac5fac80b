"""Validation during training on the CPU: the golden metrics op (eval/metrics.py) against the
numpy code of the stand-alone validators, its boundary pixels, the held-out FlyingChairs split,
the streaming ``evaluate`` against ``validate_sintel`` / ``validate_kitti`` on generated trees, and
the trainer's in-loop validation, which must not change the run.

The bound on sums: two fp64 summation orders of N non-negative terms differ by at most
2 * N * 2^-53 relative (:func:`close`); it is derived, not measured.

The generated frames are 128 x 136 and larger, not smaller: the correlation pyramid refuses
feature maps below 16 x 16, i.e. frames below 128 x 128 (models/reference.py:build_pyramid)."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from jax_raft_amd import flow_metrics, metrics_from, raft_small
from jax_raft_amd.eval.kitti import _pair_sums, validate_kitti
from jax_raft_amd.eval.sintel import epe_metrics, validate_sintel
from jax_raft_amd.eval.validate import evaluate
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import FlowPairs
from jax_raft_amd.train.trainer import TrainConfig, Trainer
from test_augment import write_chairs
from test_eval import _make_sintel
from test_sparse import write_kitti
from test_train import _free_port

F32 = np.float32
SINTEL = (128, 136)
KITTI_SIZES = ((132, 140), (129, 137), (132, 140))
CPU = torch.device("cpu")


def close(a, b, n):
    """|a - b| within the summation-order bound of ``n`` terms; NaN equals NaN."""
    a, b = float(a), float(b)
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= 2.0 * n * 2.0 ** -53 * max(abs(a), abs(b))


# ---------------------------------------------------------------- boundary pixels
def _d2(dx, dy):
    dx, dy = F32(dx), F32(dy)
    return F32(F32(dx * dx) + F32(dy * dy))


def find_offset(target):
    """(dx, dy) fp32 with fl(fl(dx * dx) + fl(dy * dy)) == target bit for bit."""
    target = F32(target)
    dx = F32(np.sqrt(target) * F32(0.8))
    for _ in range(4096):
        a = F32(dx * dx)
        dy = np.sqrt(F32(target - a), dtype=F32)
        for cand in (dy, np.nextafter(dy, F32(0)), np.nextafter(dy, F32(9))):
            if _d2(dx, cand) == target:
                return F32(dx), F32(cand)
        dx = np.nextafter(dx, F32(0))
    raise AssertionError(f"no (dx, dy) for {target!r}")


def boundary_case():
    """pred, gt (3, 4, 6, 2), valid (3, 4, 6) and the table of sample 0's pixels: sample 0 holds the
    boundary pixels, sample 1 no valid pixel, sample 2 one NaN prediction among valid pixels."""
    up, down = lambda v: np.nextafter(F32(v), F32(np.inf)), lambda v: np.nextafter(F32(v), F32(0))
    px = []   # (name, pred, gt, valid byte)
    for t in (1, 9, 25):
        for name, tgt in ((f"below{t}", down(t)), (f"at{t}", F32(t)), (f"above{t}", up(t))):
            px.append((name, find_offset(tgt), (F32(0), F32(0)), 1 if len(px) % 2 else 255))
    px.append(("ratio_exact", (F32(3), F32(60)), (F32(0), F32(60)), 1))          # epe == 3, |gt| == 60
    px.append(("ratio_above", (up(3), F32(60)), (F32(0), F32(60)), 255))         # the next float up
    px.append(("mag0_far", (F32(4), F32(0)), (F32(0), F32(0)), 1))
    px.append(("both0", (F32(0), F32(0)), (F32(0), F32(0)), 1))
    px.append(("masked_below1", find_offset(down(1)), (F32(0), F32(0)), 0))      # valid byte 0: not counted
    px.append(("masked_far", (F32(100), F32(0)), (F32(0), F32(0)), 0))
    pred, gt = np.zeros((3, 4, 6, 2), F32), np.zeros((3, 4, 6, 2), F32)
    valid = np.zeros((3, 4, 6), np.uint8)
    for k, (_, p, g, v) in enumerate(px):
        pred[0, k // 6, k % 6], gt[0, k // 6, k % 6], valid[0, k // 6, k % 6] = p, g, v
    rng = np.random.default_rng(3)
    pred[1], gt[1] = rng.standard_normal((2, 4, 6, 2)).astype(F32) * 4       # valid[1] stays 0
    pred[2], gt[2] = rng.standard_normal((2, 4, 6, 2)).astype(F32) * 4
    valid[2] = rng.integers(0, 2, (4, 6)) * 255
    valid[2, 1, 2] = 1
    pred[2, 1, 2, 0] = np.nan
    return torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(valid), px


def numpy_rows(pred, gt, valid, sizes):
    """The rows by the definition, in numpy (independent of the torch golden op)."""
    rows = []
    for n, (h, w) in enumerate(sizes):
        p, g = pred[n, :h, :w].numpy(), gt[n, :h, :w].numpy()
        on = np.ones((h, w), bool) if valid is None else valid[n, :h, :w].numpy() != 0
        d = p - g
        epe = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])[on]
        mag = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1])[on]
        with np.errstate(divide="ignore", invalid="ignore"):
            out = (epe > 3) & (epe.astype(np.float64) / mag.astype(np.float64) > 0.05)
        rows.append([epe.astype(np.float64).sum(), on.sum(), (epe < 1).sum(), (epe < 3).sum(), (epe < 5).sum(), out.sum()])
    return np.array(rows, np.float64)


def assert_rows(got, want, sizes):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape
    assert np.array_equal(got[:, 1:], want[:, 1:])                            # the counts: exact
    for n, (h, w) in enumerate(sizes):
        assert close(got[n, 0], want[n, 0], h * w), (n, got[n, 0], want[n, 0])


def test_boundary_construction_and_flags():
    pred, gt, valid, px = boundary_case()
    by = {name: (p, g) for name, p, g, _ in px}
    for t, below_is_less in ((1, True), (9, True), (25, False)):
        for name, tgt in ((f"below{t}", np.nextafter(F32(t), F32(0))), (f"at{t}", F32(t)),
                          (f"above{t}", np.nextafter(F32(t), F32(np.inf)))):
            d2 = _d2(*by[name][0])
            assert d2.view(np.uint32) == F32(tgt).view(np.uint32), name      # the construction itself
        root = np.sqrt(np.nextafter(F32(t), F32(0)), dtype=F32)
        assert (root < F32(math.sqrt(t))) == below_is_less                   # the float below 25 has the square root 5.0
    rows, acc = flow_metrics(pred, gt, valid)
    want = numpy_rows(pred, gt, valid, [(4, 6)] * 3)
    assert_rows(rows, want, [(4, 6)] * 3)
    # sample 0 by hand.  counted: 9 boundary pixels + ratio_exact, ratio_above, mag0_far, both0
    #  < 1: below1, both0 | < 3: those, at1, above1, below9 | < 5: those, at9, above9, ratio_exact, ratio_above, mag0_far
    #  outliers: above9, below25, at25, above25 (|gt| == 0, epe > 3), ratio_above, mag0_far; ratio_exact is none
    assert rows[0, 1:].tolist() == [13.0, 2.0, 5.0, 10.0, 6.0]
    assert rows[1].tolist() == [0.0] * 6                                     # no valid pixel
    assert math.isnan(float(rows[2, 0])) and rows[2, 1] == float((valid[2] != 0).sum())
    assert acc[7] == 3.0 and math.isnan(float(acc[0])) and math.isnan(float(acc[6]))
    # without the NaN sample: the image mean counts the empty sample as 0, and it is an image
    rows2, acc2 = flow_metrics(pred[:2], gt[:2], valid[:2])
    assert acc2[7] == 2.0 and close(acc2[6], rows2[0, 0] / 13.0, 24) and metrics_from(acc2)["pixels"] == 13


def test_golden_op_equals_the_validators_numpy_code():
    g = torch.Generator().manual_seed(5)
    pred, gt = torch.randn(3, 21, 37, 2, generator=g) * 4, torch.randn(3, 23, 41, 2, generator=g) * 30
    gt[0, :4] = 0                                                            # |gt| == 0 rows
    valid = (torch.rand(3, 23, 41, generator=g) < 0.6).to(torch.uint8) * 255
    sizes = [(21, 37), (20, 33), (9, 5)]
    rows, acc = flow_metrics(pred, gt, valid, sizes)
    assert_rows(rows, numpy_rows(pred, gt, valid, sizes), sizes)
    for n, (h, w) in enumerate(sizes):
        s = _pair_sums(pred[n, :h, :w].numpy(), gt[n, :h, :w].numpy(), valid[n, :h, :w].numpy())
        assert rows[n, 1] == s[2] and rows[n, 5] == s[1] and close(rows[n, 0], s[0], h * w)
    assert acc[7] == 3 and torch.equal(acc[1:6], rows[:, 1:].sum(0))
    # dense: metrics_from against eval.sintel.epe_metrics
    rows, acc = flow_metrics(pred[:, :, :, :], gt[:, :21, :37].contiguous())
    epe = np.sqrt(((pred.numpy() - gt[:, :21, :37].numpy()) ** 2).sum(-1)).reshape(-1)
    want, got = epe_metrics(epe), metrics_from(acc)
    assert all(got[k] == want[k] for k in ("1px", "3px", "5px")) and got["pixels"] == epe.size
    # the validator's mean is fp32 pairwise; its own error against an exact sum is far below fp32's eps
    assert abs(got["epe"] - want["epe"]) <= 1e-6 * want["epe"]
    assert close(got["epe"], epe.astype(np.float64).mean(), epe.size)


def test_nothing_outside_a_sample_is_read():
    g = torch.Generator().manual_seed(6)
    pred, gt = torch.randn(2, 9, 11, 2, generator=g), torch.randn(2, 12, 13, 2, generator=g)
    valid = (torch.rand(2, 12, 13, generator=g) < 0.5).to(torch.uint8)
    sizes = [(9, 11), (5, 7)]
    base = flow_metrics(pred, gt, valid, sizes)
    p2, g2, v2 = pred.clone(), gt.clone(), valid.clone()
    p2[1, 5:], p2[1, :, 7:], g2[:, 9:], g2[:, :, 11:], g2[1, 5:], g2[1, :, 7:] = (float("nan"),) * 6
    v2[:, 9:], v2[:, :, 11:], v2[1, 5:], v2[1, :, 7:] = (255,) * 4
    other = flow_metrics(p2, g2, v2, sizes)
    assert all(torch.equal(a, b) for a, b in zip(base, other))


def test_accumulation_and_host_checks():
    g = torch.Generator().manual_seed(7)
    pred, gt = torch.randn(5, 16, 20, 2, generator=g) * 3, torch.randn(5, 16, 20, 2, generator=g) * 3
    valid = (torch.rand(5, 16, 20, generator=g) < 0.7).to(torch.uint8)
    _, whole = flow_metrics(pred, gt, valid)
    _, acc = flow_metrics(pred[:2], gt[:2], valid[:2])
    rows, again = flow_metrics(pred[2:], gt[2:], valid[2:], acc=acc)
    assert again is acc and rows.shape == (3, 6)
    assert torch.equal(acc[1:6], whole[1:6]) and acc[7] == whole[7] == 5
    assert close(acc[0], whole[0], 5 * 320) and close(acc[6], whole[6], 5 * 320)
    for bad in (dict(sizes=[(17, 20)] * 5), dict(sizes=[(16, 21)] * 5), dict(sizes=[(16, 20)] * 4),
                dict(sizes=[(0, 20)] * 5), dict(acc=torch.zeros(8)), dict(acc=torch.zeros(6, dtype=torch.float64))):
        with pytest.raises(ValueError):
            flow_metrics(pred, gt, valid, **bad)
    for args in ((pred.double(), gt, valid), (pred, gt, valid.bool()), (pred, gt[:4], valid[:4]), (pred[..., :1], gt, valid)):
        with pytest.raises(ValueError):
            nat.flow_metrics(*args)


# ---------------------------------------------------------------- the chairs split
def test_chairs_split(tmp_path):
    root = tmp_path / "data"
    root.mkdir()
    write_chairs(root, 6, 16, 24)
    full = FlowPairs.chairs(str(root)).items
    with pytest.raises(FileNotFoundError) as e:
        FlowPairs.chairs(str(root), "validation")
    assert "FlyingChairs_train_val.txt" in str(e.value) and "chairs_split.txt" in str(e.value)
    (tmp_path / "chairs_split.txt").write_text("1\n2\n1\n1\n2\n1\n")        # found in the parent
    tr, va = FlowPairs.chairs(str(root), "training").items, FlowPairs.open(str(root), "chairs-val").items
    assert va == [full[1], full[4]] and tr == [full[0], full[2], full[3], full[5]]
    assert FlowPairs.open(str(root), "chairs-train").items == tr
    assert not set(tr) & set(va) and sorted(tr + va) == full
    assert FlowPairs.chairs(str(root)).items == full and FlowPairs.open(str(root), "chairs").items == full
    (root / "FlyingChairs_train_val.txt").write_text("2 1 1 1 1 1")         # the first name in root wins
    assert FlowPairs.chairs(str(root), "validation").items == [full[0]]
    own = tmp_path / "own.txt"
    for text in ("1\n2\n1\n", "1\n2\n1\n1\n3\n1\n", "1\n2\n1\n1\nx\n1\n"):
        own.write_text(text)
        with pytest.raises(ValueError, match="own.txt"):
            FlowPairs.chairs(str(root), "training", str(own))
    with pytest.raises(FileNotFoundError, match="missing.txt"):
        FlowPairs.chairs(str(root), "training", str(tmp_path / "missing.txt"))
    with pytest.raises(ValueError):
        FlowPairs.chairs(str(root), "test")


def test_sequential_loader_order_tail_and_ranks(tmp_path):
    from jax_raft_amd.train import SequentialLoader
    from jax_raft_amd.train.datasets import decode_threads

    truth = write_chairs(tmp_path, 5, 16, 24)
    ds = FlowPairs.chairs(str(tmp_path))
    ld = SequentialLoader(ds, batch=2)
    assert ld.batches == [[0, 1], [2, 3], [4]] and len(ld) == 3 and ld.pairs == 5     # the tail is kept
    assert ld._pool._max_workers <= decode_threads()
    seen = []
    for i1, i2, flow, valid, idx in ld:
        assert valid is None and i1.dtype == torch.uint8 and i1.shape == (len(idx), 16, 24, 3) and flow.shape == (len(idx), 16, 24, 2)
        for n, i in enumerate(idx):
            a, b, f = truth[i]
            assert np.array_equal(i1[n].numpy(), a) and np.array_equal(i2[n].numpy(), b) and np.array_equal(flow[n].numpy(), f)
        seen += idx
    ld.close()
    assert seen == [0, 1, 2, 3, 4]
    odd = SequentialLoader(ds, batch=4, rank=1, world=2, max_pairs=4)
    assert odd.batches == [[1, 3]] and odd.pairs == 4
    odd.close()
    kroot = tmp_path / "kitti"
    ktruth = write_kitti(kroot, [(20, 30), (20, 30), (18, 28)])
    kl = SequentialLoader(FlowPairs.kitti(str(kroot)), batch=4)
    assert kl.batches == [[0], [1], [2]]                                              # a sparse list runs batch 1
    for (i1, i2, flow, valid, idx), (a, b, f, v) in zip(kl, ktruth):
        assert i1.shape == (1,) + a.shape and np.array_equal(i1[0].numpy(), a) and np.array_equal(i2[0].numpy(), b)
        assert np.array_equal(flow[0].numpy(), f) and np.array_equal(valid[0].numpy(), v)
    kl.close()


# ---------------------------------------------------------------- evaluate on generated trees
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = tmp_path_factory.mktemp("val_trees")
    sintel, kitti = root / "Sintel", root / "KITTI"
    _make_sintel(str(sintel), scenes=2, frames=4, H=SINTEL[0], W=SINTEL[1])   # 6 pairs a pass
    write_kitti(kitti, KITTI_SIZES)
    return str(sintel), str(kitti)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return raft_small(seed=0)[0].eval()


class Recorder:
    """A model as the validators call it that keeps the final flow of every forward."""

    def __init__(self, model):
        self.model, self.flows = model, []

    def to(self, device):
        self.model = self.model.to(device)
        return self

    def eval(self):
        self.model.eval()
        return self

    def __call__(self, *args, **kw):
        out = self.model(*args, **kw)
        self.flows.append(out[-1].float().cpu().clone())
        return out


def sintel_with_fp64_epe(model, root, device, **kw):
    """``validate_sintel`` of the clean pass, plus ``epe64``: the EPE of the very flows it saw, summed
    in fp64.  The validator itself adds each pair's fp32 ``epe`` array in fp32 (numpy's pairwise sum,
    blocks of 128 in 8 lanes) before it accumulates in fp64, so its ``epe`` carries an error of its own of
    up to about (128 / 8 + log2(pixels / 128)) * 2^-24 relative; the bound on fp64 summation orders
    applies to ``epe64``.  The frame size is a multiple of 8, so no flow is padded."""
    from jax_raft_amd.eval.sintel import MpiSintel

    rec = Recorder(model)
    res = validate_sintel(rec, root, dstypes=("clean",), device=device, verbose=False, **kw)["clean"]
    ds = MpiSintel(root, "training", "clean")
    flows = np.concatenate([f.numpy() for f in rec.flows])
    total = 0.0
    for i, f in enumerate(flows):
        total += np.sqrt(((f - ds[i][2]) ** 2).sum(-1)).astype(np.float64).sum()
    res["epe64"] = total / flows[..., 0].size
    return res


@pytest.fixture(scope="module")
def sintel_reference(trees, model):
    """validate_sintel on the clean pass, batches of 4 (4 + a tail of 2) and the first 3 pairs: computed once."""
    return {n: sintel_with_fp64_epe(model, trees[0], CPU, iters=2, batch_size=4, max_pairs=n) for n in (None, 3)}


def assert_like_sintel(got, want, pairs):
    assert got["pairs"] == want["pairs"] == pairs and got["pixels"] == pairs * SINTEL[0] * SINTEL[1]
    assert all(got[k] == want[k] for k in ("1px", "3px", "5px"))
    assert close(got["epe"], want["epe64"], got["pixels"])
    per_pair = SINTEL[0] * SINTEL[1]
    assert abs(got["epe"] - want["epe"]) <= (128 / 8 + math.log2(per_pair / 128)) * 2.0 ** -24 * want["epe"]


def test_evaluate_equals_validate_sintel_cpu(trees, model, sintel_reference):
    got = evaluate(model, "sintel-clean", trees[0], iters=2, batch=4, device=CPU)
    assert_like_sintel(got, sintel_reference[None], 6)
    assert got["world"] == 1 and got["seconds"] > 0 and model.training is False
    assert_like_sintel(evaluate(model, "sintel-clean", trees[0], iters=2, batch=4, max_pairs=3, device=CPU),
                       sintel_reference[3], 3)
    with pytest.raises(ValueError):
        evaluate(model, "things", trees[0], device=CPU)


def test_evaluate_equals_validate_kitti_cpu(trees, model):
    want = validate_kitti(model, trees[1], iters=2, device=CPU, verbose=False)
    got = evaluate(model, "kitti", trees[1], iters=2, device=CPU)
    assert got["pairs"] == want["pairs"] == 3 and got["f1"] == want["f1"]     # outliers / valid pixels: counts
    assert close(got["epe_image_mean"], want["epe"], sum(h * w for h, w in KITTI_SIZES))
    two = evaluate(model, "kitti", trees[1], iters=2, max_pairs=2, device=CPU)
    assert two["pairs"] == 2 and two["f1"] == validate_kitti(model, trees[1], iters=2, device=CPU, verbose=False, max_pairs=2)["f1"]


def _rank_worker(rank, world, port, root, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    res = evaluate(raft_small(seed=0)[0].eval(), "sintel-clean", root, iters=2, batch=1, max_pairs=5, device=CPU)
    if rank == 0:
        with open(out, "w") as f:
            json.dump(res, f)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_evaluate_two_gloo_ranks_equal_one(trees, tmp_path):
    """Ranks 0 / 1 take pairs 0, 2, 4 / 1, 3 of the first 5, one pair per forward; one rank runs the
    same forwards one after the other, so the flows -- and with them every count -- are the same."""
    out = str(tmp_path / "r.json")
    mp.spawn(_rank_worker, args=(2, _free_port(), trees[0], out), nprocs=2, join=True)
    got = json.load(open(out))
    want = evaluate(raft_small(seed=0)[0].eval(), "sintel-clean", trees[0], iters=2, batch=1, max_pairs=5, device=CPU)
    assert got["world"] == 2 and want["world"] == 1 and got["pairs"] == want["pairs"] == 5
    assert all(got[k] == want[k] for k in ("1px", "3px", "5px", "f1", "pixels"))
    assert close(got["epe"], want["epe"], got["pixels"]) and close(got["epe_image_mean"], want["epe_image_mean"], got["pixels"])


# ---------------------------------------------------------------- the trainer
def _state(tr):
    out = {"p." + n: p.detach().clone() for n, p in tr.model.named_parameters()}
    out.update({"b." + n: b.detach().clone() for n, b in tr.model.named_buffers()})
    for k, st in tr.opt.state_dict()["state"].items():
        out.update({f"o.{k}.{n}": (v.detach().clone() if isinstance(v, torch.Tensor) else torch.tensor(v)) for n, v in st.items()})
    out["lr"] = torch.tensor(tr.sched.get_last_lr())
    return out


def test_trainer_validates_without_changing_the_run(tmp_path):
    data, ck = tmp_path / "chairs", tmp_path / "ck"
    data.mkdir()
    write_chairs(data, 6, 136, 144)
    (data / "FlyingChairs_train_val.txt").write_text("1\n1\n2\n1\n1\n2\n")
    base = dict(arch="raft_small", data=str(data), size=(128, 128), batch=1, iters=1, steps=6, log_every=3,
                chairs_split=str(data / "FlyingChairs_train_val.txt"))
    plain = Trainer(TrainConfig(**base), device=CPU)
    assert len(plain.loader.ds) == 4                                          # the label-2 pairs are gone
    assert plain.loader.ds.items == FlowPairs.chairs(str(data), "training").items
    logs = []
    plain.fit(log=logs.append)
    assert plain.val_history == [] and not any("val" in line for line in logs)
    tr = Trainer(TrainConfig(**base, val=(f"chairs-val={data}",), val_every=2, val_iters=1, val_batch=2,
                             ckpt_dir=str(ck)), device=CPU)
    logs = []
    tr.fit(log=logs.append)
    assert [e["step"] for e in tr.val_history] == [2, 4, 6]
    lines = [json.loads(l) for l in open(ck / "val.jsonl")]
    assert lines == json.loads(json.dumps(tr.val_history))
    logged = [json.loads(l)["val"] for l in logs if '"val":' in l]
    assert logged == lines and all(e["chairs-val"]["pairs"] == 2 and e["chairs-val"]["pixels"] == 2 * 136 * 144 for e in lines)
    periodic = [json.loads(l) for l in logs if '"val":' not in l]
    assert [p["step"] for p in periodic] == [3, 6] and all(p["val_s"] >= 0 for p in periodic)
    a, b = _state(plain), _state(tr)
    assert a.keys() == b.keys() and len(a) > 100
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8) if a[k].ndim else a[k], b[k].view(torch.uint8) if b[k].ndim else b[k]), k
    assert tr.loader.indices_for(6) == plain.loader.indices_for(6)
    # the metrics of step 6 are those of the saved weights
    fresh = raft_small(weights=str(ck / "step_6.msgpack"))[0]
    again = evaluate(fresh, "chairs-val", str(data), iters=1, batch=2, device=CPU)
    assert all(again[k] == lines[-1]["chairs-val"][k] for k in ("1px", "3px", "5px", "f1", "pixels"))
    assert close(again["epe"], lines[-1]["chairs-val"]["epe"], again["pixels"])
    assert json.load(open(ck / "latest.json"))["config"]["val_every"] == 2
    plain.loader.close()
    tr.loader.close()


def test_trainer_refusals(tmp_path):
    with pytest.raises(ValueError, match="training data"):
        TrainConfig(data=str(tmp_path), dataset="chairs", val=(f"chairs-val={tmp_path}",))
    TrainConfig(data=str(tmp_path), dataset="chairs", val=(f"chairs-val={tmp_path}",), chairs_split="split.txt")
    with pytest.raises(ValueError, match="name=root"):
        TrainConfig(val=("things=/x",))
    with pytest.raises(ValueError, match="name=root"):
        TrainConfig(val=("kitti",))
    with pytest.raises(ValueError, match="graph_step"):
        TrainConfig(val=(f"kitti={tmp_path}",), graph_step=True)
    with pytest.raises(NotImplementedError, match="cp_group"):
        evaluate(raft_small(seed=0)[0], "kitti", str(tmp_path), device=CPU, cp_group=object())
    cfg = TrainConfig()
    assert (cfg.val, cfg.val_every, cfg.val_iters, cfg.val_batch, cfg.val_max_pairs, cfg.chairs_split) == ((), 0, 0, 4, None, None)


def test_cli_config(tmp_path):
    import argparse

    from jax_raft_amd.train import trainer as T

    ns = argparse.Namespace(**{**TrainConfig().__dict__, "mix": None, "val": f"kitti={tmp_path},sintel-clean={tmp_path}",
                               "val_max_pairs": "5"})
    del ns.mix_weights
    cfg = T.config_from_args(ns)
    assert cfg.val == (f"kitti={tmp_path}", f"sintel-clean={tmp_path}") and cfg.val_max_pairs == 5
