"""Sparse ground truth on the GPU: the kernels of csrc/kernels/augment_sparse.hip bitwise against
the golden op (train/augment.py:augment_pairs_sparse) on samples of several sizes whose padding
would show if it were read, their launch builders' checks, the loader's upload path without host
synchronisation, the trainer and the KITTI validation on generated trees."""
import math

import numpy as np
import pytest
import torch

from jax_raft_amd.eval.kitti import kitti_metrics, validate_kitti
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import FlowPairs, PairLoader, SparseAugmentParams, augment_pairs_sparse, sample_sparse
from test_sparse import CASES, HB, SIZES, WB, bits, case_records, records, same, sparse_frames, write_kitti

pytestmark = pytest.mark.gpu

NAMES = ("image1", "image2", "flow", "valid")
_golden = {}


def golden(case):
    """The golden op's outputs, lander counts and dropped points of a case: computed once."""
    if case not in _golden:
        crop, rec = case_records(case)
        _golden[case] = augment_pairs_sparse(*sparse_frames(seed=7), rec, crop, return_landers=True)
    return _golden[case]


def run_kernels(case, frames=None):
    crop, rec = case_records(case)
    return nat.augment_pairs_sparse(*(t.cuda() for t in (frames or sparse_frames(seed=7))), rec, crop)


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_equals_golden_bitwise(case):
    want = golden(case)
    got = run_kernels(case)
    for name, g, w_ in zip(NAMES, got, want):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w_.shape, name
        print(f"{case}: {name} max |kernel - golden| = {float((g.cpu() - w_).abs().max()):.3g}")
        assert same(g.cpu(), w_), name
    flow, valid, landers, dropped = want[2], want[3], want[4], want[5]
    assert float(want[0].min()) >= -1 and float(want[0].max()) <= 1 and bool(torch.isfinite(flow).all())
    assert bool((valid == (landers > 0).float()).all()) and bool((flow[valid == 0] == 0).all())
    landed = int((landers > 0).sum())
    multi = int((landers >= 2).sum()) / max(landed, 1)
    print(f"{case}: {landed} landed cells of {landers.numel()}, {100 * multi:.0f} % with two or more landers, "
          f"dropped at X == Wr: {dropped}")
    assert 0 < landed < landers.numel() or case == "ratio4"
    # the cases are not vacuous: contested cells where the map shrinks, holes where it grows
    if case == "downscale":
        assert multi >= 0.25
    if case == "ratio4":
        assert multi >= 0.90 and sum(dropped) >= 1
    if case == "upscale":
        assert float(valid.mean()) <= 0.50


@pytest.mark.parametrize("fill", ["random", "all255"])
def test_sized_colour_sums_are_exact(fill):
    if fill == "random":
        i1, i2, _, _ = sparse_frames(seed=1)
        sizes = SIZES
    else:                                           # several blocks per sample; 255 everywhere, padding included
        sizes = [(130, 260), (127, 255)]
        i1 = torch.full((2, 130, 260, 3), 255, dtype=torch.uint8)
        i2 = torch.full_like(i1, 255)
        i2[1, 126, 254, 2] = 0
    rec = SparseAugmentParams.identity(sizes).packed().cuda()
    got = nat.augment_sums_sparse(i1.cuda(), i2.cuda(), rec)
    want = torch.stack([torch.stack([img[n, :Hs, :Ws].to(torch.int64).sum((0, 1)) for n, (Hs, Ws) in enumerate(sizes)])
                        for img in (i1, i2)])
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want)


def test_out_of_range_winners():
    """NaN, inf and 1000 or more among the winners: valid = 0 and flow 0, no fallback to another lander."""
    case = "downscale"
    crop, rec = case_records(case)
    i1, i2, flow, valid = sparse_frames(seed=7)
    clean = golden(case)
    g = torch.Generator().manual_seed(5)
    for n, (Hs, Ws) in enumerate(SIZES):
        on = (valid[n, :Hs, :Ws] != 0).nonzero()
        pick = on[torch.randperm(len(on), generator=g)[:120]]
        for k, bad in enumerate((float("nan"), float("inf"), -float("inf"), 1700.0, -2e3, 4e4)):
            for y, x in pick[k::6].tolist():
                flow[n, y, x, k % 2] = bad           # 1700 scales to 1013 .. 1103 by the ratios 0.596 .. 0.649
    want = augment_pairs_sparse(i1, i2, flow, valid, rec, crop)
    got = nat.augment_pairs_sparse(i1.cuda(), i2.cuda(), flow.cuda(), valid.cuda(), rec, crop)
    for name, g_, w_ in zip(NAMES, got, want):
        assert same(g_.cpu(), w_), name
    hit = (want[3] == 0) & (clean[3] == 1)          # cells whose winner went out of range
    assert all(int(hit[n].sum()) >= 10 for n in range(len(SIZES)))
    assert bool((got[2].cpu()[hit] == 0).all()) and bool(torch.isfinite(got[2]).all())
    assert same(got[0].cpu(), clean[0]) and same(got[1].cpu(), clean[1])       # the images do not change
    keep = want[3] == 1
    assert bool(keep.any()) and same(got[2].cpu()[keep], clean[2][keep])       # ... nor any other cell


def test_repeatable_and_ordered_across_streams():
    case = "downscale"
    crop, rec = case_records(case)
    frames = tuple(t.cuda() for t in sparse_frames(seed=7))
    first = nat.augment_pairs_sparse(*frames, rec, crop)
    second = nat.augment_pairs_sparse(*frames, rec, crop)
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))
    # the same sums buffer, dirty from the first stream, reused on a second one: the clear is in-stream
    packed = rec.packed().cuda()
    sums = nat.augment_sums_sparse(frames[0], frames[1], packed)
    want = sums.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nat.augment_sums_sparse(frames[0], frames[1], packed, out=sums)
        third = nat.augment_pairs_sparse(*frames, rec, crop)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(sums, want)
    for a, b in zip(first, third):
        assert torch.equal(bits(a), bits(b))
    assert all(same(a.cpu(), b) for a, b in zip(first, golden(case)))


def test_fetch_and_augment_do_not_synchronise(tmp_path):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    write_kitti(tmp_path, [(37, 52), (40, 49)] * 4)
    ld = PairLoader(FlowPairs.kitti(str(tmp_path)), batch=2, device="cuda")
    crop = (24, 32)

    def batch(step):
        *bufs, sizes = ld.fetch(step)
        params = sample_sparse(2, sizes, "kitti", crop, step=step)
        return bufs, params, nat.augment_pairs_sparse(*bufs, params, crop)

    for step in range(2):      # warm: staging buffers, allocator blocks, the library
        batch(step)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bufs, params, out = batch(2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = augment_pairs_sparse(*(t.cpu() for t in bufs), params, crop)
    ld.close()
    assert all(same(g.cpu(), w_) for g, w_ in zip(out, want))


def test_launch_builder_checks():
    B, Hb, Wb, h, w = 1, 16, 24, 8, 12
    dev = "cuda"
    i1 = torch.zeros(B, Hb, Wb, 3, dtype=torch.uint8, device=dev)
    i2 = torch.zeros_like(i1)
    flow = torch.zeros(B, Hb, Wb, 2, device=dev)
    vin = torch.ones(B, Hb, Wb, dtype=torch.uint8, device=dev)
    rec = SparseAugmentParams.identity([(Hb, Wb)]).packed().to(dev)
    sums = torch.zeros(2, B, 3, dtype=torch.int32, device=dev)
    o1, o2 = torch.zeros(B, h, w, 3, device=dev), torch.zeros(B, h, w, 3, device=dev)
    of, ov = torch.zeros(B, h, w, 2, device=dev), torch.zeros(B, h, w, device=dev)
    ints = [B, Hb, Wb, h, w]
    good = [i1, i2, flow, vin, rec, sums, o1, o2, of, ov]
    marker = 7.0
    for t in (o1, o2, of, ov):
        t.fill_(marker)

    def rejected(pos, bad, i=ints):
        t = list(good)
        t[pos] = bad
        with pytest.raises(RuntimeError, match="augment_sparse"):
            nat.ops().augment_sparse(t, i)

    wide = torch.zeros(B, Hb, 2 * Wb, 3, dtype=torch.uint8, device=dev)
    rejected(0, wide[:, :, :Wb])                                             # a non-contiguous image
    rejected(1, i2.float())                                                  # dtype of an image
    rejected(2, flow.double())                                               # dtype of the flow
    rejected(3, vin.float())                                                 # dtype of valid
    rejected(3, torch.ones(B, Hb, Wb + 1, dtype=torch.uint8, device=dev))    # size of valid
    rejected(4, rec.float())                                                 # dtype of the records
    rejected(4, rec[:, :48].contiguous())                                    # the dense record's size
    rejected(4, rec.cpu())                                                   # records on the host
    rejected(5, sums.long())                                                 # dtype of the sums
    rejected(6, flow.view(-1)[: B * h * w * 3].view(B, h, w, 3))             # an output aliasing an input
    rejected(7, o1)                                                          # an output aliasing another
    rejected(8, torch.zeros(B * h * w * 2 + 1, device=dev)[1:].view(B, h, w, 2))   # 4-byte aligned only
    rejected(9, torch.zeros(B, h, w + 1, device=dev))                        # size of an output
    rejected(6, o1, [B, Hb, Wb, 0, w])                                       # an empty crop
    with pytest.raises(RuntimeError, match="augment_sparse_sums"):
        nat.ops().augment_sparse_sums([i1, wide[:, :, :Wb], rec, sums], [B, Hb, Wb])
    with pytest.raises(RuntimeError, match="augment_sparse_sums"):
        nat.ops().augment_sparse_sums([i1, i2, rec[:, :48].contiguous(), sums], [B, Hb, Wb])
    with pytest.raises(RuntimeError, match="augment_sparse_sums"):
        nat.ops().augment_sparse_sums([i1, i2, rec, sums], [B, Hb, Wb + 1])
    for name, n in (("augment_sparse_sums", 3), ("augment_sparse", 5)):     # rows of the op table
        assert list(torch.ops.jax_raft_amd.op_arity(name)) == [1, n, n]
    # the front-end checks the records on the host: a shrink beyond 4, a sample beyond the buffer, a wrong dtype
    with pytest.raises(ValueError, match="shrinks an axis"):
        nat.augment_pairs_sparse(i1, i2, flow, vin, SparseAugmentParams.record((Hb, Wb), resized=(8, 5)), (h, 5))
    with pytest.raises(ValueError, match="does not fit the buffer"):
        nat.augment_pairs_sparse(i1, i2, flow, vin, SparseAugmentParams.record((Hb + 1, Wb)), (h, w))
    with pytest.raises(ValueError, match="uint8"):
        nat.augment_pairs_sparse(i1, i2, flow, vin.float(), SparseAugmentParams.identity([(Hb, Wb)]), (h, w))
    torch.cuda.synchronize()
    assert all(bool((t == marker).all()) for t in (o1, o2, of, ov))          # nothing was launched
    nat.ops().augment_sparse_sums([i1, i2, rec, sums], [B, Hb, Wb])
    nat.ops().augment_sparse(good, ints)                                     # ... and the good call is accepted
    torch.cuda.synchronize()
    assert bool((ov == 1).all()) and bool((o1 == -1).all()) and bool((of == 0).all())


def test_trainer_on_a_generated_kitti_tree_gpu(tmp_path):
    from jax_raft_amd.train.trainer import TrainConfig, Trainer

    h, w = 128, 160                                 # the smallest size the pyramid accepts
    sizes = [(136, 176), (132, 168)] * 4
    write_kitti(tmp_path, sizes)
    cfg = TrainConfig(arch="raft_small", data=str(tmp_path), dataset="kitti", stage="kitti", size=(h, w), batch=2, iters=3,
                      steps=2, lr=2e-4)
    tr = Trainer(cfg)
    assert tr.device.type == "cuda" and tr.loader.sparse
    losses = [float(tr.train_step(tr.batch_for(s))["loss"]) for s in range(2)]
    tr.flush()
    assert all(math.isfinite(v) for v in losses) and tr.skipped == 0
    ds = FlowPairs.kitti(str(tmp_path))
    got = tr.batch_for(1)
    idx = tr.loader.indices_for(1)
    i1, i2 = (torch.full((2, 136, 176, 3), 255, dtype=torch.uint8) for _ in range(2))
    fl, va = torch.full((2, 136, 176, 2), 3e4), torch.ones((2, 136, 176), dtype=torch.uint8)
    for n, i in enumerate(idx):                     # the same samples in buffers with other padding
        Hs, Ws = sizes[i]
        for buf, arr in zip((i1, i2, fl, va), ds[i]):
            buf[n, :Hs, :Ws] = torch.from_numpy(arr)
    params = sample_sparse(2, [sizes[i] for i in idx], "kitti", (h, w), seed=cfg.seed, step=1, rank=0)
    want = augment_pairs_sparse(i1, i2, fl, va, params, (h, w))
    assert all(g.is_cuda and same(g.cpu(), w_) for g, w_ in zip(got, want))
    tr.loader.close()


def test_validate_kitti_gpu(tmp_path):
    from jax_raft_amd import raft_small

    truth = write_kitti(tmp_path, [(136, 176), (132, 168)])
    model, _ = raft_small(seed=0)
    res = validate_kitti(model, str(tmp_path), iters=3, verbose=False)
    assert math.isfinite(res["epe"]) and math.isfinite(res["f1"]) and res["pairs"] == 2
    model = model.cuda().eval()
    epes, out, n = [], 0.0, 0
    with torch.no_grad():
        for a, b, gt, valid in truth:
            flow = model(torch.from_numpy(a)[None].cuda(), torch.from_numpy(b)[None].cuda(), num_flow_updates=3)[-1]
            m = kitti_metrics(flow[0].float().cpu().numpy(), gt, valid)
            epes.append(m["epe"])
            out += m["f1"] / 100 * int(valid.sum())
            n += int(valid.sum())
    # RAFT's protocol: the mean of the per-image EPE, F1 over all valid pixels of the split
    assert res["epe"] == pytest.approx(float(np.mean(epes)), rel=1e-6)
    assert res["f1"] == pytest.approx(100 * out / n, rel=1e-6)
