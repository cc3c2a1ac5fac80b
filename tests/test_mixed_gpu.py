"""Dense and sparse samples in one batch on the GPU: the kernels of csrc/kernels/augment_mixed.hip
bitwise against the golden op (train/augment.py:augment_pairs_mixed) on packed slots whose padding
would show if it were read, against the dense and the sparse kernels on batches of one kind, their
launch builders' checks, the loader's prefix uploads without host synchronisation, and the trainer
on a generated five-part tree."""
import math

import pytest
import torch

from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import (AugmentParams, FlowPairs, MixedAugmentParams, PairLoader, SparseAugmentParams,
                                augment_pairs_mixed, augment_pairs_sparse, sample_mixed)
from test_mixed import (CROPS, DENSE, S_SLOT, mixed_records, packed_frames, sizes_for, write_mix)
from test_sparse import bits, same

pytestmark = pytest.mark.gpu

NAMES = ("image1", "image2", "flow", "valid")
_golden = {}


def golden(crop):
    """The golden op's outputs at ``crop``: computed once."""
    if crop not in _golden:
        _golden[crop] = augment_pairs_mixed(*packed_frames(sizes_for(crop)), mixed_records(crop), crop)
    return _golden[crop]


@pytest.mark.parametrize("crop", CROPS)
def test_kernel_equals_golden_bitwise(crop):
    """Slot 24 x 40, batch 4: dense 20x33 -> 27x41 (both flips, two rectangles, asymmetric colour), sparse
    24x40 -> 19x32 (h-flip), sparse 17x29 -> 21x36, dense identity 13x19 at origin (1, 1) (13x21 at the crop
    of width 20, which 13x19 cannot hold); crop widths 18 (the scalar tail) and 20."""
    sizes, rec = sizes_for(crop), mixed_records(crop)
    frames = packed_frames(sizes)
    # the preconditions: contested cells where the sparse map shrinks, holes where it grows, flow out of range
    for n, need in ((1, "multi"), (2, "empty")):
        Hs, Ws = sizes[n]
        N = Hs * Ws
        one = augment_pairs_sparse(*(t[n, :N].reshape(1, Hs, Ws, -1) for t in frames[:3]), frames[3][n, :N].reshape(1, Hs, Ws),
                                   rec.part(n), crop, return_landers=True)
        landers = one[4]
        assert int((landers >= 2).sum()) >= 1 if need == "multi" else int((landers == 0).sum()) >= 1, (n, need)
    for n in (0, 1):
        N = sizes[n][0] * sizes[n][1]
        assert int(torch.isnan(frames[2][n, :N]).sum()) == 1 and int((frames[2][n, :N] > 1000).sum()) == 1
    want = golden(crop)
    got = nat.augment_pairs_mixed(*(t.cuda() for t in frames), rec, crop)
    for name, g, w_ in zip(NAMES, got, want):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w_.shape, name
        print(f"{crop}: {name} max |kernel - golden| = {float((g.cpu() - w_).abs().max()):.3g}")
        assert same(g.cpu(), w_), name
    assert bool(torch.isfinite(want[2]).all()) and bool((want[2][want[3] == 0] == 0).all())
    assert float(want[3][0].mean()) < 1 and float(want[3][3].mean()) == 1      # the NaN / 1700 of sample 0 reach its crop


def test_padding_is_never_read():
    crop = CROPS[0]
    rec = mixed_records(crop)
    a = nat.augment_pairs_mixed(*(t.cuda() for t in packed_frames(pad=(0x00, 0.0))), rec, crop)
    b = nat.augment_pairs_mixed(*(t.cuda() for t in packed_frames(pad=(0xFF, float("nan")))), rec, crop)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(bits(x), bits(y)), name
    assert all(same(x.cpu(), w_) for x, w_ in zip(a, golden(crop)))


def test_agrees_with_the_sparse_and_the_dense_kernels():
    crop = (12, 18)
    # all sparse: the same samples in the padded layout through augment_sparse.hip
    sizes = [(24, 40), (17, 29), (22, 31)]
    kw = [dict(resized=(19, 32), origin=(2, 4), hflip=True), dict(resized=(21, 36), origin=(1, 3)), dict(origin=(5, 7))]
    i1, i2, fl, va = packed_frames(sizes, [False] * 3, bad=False)
    mixed = MixedAugmentParams.cat([MixedAugmentParams.record(s, False, **k) for s, k in zip(sizes, kw)])
    got = nat.augment_pairs_mixed(i1.cuda(), i2.cuda(), fl.cuda(), va.cuda(), mixed, crop)
    p1, p2 = (torch.full((3, 24, 40, 3), 255, dtype=torch.uint8) for _ in range(2))
    pf, pv = torch.full((3, 24, 40, 2), 3e4), torch.ones((3, 24, 40), dtype=torch.uint8)
    for n, (Hs, Ws) in enumerate(sizes):
        for dst, src in ((p1, i1), (p2, i2), (pf, fl), (pv, va)):
            dst[n, :Hs, :Ws] = src[n, :Hs * Ws].reshape((Hs, Ws) + tuple(src.shape[2:]))
    sparse = SparseAugmentParams.cat([SparseAugmentParams.record(s, **k) for s, k in zip(sizes, kw)])
    want = nat.augment_pairs_sparse(p1.cuda(), p2.cuda(), pf.cuda(), pv.cuda(), sparse, crop)
    assert all(torch.equal(bits(g), bits(w_)) for g, w_ in zip(got, want))
    assert 0 < float(got[3].mean()) < 1
    # all dense, one size: augment.hip; the slot is exactly the frame
    src = (20, 33)
    kw = [dict(resized=(27, 41), origin=(3, 5), hflip=True, vflip=True, rects=[(4, 3, 15, 11)]), dict(origin=(1, 1))]
    i1, i2, fl, va = packed_frames([src] * 2, [True] * 2, slot=20 * 33, bad=False)
    mixed = MixedAugmentParams.cat([MixedAugmentParams.record(src, True, **k) for k in kw])
    got = nat.augment_pairs_mixed(i1.cuda(), i2.cuda(), fl.cuda(), va.cuda(), mixed, crop)
    dense = AugmentParams.cat([AugmentParams.record(src, **k) for k in kw])
    want = nat.augment_pairs(i1.view(2, 20, 33, 3).cuda(), i2.view(2, 20, 33, 3).cuda(), fl.view(2, 20, 33, 2).cuda(), dense, crop)
    assert all(torch.equal(bits(g), bits(w_)) for g, w_ in zip(got, want))
    # a batch of one sample
    for dense_one in (True, False):
        f1 = packed_frames([(20, 33)], [dense_one], bad=False)
        r1 = MixedAugmentParams.record((20, 33), dense_one, resized=(16, 30), origin=(2, 5))
        got = nat.augment_pairs_mixed(*(t.cuda() for t in f1), r1, crop)
        assert all(same(g.cpu(), w_) for g, w_ in zip(got, augment_pairs_mixed(*f1, r1, crop)))


def test_sums_cover_each_sample_s_packed_pixels():
    sizes = [(130, 260), (127, 255), (3, 5)]       # several blocks per sample; 255 everywhere, padding included
    S = 130 * 260
    i1 = torch.full((3, S, 3), 255, dtype=torch.uint8)
    i2 = torch.full_like(i1, 255)
    i2[1, 127 * 255 - 1, 2] = 0
    rec = MixedAugmentParams.identity(sizes, [True, False, True]).packed().cuda()
    got = nat.augment_sums_mixed(i1.cuda(), i2.cuda(), rec)
    want = torch.stack([torch.stack([img[n, :Hs * Ws].to(torch.int64).sum(0) for n, (Hs, Ws) in enumerate(sizes)])
                        for img in (i1, i2)])
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want)


def test_the_three_sums_agree_across_a_block_boundary():
    """A sums block covers 4096 pixels: 70 x 61 = 4270 is two blocks with a ragged second one, and the second block
    of 3 x 5 returns early.  Dense (each sample a batch of one), sparse ((70, 61) buffers, padding 255) and mixed
    (slots of 4270 pixels, tails 255) all give the int64 sums of the host."""
    sizes = [(70, 61), (3, 5)]
    Hb, Wb = sizes[0]
    g = torch.Generator().manual_seed(0)
    frames = [[torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.uint8) for Hs, Ws in sizes] for _ in range(2)]
    want = torch.stack([torch.stack([f.to(torch.int64).sum((0, 1)) for f in img]) for img in frames])     # (2, B, 3)
    dense = torch.cat([nat.augment_sums(frames[0][n][None].cuda(), frames[1][n][None].cuda()) for n in range(2)], 1)
    padded = torch.full((2, 2, Hb, Wb, 3), 255, dtype=torch.uint8)
    packed = torch.full((2, 2, Hb * Wb, 3), 255, dtype=torch.uint8)
    for k in range(2):
        for n, (Hs, Ws) in enumerate(sizes):
            padded[k, n, :Hs, :Ws] = frames[k][n]
            packed[k, n, :Hs * Ws] = frames[k][n].reshape(Hs * Ws, 3)
    sparse = nat.augment_sums_sparse(padded[0].cuda(), padded[1].cuda(), SparseAugmentParams.identity(sizes).packed().cuda())
    mixed = nat.augment_sums_mixed(packed[0].cuda(), packed[1].cuda(),
                                   MixedAugmentParams.identity(sizes, [True, False]).packed().cuda())
    for name, got in (("dense", dense), ("sparse", sparse), ("mixed", mixed)):
        assert got.dtype == torch.int32 and torch.equal(got.cpu().to(torch.int64), want), name
    assert torch.equal(dense, sparse) and torch.equal(sparse, mixed)


def test_host_checks_raise_before_anything_is_launched():
    B, S, h, w = 1, 16 * 24, 8, 12
    dev = "cuda"
    i1 = torch.zeros(B, S, 3, dtype=torch.uint8, device=dev)
    i2 = torch.zeros_like(i1)
    flow = torch.zeros(B, S, 2, device=dev)
    vin = torch.ones(B, S, dtype=torch.uint8, device=dev)
    rec = MixedAugmentParams.identity([(16, 24)], [False]).packed().to(dev)
    sums = torch.zeros(2, B, 3, dtype=torch.int32, device=dev)
    o1, o2 = torch.zeros(B, h, w, 3, device=dev), torch.zeros(B, h, w, 3, device=dev)
    of, ov = torch.zeros(B, h, w, 2, device=dev), torch.zeros(B, h, w, device=dev)
    ints = [B, S, h, w]
    good = [i1, i2, flow, vin, rec, sums, o1, o2, of, ov]
    marker = 7.0
    for t in (o1, o2, of, ov):
        t.fill_(marker)

    def rejected(pos, bad, i=ints):
        t = list(good)
        t[pos] = bad
        with pytest.raises(RuntimeError, match="augment_mixed"):
            nat.ops().augment_mixed(t, i)

    rejected(4, rec[:, :48].contiguous())                                    # a wrong record width
    rejected(4, rec.cpu())                                                   # records on the host
    rejected(1, i2.float())                                                  # dtype of an image
    rejected(3, torch.ones(B, S + 1, dtype=torch.uint8, device=dev))         # size of valid
    rejected(6, flow.view(-1)[: B * h * w * 3].view(B, h, w, 3))             # an output aliasing an input
    rejected(7, o1)                                                          # an output aliasing another
    rejected(9, torch.zeros(B, h, w + 1, device=dev))                        # size of an output
    rejected(6, o1, [B, S, 0, w])                                            # an empty crop
    rejected(0, i1, [B, S + 1, h, w])                                        # a slot size the buffers do not have
    with pytest.raises(RuntimeError, match="augment_mixed_sums"):
        nat.ops().augment_mixed_sums([i1, i2, rec[:, :48].contiguous(), sums], [B, S])
    with pytest.raises(RuntimeError, match="augment_mixed_sums"):
        nat.ops().augment_mixed_sums([i1, i2, rec, sums], [B, S + 1])
    for name, n in (("augment_mixed_sums", 2), ("augment_mixed", 4)):        # rows of the op table
        assert list(torch.ops.jax_raft_amd.op_arity(name)) == [1, n, n]
    # the front-end checks the records on the host: a slot too small for a record, a bad flag, a wrong record class
    with pytest.raises(ValueError, match="does not fit a slot"):
        nat.augment_pairs_mixed(i1, i2, flow, vin, MixedAugmentParams.record((16, 25), True), (h, w))
    bad = MixedAugmentParams.identity([(16, 24)], [True])
    bad.ints[0, 18] = 3
    with pytest.raises(ValueError, match="dense flag"):
        nat.augment_pairs_mixed(i1, i2, flow, vin, bad, (h, w))
    with pytest.raises(ValueError, match="MixedAugmentParams"):
        nat.augment_pairs_mixed(i1, i2, flow, vin, SparseAugmentParams.identity([(16, 24)]), (h, w))
    with pytest.raises(ValueError, match="shrinks an axis"):
        nat.augment_pairs_mixed(i1, i2, flow, vin, MixedAugmentParams.record((16, 24), False, resized=(8, 5)), (h, 5))
    torch.cuda.synchronize()
    assert all(bool((t == marker).all()) for t in (o1, o2, of, ov))          # nothing was launched
    nat.ops().augment_mixed_sums([i1, i2, rec, sums], [B, S])
    nat.ops().augment_mixed(good, ints)                                      # ... and the good call is accepted
    torch.cuda.synchronize()
    assert bool((ov == 1).all()) and bool((o1 == -1).all()) and bool((of == 0).all())


def test_fetch_and_augment_do_not_synchronise(tmp_path):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    write_mix(tmp_path)
    ld = PairLoader(FlowPairs.open(str(tmp_path), "mix", parts=["sintel-clean", "kitti", "hd1k", "things-clean"]), batch=3,
                    device="cuda")
    crop = (24, 32)

    def batch(step):
        *bufs, sizes, dense = ld.fetch(step)
        params = sample_mixed(3, sizes, dense, "sintel", crop, step=step)
        return bufs, params, nat.augment_pairs_mixed(*bufs, params, crop)

    for step in range(2):      # warm: staging buffers, allocator blocks, the library
        batch(step)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        bufs, params, out = batch(2)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert ld.last_upload_bytes == sum(Hs * Ws * (14 + (not d)) for (Hs, Ws), d in zip(params.sizes, params.dense_flags))
    host = [t.cpu() for t in bufs]
    for n, (Hs, Ws) in enumerate(params.sizes):    # what was not uploaded is unspecified: give it a value
        for t in host:
            t[n, Hs * Ws:] = 0
        if params.dense_flags[n]:
            host[3][n] = 0
    want = augment_pairs_mixed(*host, params, crop)
    ld.close()
    assert all(same(g.cpu(), w_) for g, w_ in zip(out, want))


def test_trainer_on_a_generated_mixture_gpu(tmp_path):
    from jax_raft_amd.train.trainer import TrainConfig, Trainer

    h, w = 128, 160                                 # the smallest size the pyramid accepts
    want = write_mix(tmp_path, dict(sintel=(136, 168), things=(132, 176), kitti=[(136, 176), (132, 168)], hd1k=(140, 180)))
    names = ("sintel-clean", "sintel-final", "kitti", "hd1k", "things-clean")
    cfg = TrainConfig(arch="raft_small", data=str(tmp_path), dataset="mix", stage="sintel", mix=names,
                      mix_weights=(2, 2, 1, 2, 1), size=(h, w), batch=2, iters=3, steps=2, lr=2e-4)
    tr = Trainer(cfg)
    assert tr.device.type == "cuda" and tr.loader.mixed
    losses = [float(tr.train_step(tr.batch_for(s))["loss"]) for s in range(2)]
    tr.flush()
    assert all(math.isfinite(v) for v in losses) and tr.skipped == 0
    got = tr.batch_for(0)
    S = tr.loader.slot_pixels
    i1, i2 = (torch.full((2, S, 3), 255, dtype=torch.uint8) for _ in range(2))
    fl, va = torch.full((2, S, 2), 3e4), torch.ones((2, S), dtype=torch.uint8)
    sizes, dense = [], []
    for n, i in enumerate(tr.loader.indices_for(0)):    # the same samples from the arrays the files were written from
        k, j = tr.loader.ds.locate(i)
        truth = want[names[k]][j]
        Hs, Ws = truth[0].shape[:2]
        sizes.append((Hs, Ws))
        dense.append(len(truth) == 3)
        for buf, arr in zip((i1, i2, fl, va), truth):
            buf[n, :Hs * Ws] = torch.from_numpy(arr.copy()).reshape((Hs * Ws,) + arr.shape[2:])
    params = sample_mixed(2, sizes, dense, "sintel", (h, w), seed=cfg.seed, step=0, rank=0)
    ref = augment_pairs_mixed(i1, i2, fl, va, params, (h, w))
    assert all(g.is_cuda and same(g.cpu(), w_) for g, w_ in zip(got, ref))
    tr.loader.close()
