"""Training on real data on the GPU: the augmentation kernels (csrc/kernels/augment.hip) bitwise
against the golden op (train/augment.py), their launch builders' checks, the loader's upload
path without host synchronisation, and the trainer on a generated dataset."""
import math

import numpy as np
import pytest
import torch

from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import AugmentParams, FlowPairs, PairLoader, augment_pairs
from jax_raft_amd.train import augment as A
from test_augment import bits, frames, same, write_chairs

pytestmark = pytest.mark.gpu

BIG_HUE = 2 * math.pi * 0.5 / 3.14


def _records_37x53():
    """Four deliberately different records for source 37 x 53, crop 24 x 32."""
    src, (h, w) = (37, 53), (24, 32)
    stretched = (round(37 * 0.7 * 1.1), round(53 * 0.7 * 0.95))        # 28 x 35: scale 0.7 x stretch
    big = (round(37 * 1.9), round(53 * 1.9))                            # 70 x 101
    return AugmentParams.cat([
        AugmentParams.record(src, origin=(5, 7)),
        AugmentParams.record(src, stretched, origin=(2, 3), hflip=True, vflip=True, colour1=(1.1, 0.9, 1.2, 0.2),
                             colour2=(1.1, 0.9, 1.2, 0.2)),
        # the crop's last row / column are the resized image's: the clamped last source row / column are taps
        AugmentParams.record(src, big, origin=(big[0] - h, big[1] - w), colour1=(0.8, 1.0, 1.0, 0.0),
                             colour2=(0.8, 1.0, 1.0, 0.0)),
        AugmentParams.record(src, origin=(13, 21), colour1=(0.6, 1.4, 0.6, BIG_HUE), colour2=(1.4, 0.6, 1.4, -BIG_HUE),
                             rects=[(30, 18, 45, 30), (45, 25, 120, 90)]),     # the second crosses the border
    ])


def _tail_records():
    src = (37, 53)
    return AugmentParams.cat([
        AugmentParams.record(src, (50, 61), origin=(3, 31), hflip=True, colour1=(1.3, 0.7, 1.3, -0.5),
                             colour2=(0.7, 1.2, 0.9, 0.5), rects=[(0, 0, 20, 20)]),
        AugmentParams.record(src, origin=(0, 23), vflip=True),
    ])


CASES = {
    # name: (B, Hs, Ws, crop, records)
    "b4_37x53_crop24x32": (4, 37, 53, (24, 32), _records_37x53),
    "b1_40x56_whole": (1, 40, 56, (40, 56), lambda: AugmentParams.identity(1, (40, 56))),
    # a width that is no multiple of the 4-pixel run: unaligned rows, the scalar-store path and its tail
    "b2_37x53_crop21x30_tail": (2, 37, 53, (21, 30), _tail_records),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_equals_golden_bitwise(case):
    B, Hs, Ws, crop, records = CASES[case]
    i1, i2, flow = frames(B, Hs, Ws, seed=7)
    params = records()
    want = augment_pairs(i1, i2, flow, params, crop)
    got = nat.augment_pairs(i1.cuda(), i2.cuda(), flow.cuda(), params, crop)
    names = ("image1", "image2", "flow", "valid")
    for name, g, w_ in zip(names, got, want):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w_.shape, name
        diff = (g.cpu() - w_).abs().max()
        print(f"{case}: {name} max |kernel - golden| = {float(diff):.3g}")
        assert same(g.cpu(), w_), name
    assert bool((want[3] == 1).all()) and float(want[0].min()) >= -1 and float(want[0].max()) <= 1


@pytest.mark.parametrize("fill", ["random", "all255"])
def test_colour_sums_are_exact(fill):
    i1, i2, _ = frames(3, 37, 53, seed=1)
    if fill == "all255":
        i1 = torch.full((2, 130, 260, 3), 255, dtype=torch.uint8)      # several blocks per frame
        i2 = torch.full_like(i1, 255)
        i2[1, 129, 259, 2] = 0
    got = nat.augment_sums(i1.cuda(), i2.cuda())
    want = torch.stack([A.colour_sums(i1), A.colour_sums(i2)])
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), want)


def test_repeatable_and_ordered_across_streams():
    B, Hs, Ws, crop, records = CASES["b4_37x53_crop24x32"]
    i1, i2, flow = (t.cuda() for t in frames(B, Hs, Ws, seed=7))
    params = records()
    first = nat.augment_pairs(i1, i2, flow, params, crop)
    second = nat.augment_pairs(i1, i2, flow, params, crop)
    for a, b in zip(first, second):
        assert torch.equal(bits(a), bits(b))
    # the same sums buffer, dirty from the first stream, reused on a second one: the clear is in-stream
    sums = nat.augment_sums(i1, i2)
    want = sums.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nat.augment_sums(i1, i2, out=sums)
        third = nat.augment_pairs(i1, i2, flow, params, crop)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(sums, want)
    for a, b in zip(first, third):
        assert torch.equal(bits(a), bits(b))


def test_invalid_flow_texels():
    B, Hs, Ws, crop, records = CASES["b4_37x53_crop24x32"]
    i1, i2, flow = frames(B, Hs, Ws, seed=7)
    clean = augment_pairs(i1, i2, flow, records(), crop)
    clean_flow = flow.clone()
    for n in range(B):
        flow[n, 12, 20, 0] = float("nan")
        flow[n, 20, 30, 1] = float("inf")
        flow[n, 25, 40, 0] = 1e4
        flow[n, 36, 52] = -1e4
    want = augment_pairs(i1, i2, flow, records(), crop)
    got = nat.augment_pairs(i1.cuda(), i2.cuda(), flow.cuda(), records(), crop)
    for g, w_ in zip(got, want):
        assert same(g.cpu(), w_)
    hit = want[3] == 0
    assert all(bool(hit[n].any()) for n in range(B)) and not bool(hit.all())
    assert bool((got[2].cpu()[hit] == 0).all()) and bool(torch.isfinite(got[2]).all())
    assert same(got[0].cpu(), clean[0]) and same(got[1].cpu(), clean[1])        # nothing else changes
    # a finite 1e4 texel may be blended into a pixel that stays valid: the pixels that weigh no poisoned texel
    # (an indicator field through the same op) and are valid keep their flow
    poisoned = (flow != clean_flow) | torch.isnan(flow)
    weighed = augment_pairs(i1, i2, poisoned.any(-1, keepdim=True).float().expand(-1, -1, -1, 2).contiguous(), records(), crop)[2]
    keep = ~hit & (weighed == 0).all(-1)
    assert bool(keep.any()) and same(got[2].cpu()[keep], clean[2][keep])


def test_fetch_and_augment_do_not_synchronise(tmp_path):
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    write_chairs(tmp_path, 8, 40, 56)
    ld = PairLoader(FlowPairs.chairs(str(tmp_path)), batch=2, device="cuda")
    crop = (24, 32)
    for step in range(2):      # warm: staging buffers, allocator blocks, the library
        nat.augment_pairs(*ld.fetch(step), AugmentParams.sample(2, ld.frame, "chairs", crop, step=step), crop)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        params = AugmentParams.sample(2, ld.frame, "chairs", crop, step=2)
        out = nat.augment_pairs(*ld.fetch(2), params, crop)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = augment_pairs(*(t.cpu() for t in ld.fetch(2)), params, crop)
    ld.close()
    assert all(same(g.cpu(), w_) for g, w_ in zip(out, want))


def test_trainer_on_a_generated_dataset_gpu(tmp_path):
    from jax_raft_amd.train.trainer import TrainConfig, Trainer

    h, w = 128, 160
    write_chairs(tmp_path, 8, h + 56, w + 56)
    cfg = TrainConfig(arch="raft_small", data=str(tmp_path), size=(h, w), batch=2, iters=3, steps=3, lr=2e-4)
    tr = Trainer(cfg)
    assert tr.device.type == "cuda"
    losses = [float(tr.train_step(tr.batch_for(s))["loss"]) for s in range(3)]
    tr.flush()
    assert all(math.isfinite(v) for v in losses) and tr.skipped == 0
    ds = FlowPairs.chairs(str(tmp_path))
    for step in (1, 3):
        got = tr.batch_for(step)
        idx = tr.loader.indices_for(step)
        raw = [ds[i] for i in idx]
        i1, i2, fl = (torch.from_numpy(np.stack([r[k] for r in raw])) for k in range(3))
        params = AugmentParams.sample(2, (h + 56, w + 56), "chairs", (h, w), seed=cfg.seed, step=step, rank=0)
        want = augment_pairs(i1, i2, fl, params, (h, w))
        assert all(g.is_cuda and same(g.cpu(), w_) for g, w_ in zip(got, want))
    tr.loader.close()


def test_launch_builder_checks():
    B, Hs, Ws, h, w = 1, 16, 24, 8, 12
    dev = "cuda"
    i1 = torch.zeros(B, Hs, Ws, 3, dtype=torch.uint8, device=dev)
    i2 = torch.zeros_like(i1)
    flow = torch.zeros(B, Hs, Ws, 2, device=dev)
    rec = AugmentParams.identity(B, (Hs, Ws)).packed().to(dev)
    sums = torch.zeros(2, B, 3, dtype=torch.int32, device=dev)
    o1, o2 = torch.zeros(B, h, w, 3, device=dev), torch.zeros(B, h, w, 3, device=dev)
    of, ov = torch.zeros(B, h, w, 2, device=dev), torch.zeros(B, h, w, device=dev)
    ints = [B, Hs, Ws, h, w]
    good = [i1, i2, flow, rec, sums, o1, o2, of, ov]
    marker = 7.0
    for t in (o1, o2, of, ov):
        t.fill_(marker)

    def rejected(pos, bad, i=ints):
        t = list(good)
        t[pos] = bad
        with pytest.raises(RuntimeError, match="augment"):
            nat.ops().augment(t, i)

    wide = torch.zeros(B, Hs, 2 * Ws, 3, dtype=torch.uint8, device=dev)
    rejected(0, wide[:, :, :Ws])                                             # a non-contiguous image
    rejected(1, i2.float())                                                  # dtype of an image
    rejected(2, flow.double())                                               # dtype of the flow
    rejected(3, rec.float())                                                 # dtype of the records
    rejected(3, rec[:, :40].contiguous())                                    # size of the records
    rejected(4, sums.long())                                                 # dtype of the sums
    rejected(5, flow.view(-1)[: B * h * w * 3].view(B, h, w, 3))             # an output aliasing an input
    rejected(6, o1)                                                          # an output aliasing another
    rejected(7, torch.zeros(B * h * w * 2 + 1, device=dev)[1:].view(B, h, w, 2))   # 4-byte aligned only
    rejected(8, torch.zeros(B, h, w + 1, device=dev))                        # size of an output
    rejected(5, o1, [B, Hs, Ws, 0, w])                                       # an empty crop
    with pytest.raises(RuntimeError, match="augment_sums"):
        nat.ops().augment_sums([i1, wide[:, :, :Ws], sums], [B, Hs, Ws])
    with pytest.raises(RuntimeError, match="augment_sums"):
        nat.ops().augment_sums([i1, i2, sums], [B, Hs, Ws + 1])
    # the front-end checks the records on the host: a crop larger than the resized size, a wrong dtype
    with pytest.raises(ValueError, match="larger than the resized"):
        nat.augment_pairs(i1, i2, flow, AugmentParams.record((Hs, Ws), resized=(6, 30)), (h, w))
    with pytest.raises(ValueError, match="uint8"):
        nat.augment_pairs(i1.float(), i2, flow, AugmentParams.identity(B, (Hs, Ws)), (h, w))
    torch.cuda.synchronize()
    assert all(bool((t == marker).all()) for t in (o1, o2, of, ov))          # nothing was launched
    nat.ops().augment(good, ints)                                            # ... and the good call is accepted
    torch.cuda.synchronize()
    assert bool((ov == 1).all()) and bool((o1 == -1).all())
