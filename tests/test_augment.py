"""Training on real data, host side: the golden augmentation op (train/augment.py), the
record sampler, the dataset readers and pair loader (train/datasets.py), the trainer on a CPU
device, and the new ops' rows in the binding table.  The GPU kernels are checked against the
golden op in test_augment_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import AugmentParams, FlowPairs, PairLoader, augment_pairs
from jax_raft_amd.train import augment as A
from jax_raft_amd.train.loss import sequence_loss_reference
from jax_raft_amd.utils.flow_io import normalize_image, write_flo

HS, WS = 37, 53


def frames(B=2, Hs=HS, Ws=WS, seed=0):
    g = torch.Generator().manual_seed(seed)
    i1 = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    i2 = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8)
    flow = torch.randn(B, Hs, Ws, 2, generator=g) * 5
    return i1, i2, flow


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def write_chairs(root, n, Hs, Ws, seed=0):
    from PIL import Image

    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        a, b = (rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(2))
        f = rng.standard_normal((Hs, Ws, 2)).astype(np.float32) * 3
        stem = os.path.join(str(root), f"{k + 1:05d}")
        Image.fromarray(a).save(stem + "_img1.ppm")
        Image.fromarray(b).save(stem + "_img2.ppm")
        write_flo(stem + "_flow.flo", f)
        out.append((a, b, f))
    return out


# ---------------------------------------------------------------- golden op
def test_identity_record_is_crop_plus_normalisation():
    i1, i2, flow = frames()
    h, w, y0, x0 = 24, 32, 5, 7
    o1, o2, of, ov = augment_pairs(i1, i2, flow, AugmentParams.identity(2, (HS, WS), (y0, x0)), (h, w))
    for got, src in ((o1, i1), (o2, i2)):
        want = torch.cat([normalize_image(s[y0:y0 + h, x0:x0 + w].numpy()) for s in src])
        assert same(got, want)
    assert same(of, flow[:, y0:y0 + h, x0:x0 + w])
    assert ov.shape == (2, h, w) and bool((ov == 1).all())


@pytest.mark.parametrize("axis", ["h", "v"])
def test_flip_equals_torch_flip_of_identity(axis):
    i1, i2, flow = frames()
    h, w, y0, x0 = 24, 32, 5, 7
    ident = augment_pairs(i1, i2, flow, AugmentParams.identity(2, (HS, WS), (y0, x0)), (h, w))
    # the mirrored crop window: u = Wr - 1 - (x + x0') runs over the identity's columns backwards
    origin = (y0, WS - w - x0) if axis == "h" else (HS - h - y0, x0)
    rec = AugmentParams.cat([AugmentParams.record((HS, WS), origin=origin, hflip=axis == "h", vflip=axis == "v")] * 2)
    got = augment_pairs(i1, i2, flow, rec, (h, w))
    dim, comp = (2, 0) if axis == "h" else (1, 1)
    want_flow = torch.flip(ident[2], (dim,)).clone()
    want_flow[..., comp] = -want_flow[..., comp]
    assert same(got[0], torch.flip(ident[0], (dim,))) and same(got[1], torch.flip(ident[1], (dim,)))
    assert same(got[2], want_flow)
    assert same(got[3], torch.flip(ident[3], (dim,)))


def _texel_by_hand(c, col, mean):
    """The texel transform of the module docstring in numpy fp32, one operation at a time."""
    f = np.float32
    b, k, s, theta = col
    M = A.hue_matrix(theta)
    luma = lambda v: f(f(f(0.299) * v[0]) + f(f(0.587) * v[1])) + f(f(0.114) * v[2])
    cl = lambda v: np.minimum(np.maximum(v, f(0)), f(255))
    c = [cl(f(x) * f(b)) for x in c]
    m = min(f(255), f(f(b) * luma([f(x) for x in mean])))
    if f(k) != 1:
        c = [cl(f(f(x - m) * f(k)) + m) for x in c]
    if f(s) != 1:
        g = luma(c)
        c = [cl(f(f(x - g) * f(s)) + g) for x in c]
    c = [cl(f(f(c[0] * M[j, 0]) + f(c[1] * M[j, 1])) + f(c[2] * M[j, 2])) for j in range(3)]
    return [f(f(x / f(255)) * f(2)) - f(1) for x in c]


def test_eraser_writes_the_transformed_mean_colour_on_image_2_only():
    i1, i2, flow = frames(B=1)
    col = (1.3, 0.7, 1.2, 0.4)
    rect = (40, 20, 70, 60)            # crosses the right and bottom borders of the 37 x 53 frame: clipped
    plain = AugmentParams.record((HS, WS), colour1=col, colour2=col)
    erased = AugmentParams.record((HS, WS), colour1=col, colour2=col, rects=[rect])
    a = augment_pairs(i1, i2, flow, plain, (HS, WS))
    b = augment_pairs(i1, i2, flow, erased, (HS, WS))
    assert same(a[0], b[0]) and same(a[2], b[2]) and same(a[3], b[3])      # image 1 and the flow are untouched
    N = HS * WS
    mean = [(int(s) + N // 2) // N for s in i2[0].to(torch.int64).sum((0, 1))]
    want = torch.tensor(np.array(_texel_by_hand(mean, col, mean), dtype=np.float32))
    # scale 1: the taps of pixel (y, x) are (y..y+1, x..x+1) clamped, so every pixel of the clipped rectangle is inside
    assert same(b[1][0, 20:, 40:], want.expand(HS - 20, WS - 40, 3))
    assert same(b[1][0, :20], a[1][0, :20]) and same(b[1][0, :, :40], a[1][0, :, :40])
    assert not same(a[1], b[1])


def test_colour_transform_matches_the_definition_texel_by_texel():
    i1, i2, flow = frames(B=1)
    c1, c2 = (0.6, 1.4, 0.6, 2 * math.pi * 0.5 / 3.14), (1.4, 0.6, 1.4, -0.3)
    o1, o2, _, _ = augment_pairs(i1, i2, flow, AugmentParams.record((HS, WS), colour1=c1, colour2=c2), (HS, WS))
    N = HS * WS
    for img, out, col in ((i1, o1, c1), (i2, o2, c2)):
        mean = [(int(s) + N // 2) // N for s in img[0].to(torch.int64).sum((0, 1))]
        for y, x in ((0, 0), (11, 29), (36, 52)):
            want = _texel_by_hand([int(v) for v in img[0, y, x]], col, mean)
            assert [float(v) for v in out[0, y, x]] == [float(v) for v in want]
    assert float(o1.min()) >= -1 and float(o1.max()) <= 1


def test_scale_two_on_a_linear_flow_field():
    Hs, Ws, h, w = 20, 24, 18, 22
    i1, i2, _ = frames(B=1, Hs=Hs, Ws=Ws)
    xs = torch.arange(Ws, dtype=torch.float32)
    flow = torch.stack([(0.5 * xs + 1).expand(Hs, Ws), torch.full((Hs, Ws), 2.0)], -1)[None].contiguous()
    rec = AugmentParams.record((Hs, Ws), resized=(2 * Hs, 2 * Ws), origin=(3, 4))
    _, _, of, ov = augment_pairs(i1, i2, flow, rec, (h, w))
    # resized column u samples source x = (u + 0.5) / 2 - 0.5 (clamped); a linear field is exact under bilinear taps
    src = ((torch.arange(w, dtype=torch.float32) + 4 + 0.5) * 0.5 - 0.5).clamp(0, Ws - 1)
    assert torch.allclose(of[0, :, :, 0], (2 * (0.5 * src + 1)).expand(h, w), rtol=0, atol=1e-5)
    assert torch.equal(of[0, :, :, 1], torch.full((h, w), 4.0))      # the magnitude doubles
    assert bool((ov == 1).all())


def test_invalid_flow_is_masked_and_zeroed():
    i1, i2, flow = frames(B=1)
    flow[0, 10, 10, 0] = float("nan")
    flow[0, 20, 30, 1] = 1000.0
    flow[0, 30, 40, 0] = -float("inf")
    o1, o2, of, ov = augment_pairs(i1, i2, flow, AugmentParams.identity(1, (HS, WS)), (HS, WS))
    bad = torch.zeros(HS, WS, dtype=torch.bool)
    for y, x in ((10, 10), (30, 40)):
        bad[y - 1:y + 1, x - 1:x + 1] = True       # NaN / inf: every pixel one of whose 4 taps is the bad texel
    bad[20, 30] = True                             # a finite texel reaches only pixels that weigh it: itself (scale 1)
    assert torch.equal(ov[0] == 0, bad)
    assert bool((of[0][bad] == 0).all()) and bool(torch.isfinite(of).all())
    assert same(of[0][~bad], flow[0][~bad])
    preds = torch.stack([torch.zeros_like(of), of.clone()])
    loss, _ = sequence_loss_reference(preds, of, ov)
    assert math.isfinite(float(loss))


def test_bad_records_are_refused_on_the_host():
    i1, i2, flow = frames(B=1)
    with pytest.raises(ValueError, match="smaller than the crop"):
        augment_pairs(i1, i2, flow, AugmentParams.identity(1, (HS, WS)), (HS + 1, WS))
    with pytest.raises(ValueError, match="larger than the resized"):
        augment_pairs(i1, i2, flow, AugmentParams.record((HS, WS), resized=(20, 30)), (24, 32))
    with pytest.raises(ValueError, match="origin"):
        augment_pairs(i1, i2, flow, AugmentParams.identity(1, (HS, WS), (14, 0)), (24, 32))
    rec = AugmentParams.identity(1, (HS, WS))
    rec.floats[0, A.F_SX] = 2.0
    with pytest.raises(ValueError, match="ratios"):
        augment_pairs(i1, i2, flow, rec, (24, 32))
    with pytest.raises(ValueError, match="smaller than the crop"):
        AugmentParams.sample(1, (300, 512), "chairs")


# ------------------------------------------------------------------ sampler
@pytest.mark.parametrize("stage,src", [("chairs", (384, 512)), ("things", (436, 1024)), ("sintel", (436, 1024))])
def test_sampler_invariants(stage, src):
    h, w = A.STAGES[stage].crop
    recs = AugmentParams.cat([AugmentParams.sample(100, src, stage, seed=3, step=s, rank=s % 2) for s in range(100)])
    assert len(recs) == 10000
    recs.validate(src, (h, w))
    i = recs.ints.astype(np.int64)
    Hr, Wr, y0, x0 = i[:, A.I_HR], i[:, A.I_WR], i[:, A.I_Y0], i[:, A.I_X0]
    assert (h <= Hr).all() and (w <= Wr).all()
    assert (0 <= y0).all() and (y0 <= Hr - h).all() and (0 <= x0).all() and (x0 <= Wr - w).all()
    asym = (recs.floats[:, A.F_COL1:A.F_COL1 + 12] != recs.floats[:, A.F_COL2:A.F_COL2 + 12]).any(axis=1)
    assert 0.17 < asym.mean() < 0.23                      # p = 0.2, sigma = 0.004
    assert 0.46 < i[:, A.I_HFLIP].mean() < 0.54 and 0.07 < i[:, A.I_VFLIP].mean() < 0.13
    assert 0.45 < (i[:, A.I_NRECT] > 0).mean() < 0.55
    assert 0.17 < ((Hr == src[0]) & (Wr == src[1])).mean() < 0.30    # no spatial augmentation: p = 0.2 (+ scale ~ 1)
    b = recs.floats[:, A.F_COL1:A.F_COL1 + 3]
    assert b.min() >= np.float32(0.6) and b.max() <= np.float32(1.4)


def test_sampler_is_a_pure_function_of_seed_step_rank():
    kw = dict(src=(384, 512), stage="chairs")
    a = AugmentParams.sample(6, seed=1, step=5, rank=0, **kw)
    assert a == AugmentParams.sample(6, seed=1, step=5, rank=0, **kw)
    assert a != AugmentParams.sample(6, seed=1, step=6, rank=0, **kw)
    assert a != AugmentParams.sample(6, seed=1, step=5, rank=1, **kw)
    assert a != AugmentParams.sample(6, seed=2, step=5, rank=0, **kw)
    plain = AugmentParams.sample(6, seed=1, step=5, augment=False, **kw)
    ident = AugmentParams.identity(6, (384, 512))
    cols = [k for k in range(A.N_INTS) if k not in (A.I_Y0, A.I_X0)]
    assert np.array_equal(plain.ints[:, cols], ident.ints[:, cols]) and np.array_equal(plain.floats, ident.floats)
    assert a.packed().shape == (6, 48) and a.packed().dtype == torch.int32


def test_hue_matrix():
    assert np.array_equal(A.hue_matrix(0.0), np.eye(3, dtype=np.float32))
    M = A.hue_matrix(0.7).astype(np.float64)
    assert np.allclose(M @ np.ones(3), np.ones(3), atol=2e-3)        # greys stay grey
    assert np.allclose(A.hue_matrix(0.7).astype(np.float64) @ A.hue_matrix(-0.7).astype(np.float64), np.eye(3), atol=1e-6)


# -------------------------------------------------------- readers and loader
def test_chairs_layout_reads_back_bit_for_bit(tmp_path):
    want = write_chairs(tmp_path, 5, 20, 28)
    ds = FlowPairs.chairs(str(tmp_path))
    assert len(ds) == 5
    for (a, b, f), (wa, wb, wf) in zip((ds[i] for i in range(5)), want):
        assert np.array_equal(a, wa) and np.array_equal(b, wb) and np.array_equal(f.view(np.int32), wf.view(np.int32))
    assert len(FlowPairs.open(str(tmp_path), "chairs")) == 5
    with pytest.raises(NotImplementedError):
        FlowPairs.open(str(tmp_path), "kitti")


def test_direct_ppm_read_equals_read_image(tmp_path):
    from PIL import Image

    from jax_raft_amd.train.datasets import read_frame
    from jax_raft_amd.utils.flow_io import read_image

    for k, first in enumerate((10, 32, 9, 200)):       # pixel bytes that look like header whitespace
        a = np.random.default_rng(k).integers(0, 256, (5, 7, 3), dtype=np.uint8)
        a[0, 0, :] = first
        p = str(tmp_path / f"{k}.ppm")
        Image.fromarray(a).save(p)
        assert np.array_equal(read_frame(p), a) and np.array_equal(read_image(p), a)
    commented = str(tmp_path / "c.ppm")                # a header the direct read does not take: the generic decoder
    open(commented, "wb").write(b"P6\n# made by hand\n2 1\n255\n" + bytes(range(6)))
    assert np.array_equal(read_frame(commented), np.arange(6, dtype=np.uint8).reshape(1, 2, 3))
    short = str(tmp_path / "s.ppm")
    open(short, "wb").write(b"P6\n2 2\n255\n" + bytes(5))
    with pytest.raises(Exception):
        read_frame(short)


def test_sintel_layout_reads_back_bit_for_bit(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(1)
    want = {}
    for scene, n in (("alley_1", 3), ("cave_2", 2)):
        for d in ("clean", "final", "flow"):
            os.makedirs(tmp_path / "training" / d / scene)
        for dst in ("clean", "final"):
            for k in range(n):
                img = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
                Image.fromarray(img).save(tmp_path / "training" / dst / scene / f"frame_{k + 1:04d}.png")
                want[dst, scene, k] = img
        for k in range(n - 1):
            f = rng.standard_normal((16, 24, 2)).astype(np.float32)
            write_flo(str(tmp_path / "training" / "flow" / scene / f"frame_{k + 1:04d}.flo"), f)
            want["flow", scene, k] = f
    for dst in ("clean", "final"):
        ds = FlowPairs.open(str(tmp_path), "sintel-" + dst)
        assert len(ds) == 3
        for i, (scene, k) in enumerate((("alley_1", 0), ("alley_1", 1), ("cave_2", 0))):
            a, b, f = ds[i]
            assert np.array_equal(a, want[dst, scene, k]) and np.array_equal(b, want[dst, scene, k + 1])
            assert np.array_equal(f, want["flow", scene, k])


def test_truncated_flo_raises_naming_the_file(tmp_path):
    write_chairs(tmp_path, 2, 20, 28)
    bad = str(tmp_path / "00002_flow.flo")
    data = open(bad, "rb").read()
    for cut in (len(data) - 40, 6, 2):
        open(bad, "wb").write(data[:cut])
        with pytest.raises(ValueError, match="00002_flow.flo"):
            FlowPairs.chairs(str(tmp_path))[1]
    open(bad, "wb").write(b"\0\0\0\0" + data[4:])
    with pytest.raises(ValueError, match="00002_flow.flo"):
        FlowPairs.chairs(str(tmp_path))[1]


def test_loader_order_and_batches(tmp_path):
    want = write_chairs(tmp_path, 13, 20, 28)
    ds = FlowPairs.chairs(str(tmp_path))
    loaders = [PairLoader(ds, batch=3, seed=4, rank=r, world=2) for r in range(2)]
    spe = loaders[0].steps_per_epoch
    assert spe == 2
    for epoch in range(2):
        seen = [i for s in range(spe) for ld in loaders for i in ld.indices_for(epoch * spe + s)]
        assert len(seen) == len(set(seen)) == 12 and set(seen) <= set(range(13))      # disjoint; one pair dropped
    assert [loaders[0].indices_for(s) for s in range(4)] == [PairLoader(ds, 3, 4, 0, 2).indices_for(s) for s in range(4)]
    assert loaders[0].indices_for(0) != loaders[0].indices_for(spe)                   # a new permutation per epoch
    assert loaders[0].indices_for(0) != PairLoader(ds, 3, 5, 0, 2).indices_for(0)
    ld = loaders[1]
    for step in (0, 1, 2, 1, 5):       # in order (prefetched) and out of order (decoded on the spot)
        a, b, f = ld.fetch(step)
        assert a.dtype == torch.uint8 and a.shape == (3, 20, 28, 3) and f.shape == (3, 20, 28, 2)
        for n, i in enumerate(ld.indices_for(step)):
            assert np.array_equal(a[n].numpy(), want[i][0]) and np.array_equal(b[n].numpy(), want[i][1])
            assert np.array_equal(f[n].numpy(), want[i][2])
    for ld in loaders:
        ld.close()
    with pytest.raises(ValueError, match="do not fill"):
        PairLoader(ds, batch=7, world=2)


def test_loader_refuses_a_second_frame_size(tmp_path):
    from PIL import Image

    write_chairs(tmp_path, 3, 20, 28)
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(tmp_path / "00003_img2.ppm")
    ld = PairLoader(FlowPairs.chairs(str(tmp_path)), batch=3)
    with pytest.raises(ValueError, match="00003_img2.ppm"):
        ld.fetch(0)
    ld.close()


def test_decode_threads_follow_the_job_share(monkeypatch):
    from jax_raft_amd.train import datasets as D

    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    assert D.decode_threads() == 4
    monkeypatch.setenv("OMP_NUM_THREADS", "512")
    assert D.decode_threads() == 16
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert D.decode_threads() == 16


# ------------------------------------------------------------------ trainer
def test_trainer_on_a_generated_dataset_cpu(tmp_path):
    from jax_raft_amd.train.trainer import TrainConfig, Trainer

    data, ck = tmp_path / "data", tmp_path / "ckpt"
    data.mkdir()
    write_chairs(data, 4, 140, 150)
    cfg = TrainConfig(arch="raft_small", data=str(data), size=(128, 128), batch=1, iters=2, steps=2, ckpt_dir=str(ck))
    cpu = torch.device("cpu")
    tr = Trainer(cfg, device=cpu)
    before = tr.batch_for(1)
    assert [tuple(t.shape) for t in before] == [(1, 128, 128, 3), (1, 128, 128, 3), (1, 128, 128, 2), (1, 128, 128)]
    losses = [float(tr.train_step(tr.batch_for(s))["loss"]) for s in range(2)]
    assert all(math.isfinite(v) for v in losses)
    tr.save(str(ck))
    again = Trainer(TrainConfig(**{**cfg.__dict__, "resume": True}), device=cpu)
    assert again.step == 2
    assert all(same(a, b) for a, b in zip(before, again.batch_for(1)))
    # augment=False: identity records, a plain crop of the files
    plain = Trainer(TrainConfig(**{**cfg.__dict__, "augment": False, "ckpt_dir": None}), device=cpu)
    i1, _, fl, va = plain.batch_for(0)
    rec = AugmentParams.sample(1, (140, 150), "chairs", (128, 128), seed=0, step=0, augment=False)
    y0, x0 = int(rec.ints[0, A.I_Y0]), int(rec.ints[0, A.I_X0])
    a, _, f = FlowPairs.chairs(str(data))[plain.loader.indices_for(0)[0]]
    assert same(i1, normalize_image(a[y0:y0 + 128, x0:x0 + 128]))
    assert same(fl[0], torch.from_numpy(f[y0:y0 + 128, x0:x0 + 128].copy())) and bool((va == 1).all())


def test_config_defaults_and_stage_sizes():
    from jax_raft_amd.train.data import SyntheticFlow
    from jax_raft_amd.train.trainer import TrainConfig

    cfg = TrainConfig()
    assert cfg.data is None and cfg.dataset == "chairs" and cfg.stage == "chairs" and cfg.augment is True
    assert tuple(cfg.size) == (384, 512)                                   # no data: nothing changes
    assert tuple(TrainConfig(stage="sintel").size) == (384, 512)
    assert tuple(TrainConfig(data="x").size) == (368, 496)
    assert tuple(TrainConfig(data="x", stage="things").size) == (400, 720)
    assert tuple(TrainConfig(data="x", stage="sintel", size=(256, 256)).size) == (256, 256)
    with pytest.raises(ValueError, match="stage"):
        TrainConfig(data="x", stage="kitti")
    assert SyntheticFlow is not None


# ---------------------------------------------------------- binding surface
@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_new_ops_are_table_rows():
    for name, n in (("augment_sums", 3), ("augment", 5)):
        assert list(torch.ops.jax_raft_amd.op_arity(name)) == [1, n, n]
        for k in (n - 1, n + 1):    # before any tensor check: the tensor list is [None]
            with pytest.raises(RuntimeError, match=rf"{name}: expected {n} ints, got {k}\b"):
                getattr(torch.ops.jax_raft_amd, name)([None], [1] * k)
            with pytest.raises(RuntimeError, match=rf"{name}: expected {n} ints, got {k}\b"):
                getattr(torch.classes.jax_raft_amd.Plan(), "add_" + name)([None], [1] * k)
        with pytest.raises(RuntimeError, match="images must be"):      # the right arity reaches the tensor checks
            getattr(torch.ops.jax_raft_amd, name)([None], [1, 8, 8] + [4] * (n - 3))
