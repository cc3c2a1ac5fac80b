"""Sparse ground truth (KITTI / HD1K), host side: the PNG reader and KITTI's flow coding
(utils/flow_io.py, csrc/runtime/png.cpp), the golden sparse augmentation op, its records and
sampler (train/augment.py), the file lists and the loader for frames of several sizes
(train/datasets.py), the KITTI metrics (eval/kitti.py) and the trainer on a CPU device.  The GPU
kernels are checked against the golden op in test_sparse_gpu.py."""
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch

from jax_raft_amd.eval.kitti import kitti_metrics
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import (FlowPairs, PairLoader, SparseAugmentParams, SparseFlowPairs, augment_pairs_sparse,
                                sample_sparse)
from jax_raft_amd.train import augment as A
from jax_raft_amd.utils import flow_io as F
from jax_raft_amd.utils.flow_io import normalize_image, read_flow_png, read_png, write_flow_png

needs_native = pytest.mark.skipif(not nat.available(), reason="native library not built")

BIG_HUE = 2 * math.pi * 0.5 / 3.14
HB, WB = 40, 52                                   # the buffers
SIZES = [(40, 52), (37, 49), (40, 49)]            # the samples in their top-left corners


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sparse_frames(seed=0, density=0.5, sizes=SIZES):
    """Buffers HB x WB with one sample each; everything outside a sample's own region is filled with
    what would show if it were read: 255 in the images, 1 in valid, huge values in the flow."""
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    i1 = torch.full((B, HB, WB, 3), 255, dtype=torch.uint8)
    i2 = torch.full((B, HB, WB, 3), 255, dtype=torch.uint8)
    flow = torch.full((B, HB, WB, 2), 3e4)
    valid = torch.ones((B, HB, WB), dtype=torch.uint8)
    for n, (Hs, Ws) in enumerate(sizes):
        i1[n, :Hs, :Ws] = torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.uint8)
        i2[n, :Hs, :Ws] = torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.uint8)
        flow[n, :Hs, :Ws] = torch.randn(Hs, Ws, 2, generator=g) * 5
        valid[n, :Hs, :Ws] = (torch.rand(Hs, Ws, generator=g) < density).to(torch.uint8)
    return i1, i2, flow, valid


def records(sizes=SIZES, **kw):
    """One record per sample with the same settings; ``origin='far'``: the crop in the far corner."""
    out = []
    for Hs, Ws in sizes:
        k = dict(kw)
        crop = k.pop("crop")
        Hr, Wr = k.get("resized") or (Hs, Ws)
        if k.get("origin") == "far":
            k["origin"] = (Hr - crop[0], Wr - crop[1])
        out.append(SparseAugmentParams.record((Hs, Ws), **k))
    return SparseAugmentParams.cat(out)


STRONG = (0.6, 1.4, 0.6, BIG_HUE)
# name: (crop, settings of the records); the resize cases come first
CASES = {
    "identity": ((24, 32), dict(origin=(5, 7))),
    "upscale": ((24, 32), dict(resized=(52, 70), origin=(9, 13))),
    "downscale": ((23, 30), dict(resized=(24, 31), origin=(1, 1))),          # the scalar-store tail
    "ratio4": ((8, 12), dict(resized=(10, 13), origin=(1, 1))),              # 40 x 52 -> 10 x 13: exactly the limit
    "hflip": ((24, 32), dict(resized=(33, 44), origin=(4, 6), hflip=True)),
    "vflip": ((24, 32), dict(resized=(33, 44), origin=(4, 6), vflip=True)),
    "both_flips": ((24, 32), dict(resized=(33, 44), origin=(4, 6), hflip=True, vflip=True)),
    "far_corner": ((24, 32), dict(resized=(52, 70), origin="far")),
    "eraser": ((24, 32), dict(origin=(5, 7), rects=[(10, 8, 30, 20), (40, 25, 120, 90)])),
    "colour": ((24, 32), dict(origin=(5, 7), colour1=STRONG, colour2=STRONG)),
}
RESIZES = {"identity": None, "upscale": (52, 70), "downscale": (24, 31), "ratio4": (10, 13)}


def case_records(name):
    crop, kw = CASES[name]
    return crop, records(crop=crop, **kw)


def write_kitti(root, sizes, seed=0, density=0.5):
    """A KITTI-2015 training tree of len(sizes) pairs; returns [(image1, image2, flow, valid)] as the
    files hold them (the flow quantised to 1 / 64)."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    for d in ("image_2", "flow_occ"):
        os.makedirs(os.path.join(str(root), "training", d), exist_ok=True)
    out = []
    for k, (Hs, Ws) in enumerate(sizes):
        a, b = (rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(2))
        f = np.rint(rng.standard_normal((Hs, Ws, 2)) * 3 * 64).astype(np.float32) / 64 + np.float32(0)   # no -0: the file has none
        v = (rng.random((Hs, Ws)) < density).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(str(root), "training", "image_2", f"{k:06d}_10.png"))
        Image.fromarray(b).save(os.path.join(str(root), "training", "image_2", f"{k:06d}_11.png"))
        write_flow_png(os.path.join(str(root), "training", "flow_occ", f"{k:06d}_10.png"), f, v, filters=k % 5)
        out.append((a, b, f, v))
    return out


# ----------------------------------------------------------------------- PNG
def _chunks(path):
    data = open(path, "rb").read()
    at, out = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        out.append((kind, data[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def _write_chunks(path, chunks, signature=F.PNG_SIGNATURE, break_crc_of=None):
    with open(path, "wb") as f:
        f.write(signature)
        for kind, body in chunks:
            crc = zlib.crc32(kind + body) ^ (1 if kind == break_crc_of else 0)
            f.write(struct.pack(">I", len(body)) + kind + body + struct.pack(">I", crc))


def _banded(dtype):
    """48 x 64: a horizontal-gradient band, a diagonal-gradient band, a noise band."""
    top = np.iinfo(dtype).max
    ys, xs = np.mgrid[0:16, 0:64]
    horiz = xs * top // 63
    diag = (xs + ys) * top // 78
    noise = np.random.default_rng(3).integers(0, top + 1, (16, 64))
    return np.concatenate([horiz, diag, noise]).astype(dtype)


@pytest.mark.parametrize("kind", ["rgb8", "gray16"])
def test_read_png_equals_pillow(tmp_path, kind):
    from PIL import Image

    if kind == "rgb8":
        g = _banded(np.uint8)
        img = np.stack([g, g[:, ::-1], np.roll(g, 5, 1)], -1)
    else:
        img = _banded(np.uint16)
    p = str(tmp_path / "a.png")
    Image.fromarray(img).save(p)
    ch = dict(_chunks(p))
    W, H, depth = struct.unpack(">IIB", ch[b"IHDR"][:9])
    raw = zlib.decompress(b"".join(b for k, b in _chunks(p) if k == b"IDAT"))
    used = set(raw[:: len(raw) // H])
    print(f"{kind}: filter types in the file {sorted(used)}")
    assert (H, W) == (48, 64) and len(used) >= 3                     # the un-filter has something to do
    want = np.array(Image.open(p))
    assert want.dtype == img.dtype and np.array_equal(want, img)
    for native in ([False, True] if nat.available() else [False]):
        got = read_png(p, native=native)
        assert got.dtype == img.dtype and got.shape == img.shape and np.array_equal(got, want)
    assert F.png_size(p) == (48, 64)


@needs_native
@pytest.mark.parametrize("shape", [(5, 7), (37, 52)])
def test_flow_png_round_trip_with_every_filter(tmp_path, shape):
    rng = np.random.default_rng(1)
    f = (rng.standard_normal(shape + (2,)) * 20).astype(np.float32)
    v = (rng.random(shape) < 0.5).astype(np.uint8)
    q = np.rint(f.astype(np.float64) * 64).astype(np.float32) / 64          # what 1 / 64 steps keep of f
    for filters in (0, 1, 2, 3, 4, rng.integers(0, 5, shape[0])):
        p = str(tmp_path / "f.png")
        write_flow_png(p, f, v, filters)
        raw = zlib.decompress(dict(_chunks(p))[b"IDAT"])
        assert list(raw[:: 1 + shape[1] * 6]) == list(np.broadcast_to(filters, shape[0]))
        c, n = read_png(p, native=True), read_png(p, native=False)
        assert c.dtype == np.uint16 and c.shape == shape + (3,) and np.array_equal(c, n)     # identical bytes
        for native in (True, False):
            gf, gv = read_flow_png(p, native=native)
            assert gf.dtype == np.float32 and np.array_equal(gf, q) and gv.dtype == np.uint8 and np.array_equal(gv, v)


def test_flow_png_quantisation_and_clipping(tmp_path):
    f = np.array([[[0.0, 1 / 128], [3 / 128, -1 / 128], [511.99, -512.0], [600.0, -600.0]]], dtype=np.float32)
    p = str(tmp_path / "q.png")
    write_flow_png(p, f)
    got, valid = read_flow_png(p, native=False)
    want = np.array([[[0.0, 0.0], [2 / 64, 0.0], [32767 / 64, -512.0], [32767 / 64, -512.0]]], dtype=np.float32)
    want[0, 2, 0] = np.rint(511.99 * 64) / 64
    assert np.array_equal(got, want) and bool((valid == 1).all())            # halves go to even; uint16 clips


def test_malformed_png_raises_naming_the_file(tmp_path):
    good = str(tmp_path / "good.png")
    write_flow_png(good, np.zeros((4, 5, 2), np.float32))
    chunks = _chunks(good)
    ihdr = dict(chunks)[b"IHDR"]
    rows = bytearray(zlib.decompress(dict(chunks)[b"IDAT"]))
    swap = lambda kind, body: [(k, body if k == kind else b) for k, b in chunks]
    bad_filter = bytearray(rows)
    bad_filter[2 * 31] = 5                                                   # the filter byte of row 2
    cases = {
        "interlace": dict(chunks=swap(b"IHDR", ihdr[:12] + b"\x01")),
        "palette": dict(chunks=swap(b"IHDR", ihdr[:9] + b"\x03" + ihdr[10:])),
        "depth4": dict(chunks=swap(b"IHDR", ihdr[:8] + b"\x04" + ihdr[9:])),
        "signature": dict(chunks=chunks, signature=b"\x89PNG\r\n\x1a\r"),
        "crc": dict(chunks=chunks, break_crc_of=b"IDAT"),
        "short": dict(chunks=swap(b"IDAT", zlib.compress(bytes(rows[:-3])))),
        "long": dict(chunks=swap(b"IDAT", zlib.compress(bytes(rows) + b"\0"))),
        "filter": dict(chunks=swap(b"IDAT", zlib.compress(bytes(bad_filter)))),
        "garbage": dict(chunks=swap(b"IDAT", b"not zlib")),
    }
    for name, kw in cases.items():
        p = str(tmp_path / f"bad_{name}.png")
        _write_chunks(p, **kw)
        for native in ([False, True] if nat.available() else [False]):
            with pytest.raises(ValueError, match=f"bad_{name}.png"):
                read_png(p, native=native)
    assert read_png(good).shape == (4, 5, 3)
    with pytest.raises(ValueError, match="16-bit RGB"):
        from PIL import Image

        Image.fromarray(np.zeros((4, 5, 3), np.uint8)).save(tmp_path / "rgb8.png")
        read_flow_png(str(tmp_path / "rgb8.png"))


# ----------------------------------------------------------------- golden op
def _raft_scatter(flow, valid, Hr, Wr):
    """RAFT's ``SparseFlowAugmentor.resize_sparse_flow_map`` in numpy, line by line, with fp32 products
    and this project's ``>= 0`` bound (RAFT: ``> 0``)."""
    ht, wd = flow.shape[:2]
    coords = np.meshgrid(np.arange(wd), np.arange(ht))
    coords = np.stack(coords, axis=-1)
    coords = coords.reshape(-1, 2).astype(np.float32)
    flow = flow.reshape(-1, 2).astype(np.float32)
    valid = valid.reshape(-1).astype(np.float32)
    coords0 = coords[valid >= 1]
    flow0 = flow[valid >= 1]
    scale = np.array([np.float32(Wr / wd), np.float32(Hr / ht)], dtype=np.float32)
    coords1 = coords0 * scale
    flow1 = flow0 * scale
    xx = np.round(coords1[:, 0]).astype(np.int32)
    yy = np.round(coords1[:, 1]).astype(np.int32)
    v = (xx >= 0) & (xx < Wr) & (yy >= 0) & (yy < Hr)
    xx, yy, flow1 = xx[v], yy[v], flow1[v]
    flow_img = np.zeros([Hr, Wr, 2], dtype=np.float32)
    valid_img = np.zeros([Hr, Wr], dtype=np.int32)
    flow_img[yy, xx] = flow1
    valid_img[yy, xx] = 1
    return flow_img, valid_img


@pytest.mark.parametrize("case", sorted(RESIZES))
def test_golden_scatter_equals_raft_transcription(case):
    i1, i2, flow, valid = sparse_frames(seed=7)
    h_min, w_min = min(s[0] for s in SIZES), min(s[1] for s in SIZES)
    sizes_r = [RESIZES[case] or s for s in SIZES]
    # a no-flip record whose crop is as much of the resized map as every sample holds, at the four corners
    h, w = min(min(s[0] for s in sizes_r), h_min), min(min(s[1] for s in sizes_r), w_min)
    want = [_raft_scatter(flow[n, :Hs, :Ws].numpy(), valid[n, :Hs, :Ws].numpy(), *sizes_r[n]) for n, (Hs, Ws) in enumerate(SIZES)]
    covered = [np.zeros(s, bool) for s in sizes_r]
    for cy in (0, 1):
        for cx in (0, 1):
            origins = [((Hr - h) * cy, (Wr - w) * cx) for Hr, Wr in sizes_r]
            rec = SparseAugmentParams.cat([SparseAugmentParams.record(s, r, o) for s, r, o in zip(SIZES, sizes_r, origins)])
            _, _, gf, gv = augment_pairs_sparse(i1, i2, flow, valid, rec, (h, w))
            for n, (y0, x0) in enumerate(origins):
                wf, wv = want[n]
                assert np.array_equal(gf[n].numpy().view(np.int32), wf[y0:y0 + h, x0:x0 + w].view(np.int32)), (case, n)
                assert np.array_equal(gv[n].numpy(), wv[y0:y0 + h, x0:x0 + w].astype(np.float32)), (case, n)
                covered[n][y0:y0 + h, x0:x0 + w] = True
    assert all(c.all() for c in covered)
    assert all(0 < wv.sum() for _, wv in want)


def test_identity_record_is_a_plain_crop():
    i1, i2, flow, valid = sparse_frames(seed=2)
    h, w = 24, 32
    origins = [(5, 7), (13, 17), (0, 0)]
    o1, o2, of, ov = augment_pairs_sparse(i1, i2, flow, valid, SparseAugmentParams.identity(SIZES, origins), (h, w))
    for n, (y0, x0) in enumerate(origins):
        for got, src in ((o1, i1), (o2, i2)):
            assert same(got[n:n + 1], normalize_image(src[n, y0:y0 + h, x0:x0 + w].numpy()))
        on = valid[n, y0:y0 + h, x0:x0 + w] != 0
        assert same(ov[n], on.float()) and 0 < int(on.sum()) < h * w
        assert same(of[n], torch.where(on[..., None], flow[n, y0:y0 + h, x0:x0 + w], torch.zeros(())))


def test_golden_reads_nothing_outside_a_sample():
    crop, rec = case_records("upscale")
    a = augment_pairs_sparse(*sparse_frames(seed=7), rec, crop)
    i1, i2, flow, valid = sparse_frames(seed=7)
    for n, (Hs, Ws) in enumerate(SIZES):           # other padding, the same samples
        for t, fill in ((i1, 0), (i2, 7), (flow, float("nan")), (valid, 0)):
            t[n, Hs:] = fill
            t[n, :, Ws:] = fill
    b = augment_pairs_sparse(i1, i2, flow, valid, rec, crop)
    assert all(same(x, y) for x, y in zip(a, b))


def test_flip_mirrors_the_cells_and_negates_the_component():
    i1, i2, flow, valid = sparse_frames(seed=3)
    h, w, r = 24, 32, (33, 44)
    plain = augment_pairs_sparse(i1, i2, flow, valid, records(crop=(h, w), resized=r, origin=(4, 6)), (h, w))
    # the mirrored window: u = Wr - 1 - (x + x0') runs over the plain crop's columns backwards
    hf = augment_pairs_sparse(i1, i2, flow, valid, records(crop=(h, w), resized=r, origin=(4, r[1] - w - 6), hflip=True), (h, w))
    vf = augment_pairs_sparse(i1, i2, flow, valid, records(crop=(h, w), resized=r, origin=(r[0] - h - 4, 6), vflip=True), (h, w))
    for got, dim, comp in ((hf, 2, 0), (vf, 1, 1)):
        want = torch.flip(plain[2], (dim,)).clone()
        want[..., comp] = -want[..., comp]
        want = torch.where(want == 0, torch.zeros(()), want)               # -0 where valid = 0: the op writes +0
        assert same(got[3], torch.flip(plain[3], (dim,)))
        assert torch.equal(got[2], want) and same(got[0], torch.flip(plain[0], (dim,)))


def test_scan_window_contains_every_lander():
    """The kernel's scan window (its Python mirror) against the forward map itself, per axis."""
    for Ws in (52, 1242, 2560):
        xs = np.arange(Ws)
        for Wr in range(-(-Ws // 4), 2 * Ws + 1):
            isx, sx = np.float32(Wr / Ws), np.float32(Ws / Wr)
            X = np.rint(xs.astype(np.float32) * isx).astype(np.int64)
            keep = X < Wr
            lo, hi = A.scan_window(np.arange(Wr), sx, Ws)
            assert bool(((lo[X[keep]] <= xs[keep]) & (xs[keep] <= hi[X[keep]])).all()), (Ws, Wr)
            assert int((hi - lo).max()) < 9 <= A.MAX_SCAN                   # sx + 5 candidates at most


# ------------------------------------------------------- records and sampler
def test_sampler():
    sizes = [(375, 1242), (370, 1226), (376, 1241), (374, 1238), (375, 1242), (370, 1224)]
    kw = dict(batch=6, sizes=sizes, stage="kitti")
    a = sample_sparse(seed=1, step=5, rank=0, **kw)
    assert a == sample_sparse(seed=1, step=5, rank=0, **kw)
    assert a != sample_sparse(seed=1, step=6, rank=0, **kw) and a != sample_sparse(seed=1, step=5, rank=1, **kw)
    assert a != sample_sparse(seed=2, step=5, rank=0, **kw)
    assert a.packed().shape == (6, 52) and a.packed().dtype == torch.int32 and a.sizes == sizes
    assert A.SPARSE_STAGES["kitti"].crop == (288, 960)
    flips, resized = 0, 0
    for stage, crop in (("kitti", None), ("sintel", None), ("kitti", (128, 160))):
        h, w = crop or A.SPARSE_STAGES[stage].crop
        lo, hi = A.SPARSE_STAGES[stage].min_scale, A.SPARSE_STAGES[stage].max_scale
        for step in range(40):
            r = sample_sparse(6, sizes, stage, crop, seed=3, step=step)
            r.validate((376, 1242), (h, w))
            i, f = r.ints, r.floats
            assert np.array_equal(f[:, A.F_COL1:A.F_COL1 + 12], f[:, A.F_COL2:A.F_COL2 + 12])      # colour is symmetric
            assert not i[:, A.I_VFLIP].any() and (stage == "sintel" or not i[:, A.I_HFLIP].any())
            flips += int(i[:, A.I_HFLIP].sum()) if stage == "sintel" else 0
            for n, (Hs, Ws) in enumerate(sizes):
                Hr, Wr = int(i[n, A.I_HR]), int(i[n, A.I_WR])
                if (Hr, Wr) == (Hs, Ws):
                    continue                                                   # no spatial augmentation drawn
                resized += 1
                floor_ = max((h + 1) / Hs, (w + 1) / Ws)
                scale = Wr / Ws
                assert Hr >= h + 1 and Wr >= w + 1 and scale >= floor_ - 0.5 / Ws          # never below the floor
                assert scale <= max(2.0 ** hi, floor_) + 0.5 / Ws and abs(Hr / Hs - scale) <= 1 / Hs   # one scale, no stretch
                assert 2.0 ** lo - 0.5 / Ws <= scale or scale <= floor_ + 0.5 / Ws
    assert flips > 20 and resized > 300
    plain = sample_sparse(6, sizes, "kitti", seed=1, step=5, augment=False)
    ident = SparseAugmentParams.identity(sizes)
    cols = [k for k in range(A.N_INTS_SPARSE) if k not in (A.I_Y0, A.I_X0)]
    assert np.array_equal(plain.ints[:, cols], ident.ints[:, cols]) and np.array_equal(plain.floats, ident.floats)
    with pytest.raises(ValueError, match="smaller than the crop"):
        sample_sparse(1, [(280, 1242)], "kitti")
    with pytest.raises(ValueError, match="stage"):
        sample_sparse(1, [(375, 1242)], "chairs")


def test_validate_rejects_bad_sparse_records():
    ok = SparseAugmentParams.record((40, 52), (10, 13))
    ok.validate((HB, WB), (8, 12))                                            # exactly 4: accepted
    with pytest.raises(ValueError, match="shrinks an axis by more than 4"):
        SparseAugmentParams.record((40, 52), (10, 12)).validate((HB, WB), (8, 12))
    with pytest.raises(ValueError, match="shrinks an axis by more than 4"):
        SparseAugmentParams.record((40, 52), (9, 13)).validate((HB, WB), (8, 12))
    with pytest.raises(ValueError, match="does not fit the buffer"):
        SparseAugmentParams.record((41, 52)).validate((HB, WB), (8, 12))
    with pytest.raises(ValueError, match="does not fit the buffer"):
        SparseAugmentParams.record((40, 53)).validate((HB, WB), (8, 12))
    both = SparseAugmentParams.cat([ok, SparseAugmentParams.record((37, 49), (20, 30), origin=(13, 0))])
    with pytest.raises(ValueError, match="record 1: the crop origin"):      # the dense checks, per sample
        both.validate((HB, WB), (8, 12))
    i1, i2, flow, valid = sparse_frames()
    with pytest.raises(ValueError, match="shrinks"):
        augment_pairs_sparse(i1, i2, flow, valid, records(crop=(8, 12), resized=(9, 13)), (8, 12))
    with pytest.raises(ValueError, match="SparseAugmentParams"):
        augment_pairs_sparse(i1, i2, flow, valid, A.AugmentParams.identity(3, (HB, WB)), (8, 12))
    with pytest.raises(ValueError, match="uint8"):
        augment_pairs_sparse(i1, i2, flow, valid.float(), SparseAugmentParams.identity(SIZES), (8, 12))
    assert A.AugmentParams.identity(2, (40, 52)).packed().shape == (2, 48)  # the dense layout is what it was


# ------------------------------------------------------- file lists, loader
def test_kitti_and_hd1k_file_lists(tmp_path):
    from PIL import Image

    kitti = tmp_path / "kitti"
    want = write_kitti(kitti, [(37, 52), (40, 49), (37, 52)])
    ds = FlowPairs.open(str(kitti), "kitti")                                  # no longer NotImplementedError
    assert isinstance(ds, SparseFlowPairs) and len(ds) == 3 and len(FlowPairs.kitti(str(kitti))) == 3
    assert ds.sizes() == [(37, 52), (40, 49), (37, 52)]
    for i in range(3):
        a, b, f, v = ds[i]
        wa, wb, wf, wv = want[i]
        assert np.array_equal(a, wa) and np.array_equal(b, wb) and v.dtype == np.uint8 and np.array_equal(v, wv)
        assert f.dtype == np.float32 and np.array_equal(f, wf)
    hd = tmp_path / "hd1k"
    os.makedirs(hd / "hd1k_input" / "image_2")
    os.makedirs(hd / "hd1k_flow_gt" / "flow_occ")
    rng = np.random.default_rng(0)
    frames = {}
    for seq, n in ((0, 3), (1, 2)):
        for k in range(n):
            name = f"{seq:06d}_{k + 10:04d}.png"
            frames[name] = rng.integers(0, 256, (20, 28, 3), dtype=np.uint8)
            Image.fromarray(frames[name]).save(hd / "hd1k_input" / "image_2" / name)
            write_flow_png(str(hd / "hd1k_flow_gt" / "flow_occ" / name), np.full((20, 28, 2), seq + k / 64, np.float32))
    ds = FlowPairs.open(str(hd), "hd1k")
    names = [tuple(os.path.basename(p) for p in t) for t in ds.items]
    assert names == [("000000_0010.png", "000000_0011.png", "000000_0010.png"),
                     ("000000_0011.png", "000000_0012.png", "000000_0011.png"),
                     ("000001_0010.png", "000001_0011.png", "000001_0010.png")]     # no pair across sequences
    a, b, f, v = ds[1]
    assert np.array_equal(a, frames["000000_0011.png"]) and np.array_equal(b, frames["000000_0012.png"])
    assert bool((f == np.float32(1 / 64)).all()) and bool((v == 1).all())
    with pytest.raises(NotImplementedError):
        FlowPairs.open(str(hd), "things")
    with pytest.raises(ValueError, match="kitti, hd1k"):
        FlowPairs.open(str(hd), "middlebury")
    for kind in (FileNotFoundError, NotImplementedError):     # the layout is not there: both, as open's earlier callers expect
        with pytest.raises(kind, match="image_2"):
            FlowPairs.open(str(hd), "kitti")
        with pytest.raises(kind, match="flow_occ"):
            FlowPairs.open(str(kitti), "hd1k")


def test_loader_over_frames_of_two_sizes(tmp_path):
    sizes = [(37, 52), (40, 49)] * 4
    want = write_kitti(tmp_path, sizes)
    ds = FlowPairs.kitti(str(tmp_path))
    ld = PairLoader(ds, batch=3, seed=4)
    assert ld.sparse and ld.frame_max == (40, 52) and ld.frame_min == (37, 49) and ld.steps_per_epoch == 2
    assert [ld.indices_for(s) for s in range(4)] == [PairLoader(ds, 3, 4).indices_for(s) for s in range(4)]
    for step in (0, 1, 2, 1, 5):                   # in order (prefetched) and out of order
        a, b, f, v, got_sizes = ld.fetch(step)
        idx = ld.indices_for(step)
        assert got_sizes == [sizes[i] for i in idx] == ld.sizes_for(step)
        assert a.dtype == torch.uint8 and a.shape == (3, 40, 52, 3) and f.shape == (3, 40, 52, 2)
        assert v.dtype == torch.uint8 and v.shape == (3, 40, 52)
        for n, i in enumerate(idx):
            Hs, Ws = sizes[i]
            for got, w_ in zip((a, b, f, v), want[i]):
                assert np.array_equal(got[n, :Hs, :Ws].numpy(), w_)
    ld.close()


# ------------------------------------------------------------------- metrics
def test_kitti_metrics_by_hand():
    gt = np.zeros((2, 3, 2), np.float32)
    flow = np.zeros((2, 3, 2), np.float32)
    valid = np.ones((2, 3), np.uint8)
    gt[0, 0] = (100, 0); flow[0, 0] = (104, 0)      # epe 4 > 3, but 4 % of |gt|: no outlier
    gt[0, 1] = (10, 0); flow[0, 1] = (10, 4)        # epe 4, 40 %: outlier
    gt[0, 2] = (1, 0); flow[0, 2] = (3, 0)          # epe 2 <= 3: no outlier, whatever the ratio
    gt[1, 0] = (0, 0); flow[1, 0] = (0, 5)          # |gt| = 0: the ratio is inf, outlier
    gt[1, 1] = (3, 4); flow[1, 1] = (3, 4)          # exact
    gt[1, 2] = (0, 0); flow[1, 2] = (300, 400)      # not valid: ignored
    valid[1, 2] = 0
    m = kitti_metrics(flow, gt, valid)
    assert m["epe"] == pytest.approx((4 + 4 + 2 + 5 + 0) / 5) and m["f1"] == pytest.approx(100 * 2 / 5)
    assert kitti_metrics(flow, gt, np.zeros((2, 3), np.uint8)) == {"epe": 0.0, "f1": 0.0}


# ------------------------------------------------------------------- trainer
def test_trainer_on_a_generated_kitti_tree_cpu(tmp_path):
    from jax_raft_amd.train.trainer import TrainConfig, Trainer

    data, ck = tmp_path / "data", tmp_path / "ckpt"
    sizes = [(136, 176), (132, 168)] * 2
    want = write_kitti(data, sizes)
    assert tuple(TrainConfig(data="x", dataset="kitti", stage="kitti").size) == (288, 960)
    assert tuple(TrainConfig(data="x", dataset="hd1k", stage="sintel").size) == (368, 768)
    with pytest.raises(ValueError, match="stage"):
        TrainConfig(data="x", dataset="kitti", stage="chairs")
    cfg = TrainConfig(arch="raft_small", data=str(data), dataset="kitti", stage="kitti", size=(128, 160), batch=1, iters=2,
                      steps=2, ckpt_dir=str(ck))
    cpu = torch.device("cpu")
    tr = Trainer(cfg, device=cpu)
    assert tr.loader.sparse and tr.loader.frame_min == (132, 168)
    before = tr.batch_for(1)
    assert [tuple(t.shape) for t in before] == [(1, 128, 160, 3), (1, 128, 160, 3), (1, 128, 160, 2), (1, 128, 160)]
    assert 0 < float(before[3].mean()) < 1
    losses = [float(tr.train_step(tr.batch_for(s))["loss"]) for s in range(2)]
    assert all(math.isfinite(v) for v in losses)
    tr.save(str(ck))
    again = Trainer(TrainConfig(**{**cfg.__dict__, "resume": True}), device=cpu)
    assert again.step == 2
    assert all(same(a, b) for a, b in zip(before, again.batch_for(1)))
    # augment=False: identity records, a plain crop of the files
    plain = Trainer(TrainConfig(**{**cfg.__dict__, "augment": False, "ckpt_dir": None}), device=cpu)
    i1, _, fl, va = plain.batch_for(0)
    k = plain.loader.indices_for(0)[0]
    rec = sample_sparse(1, [sizes[k]], "kitti", (128, 160), seed=0, step=0, augment=False)
    y0, x0 = int(rec.ints[0, A.I_Y0]), int(rec.ints[0, A.I_X0])
    a, _, f, v = want[k]
    win = (slice(y0, y0 + 128), slice(x0, x0 + 160))
    assert same(i1, normalize_image(a[win]))
    assert same(va[0], torch.from_numpy(v[win].astype(np.float32)))
    assert same(fl[0], torch.from_numpy(np.where(v[win][..., None] != 0, f[win], np.float32(0))))
    with pytest.raises(ValueError, match="smaller than the crop"):
        Trainer(TrainConfig(arch="raft_small", data=str(data), dataset="kitti", stage="kitti", size=(136, 160), batch=1),
                device=cpu)
    for t in (tr, again, plain):
        t.loader.close()
