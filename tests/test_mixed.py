"""RAFT's Sintel stage, host side: the ``.pfm`` reader (utils/flow_io.py), the FlyingThings3D list and
the weighted mixture of dense and sparse lists (train/datasets.py), the mixed records, their sampler
and the golden op on packed slots (train/augment.py), the loader's packed slots and the trainer on
a CPU device.  The GPU kernels are checked against the golden op in test_mixed_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from jax_raft_amd.train import (AugmentParams, FlowPairs, MixedAugmentParams, MixedFlowPairs, PairLoader,
                                SparseAugmentParams, SparseFlowPairs, augment_pairs, augment_pairs_mixed,
                                augment_pairs_sparse, sample_mixed, sample_sparse)
from jax_raft_amd.train import augment as A
from jax_raft_amd.utils.flow_io import read_pfm, write_flo, write_flow_png, write_pfm
from test_sparse import BIG_HUE, same, write_kitti

# ------------------------------------------------------- the batch of the kernel tests
# (kind, source size, settings of the record); slot S = 24 * 40
S_SLOT = 24 * 40
SAMPLES = [
    (True, (20, 33), dict(resized=(27, 41), origin=(3, 5), hflip=True, vflip=True, colour1=(0.7, 1.3, 0.6, BIG_HUE),
                          colour2=(1.3, 0.7, 1.4, -BIG_HUE), rects=[(4, 3, 15, 11), (25, 12, 90, 70)])),
    (False, (24, 40), dict(resized=(19, 32), origin=(2, 4), hflip=True)),
    (False, (17, 29), dict(resized=(21, 36), origin=(1, 3))),
    (True, (13, 19), dict(origin=(1, 1))),
]
CROPS = [(12, 18), (12, 20)]
DENSE = [d for d, _, _ in SAMPLES]


def samples_for(crop=CROPS[0]):
    """The batch at ``crop``.  An identity record with origin (1, 1) needs a source one pixel larger than
    the crop, and 13 x 19 cannot hold the 20 columns of the second crop: there, and only there, the last
    sample is 13 x 21."""
    return SAMPLES if crop[1] <= 18 else SAMPLES[:3] + [(True, (13, 21), SAMPLES[3][2])]


def sizes_for(crop=CROPS[0]):
    return [s for _, s, _ in samples_for(crop)]


SIZES = sizes_for()


def mixed_records(crop=CROPS[0]):
    return MixedAugmentParams.cat([MixedAugmentParams.record(src, dense, **kw) for dense, src, kw in samples_for(crop)])


def packed_frames(sizes=SIZES, dense=DENSE, slot=S_SLOT, seed=0, pad=(0xFF, float("nan")), density=0.5, bad=True):
    """Packed slots of ``slot`` pixels with one sample each.  Everything past a sample's prefix, and the
    valid bytes of a dense sample, hold ``pad`` (a byte, a float): what would show if it were read.
    ``bad``: one NaN and one value above 1000 in the flow of the first dense and the first sparse sample."""
    g = torch.Generator().manual_seed(seed)
    B = len(sizes)
    i1 = torch.full((B, slot, 3), pad[0], dtype=torch.uint8)
    i2 = torch.full((B, slot, 3), pad[0], dtype=torch.uint8)
    flow = torch.full((B, slot, 2), pad[1])
    valid = torch.full((B, slot), pad[0], dtype=torch.uint8)
    seen = set()
    for n, ((Hs, Ws), d) in enumerate(zip(sizes, dense)):
        N = Hs * Ws
        i1[n, :N] = torch.randint(0, 256, (N, 3), generator=g, dtype=torch.uint8)
        i2[n, :N] = torch.randint(0, 256, (N, 3), generator=g, dtype=torch.uint8)
        flow[n, :N] = torch.randn(N, 2, generator=g) * 5
        v = (torch.rand(N, generator=g) < density).to(torch.uint8)
        if not d:
            valid[n, :N] = v
        if bad and d not in seen:
            seen.add(d)
            at = (Hs // 2) * Ws + Ws // 2
            flow[n, at, 0] = float("nan")
            flow[n, at + 2, 1] = 1700.0
            if not d:
                valid[n, at] = valid[n, at + 2] = 1
    return i1, i2, flow, valid


def per_sample_golden(frames, params, crop):
    """The two existing golden ops applied sample by sample, written out here (not through ``part``)."""
    i1, i2, flow, valid = frames
    outs = []
    for n, (Hs, Ws) in enumerate(params.sizes):
        N = Hs * Ws
        a, b, f = (t[n, :N].reshape(1, Hs, Ws, -1) for t in (i1, i2, flow))
        if params.ints[n, A.I_DENSE]:
            outs.append(augment_pairs(a, b, f, AugmentParams(params.ints[n:n + 1, :16], params.floats[n:n + 1]), crop))
        else:
            ints = params.ints[n:n + 1].copy()
            ints[0, 18:] = 0
            outs.append(augment_pairs_sparse(a, b, f, valid[n, :N].reshape(1, Hs, Ws),
                                             SparseAugmentParams(ints, params.floats[n:n + 1]), crop))
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))


# ------------------------------------------------------------ generated trees
def _png(path, arr):
    from PIL import Image

    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _quantised_flow(rng, Hs, Ws):
    return np.rint(rng.standard_normal((Hs, Ws, 2)) * 3 * 64).astype(np.float32) / 64 + np.float32(0)


def write_things(root, size, scenes=(("A", "0000"), ("B", "0003")), frames=3, seed=0, passes=("clean", "final")):
    """A FlyingThings3D tree (left camera): returns {pass: [images of scene 0, of scene 1]},
    {direction: [flows of scene 0, of scene 1]} as the files hold them."""
    rng = np.random.default_rng(seed)
    Hs, Ws = size
    images, flows = {}, {}
    for p in passes:
        images[p] = []
        for a, b in scenes:
            imgs = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(frames)]
            for k, im in enumerate(imgs):
                _png(os.path.join(str(root), f"frames_{p}pass", "TRAIN", a, b, "left", f"{k + 6:04d}.png"), im)
            images[p].append(imgs)
    for direction, tag in (("into_future", "IntoFuture"), ("into_past", "IntoPast")):
        flows[direction] = []
        for a, b in scenes:
            fl = [rng.standard_normal((Hs, Ws, 3)).astype(np.float32) * 4 for _ in range(frames)]
            d = os.path.join(str(root), "optical_flow", "TRAIN", a, b, direction, "left")
            os.makedirs(d, exist_ok=True)
            for k, f in enumerate(fl):
                write_pfm(os.path.join(d, f"OpticalFlow{tag}_{k + 6:04d}_L.pfm"), f, little_endian=k % 2 == 0)
            flows[direction].append(fl)
    return images, flows


def write_sintel(root, size, frames=3, seed=0):
    """A Sintel training tree with one scene: returns {pass: images}, flows."""
    rng = np.random.default_rng(seed)
    Hs, Ws = size
    images = {}
    for p in ("clean", "final"):
        images[p] = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(frames)]
        for k, im in enumerate(images[p]):
            _png(os.path.join(str(root), "training", p, "alley_1", f"frame_{k + 1:04d}.png"), im)
    flows = [rng.standard_normal((Hs, Ws, 2)).astype(np.float32) * 4 for _ in range(frames - 1)]
    os.makedirs(os.path.join(str(root), "training", "flow", "alley_1"))
    for k, f in enumerate(flows):
        write_flo(os.path.join(str(root), "training", "flow", "alley_1", f"frame_{k + 1:04d}.flo"), f)
    return images, flows


def write_hd1k(root, size, frames=3, seed=0):
    """An HD1K tree with one sequence: returns [(image1, image2, flow, valid)]."""
    rng = np.random.default_rng(seed)
    Hs, Ws = size
    imgs, truth = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(frames)], []
    for k, im in enumerate(imgs):
        name = f"000000_{k + 10:04d}.png"
        _png(os.path.join(str(root), "hd1k_input", "image_2", name), im)
        f, v = _quantised_flow(rng, Hs, Ws), (rng.random((Hs, Ws)) < 0.5).astype(np.uint8)
        os.makedirs(os.path.join(str(root), "hd1k_flow_gt", "flow_occ"), exist_ok=True)
        write_flow_png(os.path.join(str(root), "hd1k_flow_gt", "flow_occ", name), f, v, filters=k % 5)
        if k + 1 < frames:
            truth.append((im, imgs[k + 1], f, v))
    return truth


MIX_SIZES = dict(sintel=(30, 44), things=(34, 40), kitti=[(29, 52), (31, 50)], hd1k=(36, 56))


def write_mix(root, sizes=MIX_SIZES):
    """The five parts of RAFT's Sintel stage under ``root``; returns {part name: [(image1, image2, flow[, valid])]}
    in the order of each part's list."""
    root = str(root)
    want = {}
    si, sf = write_sintel(os.path.join(root, "Sintel"), sizes["sintel"])
    for p in ("clean", "final"):
        want["sintel-" + p] = [(si[p][k], si[p][k + 1], sf[k]) for k in range(len(sf))]
    want["kitti"] = write_kitti(os.path.join(root, "KITTI"), sizes["kitti"] * 2)
    want["hd1k"] = write_hd1k(os.path.join(root, "HD1K"), sizes["hd1k"])
    ti, tf = write_things(os.path.join(root, "FlyingThings3D"), sizes["things"], passes=("clean",))
    want["things-clean"] = things_pairs(ti["clean"], tf)
    return want


def things_pairs(images, flows):
    """RAFT's listing over what ``write_things`` returned for one pass."""
    out = []
    for direction in ("into_future", "into_past"):
        for imgs, fl in zip(images, flows[direction]):
            for i in range(len(fl) - 1):
                if direction == "into_future":
                    out.append((imgs[i], imgs[i + 1], fl[i][..., :2]))
                else:
                    out.append((imgs[i + 1], imgs[i], fl[i + 1][..., :2]))
    return out


# ----------------------------------------------------------------------- PFM
@pytest.mark.parametrize("little", [True, False])
@pytest.mark.parametrize("channels", [1, 3])
def test_pfm_round_trip(tmp_path, little, channels):
    rng = np.random.default_rng(channels)
    a = rng.standard_normal((5, 7, 3) if channels == 3 else (5, 7)).astype(np.float32)
    a.flat[3] = np.float32(1e-40)                                             # a subnormal survives
    p = str(tmp_path / "a.pfm")
    write_pfm(p, a, little_endian=little)
    head = open(p, "rb").read(20).split(b"\n")
    assert head[0] == (b"PF" if channels == 3 else b"Pf") and head[1] == b"7 5" and (float(head[2]) < 0) == little
    got = read_pfm(p)
    assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got.view(np.int32), a.view(np.int32))


def test_pfm_rows_are_bottom_up(tmp_path):
    p = str(tmp_path / "hand.pfm")
    rows = np.arange(6, dtype="<f4").reshape(2, 3)                            # the file's first row is 0 1 2
    with open(p, "wb") as f:
        f.write(b"Pf\n3 2\n-1.0\n" + rows.tobytes())
    assert np.array_equal(read_pfm(p), np.array([[3, 4, 5], [0, 1, 2]], np.float32))
    with open(p, "wb") as f:
        f.write(b"PF\n1 2\n1.0\n" + np.arange(6, dtype=">f4").tobytes())      # big endian, 3 channels
    assert np.array_equal(read_pfm(p), np.array([[[3, 4, 5]], [[0, 1, 2]]], np.float32))


def test_malformed_pfm_raises_naming_the_file(tmp_path):
    body = np.zeros(6, "<f4").tobytes()
    cases = {"magic": b"P6\n3 2\n-1.0\n" + body, "header": b"Pf\n3 x\n-1.0\n" + body, "dims": b"Pf\n3\n-1.0\n" + body,
             "scale": b"Pf\n3 2\n0.0\n" + body, "noscale": b"Pf\n3 2\nabc\n" + body, "short": b"Pf\n3 2\n-1.0\n" + body[:-1],
             "short3": b"PF\n3 2\n-1.0\n" + body, "empty": b""}
    for name, data in cases.items():
        p = tmp_path / f"bad_{name}.pfm"
        p.write_bytes(data)
        with pytest.raises(ValueError, match=f"bad_{name}.pfm"):
            read_pfm(str(p))


# ------------------------------------------------------------ Things listing
def test_things_listing(tmp_path):
    images, flows = write_things(tmp_path, (10, 14))
    ds = FlowPairs.things(str(tmp_path), "clean")
    assert type(ds) is FlowPairs and len(ds) == 2 * 2 * 2                     # directions x scenes x (frames - 1)
    names = [tuple(os.path.basename(p) for p in t) for t in ds.items]
    assert names[0] == ("0006.png", "0007.png", "OpticalFlowIntoFuture_0006_L.pfm")
    assert names[4] == ("0007.png", "0006.png", "OpticalFlowIntoPast_0007_L.pfm")       # into_past: reversed, flow[i + 1]
    assert names[5] == ("0008.png", "0007.png", "OpticalFlowIntoPast_0008_L.pfm")
    assert "/A/0000/" in ds.items[0][0] and "/B/0003/" in ds.items[2][0] and "/A/0000/into_past/" in ds.items[4][2]
    want = things_pairs(images["clean"], flows)
    for i in range(len(ds)):
        a, b, f = ds[i]
        assert np.array_equal(a, want[i][0]) and np.array_equal(b, want[i][1])
        assert f.shape == (10, 14, 2) and f.dtype == np.float32 and np.array_equal(f, want[i][2])
    both = FlowPairs.open(str(tmp_path), "things")                            # no longer NotImplementedError
    clean, final = FlowPairs.open(str(tmp_path), "things-clean"), FlowPairs.open(str(tmp_path), "things-final")
    assert both.items == clean.items + final.items and clean.items == ds.items and len(final) == 8
    assert all("frames_finalpass" in t[0] for t in final.items)
    ld = PairLoader(both, batch=2, seed=1)                                    # the dense loader decodes .pfm by extension
    a, b, f = ld.fetch(0)
    wantf = things_pairs(images["clean"], flows) + things_pairs(images["final"], flows)
    for n, i in enumerate(ld.indices_for(0)):
        assert np.array_equal(f[n].numpy(), wantf[i][2]) and np.array_equal(a[n].numpy(), wantf[i][0])
    ld.close()
    with pytest.raises(FileNotFoundError, match="frames_cleanpass"):
        FlowPairs.open(str(tmp_path / "nowhere"), "things")


# ---------------------------------------------------------------- the mixture
def _lists(tmp_path):
    write_kitti(tmp_path / "k", [(9, 12), (8, 13), (9, 12)])
    write_things(tmp_path / "t", (10, 14), passes=("clean",))
    return FlowPairs.kitti(str(tmp_path / "k")), FlowPairs.things(str(tmp_path / "t"))


def test_mixed_list_maps_items_under_weights(tmp_path):
    kitti, things = _lists(tmp_path)
    mix = MixedFlowPairs([(things, 2), (kitti, 3)])
    assert len(mix) == 2 * 8 + 3 * 3 == 25 and mix.slot_pixels == 140
    want = [(0, j) for _ in range(2) for j in range(8)] + [(1, j) for _ in range(3) for j in range(3)]
    assert [mix.locate(i) for i in range(25)] == want
    for i, (k, j) in enumerate(want):
        assert mix.dense(i) == (k == 0) and mix.paths(i) == (things, kitti)[k].items[j]
        assert mix.size(i) == ((10, 14) if k == 0 else [(9, 12), (8, 13), (9, 12)][j])
    assert len(mix[3]) == 3 and len(mix[20]) == 4 and np.array_equal(mix[20][3], kitti[1][3])
    with pytest.raises(IndexError):
        mix.locate(25)
    with pytest.raises(ValueError, match="weight"):
        MixedFlowPairs([(things, 0)])
    ld = PairLoader(mix, batch=4, seed=3, rank=1, world=2)                    # indices_for keeps its definition
    perm = np.random.default_rng([3, 0]).permutation(25)
    assert ld.steps_per_epoch == 3 and ld.indices_for(1) == [int(v) for v in perm[12:16]]
    ld.close()


def test_mixture_opens_by_directory_and_missing_part_raises(tmp_path):
    want = write_mix(tmp_path)
    mix = FlowPairs.open(str(tmp_path), "mix")
    lens = [2, 2, 4, 2, 8]
    assert [type(p) for p, _ in mix.parts] == [FlowPairs, FlowPairs, SparseFlowPairs, SparseFlowPairs, FlowPairs]
    assert [w for _, w in mix.parts] == [100, 100, 200, 5, 1] and [len(p) for p, _ in mix.parts] == lens
    assert len(mix) == sum(w * n for w, n in zip([100, 100, 200, 5, 1], lens))
    assert mix.slot_pixels == 36 * 56 and [len(want[k]) for k in want] == lens
    two = FlowPairs.open(str(tmp_path), "mix", parts=[("hd1k", 2), "things-clean"])
    assert len(two) == 2 * 2 + 8
    os.rename(tmp_path / "HD1K", tmp_path / "HD1K_")
    with pytest.raises(FileNotFoundError, match="HD1K"):
        FlowPairs.open(str(tmp_path), "mix")
    with pytest.raises(ValueError, match="unknown part"):
        FlowPairs.open(str(tmp_path), "mix", parts=["chairs"])


def test_dense_part_with_two_sizes_raises(tmp_path):
    kitti, things = _lists(tmp_path)
    odd = things.items[5][0]
    _png(odd, np.zeros((10, 15, 3), np.uint8))
    with pytest.raises(ValueError, match=os.path.basename(os.path.dirname(os.path.dirname(odd))) + ".*" + os.path.basename(odd)):
        MixedFlowPairs([(things, 1), (kitti, 1)])
    MixedFlowPairs([(kitti, 1)])                                              # a sparse part may have several


# ------------------------------------------------------- records and sampler
def test_sampler_equals_the_existing_samplers():
    sizes = [(436, 1024), (540, 960), (436, 1024), (540, 960)]
    for step in range(12):
        kw = dict(seed=5, step=step, rank=1)
        for augment in (True, False):
            got = sample_mixed(4, sizes, [True] * 4, "sintel", augment=augment, **kw)
            for n, s in enumerate(sizes):           # sample n of a mixed batch: draw n of a dense batch of that size
                dense = AugmentParams.sample(4, s, "sintel", augment=augment, **kw)
                assert np.array_equal(got.ints[n, :16], dense.ints[n]) and same(torch.from_numpy(got.floats[n]), torch.from_numpy(dense.floats[n]))
            assert got.sizes == sizes and bool((got.ints[:, A.I_DENSE] == 1).all()) and not got.ints[:, 19].any()
            ksizes = [(375, 1242), (370, 1226), (1080, 2560), (375, 1242)]
            got = sample_mixed(4, ksizes, [False] * 4, "sintel", augment=augment, **kw)
            sparse = sample_sparse(4, ksizes, "sintel", augment=augment, **kw)
            assert np.array_equal(got.ints, sparse.ints) and same(torch.from_numpy(got.floats), torch.from_numpy(sparse.floats))
    same_size = AugmentParams.sample(3, (436, 1024), "sintel", (128, 160), seed=2, step=9)
    got = sample_mixed(3, [(436, 1024)] * 3, [True] * 3, "sintel", (128, 160), seed=2, step=9)
    assert np.array_equal(got.ints[:, :16], same_size.ints) and np.array_equal(got.floats, same_size.floats)


def test_sampler_is_a_function_of_seed_step_rank():
    sizes, dense = [(436, 1024), (375, 1242), (540, 960), (1080, 2560)], [True, False, True, False]
    kw = dict(batch=4, sizes=sizes, dense_flags=dense)
    a = sample_mixed(seed=1, step=5, rank=0, **kw)
    assert a == sample_mixed(seed=1, step=5, rank=0, **kw) and a.dense_flags == dense and a.sizes == sizes
    assert a != sample_mixed(seed=1, step=6, rank=0, **kw) and a != sample_mixed(seed=1, step=5, rank=1, **kw)
    assert a != sample_mixed(seed=2, step=5, rank=0, **kw)
    assert a.packed().shape == (4, 52) and a.packed().dtype == torch.int32
    for step in range(30):
        r = sample_mixed(seed=3, step=step, **kw)
        r.validate(1080 * 2560, (368, 768))
        assert not r.ints[[1, 3], A.I_VFLIP].any()                            # the sparse draws have no v-flip
    with pytest.raises(ValueError, match="stage"):
        sample_mixed(stage="kitti", **kw)
    with pytest.raises(ValueError, match="smaller than the crop"):
        sample_mixed(1, [(360, 1242)], [False])
    with pytest.raises(ValueError, match="flags"):
        sample_mixed(2, sizes[:2], [True])


def test_validate_rejects_bad_mixed_records():
    crop = (8, 12)
    ok = mixed_records()
    ok.validate(S_SLOT, (12, 18))
    bad = mixed_records()
    bad.ints[2, A.I_DENSE] = 2
    with pytest.raises(ValueError, match="record 2: the dense flag"):
        bad.validate(S_SLOT, (12, 18))
    with pytest.raises(ValueError, match="record 1: the sample 24x40 does not fit a slot of 959"):
        ok.validate(S_SLOT - 1, (12, 18))
    shrink = dict(resized=(8, 12))                                            # 40 x 52 -> 8 x 12: more than 4
    MixedAugmentParams.record((40, 52), True, **shrink).validate(40 * 52, crop)           # fine for a dense sample
    with pytest.raises(ValueError, match="record 1: .*shrinks an axis by more than 4"):
        MixedAugmentParams.cat([MixedAugmentParams.record((40, 52), True, **shrink),
                                MixedAugmentParams.record((40, 52), False, **shrink)]).validate(40 * 52, crop)
    with pytest.raises(ValueError, match="record 0: the crop origin"):        # the dense checks, per sample
        MixedAugmentParams.record((40, 52), True, origin=(33, 0)).validate(40 * 52, crop)
    frames = packed_frames()
    with pytest.raises(ValueError, match="MixedAugmentParams"):
        augment_pairs_mixed(*frames, SparseAugmentParams.identity(SIZES), (12, 18))
    with pytest.raises(ValueError, match="uint8"):
        augment_pairs_mixed(frames[0], frames[1], frames[2], frames[3].float(), ok, (12, 18))
    assert SparseAugmentParams.identity(SIZES).packed().shape == (4, 52) and not SparseAugmentParams.identity(SIZES).ints[:, 18:].any()


# ----------------------------------------------------------------- golden op
@pytest.mark.parametrize("crop", CROPS)
def test_golden_is_the_two_ops_per_sample(crop):
    frames, rec = packed_frames(sizes_for(crop)), mixed_records(crop)
    got = augment_pairs_mixed(*frames, rec, crop)
    want = per_sample_golden(frames, rec, crop)
    assert [tuple(t.shape) for t in got] == [(4, *crop, 3), (4, *crop, 3), (4, *crop, 2), (4, *crop)]
    assert all(same(g, w_) for g, w_ in zip(got, want))
    assert bool(torch.isfinite(got[2]).all()) and float(got[0].min()) >= -1 and float(got[0].max()) <= 1
    assert all(0 < float(got[3][n].mean()) for n in range(4)) and float(got[3][1].mean()) < 1   # the sparse rule leaves holes
    assert float(got[3][3].mean()) == 1                                       # the dense rule: |f| < 1000 everywhere here
    other = augment_pairs_mixed(*packed_frames(sizes_for(crop), pad=(0, 0.0)), rec, crop)      # padding and dense valid bytes are not read
    assert all(same(g, o) for g, o in zip(got, other))


# -------------------------------------------------------------------- loader
def test_loader_packs_prefixes_and_counts_upload_bytes(tmp_path):
    want = write_mix(tmp_path)
    names = ["sintel-clean", "sintel-final", "kitti", "hd1k", "things-clean"]
    mix = FlowPairs.open(str(tmp_path), "mix", parts=[(n, 2) for n in names])
    ld = PairLoader(mix, batch=5, seed=2)
    S = 36 * 56
    assert ld.mixed and ld.slot_pixels == S and ld.frame_min == (29, 40) and ld.frame_max == (36, 56)
    kinds = set()
    for step in (0, 1, 2, 1, 6):                   # in order (prefetched) and out of order
        a, b, f, v, sizes, dense = ld.fetch(step)
        assert a.dtype == torch.uint8 and a.shape == (5, S, 3) and b.shape == (5, S, 3)
        assert f.dtype == torch.float32 and f.shape == (5, S, 2) and v.dtype == torch.uint8 and v.shape == (5, S)
        idx = ld.indices_for(step)
        assert sizes == ld.sizes_for(step) and dense == ld.dense_for(step)
        nbytes = 0
        for n, i in enumerate(idx):
            k, j = mix.locate(i)
            truth = want[names[k]][j]
            Hs, Ws = truth[0].shape[:2]
            assert sizes[n] == (Hs, Ws) and dense[n] == (len(truth) == 3)
            for got, w_ in zip((a, b, f, v), truth):
                assert np.array_equal(got[n, :Hs * Ws].numpy().reshape(w_.shape), w_)
            nbytes += Hs * Ws * (14 + (not dense[n]))
            kinds.add(names[k])
        assert ld.last_upload_bytes == nbytes
    assert len(kinds) == 5
    ld.close()


# ------------------------------------------------------------------- trainer
def test_trainer_on_a_generated_mixture_cpu(tmp_path):
    from jax_raft_amd.train.trainer import TrainConfig, Trainer, config_from_args

    data, ck = tmp_path / "data", tmp_path / "ckpt"
    write_mix(data, dict(sintel=(136, 168), things=(132, 176), kitti=[(136, 176), (132, 168)], hd1k=(140, 180)))
    assert tuple(TrainConfig(data="x", dataset="mix", stage="sintel").size) == (368, 768)
    assert tuple(TrainConfig(data="x", dataset="things", stage="things").size) == (400, 720)
    assert TrainConfig(data="x", dataset="mix", stage="sintel").mix_parts == [
        ("sintel-clean", 100), ("sintel-final", 100), ("kitti", 200), ("hd1k", 5), ("things-clean", 1)]
    for stage in ("chairs", "kitti", "things"):
        with pytest.raises(ValueError, match="stage"):
            TrainConfig(data="x", dataset="mix", stage=stage)
    with pytest.raises(ValueError, match="weights"):
        TrainConfig(data="x", dataset="mix", stage="sintel", mix=("kitti", "hd1k"), mix_weights=(1,))
    assert TrainConfig().mix_weights is None and TrainConfig().dataset == "chairs"
    mix = ("sintel-clean", "kitti", "hd1k", "things-clean", "sintel-final")
    cfg = TrainConfig(arch="raft_small", data=str(data), dataset="mix", stage="sintel", mix=mix, mix_weights=(2, 1, 2, 1, 2),
                      size=(128, 160), batch=2, iters=2, steps=2, ckpt_dir=str(ck))
    cpu = torch.device("cpu")
    tr = Trainer(cfg, device=cpu)
    assert tr.loader.mixed and tr.loader.frame_min == (132, 168) and len(tr.loader.ds) == 4 + 4 + 4 + 8 + 4
    before = tr.batch_for(1)
    assert [tuple(t.shape) for t in before] == [(2, 128, 160, 3), (2, 128, 160, 3), (2, 128, 160, 2), (2, 128, 160)]
    losses = [float(tr.train_step(tr.batch_for(s))["loss"]) for s in range(2)]
    assert all(math.isfinite(v) for v in losses)
    tr.save(str(ck))
    again = Trainer(TrainConfig(**{**cfg.__dict__, "resume": True}), device=cpu)
    assert again.step == 2
    assert all(same(a, b) for a, b in zip(before, again.batch_for(1)))
    kinds = {d for s in range(tr.loader.steps_per_epoch) for d in tr.loader.dense_for(s)}
    assert kinds == {True, False}                                             # both kinds were drawn
    for t in (tr, again):
        t.loader.close()
    # the command line: --mix name[:weight],...
    import argparse

    ns = argparse.Namespace(**{**{k: v for k, v in TrainConfig().__dict__.items() if k != "mix_weights"},
                               "data": "x", "dataset": "mix", "stage": "sintel", "mix": "kitti:200,hd1k:5,things-clean"})
    got = config_from_args(ns)
    assert got.mix == ("kitti", "hd1k", "things-clean") and got.mix_weights == (200, 5, 1)
