"""Frame interpolation by forward splatting, without a GPU: the golden op
(models/reference.py:interpolate_frames), the native front end on CPU tensors, the lowering of the
"interp" plan (recorded on a FakePlan), the rejections and the golden-path API."""
import math

import numpy as np
import pytest
import torch

import jax_raft_amd
from jax_raft_amd import (BidirectionalFlow, BidirectionalInterp, fb_consistency, interpolate_frames, raft_large,
                          raft_small)
from jax_raft_amd.models import reference as R
from jax_raft_amd.models.layers import MaskPredictor
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import tunedb
from test_engine_lowering import FakePlan

H, W, WIN = 128, 152, (122, 150, 3, 1)
H0, W0, TOP, LEFT = WIN
NAN = float("nan")


def _frame(B=1, h=H0, w=W0, seed=1):
    return torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def _flows(B, h, w, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, h, w, 2, generator=g) * scale, torch.randn(B, h, w, 2, generator=g) * scale


# ------------------------------------------------------------------ golden op
def test_zero_flows_on_equal_frames_give_the_frame():
    f = _frame(2, 20, 30)
    z = torch.zeros(2, 20, 30, 2)
    for t in (1 / 256, 0.3, 0.5, 255 / 256):
        out, holes = interpolate_frames(f, f, z, z, t)
        assert out.dtype == torch.uint8 and holes.dtype == torch.bool and holes.shape == (2, 20, 30)
        assert torch.equal(out, f) and not holes.any()


def test_translation_pair_at_the_midpoint_is_the_half_shift():
    # frame2(y, x) = frame1(y, x - 4): the flow 1 -> 2 is (+4, 0), 2 -> 1 is (-4, 0); at t = 0.5
    # frame_t(y, x) = frame1(y, x - 2), from both directions, where both cover the cell
    big = _frame(2, 24, 44, seed=2)
    f1, f2 = big[:, :, 4:].contiguous(), big[:, :, :40].contiguous()
    assert torch.equal(f2[:, :, 4:], f1[:, :, :36])
    fw = torch.zeros(2, 24, 40, 2)
    fw[..., 0] = 4.0
    out, holes = interpolate_frames(f1, f2, fw, -fw, 0.5)
    assert not holes.any()
    assert torch.equal(out[:, :, 2:38], f1[:, :, :36])
    # the borders come from the one direction that reaches them
    assert torch.equal(out[:, :, 38:], f1[:, :, 36:38]) and torch.equal(out[:, :, :2], f2[:, :, 2:4])


def test_temporal_weights():
    a = torch.zeros(1, 8, 9, 3, dtype=torch.uint8)
    b = torch.full((1, 8, 9, 3), 200, dtype=torch.uint8)
    z = torch.zeros(1, 8, 9, 2)
    out, holes = interpolate_frames(a, b, z, z, 64 / 256)
    assert not holes.any() and (out == 50).all()
    out, _ = interpolate_frames(a, b, z, z, 0.75)
    assert (out == 150).all()


def test_constant_colour_survives_random_fractional_flows():
    B, h, w = 2, 33, 41
    col = torch.tensor([7, 130, 255], dtype=torch.uint8)
    f = col.expand(B, h, w, 3).contiguous()
    fw, bw = _flows(B, h, w, 3, scale=6.0)
    occ_fw, occ_bw = torch.rand(B, h, w, generator=torch.Generator().manual_seed(4)) < 0.4, torch.zeros(B, h, w, dtype=torch.bool)
    for t in (0.1, 0.5, 0.83):
        out, holes = interpolate_frames(f, f, fw, bw, t, occ_fw, occ_bw, min_cover=0.25)
        assert 0 < int(holes.sum()) < holes.numel()
        assert (out == col).all()           # non-holes exactly; holes fall back to the same colour


def test_a_consistent_source_dominates_an_occluded_one():
    h, w = 6, 7
    f1 = torch.zeros(1, h, w, 3, dtype=torch.uint8)
    f1[0, 1, 1] = 255                       # consistent, lands on (3, 4)
    f1[0, 4, 2] = 0                         # occluded, lands on (3, 4)
    fw = torch.full((1, h, w, 2), NAN)
    fw[0, 1, 1] = torch.tensor([6.0, 4.0])  # t = 0.5: half of it
    fw[0, 4, 2] = torch.tensor([4.0, -2.0])
    occ = torch.zeros(1, h, w, dtype=torch.bool)
    occ[0, 4, 2] = True
    bw = torch.full((1, h, w, 2), NAN)
    out, holes, acc = interpolate_frames(f1, f1, fw, bw, 0.5, occ, None, return_acc=True)
    assert int((~holes).sum()) == 1 and not holes[0, 3, 4]
    assert acc[0, 0, 3, 4].tolist() == [256 * 17, 256 * 16 * 255] * 1 + [256 * 16 * 255] * 2 and not acc[1].any()
    assert out[0, 3, 4].tolist() == [240, 240, 240]
    # without the mask both weigh the same: (255 + 0) / 2 rounds half up
    out, _ = interpolate_frames(f1, f1, fw, bw, 0.5)
    assert out[0, 3, 4].tolist() == [128, 128, 128]
    assert R.CONSISTENT == 16


def test_bad_flows_contribute_nothing():
    f1, f2 = _frame(1, 9, 11, seed=5), _frame(1, 9, 11, seed=6)
    fw = torch.zeros(1, 9, 11, 2)
    fw[0, :3] = NAN
    fw[0, 3:5, :, 0] = float("inf")
    fw[0, 5:7, :, 1] = float("-inf")
    fw[0, 7:] = 1e9
    bw = torch.full((1, 9, 11, 2), -1e30)
    bw[0, 0, 0] = torch.tensor([0.0, NAN])
    out, holes, acc = interpolate_frames(f1, f2, fw, bw, 0.5, return_acc=True)
    assert holes.all() and not acc.any() and torch.equal(out, f1)
    # just inside and just outside the -1 < p < size range of the landing point
    fw = torch.full((1, 9, 11, 2), NAN)
    fw[0, 4, 0, :] = torch.tensor([-2.0 + 2.0 ** -10, 0.0])     # px = -1 + 2^-11: a sliver of weight -> quantised to 0
    fw[0, 4, 1, :] = torch.tensor([-3.0, 0.0])                  # px = -0.5: half on column 0
    fw[0, 4, 2, :] = torch.tensor([-6.0, 0.0])                  # px = -1 exactly: outside
    fw[0, 4, 10, :] = torch.tensor([1.75, 0.0])                 # px = 10.875: 2/16 on column 10
    fw[0, 5, 10, :] = torch.tensor([2.0, 0.0])                  # px = 11 = W0: outside
    _, _, acc = interpolate_frames(f1, f2, fw, bw, 0.5, return_acc=True)
    want = torch.zeros(9, 11, dtype=torch.int64)
    want[4, 0] = 8 * 16 * 16
    want[4, 10] = 2 * 16 * 16
    assert torch.equal(acc[0, 0, :, :, 0], want)


def test_hole_fallback_takes_the_nearer_frame():
    f1, f2 = _frame(1, 5, 6, seed=7), _frame(1, 5, 6, seed=8)
    bad = torch.full((1, 5, 6, 2), NAN)
    for t, want in ((128 / 256, f1), (129 / 256, f2), (0.1, f1), (0.9, f2)):
        out, holes = interpolate_frames(f1, f2, bad, bad, t)
        assert holes.all() and torch.equal(out, want)


def test_min_cover_is_in_units_of_full_double_coverage():
    f = _frame(1, 6, 6, seed=9)
    z = torch.zeros(1, 6, 6, 2)
    bad = torch.full((1, 6, 6, 2), NAN)
    assert R.interp_params(0.5, 1.0) == (128, 1 << 20) and R.interp_params(0.5, 0.0) == (128, 1)
    assert R.interp_params(0.25)[1] == (1 << 20) // 64
    assert not interpolate_frames(f, f, z, z, 0.3, min_cover=1.0)[1].any()          # D == 2^20 exactly
    assert interpolate_frames(f, f, z, bad, 0.5, min_cover=0.5 + 2.0 ** -20)[1].all()    # one direction: D == 2^19
    assert not interpolate_frames(f, f, z, bad, 0.5, min_cover=0.5)[1].any()
    occ = torch.ones(1, 6, 6, dtype=torch.bool)
    assert not interpolate_frames(f, f, z, z, 0.5, occ, occ, min_cover=1 / 16)[1].any()  # all occluded: D == 2^16
    assert interpolate_frames(f, f, z, z, 0.5, occ, occ, min_cover=1 / 16 + 2.0 ** -20)[1].all()


def test_window_equals_the_cropped_op():
    f1, f2 = _frame(2, seed=10), _frame(2, seed=11)
    fw, bw = _flows(2, H, W, 12, scale=8.0)
    g = torch.Generator().manual_seed(13)
    occ_fw, occ_bw = torch.rand(2, H, W, generator=g) < 0.3, torch.rand(2, H, W, generator=g) < 0.3
    full = interpolate_frames(f1, f2, fw, bw, 0.3, occ_fw, occ_bw, WIN, return_acc=True)
    crop = lambda v: v[:, TOP:TOP + H0, LEFT:LEFT + W0].contiguous()
    part = interpolate_frames(f1, f2, crop(fw), crop(bw), 0.3, crop(occ_fw), crop(occ_bw), return_acc=True)
    assert all(torch.equal(a, b) for a, b in zip(full, part))
    assert 0 < int(full[1].sum()) < full[1].numel()
    # what lies outside the window is not read
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[TOP:TOP + H0, LEFT:LEFT + W0] = True
    fw2, bw2, o1, o2 = fw.clone(), bw.clone(), occ_fw.clone(), occ_bw.clone()
    fw2[:, ~inside] = NAN
    bw2[:, ~inside] = 0.0
    o1[:, ~inside] = True
    o2[:, ~inside] = True
    again = interpolate_frames(f1, f2, fw2, bw2, 0.3, o1, o2, WIN, return_acc=True)
    assert all(torch.equal(a, b) for a, b in zip(full, again))


def _by_hand(f1, f2, fw, bw, t, occ_fw, occ_bw, min_cover):
    """Steps 0 to 5 of the docstring, pixel by pixel, on numpy fp32 scalars and Python integers."""
    f32 = np.float32
    B, h, w, _ = fw.shape
    tq = int(np.rint(t * 256))
    dmin = max(1, math.ceil(min_cover * 2 ** 20))
    acc = [[[[[0, 0, 0, 0] for _ in range(w)] for _ in range(h)] for _ in range(B)] for _ in range(2)]
    for d, (frame, flow, occ, step) in enumerate(((f1, fw, occ_fw, tq), (f2, bw, occ_bw, 256 - tq))):
        s = f32(step) / f32(256)
        fl = flow.numpy()
        for b in range(B):
            for y in range(h):
                for x in range(w):
                    px = f32(x) + f32(s * fl[b, y, x, 0])
                    py = f32(y) + f32(s * fl[b, y, x, 1])
                    if not (px > -1 and px < w and py > -1 and py < h):
                        continue
                    x0, y0 = np.floor(px), np.floor(py)
                    qx, qy = int(np.rint(f32(f32(px - x0) * f32(16)))), int(np.rint(f32(f32(py - y0) * f32(16))))
                    k = 1 if (occ is not None and bool(occ[b, y, x])) else 16
                    col = [1] + [int(v) for v in frame[b, y, x]]
                    for dy in (0, 1):
                        for dx in (0, 1):
                            tx, ty = int(x0) + dx, int(y0) + dy
                            wgt = (qx if dx else 16 - qx) * (qy if dy else 16 - qy) * k
                            if 0 <= tx < w and 0 <= ty < h:
                                for c in range(4):
                                    acc[d][b][ty][tx][c] += wgt * col[c]
    out = torch.zeros(B, h, w, 3, dtype=torch.uint8)
    holes = torch.zeros(B, h, w, dtype=torch.bool)
    for b in range(B):
        for y in range(h):
            for x in range(w):
                tot = [(256 - tq) * acc[0][b][y][x][c] + tq * acc[1][b][y][x][c] for c in range(4)]
                if tot[0] < dmin:
                    holes[b, y, x] = True
                    out[b, y, x] = (f1 if tq <= 128 else f2)[b, y, x]
                else:
                    out[b, y, x] = torch.tensor([(2 * n + tot[0]) // (2 * tot[0]) for n in tot[1:]], dtype=torch.uint8)
    return out, holes, torch.tensor(acc, dtype=torch.int64)


@pytest.mark.parametrize("t,with_occ", [(0.5, True), (77 / 256, False), (0.9, True)])
def test_independent_per_pixel_reading(t, with_occ):
    B, h, w = 2, 10, 12
    f1, f2 = _frame(B, h, w, seed=14), _frame(B, h, w, seed=15)
    fw, bw = _flows(B, h, w, 16, scale=2.5)
    fw[0, 2, 3] = torch.tensor([0.5 / 16 * 2, -1.5 / 16 * 2])    # ties of the 1/16 quantisation at t = 0.5
    fw[0, 3, 3] = torch.tensor([NAN, 0.0])
    bw[1, 4, 5] = torch.tensor([float("inf"), 1.0])
    fw[:, 6:9, 6:10, 0], bw[:, 6:9, 6:10, 0] = 30.0, -30.0      # nothing lands there from these: holes nearby
    g = torch.Generator().manual_seed(17)
    occ = [torch.rand(B, h, w, generator=g) < 0.3 for _ in range(2)] if with_occ else [None, None]
    got = interpolate_frames(f1, f2, fw, bw, t, occ[0], occ[1], min_cover=1 / 64, return_acc=True)
    want = _by_hand(f1, f2, fw, bw, t, occ[0], occ[1], 1 / 64)
    assert torch.equal(got[2], want[2])
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    assert 0 < int(want[1].sum()) < want[1].numel()


def test_rejected_times_and_covers():
    f = _frame(1, 4, 4)
    z = torch.zeros(1, 4, 4, 2)
    for t in (0.0, 1.0, NAN, 2.0, -0.5, 1 / 1024, float("inf")):
        with pytest.raises(ValueError, match="interpolate_frames"):
            interpolate_frames(f, f, z, z, t)
    for mc in (-0.01, 1.01, NAN):
        with pytest.raises(ValueError, match="min_cover"):
            interpolate_frames(f, f, z, z, 0.5, min_cover=mc)
    assert R.interp_params(1 / 256) == (1, 16384) and R.interp_params(255 / 256)[0] == 255


# ------------------------------------------------------------------ front end
def test_native_front_end_on_cpu_is_the_golden_op():
    f1, f2 = _frame(2, seed=18), _frame(2, seed=19)
    fw, bw = _flows(2, H, W, 20, scale=8.0)
    g = torch.Generator().manual_seed(21)
    occ_fw, occ_bw = torch.rand(2, H, W, generator=g) < 0.3, torch.rand(2, H, W, generator=g) < 0.3
    for args in ((f1, f2, fw, bw, 0.4, occ_fw, occ_bw, WIN), (f1, f2, fw, bw, 0.4, None, None, WIN),
                 (f1, f2, fw, bw, 0.7, occ_fw, None, WIN, 0.1)):
        got, want = nat.interpolate_frames(*args), interpolate_frames(*args)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ts = (0.25, 0.5, 0.75)
    frames, holes = nat.interpolate_frames(f1, f2, fw, bw, ts, occ_fw, occ_bw, WIN)
    assert frames.shape == (3, 2, H0, W0, 3) and frames.dtype == torch.uint8
    assert holes.shape == (3, 2, H0, W0) and holes.dtype == torch.bool
    for k, t in enumerate(ts):
        want = interpolate_frames(f1, f2, fw, bw, t, occ_fw, occ_bw, WIN)
        assert torch.equal(frames[k], want[0]) and torch.equal(holes[k], want[1])
    one = nat.interpolate_frames(f1, f2, fw, bw, [0.5], occ_fw, occ_bw, WIN)
    assert one[0].shape == (1, 2, H0, W0, 3) and torch.equal(one[0][0], frames[1])
    good = (f1, f2, fw, bw, 0.5, occ_fw, occ_bw, WIN)

    def bad(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        with pytest.raises(ValueError, match="interpolate_frames"):
            nat.interpolate_frames(*a)

    bad(_2=fw.double())
    bad(_3=bw[..., :1])
    bad(_3=bw[:1])
    bad(_0=f1.float())
    bad(_1=f2[:, 1:])
    bad(_5=occ_fw.byte())
    bad(_6=occ_bw[:, :H0])
    bad(_7=(122, 150, 7, 1))
    bad(_7=None)
    bad(_4=0.0)
    bad(_4=[])
    bad(_4=[0.5, 1.0])
    with pytest.raises(ValueError, match="min_cover"):
        nat.interpolate_frames(*good, min_cover=2.0)


def test_package_exports():
    assert jax_raft_amd.BidirectionalInterp is BidirectionalInterp is R.BidirectionalInterp
    assert jax_raft_amd.interpolate_frames is interpolate_frames is R.interpolate_frames
    assert BidirectionalInterp._fields == ("flows_fw", "flows_bw", "occ_fw", "occ_bw", "frames", "holes")
    for n in ("BidirectionalInterp", "interpolate_frames"):
        assert n in jax_raft_amd.__all__
    for n in ("interpolate_frames", "BidirectionalInterp"):
        assert n in R.__all__


# ------------------------------------------------------------------- lowering
@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(nat, "require", lambda: None)
    monkeypatch.setattr(nat, "new_plan", FakePlan)
    monkeypatch.setattr(tunedb, "gpu_arch", lambda device=None: "cpu")


def _shape(plan):
    """The recorded op list without addresses: tensors as (shape, dtype)."""
    def one(a):
        if isinstance(a, torch.Tensor):
            return (tuple(a.shape), str(a.dtype))
        if isinstance(a, (list, tuple)):
            return tuple(one(v) for v in a)
        return a
    return [(s, ln, d, op, one(args)) for s, ln, d, op, args in plan.ops]


def _u8_key(eng, B, n=3, all_iters=True):
    z = torch.zeros(B, H0, W0, 3, dtype=torch.uint8)
    return eng._key(z, z, n, all_iters)


def _generic_mask_model():
    model = raft_large()[0].eval()
    model.mask_predictor = MaskPredictor(in_channels=128, hidden_size=64)   # no convex-head kernel: not slot_ok
    return model


LOWERINGS = {"large_b1": (lambda: raft_large()[0].eval(), 1, True), "large_b2": (lambda: raft_large()[0].eval(), 2, True),
             "small_b1": (lambda: raft_small()[0].eval(), 1, True), "generic_mask_b1": (_generic_mask_model, 1, False),
             "generic_mask_b2": (_generic_mask_model, 2, False)}


@pytest.mark.parametrize("case", sorted(LOWERINGS))
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("all_iters", [True, False])
def test_interp_lowering(fake, case, K, all_iters):
    make, B, slot_ok = LOWERINGS[case]
    eng = E.RaftEngine(make(), "cpu", autotune=False)
    n = 3
    key = _u8_key(eng, B, n, all_iters)
    assert key[:3] == (B, H, W) and key[5:] == ("u8",) + WIN
    bidir = eng._build_key(key + ("bidir",))
    before = _shape(bidir.plan)
    st = eng._build_key(key + ("bidir", "interp", K))
    ops = st.plan.ops
    assert st.slot_ok == slot_ok
    # the bidirectional plan's list, entry for entry, then K x (memset, interp_splat, interp_resolve)
    assert len(ops) == len(before) + 3 * K and _shape(st.plan)[:len(before)] == before
    assert [op for *_, op, _ in ops[len(before):]] == ["memset", "interp_splat", "interp_resolve"] * K
    assert ops[len(before) - 1][3] == "fb_check"
    assert all((s, ln, d) == (2, 0, 0) for s, ln, d, _, _ in ops[len(before) - 1:])
    for f in ("acc", "par", "interp", "holes", "warped", "photo"):
        assert getattr(bidir, f) is None
    assert st.warped is None and st.photo is None
    assert not any(op.startswith("interp") for *_, op, _ in bidir.plan.ops)
    # the plan-owned buffers
    assert tuple(st.acc.shape) == (2, B, H0, W0, 4) and st.acc.dtype == torch.int64
    assert tuple(st.par.shape) == (K, 2) and st.par.dtype == torch.int32
    assert tuple(st.interp.shape) == (K, B, H0, W0, 3) and st.interp.dtype == torch.uint8
    assert tuple(st.holes.shape) == (K, B, H0, W0) and st.holes.dtype == torch.uint8
    (ft, fi), = [args for *_, op, args in ops if op == "fb_check"]
    last = ((n if all_iters else 1) - 1) * 2 * B * H * W * 2
    for k in range(K):
        (cleared,), = ops[len(before) + 3 * k][4]
        assert cleared is st.acc
        t, i = ops[len(before) + 3 * k + 1][4]
        # the uint8 window reaches the op, the check's ints; the frames as uploaded; the plan's masks
        assert list(i[:8]) == [B, H, W, H0, W0, TOP, LEFT, k] and list(i[:7]) == list(fi[:7])
        assert t[0] is st.inp1 and t[1] is st.inp2 and t[4] is st.occ and t[4] is ft[2] and t[5] is st.acc and t[6] is st.par
        if slot_ok:   # the flows of the final iteration through the slot
            assert t[2] is None and t[3] is None and t[7] is st.out_slot and len(t) == 8
            assert list(i[8:]) == [last, last + B * H * W * 2] == list(fi[7:])
        else:         # ... or the two halves of out[-1]
            assert len(t) == 7 and len(i) == 8
            for d in range(2):
                assert t[2 + d].data_ptr() == st.out[-1][d * B:(d + 1) * B].data_ptr() == ft[d].data_ptr()
                assert tuple(t[2 + d].shape) == (B, H, W, 2)
        rt, ri = ops[len(before) + 3 * k + 2][4]
        assert list(ri) == [B, H0, W0, k]
        assert rt[0] is st.inp1 and rt[1] is st.inp2 and rt[2] is st.acc and rt[3] is st.par
        assert rt[4].data_ptr() == st.interp[k].data_ptr() and tuple(rt[4].shape) == (B, H0, W0, 3)
        assert rt[5].data_ptr() == st.holes[k].data_ptr() and tuple(rt[5].shape) == (B, H0, W0)
    # bidirectional, warp and cold plans are rebuilt the same afterwards
    assert _shape(eng._build_key(key + ("bidir",)).plan) == before
    warp = eng._build_key(key + ("bidir", "warp"))
    assert [op for *_, op, _ in warp.plan.ops[len(before):]] == ["memset", "warp_frames"] and warp.acc is None
    cold = eng._build_key(key)
    assert not any(op in ("fb_check", "interp_splat", "interp_resolve") for *_, op, _ in cold.plan.ops)


@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_interp_int_lists_lie_inside_the_table(fake):
    arity = {op: tuple(torch.ops.jax_raft_amd.op_arity(op)) for op in ("interp_splat", "interp_resolve")}
    assert arity == {"interp_splat": (1, 8, 10), "interp_resolve": (1, 4, 4)}
    for make in (lambda: raft_small()[0].eval(), _generic_mask_model):
        eng = E.RaftEngine(make(), "cpu", autotune=False)
        for all_iters in (True, False):
            st = eng._build_key(_u8_key(eng, 1, 3, all_iters) + ("bidir", "interp", 2))
            seen = [(op, args) for *_, op, args in st.plan.ops if op in arity]
            assert len(seen) == 4
            for op, (t, i) in seen:
                assert arity[op][1] <= len(i) <= arity[op][2]
    plan = torch.classes.jax_raft_amd.Plan()
    assert hasattr(plan, "add_interp_splat") and hasattr(plan, "add_interp_resolve")


# ----------------------------------------------------------------- rejections
def _pair(B=1, Hh=128, Ww=128):
    g = torch.Generator().manual_seed(3)
    return torch.rand(B, Hh, Ww, 3, generator=g) * 2 - 1, torch.rand(B, Hh, Ww, 3, generator=g) * 2 - 1


def _u8_pair(B=1):
    return _frame(B, seed=22), _frame(B, seed=23)


def test_engine_rejections(fake):
    i1, i2 = _pair()
    u1, u2 = _u8_pair()
    eng = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False)
    with pytest.raises(ValueError, match="bidirectional=True"):
        eng.forward(u1, u2, 3, interpolate=0.5)
    with pytest.raises(ValueError, match="uint8"):
        eng.forward(i1, i2, 3, bidirectional=True, interpolate=0.5)
    with pytest.raises(ValueError, match="uint8"):
        eng.forward(u1, i2[:, :H0, :W0].contiguous(), 3, bidirectional=True, interpolate=0.5)
    with pytest.raises(ValueError, match="warp"):
        eng.forward(u1, u2, 3, bidirectional=True, warp=True, interpolate=0.5)
    for t in (0.0, 1.0, NAN, 2.0, [], [0.5] * 9, [0.5, 1.5]):
        with pytest.raises(ValueError, match="interpolate_frames"):
            eng.forward(u1, u2, 3, bidirectional=True, interpolate=t)
    with pytest.raises(ValueError, match="min_cover"):
        eng.forward(u1, u2, 3, bidirectional=True, interpolate=0.5, interp_min_cover=1.5)
    # what is out of scope for bidirectional stays out of scope, with the same errors
    for a, b in ((i1, i2), (u1, u2)):
        with pytest.raises(NotImplementedError, match="flow_init"):
            eng.forward(a, b, 3, bidirectional=True, interpolate=0.5, flow_init=torch.zeros(1, 16, 16, 2))
        with pytest.raises(NotImplementedError, match="flow_init"):
            eng.forward(a, b, 3, bidirectional=True, interpolate=0.5, flow_init="previous")
        with pytest.raises(NotImplementedError, match="return_flow_low"):
            eng.forward(a, b, 3, bidirectional=True, interpolate=0.5, return_flow_low=True)
    with pytest.raises(NotImplementedError, match="pipelined"):
        eng.pipelined(u1, u2, 3, bidirectional=True)
    assert eng.num_plans() == 0
    cp = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False, cp_group=True)
    with pytest.raises(NotImplementedError, match="context parallelism"):
        cp.forward(u1, u2, 3, bidirectional=True, interpolate=0.5)
    for precision in ("fp32", "mixed"):
        e = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False, precision=precision)
        with pytest.raises(NotImplementedError, match=precision):
            e.forward(u1, u2, 3, bidirectional=True, interpolate=0.5)
    od = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False, corr="on_demand")
    with pytest.raises(NotImplementedError, match="on_demand"):
        od.forward(u1, u2, 3, bidirectional=True, interpolate=0.5)


def test_model_rejections():
    model = raft_small()[0]
    i1, i2 = _pair()
    u1, u2 = _u8_pair()
    with pytest.raises(ValueError, match="bidirectional=True"):
        model(u1, u2, interpolate=0.5)
    with pytest.raises(ValueError, match="uint8"):
        model(i1, i2, bidirectional=True, interpolate=0.5)
    with pytest.raises(ValueError, match="warp"):
        model(u1, u2, bidirectional=True, warp=True, interpolate=0.5)
    for t in (0.0, 1.0, NAN, [0.5] * 9, []):
        with pytest.raises(ValueError, match="interpolate_frames"):
            model(u1, u2, bidirectional=True, interpolate=t)
    with pytest.raises(ValueError, match="min_cover"):
        model(u1, u2, bidirectional=True, interpolate=0.5, interp_min_cover=-1.0)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(u1, u2, train=True, bidirectional=True, interpolate=0.5)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(u1, u2, autograd=True, bidirectional=True, interpolate=0.5)
    with pytest.raises(NotImplementedError, match="flow_init"):
        model(u1, u2, bidirectional=True, interpolate=0.5, flow_init=torch.zeros(1, 16, 19, 2))
    with pytest.raises(NotImplementedError, match="return_flow_low"):
        model(u1, u2, bidirectional=True, interpolate=0.5, return_flow_low=True)


# ------------------------------------------------------------ golden-path API
def test_cpu_model_returns_the_six_field_tuple():
    model, variables = raft_small()
    f1, f2 = _u8_pair()
    res = model(f1, f2, num_flow_updates=1, bidirectional=True, interpolate=(0.25, 0.5))
    assert isinstance(res, BidirectionalInterp) and len(res) == 6
    plain = model(f1, f2, num_flow_updates=1, bidirectional=True)
    assert isinstance(plain, BidirectionalFlow)
    assert all(torch.equal(a, b) for a, b in zip(res[:4], plain))
    assert res.frames.shape == (2, 1, H0, W0, 3) and res.frames.dtype == torch.uint8
    assert res.holes.shape == (2, 1, H0, W0) and res.holes.dtype == torch.bool
    for k, t in enumerate((0.25, 0.5)):
        want = interpolate_frames(f1, f2, res.flows_fw[-1], res.flows_bw[-1], t, res.occ_fw, res.occ_bw)
        assert torch.equal(res.frames[k], want[0]) and torch.equal(res.holes[k], want[1])
    # a float is one time; through apply, with another cover
    res1 = model.apply(variables, f1, f2, num_flow_updates=1, return_all_iters=False, bidirectional=True, interpolate=0.5,
                       interp_min_cover=0.5)
    assert isinstance(res1, BidirectionalInterp) and res1.frames.shape == (1, 1, H0, W0, 3)
    want = interpolate_frames(f1, f2, res1.flows_fw[-1], res1.flows_bw[-1], 0.5, res1.occ_fw, res1.occ_bw, min_cover=0.5)
    assert torch.equal(res1.frames[0], want[0]) and torch.equal(res1.holes[0], want[1])
    assert fb_consistency is jax_raft_amd.fb_consistency
