"""Motion-compensated frames + masked photometric error, without a GPU: the golden op
(models/reference.py:warp_frames), photometric_error, the lowering of the "warp" plan (recorded on
a FakePlan), the rejections and the golden-path API."""
import math

import pytest
import torch

import jax_raft_amd
from jax_raft_amd import (BidirectionalFlow, BidirectionalWarp, fb_consistency, photometric_error, raft_large,
                          raft_small, warp_frames)
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import tunedb
from test_engine_lowering import FakePlan

H, W, WIN = 128, 152, (122, 150, 3, 1)
H0, W0, TOP, LEFT = WIN


def _translated_pair(B=2, seed=0):
    """Two frames cut from one random image: frame2(y, x) = frame1(y + 3, x - 2), so the flow
    1 -> 2 is (+2, -3) everywhere."""
    g = torch.Generator().manual_seed(seed)
    big = torch.randint(0, 256, (B, 140, 170, 3), dtype=torch.uint8, generator=g)
    return big[:, 5:127, 7:157].contiguous(), big[:, 8:130, 5:155].contiguous()


def _const(fx, fy, B=2):
    f = torch.zeros(B, H, W, 2)
    f[..., 0], f[..., 1] = fx, fy
    return f


def _frame(B=1, h=H0, w=W0, seed=1):
    return torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------ golden op
def test_integer_translation_reproduces_the_frame():
    f1, f2 = _translated_pair()
    fw = _const(2.0, -3.0)
    bw = -fw
    occ_fw, occ_bw = fb_consistency(fw, bw, window=WIN)
    for src, own, flow, occ, (dx, dy) in ((f2, f1, fw, occ_fw, (2, -3)), (f1, f2, bw, occ_bw, (-2, 3))):
        warped, photo = warp_frames(src, flow, occ, own, WIN)
        assert warped.dtype == torch.uint8 and warped.shape == own.shape
        assert photo.dtype == torch.int64 and photo.shape == (2, 2)
        assert torch.equal(warped, own)
        ys, xs = torch.meshgrid(torch.arange(H0), torch.arange(W0), indexing="ij")
        inside = (xs + dx >= 0) & (xs + dx <= W0 - 1) & (ys + dy >= 0) & (ys + dy <= H0 - 1)
        keep = inside & ~occ[:, TOP:TOP + H0, LEFT:LEFT + W0]
        assert 0 < int(keep[0].sum()) < H0 * W0
        assert photo[:, 0].tolist() == [0, 0] and photo[:, 1].tolist() == keep.sum((1, 2)).tolist()
        # the kept pixels really come from the sampled frame
        w0, _ = warp_frames(src, flow, occ, None, WIN)
        assert torch.equal(w0[keep], own[keep]) and not w0[~keep].any()


def test_edge_flows():
    src, own = _frame(seed=2), _frame(seed=3)
    flow = torch.zeros(1, H, W, 2)
    flow[0, TOP + 5, LEFT + 30, 0] = float(W0 - 1 - 30)          # px == W0 - 1 exactly: inside
    flow[0, TOP + 20, LEFT + 7, 1] = float(H0 - 1 - 20)          # py == H0 - 1 exactly: inside
    flow[0, TOP + 6, LEFT + 30, 0] = float(W0 - 1 - 30) + 0.5    # just outside
    flow[0, TOP + 7, LEFT + 3, 0] = -3.0 - 2.0 ** -10            # just outside, to the left
    flow[0, TOP + 8, LEFT + 9] = float("nan")
    flow[0, TOP + 9, LEFT + 9, 1] = 1e9                          # far outside
    flow[0, :TOP] = float("nan")                                 # outside the window: never read
    flow[0, :, :LEFT] = float("nan")
    warped, photo = warp_frames(src, flow, None, own, WIN)
    assert torch.equal(warped[0, 5, 30], src[0, 5, W0 - 1]) and torch.equal(warped[0, 20, 7], src[0, H0 - 1, 7])
    masked = [(6, 30), (7, 3), (8, 9), (9, 9)]
    for y, x in masked:
        assert torch.equal(warped[0, y, x], own[0, y, x])
    keep = torch.ones(H0, W0, dtype=torch.bool)
    for y, x in masked:
        keep[y, x] = False
    assert int(photo[0, 1]) == H0 * W0 - len(masked)
    # zero flow elsewhere: warped == src on the untouched pixels, so the sum is that of |src - own|
    same = keep.clone()
    same[5, 30] = same[20, 7] = False
    assert torch.equal(warped[0][same], src[0][same])
    want = (warped[0].long() - own[0].long()).abs().sum(-1)[keep].sum()
    assert int(photo[0, 0]) == int(want) > 0
    bare, none = warp_frames(src, flow, None, None, WIN)
    assert none is None
    for y, x in masked:
        assert not bare[0, y, x].any()
    assert torch.equal(bare[0][keep], warped[0][keep])
    # a mask drops more
    occ = torch.zeros(1, H, W, dtype=torch.bool)
    occ[0, TOP + 40:TOP + 50, LEFT + 10:LEFT + 20] = True
    occ[0, :TOP] = True                                          # outside the window: ignored
    w2, p2 = warp_frames(src, flow, occ, own, WIN)
    assert int(p2[0, 1]) == int(photo[0, 1]) - 100 and torch.equal(w2[0, 40:50, 10:20], own[0, 40:50, 10:20])


def test_half_pixel_ties_round_to_even():
    # texel pairs (a, a + d) with odd d: the midpoint a + d / 2 is x.5 exactly and rounds to even
    src = torch.zeros(1, 4, 8, 3, dtype=torch.uint8)
    row = torch.tensor([10, 11, 14, 17, 18, 23, 22, 22], dtype=torch.uint8)
    src[0, :, :, 0] = row
    src[0, :, :, 1] = 255 - row
    src[0, :, :, 2] = row
    flow = torch.zeros(1, 4, 8, 2)
    flow[..., 0] = 0.5
    flow[0, :, 7, 0] = 0.0
    warped, _ = warp_frames(src, flow)
    mid = (row[:-1].float() + row[1:].float()) / 2            # 10.5 12.5 15.5 17.5 20.5 22.5 22
    assert mid[:6].frac().eq(0.5).all()
    want = torch.tensor([10, 12, 16, 18, 20, 22, 22, 22], dtype=torch.uint8)
    assert torch.equal(warped[0, 1, :, 0], want) and torch.equal(warped[0, 2, :, 2], want)
    mid1 = ((255 - row[:-1]).float() + (255 - row[1:]).float()) / 2   # 244.5 242.5 239.5 237.5 234.5 232.5 233
    want1 = torch.tensor([244, 242, 240, 238, 234, 232, 233, 233], dtype=torch.uint8)
    assert mid1[:6].frac().eq(0.5).all() and torch.equal(warped[0, 0, :, 1], want1)
    # the same along y
    flow_y = torch.zeros(1, 8, 4, 2)
    flow_y[..., 1] = 0.5
    flow_y[0, 7, :, 1] = 0.0
    wy, _ = warp_frames(src.permute(0, 2, 1, 3).contiguous(), flow_y)
    assert torch.equal(wy[0, :, 1, 0], want)


def test_window_equals_the_cropped_op():
    g = torch.Generator().manual_seed(4)
    src, own = _frame(2, seed=5), _frame(2, seed=6)
    flow = torch.randn(2, H, W, 2, generator=g) * 8
    occ = torch.rand(2, H, W, generator=g) < 0.3
    full = warp_frames(src, flow, occ, own, WIN)
    crop = warp_frames(src, flow[:, TOP:TOP + H0, LEFT:LEFT + W0].contiguous(),
                       occ[:, TOP:TOP + H0, LEFT:LEFT + W0].contiguous(), own)
    assert torch.equal(full[0], crop[0]) and torch.equal(full[1], crop[1])
    assert (full[1][:, 1] > 0).all() and (full[1][:, 1] < H0 * W0).all() and (full[1][:, 0] > 0).all()
    # what lies outside the window is not read
    flow2, occ2 = flow.clone(), occ.clone()
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[TOP:TOP + H0, LEFT:LEFT + W0] = True
    flow2[:, ~inside] = float("nan")
    occ2[:, ~inside] = True
    again = warp_frames(src, flow2, occ2, own, WIN)
    assert torch.equal(again[0], full[0]) and torch.equal(again[1], full[1])


def test_agrees_with_grid_sample_within_one_level():
    """A sanity check of the definition against an independent primitive, not the yardstick."""
    g = torch.Generator().manual_seed(7)
    B, h, w = 2, 37, 53
    src = _frame(B, h, w, seed=8)
    flow = torch.randn(B, h, w, 2, generator=g) * 5
    warped, _ = warp_frames(src, flow)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    px, py = xs + flow[..., 0], ys + flow[..., 1]
    inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)
    grid = torch.stack([px / (w - 1) * 2 - 1, py / (h - 1) * 2 - 1], -1)
    ref = torch.nn.functional.grid_sample(src.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="border",
                                          align_corners=True).permute(0, 2, 3, 1)
    diff = (warped.float() - ref).abs()[inside]
    assert 0.3 < inside.float().mean() < 1.0 and diff.max() <= 1.0
    assert not warped[~inside].any()


def test_native_front_end_on_cpu_is_the_golden_op():
    g = torch.Generator().manual_seed(9)
    src, own = _frame(2, seed=10), _frame(2, seed=11)
    flow = torch.randn(2, H, W, 2, generator=g) * 8
    occ = torch.rand(2, H, W, generator=g) < 0.3
    for args in ((src, flow, occ, own, WIN), (src, flow, None, None, WIN), (src, flow, occ, None, WIN)):
        got, want = nat.warp_frames(*args), warp_frames(*args)
        assert torch.equal(got[0], want[0])
        assert (got[1] is None and want[1] is None) or torch.equal(got[1], want[1])
    for bad in ((src, flow.double(), occ, own, WIN), (src.float(), flow, occ, own, WIN), (src, flow, occ.byte(), own, WIN),
                (src, flow, occ, own[:, 1:], WIN), (src, flow, occ, own, (122, 150, 7, 1)), (src, flow, occ, own, None),
                (src, flow[..., :1], occ, own, WIN)):
        with pytest.raises(ValueError, match="warp_frames"):
            nat.warp_frames(*bad)


def test_photometric_error():
    photo = torch.tensor([[[300, 10], [0, 0]], [[0, 50], [7, 1]]], dtype=torch.int64)
    mae, cov = photometric_error(photo, (10, 20))
    assert mae.shape == cov.shape == (2, 2) and mae.dtype == torch.float64
    assert mae[0, 0] == 10.0 and math.isnan(mae[0, 1]) and mae[1, 0] == 0.0 and mae[1, 1] == 7 / 3
    assert cov.tolist() == [[0.05, 0.0], [0.25, 0.005]]
    with pytest.raises(ValueError):
        photometric_error(photo.float(), (10, 20))
    with pytest.raises(ValueError):
        photometric_error(photo, (0, 20))


def test_package_exports():
    assert jax_raft_amd.BidirectionalWarp is BidirectionalWarp and jax_raft_amd.warp_frames is warp_frames
    assert jax_raft_amd.photometric_error is photometric_error
    assert BidirectionalWarp._fields == ("flows_fw", "flows_bw", "occ_fw", "occ_bw", "warped_fw", "warped_bw", "photo")
    assert BidirectionalFlow._fields == ("flows_fw", "flows_bw", "occ_fw", "occ_bw")
    for n in ("BidirectionalWarp", "warp_frames", "photometric_error"):
        assert n in jax_raft_amd.__all__


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


LOWERINGS = {"large_b1": (raft_large, 1), "large_b2": (raft_large, 2), "small_b1": (raft_small, 1)}


@pytest.mark.parametrize("case", sorted(LOWERINGS))
@pytest.mark.parametrize("all_iters", [True, False])
def test_warp_lowering(fake, case, all_iters):
    factory, B = LOWERINGS[case]
    eng = E.RaftEngine(factory()[0].eval(), "cpu", autotune=False)
    n = 3
    key = _u8_key(eng, B, n, all_iters)
    assert key[:3] == (B, H, W) and key[5:] == ("u8",) + WIN
    bidir = eng._build_key(key + ("bidir",))
    before = _shape(bidir.plan)
    st = eng._build_key(key + ("bidir", "warp"))
    ops = st.plan.ops
    # the bidirectional plan's list, entry for entry, then exactly memset and warp_frames
    assert len(ops) == len(before) + 2 and _shape(st.plan)[:len(before)] == before
    assert [op for *_, op, _ in ops[-2:]] == ["memset", "warp_frames"] and ops[-3][3] == "fb_check"
    assert all((s, ln, d) == (2, 0, 0) for s, ln, d, _, _ in ops[-3:])
    assert sum(op == "warp_frames" for *_, op, _ in ops) == 1
    assert bidir.warped is None and bidir.photo is None and _shape(bidir.plan) == before
    assert not any(op == "warp_frames" for *_, op, _ in bidir.plan.ops)
    # the plan-owned buffers
    assert tuple(st.warped.shape) == (2, B, H0, W0, 3) and st.warped.dtype == torch.uint8
    assert tuple(st.photo.shape) == (2, B, 2) and st.photo.dtype == torch.int64
    (cleared,), = ops[-2][4]
    assert cleared is st.photo
    t, i = ops[-1][4]
    # the uint8 window reaches the op; both directions; the flows of the final iteration through the slot
    assert list(i[:8]) == [B, H, W, H0, W0, TOP, LEFT, 2] and st.src == WIN
    last = ((n if all_iters else 1) - 1) * 2 * B * H * W * 2
    assert list(i[8:]) == [last, last + B * H * W * 2]
    (ft, fi), = [args for *_, op, args in ops if op == "fb_check"]
    assert list(fi[7:]) == list(i[8:]) and list(fi[:7]) == list(i[:7])
    assert t[0] is st.inp2 and t[1] is st.inp1 and t[2] is st.inp1 and t[3] is st.inp2     # src (fw, bw), own (fw, bw)
    assert t[4] is None and t[5] is None and t[6] is st.occ and t[6] is ft[2]
    assert t[7] is st.warped and t[8] is st.photo and t[9] is st.out_slot
    # cold and bidirectional plans are rebuilt the same afterwards
    again = eng._build_key(key + ("bidir",))
    assert _shape(again.plan) == before
    cold = eng._build_key(key)
    assert not any(op in ("fb_check", "warp_frames") for *_, op, _ in cold.plan.ops)


@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_warp_int_lists_lie_inside_the_table(fake):
    sig, lo, hi = torch.ops.jax_raft_amd.op_arity("warp_frames")
    assert sig == 1 and (lo, hi) == (8, 10)
    eng = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False)
    for all_iters in (True, False):
        st = eng._build_key(_u8_key(eng, 1, 3, all_iters) + ("bidir", "warp"))
        (t, i), = [args for *_, op, args in st.plan.ops if op == "warp_frames"]
        assert lo <= len(i) <= hi
    assert hasattr(torch.classes.jax_raft_amd.Plan(), "add_warp_frames")


# ----------------------------------------------------------------- rejections
def _pair(B=1, Hh=128, Ww=128):
    g = torch.Generator().manual_seed(3)
    return torch.rand(B, Hh, Ww, 3, generator=g) * 2 - 1, torch.rand(B, Hh, Ww, 3, generator=g) * 2 - 1


def _u8_pair(B=1):
    return _frame(B, seed=12), _frame(B, seed=13)


def test_engine_rejections(fake):
    i1, i2 = _pair()
    u1, u2 = _u8_pair()
    eng = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False)
    with pytest.raises(ValueError, match="bidirectional=True"):
        eng.forward(u1, u2, 3, warp=True)
    with pytest.raises(ValueError, match="uint8"):
        eng.forward(i1, i2, 3, bidirectional=True, warp=True)
    with pytest.raises(ValueError, match="uint8"):
        eng.forward(u1, i2[:, :H0, :W0].contiguous(), 3, bidirectional=True, warp=True)
    # what is out of scope for bidirectional stays out of scope, with the same errors
    for a, b in ((i1, i2), (u1, u2)):
        with pytest.raises(NotImplementedError, match="flow_init"):
            eng.forward(a, b, 3, bidirectional=True, warp=True, flow_init=torch.zeros(1, 16, 16, 2))
        with pytest.raises(NotImplementedError, match="flow_init"):
            eng.forward(a, b, 3, bidirectional=True, warp=True, flow_init="previous")
        with pytest.raises(NotImplementedError, match="return_flow_low"):
            eng.forward(a, b, 3, bidirectional=True, warp=True, return_flow_low=True)
    with pytest.raises(NotImplementedError, match="pipelined"):
        eng.pipelined(u1, u2, 3, bidirectional=True)
    assert eng.num_plans() == 0
    cp = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False, cp_group=True)
    with pytest.raises(NotImplementedError, match="context parallelism"):
        cp.forward(u1, u2, 3, bidirectional=True, warp=True)
    for precision in ("fp32", "mixed"):
        e = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False, precision=precision)
        with pytest.raises(NotImplementedError, match=precision):
            e.forward(u1, u2, 3, bidirectional=True, warp=True)


def test_model_rejections():
    model = raft_small()[0]
    i1, i2 = _pair()
    u1, u2 = _u8_pair()
    with pytest.raises(ValueError, match="bidirectional=True"):
        model(u1, u2, warp=True)
    with pytest.raises(ValueError, match="uint8"):
        model(i1, i2, bidirectional=True, warp=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(u1, u2, train=True, bidirectional=True, warp=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(u1, u2, autograd=True, bidirectional=True, warp=True)
    with pytest.raises(NotImplementedError, match="flow_init"):
        model(u1, u2, bidirectional=True, warp=True, flow_init=torch.zeros(1, 16, 19, 2))
    with pytest.raises(NotImplementedError, match="return_flow_low"):
        model(u1, u2, bidirectional=True, warp=True, return_flow_low=True)


# ------------------------------------------------------------ golden-path API
def test_cpu_model_returns_the_seven_field_tuple():
    model, variables = raft_small()
    f1, f2 = _u8_pair()
    res = model(f1, f2, num_flow_updates=1, bidirectional=True, warp=True)
    assert isinstance(res, BidirectionalWarp) and len(res) == 7
    plain = model(f1, f2, num_flow_updates=1, bidirectional=True)
    assert isinstance(plain, BidirectionalFlow)
    assert all(torch.equal(a, b) for a, b in zip(res[:4], plain))
    assert res.flows_fw.shape == res.flows_bw.shape == (1, 1, H0, W0, 2)
    assert res.occ_fw.shape == res.occ_bw.shape == (1, H0, W0)
    assert res.warped_fw.shape == res.warped_bw.shape == (1, H0, W0, 3) and res.warped_fw.dtype == torch.uint8
    assert res.photo.shape == (2, 1, 2) and res.photo.dtype == torch.int64
    wf, pf = warp_frames(f2, res.flows_fw[-1], res.occ_fw, f1)
    wb, pb = warp_frames(f1, res.flows_bw[-1], res.occ_bw, f2)
    assert torch.equal(res.warped_fw, wf) and torch.equal(res.warped_bw, wb)
    assert torch.equal(res.photo, torch.stack([pf, pb]))
    # through apply, with thresholds that keep pixels
    res1 = model.apply(variables, f1, f2, num_flow_updates=1, return_all_iters=False, bidirectional=True, warp=True,
                       fb_alpha=0.0, fb_beta=1e6)
    assert isinstance(res1, BidirectionalWarp) and (res1.photo[:, :, 1] > 0).all()
    mae, cov = photometric_error(res1.photo, (H0, W0))
    assert torch.isfinite(mae).all() and ((cov > 0) & (cov <= 1)).all()
