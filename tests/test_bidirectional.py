"""Bidirectional flow + forward-backward occlusion masks, without a GPU: the golden op
(models/reference.py:fb_consistency), the lowering of the bidirectional plan (recorded on a
FakePlan), the out-of-scope rejections and the golden-path API."""
import pytest
import torch

import jax_raft_amd
from jax_raft_amd import BidirectionalFlow, fb_consistency, raft_large, raft_small
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import tunedb
from test_engine_lowering import FakePlan

H, W = 24, 40


def _grid():
    return torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")


def _const(fx, fy, B=1):
    f = torch.zeros(B, H, W, 2)
    f[..., 0], f[..., 1] = fx, fy
    return f


# ------------------------------------------------------------------ golden op
def test_zero_flows_are_consistent():
    z = torch.zeros(2, H, W, 2)
    occ_fw, occ_bw = fb_consistency(z, z)
    assert occ_fw.dtype == torch.bool and occ_fw.shape == (2, H, W)
    assert not occ_fw.any() and not occ_bw.any()


def test_constant_translation():
    fw = _const(3.25, -2.5, B=2)
    occ_fw, occ_bw = fb_consistency(fw, -fw)
    ys, xs = _grid()
    want_fw = ~((xs + 3.25 <= W - 1) & (ys - 2.5 >= 0))
    want_bw = ~((xs - 3.25 >= 0) & (ys + 2.5 <= H - 1))
    for b in range(2):
        assert torch.equal(occ_fw[b], want_fw) and torch.equal(occ_bw[b], want_bw)


def test_inconsistent_patch_is_flagged_where_fw_lands_in_it():
    # fw = (4, 2) everywhere, bw = -fw except a zeroed rectangle rows 8..13, columns 10..19: a pixel
    # whose integer landing point lies in it has err = |fw|^2 = 20 against thr = 0.01 * 20 + 0.5
    fw = _const(4.0, 2.0)
    bw = -fw.clone()
    bw[:, 8:14, 10:20] = 0.0
    occ_fw, _, err_fw, _ = fb_consistency(fw, bw, return_err=True)
    ys, xs = _grid()
    ly, lx = ys + 2, xs + 4
    outside = (lx > W - 1) | (ly > H - 1)
    in_patch = (ly >= 8) & (ly < 14) & (lx >= 10) & (lx < 20)
    assert torch.equal(occ_fw[0], outside | in_patch)
    assert (err_fw[0][in_patch & ~outside] == 20.0).all() and torch.isinf(err_fw[0][outside]).all()
    assert (err_fw[0][~in_patch & ~outside] == 0.0).all()


def test_landing_on_the_last_column_and_row_is_inside():
    fw = torch.zeros(1, H, W, 2)
    fw[0, 5, 30, 0] = float(W - 1 - 30)      # px == W - 1 exactly
    fw[0, 20, 7, 1] = float(H - 1 - 20)      # py == H - 1 exactly
    fw[0, 6, 30, 0] = float(W - 1 - 30) + 0.5   # just outside
    bw = torch.zeros(1, H, W, 2)
    bw[0, 5, W - 1, 0] = -float(W - 1 - 30)
    bw[0, H - 1, 7, 1] = -float(H - 1 - 20)
    occ_fw, _, err_fw, _ = fb_consistency(fw, bw, return_err=True)
    assert not occ_fw[0, 5, 30] and err_fw[0, 5, 30] == 0.0
    assert not occ_fw[0, 20, 7] and err_fw[0, 20, 7] == 0.0
    assert occ_fw[0, 6, 30] and torch.isinf(err_fw[0, 6, 30])


def test_nan_flow_is_occluded():
    fw = torch.zeros(1, H, W, 2)
    fw[0, 3, 4, 0] = float("nan")
    bw = torch.zeros(1, H, W, 2)
    bw[0, 10, 10] = float("nan")             # a NaN gathered from the opposite flow
    occ_fw, occ_bw = fb_consistency(fw, bw)
    # a NaN tap poisons the bilinear sum even at weight 0 (0 * NaN = NaN): with zero flow the
    # four pixels whose 2 x 2 footprint holds the NaN are occluded, and the NaN pixel itself
    want_fw = torch.zeros(H, W, dtype=torch.bool)
    want_fw[3, 4] = True
    want_fw[9:11, 9:11] = True
    want_bw = torch.zeros(H, W, dtype=torch.bool)
    want_bw[10, 10] = True
    want_bw[2:4, 3:5] = True
    assert torch.equal(occ_fw[0], want_fw) and torch.equal(occ_bw[0], want_bw)


def _random_pair(seed=0, B=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, W, 2, generator=g) * 3, torch.randn(B, H, W, 2, generator=g) * 3


def test_window_equals_the_cropped_op():
    a, b = _random_pair()
    H0, W0, top, left = 21, 37, 1, 2
    full = fb_consistency(a, b, window=(H0, W0, top, left), return_err=True)
    crop = fb_consistency(a[:, top:top + H0, left:left + W0].contiguous(),
                          b[:, top:top + H0, left:left + W0].contiguous(), return_err=True)
    inside = torch.zeros(H, W, dtype=torch.bool)
    inside[top:top + H0, left:left + W0] = True
    for f, c in zip(full, crop):
        assert torch.equal(f[:, top:top + H0, left:left + W0].nan_to_num(), c.nan_to_num())
        assert not f[:, ~inside].any()     # masks False (and err 0) outside the rectangle
    assert full[0].any() and not full[0].all()


def test_native_front_end_on_cpu_is_the_golden_op():
    a, b = _random_pair(1)
    for kw in (dict(), dict(window=(21, 37, 1, 2)), dict(return_err=True)):
        got = nat.fb_check(a, b, 0.02, 0.25, **kw)
        want = fb_consistency(a, b, 0.02, 0.25, **kw)
        assert len(got) == len(want) and all(torch.equal(g, w_) for g, w_ in zip(got, want))


def test_package_exports():
    assert jax_raft_amd.BidirectionalFlow is BidirectionalFlow and jax_raft_amd.fb_consistency is fb_consistency
    assert BidirectionalFlow._fields == ("flows_fw", "flows_bw", "occ_fw", "occ_bw")


# ------------------------------------------------------------------- lowering
@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(nat, "require", lambda: None)
    monkeypatch.setattr(nat, "new_plan", FakePlan)
    monkeypatch.setattr(tunedb, "gpu_arch", lambda device=None: "cpu")


def _summary(plan):
    """The recorded op list in a comparable form: tensors as (address, shape)."""
    def one(a):
        if isinstance(a, torch.Tensor):
            return (a.data_ptr(), tuple(a.shape), str(a.dtype))
        if isinstance(a, (list, tuple)):
            return tuple(one(v) for v in a)
        return a
    return [(s, ln, d, op, one(args)) for s, ln, d, op, args in plan.ops]


def _fe_ops(st):
    """(lane, op, int list) of every op that touches a feature-encoder buffer or writes ``fmap``."""
    fe = {t.data_ptr() for k, t in st.bufs.items() if ".fe." in k or k.startswith("p0.fe.")}
    fmap = st.bufs["p0.fmap"]
    lo, hi = fmap.data_ptr(), fmap.data_ptr() + fmap.numel() * fmap.element_size()
    res = []
    for s, ln, d, op, args in st.plan.ops:
        if op in ("record", "wait", "corr"):
            continue
        ts = [t for t in args[0] if isinstance(t, torch.Tensor)]
        if any(t.data_ptr() in fe or lo <= t.data_ptr() < hi for t in ts):
            res.append((s, ln, op, tuple(args[1]) if len(args) > 1 else ()))
    return res


LOWERINGS = {"large_b1": (raft_large, 1), "large_b2": (raft_large, 2), "small_b1": (raft_small, 1)}


@pytest.mark.parametrize("case", sorted(LOWERINGS))
def test_bidirectional_lowering(fake, case):
    factory, B = LOWERINGS[case]
    eng = E.RaftEngine(factory()[0].eval(), "cpu", autotune=False)
    Hh, Ww, n = 128, 256, 3
    h, w = Hh // 8, Ww // 8
    cold = eng._build_key((B, Hh, Ww, n, True))
    before = _summary(cold.plan)
    st = eng._build_key((B, Hh, Ww, n, True, "bidir"))
    plan = st.plan
    assert len(st.plans) == 1 and tuple(st.out.shape) == (n, 2 * B, Hh, Ww, 2)
    assert tuple(st.occ.shape) == (2, B, Hh, Ww) and st.occ.dtype == torch.uint8
    # the loop batch 2B decides the schedule: batch 2 of raft_large lands on the lane schedule
    lanes = {ln for s, ln, _, op, _ in plan.ops if s == 1}
    if case == "large_b2":
        assert eng.uses_lanes(4) and not eng.uses_lanes(2) and lanes == {0, 2}
    else:
        assert lanes == {0}
    # the feature encoder is the cold plan's, op for op
    fe_cold, fe_bidir = _fe_ops(cold), _fe_ops(st)
    assert len(fe_cold) >= 20 and fe_bidir == fe_cold
    # two correlation launches over the swapped halves of one fmap, the second into the second half
    corrs = [args for _, _, _, op, args in plan.ops if op == "corr"]
    assert len(corrs) == 2 and sum(op == "corr" for *_, op, _ in cold.plan.ops) == 1
    fmap = st.bufs["p0.fmap"]
    assert tuple(fmap.shape)[0] == 2 * B
    (t0, i0, _), (t1, i1, _) = corrs
    assert t0[0].data_ptr() == fmap[:B].data_ptr() and t0[1].data_ptr() == fmap[B:].data_ptr()
    assert t1[0].data_ptr() == fmap[B:].data_ptr() and t1[1].data_ptr() == fmap[:B].data_ptr()
    assert list(i0) == list(i1) and i0[0] == B
    for l0, l1 in zip(t0[2:], t1[2:]):
        if l0 is None:
            assert l1 is None
            continue
        assert l0.shape[0] == 2 * B * h * w and l1.shape[0] == B * h * w
        assert l1.data_ptr() == l0[B * h * w:].data_ptr()
    # the loop runs at batch 2B
    lookups = [args for s, _, _, op, args in plan.ops if op == "lookup" and s == 1]
    assert len(lookups) == 1 and lookups[0][1][1] == 2 * B
    init = [args for *_, op, args in plan.ops if op == "init_coords"]
    assert len(init) == 1 and list(init[0][1]) == [2 * B, h, w]
    # one fb_check: segment 2, lane 0, after every upsampling op, inside the table's arity
    idx = [k for k, (_, _, _, op, _) in enumerate(plan.ops) if op == "fb_check"]
    assert len(idx) == 1
    s, ln, d, _, (t, i) = plan.ops[idx[0]]
    assert (s, ln, d) == (2, 0, 0)
    ups = [k for k, (_, _, _, op, _) in enumerate(plan.ops)
           if op in ("convex_head", "upsample_bilinear", "upsample_convex", "flowin_dual")]
    assert ups and max(ups) < idx[0]
    assert len(i) == 9
    assert list(i[:7]) == [B, Hh, Ww, Hh, Ww, 0, 0]
    # the final iteration's two halves, read through the output slot
    assert t[0] is None and t[1] is None and t[2] is st.occ and t[4] is st.thr and t[5] is st.out_slot
    assert list(i[7:]) == [(n - 1) * 2 * B * Hh * Ww * 2, (n - 1) * 2 * B * Hh * Ww * 2 + B * Hh * Ww * 2]
    # the cold plan: untouched by the bidirectional build, and rebuilt the same
    assert _summary(cold.plan) == before
    again = eng._build_key((B, Hh, Ww, n, True))
    assert [(s, ln, d, op) for s, ln, d, op, _ in again.plan.ops] == [(s, ln, d, op) for s, ln, d, op, _ in before]
    assert not any(op == "fb_check" for *_, op, _ in again.plan.ops)


@pytest.mark.skipif(not nat.available(), reason="native library not built")
@pytest.mark.parametrize("case", sorted(LOWERINGS))
def test_fb_check_int_lists_lie_inside_the_table(fake, case):
    """The recorded int lists (slot form, and the tensor form of the eager front-end) against the
    op table's arity, which the built library reports."""
    factory, B = LOWERINGS[case]
    eng = E.RaftEngine(factory()[0].eval(), "cpu", autotune=False)
    sig, lo, hi = torch.ops.jax_raft_amd.op_arity("fb_check")
    assert sig == 1 and (lo, hi) == (7, 9)
    for key in ((B, 128, 256, 3, True, "bidir"), (B, 128, 256, 3, False, "bidir")):
        (t, i), = [args for *_, op, args in eng._build_key(key).plan.ops if op == "fb_check"]
        assert lo <= len(i) <= hi


@pytest.mark.parametrize("shape,dtype", [((1, 100, 150, 3), torch.uint8), ((1, 64, 64, 3), torch.float32),
                                         ((2, 32, 32, 3), torch.float32)])
def test_small_frames_are_refused_like_the_cold_plan(fake, shape, dtype):
    """Frames below the correlation pyramid's minimum map: the bidirectional key raises the cold
    key's AssertionError, and nothing is recorded or kept."""
    eng = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False)
    a = torch.zeros(shape, dtype=dtype)
    key = eng._key(a, a, 3, True)
    with pytest.raises(AssertionError, match="too small") as cold:
        eng._build_key(key)
    with pytest.raises(AssertionError, match="too small") as bidir:
        eng._build_key(key + ("bidir",))
    assert str(bidir.value) == str(cold.value)
    with pytest.raises(AssertionError, match="too small"):
        eng.forward(a, a, 3, bidirectional=True)
    assert eng.num_plans() == 0


def test_uint8_window_reaches_the_check(fake):
    eng = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False)
    key = eng._key(torch.zeros(1, 122, 150, 3, dtype=torch.uint8), torch.zeros(1, 122, 150, 3, dtype=torch.uint8),
                   3, True) + ("bidir",)
    st = eng._build_key(key)
    (t, i), = [args for *_, op, args in st.plan.ops if op == "fb_check"]
    assert list(i[:7]) == [1, 128, 152, 122, 150, 3, 1] and st.src == (122, 150, 3, 1)


# ----------------------------------------------------------------- rejections
def _pair(B=1, Hh=128, Ww=128):
    g = torch.Generator().manual_seed(3)
    return torch.rand(B, Hh, Ww, 3, generator=g) * 2 - 1, torch.rand(B, Hh, Ww, 3, generator=g) * 2 - 1


def test_engine_rejections(fake):
    i1, i2 = _pair()
    eng = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False)
    with pytest.raises(NotImplementedError, match="flow_init"):
        eng.forward(i1, i2, 3, bidirectional=True, flow_init=torch.zeros(1, 16, 16, 2))
    with pytest.raises(NotImplementedError, match="flow_init"):
        eng.forward(i1, i2, 3, bidirectional=True, flow_init="previous")
    with pytest.raises(NotImplementedError, match="return_flow_low"):
        eng.forward(i1, i2, 3, bidirectional=True, return_flow_low=True)
    with pytest.raises(NotImplementedError, match="pipelined"):
        eng.pipelined(i1, i2, 3, bidirectional=True)
    assert eng.num_plans() == 0
    cp = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False, cp_group=True)
    with pytest.raises(NotImplementedError, match="context parallelism"):
        cp.forward(i1, i2, 3, bidirectional=True)
    for precision in ("fp32", "mixed"):
        e = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False, precision=precision)
        assert e.precision == precision
        with pytest.raises(NotImplementedError, match=precision):
            e.forward(i1, i2, 3, bidirectional=True)


def test_model_rejections():
    model = raft_small()[0]
    i1, i2 = _pair()
    with pytest.raises(NotImplementedError, match="inference only"):
        model(i1, i2, train=True, bidirectional=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        model(i1, i2, autograd=True, bidirectional=True)
    with pytest.raises(NotImplementedError, match="flow_init"):
        model(i1, i2, bidirectional=True, flow_init=torch.zeros(1, 16, 16, 2))
    with pytest.raises(NotImplementedError, match="return_flow_low"):
        model(i1, i2, bidirectional=True, return_flow_low=True)


# ------------------------------------------------------------ golden-path API
def test_cpu_model_returns_the_named_tuple():
    model, variables = raft_small()
    i1, i2 = _pair()
    res = model(i1, i2, num_flow_updates=2, bidirectional=True)
    assert isinstance(res, BidirectionalFlow)
    fw, bw = model(i1, i2, num_flow_updates=2), model(i2, i1, num_flow_updates=2)
    assert torch.equal(res.flows_fw, fw) and torch.equal(res.flows_bw, bw)
    want = fb_consistency(fw[-1], bw[-1])
    assert torch.equal(res.occ_fw, want[0]) and torch.equal(res.occ_bw, want[1])
    assert res.occ_fw.shape == (1, 128, 128) and res.occ_fw.dtype == torch.bool
    # through apply, the final flow only, other thresholds
    res1 = model.apply(variables, i1, i2, num_flow_updates=2, return_all_iters=False, bidirectional=True,
                       fb_alpha=0.0, fb_beta=1e-6)
    assert torch.equal(res1.flows_fw, fw[-1:]) and torch.equal(res1.flows_bw, bw[-1:])
    want1 = fb_consistency(fw[-1], bw[-1], 0.0, 1e-6)
    assert torch.equal(res1.occ_fw, want1[0]) and torch.equal(res1.occ_bw, want1[1])


def test_cpu_uint8_frames_are_cropped():
    model = raft_small()[0]
    g = torch.Generator().manual_seed(5)
    f1 = torch.randint(0, 256, (1, 122, 150, 3), dtype=torch.uint8, generator=g)   # padded to 128 x 152
    f2 = torch.randint(0, 256, (1, 122, 150, 3), dtype=torch.uint8, generator=g)   # padded to 128 x 152
    res = model(f1, f2, num_flow_updates=1, bidirectional=True)
    assert res.flows_fw.shape == (1, 1, 122, 150, 2) and res.flows_bw.shape == (1, 1, 122, 150, 2)
    assert res.occ_fw.shape == (1, 122, 150) and res.occ_bw.shape == (1, 122, 150)
