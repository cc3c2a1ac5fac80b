"""On-demand correlation on the CPU: the golden op against the volume path, the model path, the
engine's lowering (recording stand-in for the native plan), the binding's op rows, and the
fp32 emulation of the kernels against the tolerance the GPU tests use
(tests/test_ondemand_gpu.py; derivations in tests/_ondemand_refs.py)."""
import pytest
import torch

import _ondemand_refs as O
from jax_raft_amd import raft_large, raft_small
from jax_raft_amd.models import reference as R
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import tunedb
from test_engine_lowering import FakePlan


# ------------------------------------------------------------------------------ golden op
def _golden_coords(B, h, w, seed):
    """The grid plus noise in multiples of 1/64 (|noise| < 4), with the special queries.  Every
    coordinate is a multiple of 1/64 below 2^11, so ``c / 2^l + d`` (integer d) is exact in fp32
    for l <= 3: both paths sample at identical positions with identical, exact weights."""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randint(-255, 256, (B, h, w, 2), generator=g).float() / 64.0
    return O.special_queries(O.grid(B, h, w) + noise)


@pytest.mark.parametrize("B,h,w,C,L,r", [(2, 16, 20, 128, 4, 3), (1, 17, 33, 256, 4, 4)])
def test_index_on_demand_matches_volume_path(B, h, w, C, L, r):
    """``index_on_demand`` against ``index_pyramid(build_pyramid(...))``, both fp32, per element
    within ``gamma * A`` (A: the fp64 sum of absolute products behind the element,
    tests/_ondemand_refs.py).  17 x 33: the pooling drops a row and a column at every level.

    gamma counts the fp32 roundings a term can pass through in each path (u = 2^-24):

    * volume path: the matmul's product and C - 1 additions in any order (C), the division by a
      rounded sqrt(C) (2), l 2x2 means of 3 additions each (3 l), ``1 - w`` and ``wx * wy`` (2),
      weight times value (1), 4 accumulated taps (4): C + 3 l + 9;
    * on-demand path: l feature means (3 l), product and C - 1 additions (C), the scale (2),
      ``1 - wy``, two products, a sum (vertical), the same horizontally (3 + 3): C + 3 l + 8.

    The coordinates and weights are exact in both (:func:`_golden_coords`).  The two results
    differ by at most the sum: gamma(2 C + 6 l + 17) * A."""
    g = torch.Generator().manual_seed(7 * h + w)
    f1 = torch.randn(B, h, w, C, generator=g)
    f2 = torch.randn(B, h, w, C, generator=g)
    coords = _golden_coords(B, h, w, h + w)
    got = R.index_on_demand(f1, f2, coords, r, L).reshape(B * h * w, -1)
    vol = R.index_pyramid(R.build_pyramid(f1, f2, L), coords, r).reshape(B * h * w, -1)
    _, A, _, level = O.lookup_ref(f1, f2, coords, r, L)
    n = (2 * C + 17 + 6 * level).double()
    tol = n * O.U32 / (1.0 - n * O.U32) * A
    ratio = O.ratio(got, vol, tol)
    print(f"[on-demand] golden vs volume {h}x{w} C={C}: max err/tol = {ratio:.3f}")
    assert got.shape == (B * h * w, L * (2 * r + 1) ** 2)
    assert ratio <= 1.0
    assert (tol > 0).any() and float(vol.abs().max()) > 0.1      # the comparison is not empty
    # far outside: every sample is exactly 0
    S2 = (2 * r + 1) ** 2
    far = (coords.reshape(-1, 2).abs() >= 1000).any(-1)
    assert int(far.sum()) >= 3 and (got[far][:, :S2] == 0).all()


def test_index_on_demand_rejects_small_maps():
    f = torch.zeros(1, 8, 16, 64)
    with pytest.raises(AssertionError):
        R.index_on_demand(f, f, O.grid(1, 8, 16), 4, 4)


def test_model_path_on_demand():
    """``forward_reference(corr="on_demand")`` against the default over 3 iterations at 128 x 160.

    The first lookup (coordinates = the integer grid, exact) is checked per element under the
    golden test's bound.  The flows then pass through three update blocks; their difference is
    bounded by 2^-10 of the mean flow magnitude: a budget of 2^14 unit roundoffs, 25 times the
    per-lookup gamma (2 C + 35 = 547 for raft_large's C = 256) for the amplification of three
    iterations of convolutions, whose own evaluation-order noise is of that size."""
    torch.manual_seed(0)
    model, _ = raft_large()
    g = torch.Generator().manual_seed(3)
    base = torch.rand(1, 136, 168, 3, generator=g) * 2 - 1
    i1, i2 = base[:, 4:132, 4:164].contiguous(), base[:, 2:130, 6:166].contiguous()
    with torch.no_grad():
        ref = model.forward_reference(i1, i2, False, 3)
        got = model.forward_reference(i1, i2, False, 3, corr="on_demand")
        via_call = model(i1, i2, num_flow_updates=3, corr="on_demand")
        fmap1, fmap2 = torch.chunk(model.feature_encoder(torch.cat([i1, i2], dim=0), False), 2, dim=0)
    assert got.shape == ref.shape == (3, 1, 128, 160, 2)
    assert torch.equal(via_call, got)
    mag = ref.norm(dim=-1).mean().item()
    err = (got - ref).abs().max().item()
    print(f"[on-demand] model path: max |diff| = {err:.3e}, mean |flow| = {mag:.3e}")
    assert err <= 2.0 ** -10 * mag
    L, r = model.corr_block.num_levels, model.corr_block.radius
    coords = O.grid(1, 16, 20)
    a = R.index_on_demand(fmap1, fmap2, coords, r, L).reshape(320, -1)
    b = R.index_pyramid(R.build_pyramid(fmap1, fmap2, L), coords, r).reshape(320, -1)
    _, A, _, level = O.lookup_ref(fmap1, fmap2, coords, r, L)
    n = (2 * fmap1.shape[-1] + 17 + 6 * level).double()
    assert O.ratio(a, b, n * O.U32 / (1.0 - n * O.U32) * A) <= 1.0


def test_unknown_corr_is_a_value_error():
    model, _ = raft_small()
    x = torch.zeros(1, 128, 128, 3)
    with pytest.raises(ValueError, match="corr"):
        model(x, x, num_flow_updates=1, corr="sparse")
    with pytest.raises(ValueError, match="corr"):
        model.forward_reference(x, x, False, 1, corr="sparse")
    with pytest.raises(NotImplementedError, match="on_demand"):
        model(x, x, train=True, num_flow_updates=1, corr="on_demand")
    with pytest.raises(NotImplementedError, match="on_demand"):
        model(x, x, num_flow_updates=1, corr="on_demand", autograd=True)
    with pytest.raises(NotImplementedError, match="on_demand"):
        model(x, x, num_flow_updates=1, corr="on_demand", bidirectional=True)
    with pytest.raises(NotImplementedError, match="on_demand"):
        model(x, x, num_flow_updates=1, corr="on_demand", precision="fp32")
    with pytest.raises(NotImplementedError, match="on_demand"):
        model(x, x, num_flow_updates=1, corr="on_demand", cp_group=True)


# -------------------------------------------------------------------------------- lowering
@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(nat, "require", lambda: None)
    monkeypatch.setattr(nat, "new_plan", FakePlan)
    monkeypatch.setattr(tunedb, "gpu_arch", lambda device=None: "cpu")


def _sig(plan):
    return [(s, ln, d, op) for s, ln, d, op, _ in plan.ops]


RENAME = {"corr": "feat_pool", "lookup": "lookup_od"}


@pytest.mark.parametrize("all_iters", [True, False])
@pytest.mark.parametrize("factory,B", [(raft_large, 1), (raft_large, 4), (raft_small, 1)])
@pytest.mark.parametrize("warm", [False, True])
def test_on_demand_plan_is_the_volume_plan_renamed(fake, factory, B, all_iters, warm):
    """The on-demand plan = the volume plan with ``corr`` -> ``feat_pool`` and every ``lookup`` ->
    ``lookup_od``: same segments, lanes, deferral and order (lane schedule at raft_large batch 4,
    one lane, final-only; cold and warm), no ``corr.l*`` buffer, the pooled feature levels instead,
    and the fused-update operands of every lookup unchanged."""
    model = factory()[0].eval()
    H, W = 128, 256
    vol = E.RaftEngine(model, "cpu", autotune=False)
    before = _sig(vol._build(B, H, W, 3, all_iters, warm=warm).plan)
    od = E.RaftEngine(model, "cpu", autotune=False, corr="on_demand")
    st = od._build(B, H, W, 3, all_iters, warm=warm)
    got = _sig(st.plan)
    assert [op for *_, op in before].count("lookup") >= 1 and [op for *_, op in before].count("corr") == 1
    assert got == [(s, ln, d, RENAME.get(op, op)) for s, ln, d, op in before]
    assert od.uses_lanes(B, all_iters) == vol.uses_lanes(B, all_iters)
    # the volume engine records what it recorded before the on-demand engine existed
    assert _sig(vol._build(B, H, W, 3, all_iters, warm=warm).plan) == before
    assert not any(".corr.l" in k or k.startswith("corr.l") for k in st.bufs)
    h, w, L, C = H // 8, W // 8, od.num_levels, od.fmap_ch
    for l in range(1, L):
        t = st.bufs[f"p0.fpool.l{l}"]
        assert tuple(t.shape) == (B, h >> l, w >> l, C) and t.dtype == torch.float32
    assert f"p0.fpool.l{L}" not in st.bufs and "p0.fpool.l0" not in st.bufs
    ops_v = {op: a for *_, op, a in vol._build(B, H, W, 3, all_iters, warm=warm).plan.ops if op == "lookup"}
    ops_o = {op: a for *_, op, a in st.plan.ops if op in ("lookup_od", "feat_pool")}
    tv, iv = ops_v["lookup"]
    to, io = ops_o["lookup_od"]
    assert len(to) == len(tv) + 1 and io[:5] == iv[:5] and io[5] == C and io[6:] == iv[7:]
    assert [None if t is None else tuple(t.shape) for t in to[7:]] == [None if t is None else tuple(t.shape) for t in tv[6:]]
    tp, ip = ops_o["feat_pool"]
    assert ip == [B, h, w, C, L] and len(tp) == L and tuple(tp[0].shape) == (B, h, w, C)


def test_on_demand_out_of_scope(fake):
    model = raft_small()[0].eval()
    with pytest.raises(ValueError, match="corr"):
        E.RaftEngine(model, "cpu", autotune=False, corr="sparse")
    with pytest.raises(TypeError):
        E.RaftEngine(model, "cpu", autotune=False, corr_mode="on_demand")
    for kw in (dict(precision="fp32"), dict(precision="mixed"), dict(cp_group=True)):
        with pytest.raises(NotImplementedError, match="on_demand"):
            E.RaftEngine(model, "cpu", autotune=False, corr="on_demand", **kw)
    eng = E.RaftEngine(model, "cpu", autotune=False, corr="on_demand")
    x = torch.zeros(1, 128, 128, 3)
    with pytest.raises(NotImplementedError, match="on_demand"):
        eng.forward(x, x, 2, bidirectional=True)
    with pytest.raises(NotImplementedError, match="on_demand"):
        eng.pipelined(x, x, 2)
    # a volume engine's plan keys are what they were
    vol = E.RaftEngine(model, "cpu", autotune=False)
    assert vol._key(x, x, 2, True) == eng._key(x, x, 2, True) == (1, 128, 128, 2, True)
    assert model.engine("cpu", autotune=False, corr="on_demand") is not model.engine("cpu", autotune=False)
    assert model.engine("cpu", autotune=False, corr="on_demand").corr_mode == "on_demand"
    assert model.engine("cpu", autotune=False).corr_mode == "volume"


# ----------------------------------------------------------------------------- binding rows
def _lib():
    try:
        nat.load(build_if_missing=False)
    except Exception as e:   # not built here
        pytest.skip(f"native library not built: {e}")
    return torch.ops.jax_raft_amd


def test_binding_rows_and_generated_arity_check():
    ops = _lib()
    assert list(ops.op_arity("feat_pool")) == [1, 5, 5]
    assert list(ops.op_arity("lookup_od")) == [1, 6, 8]
    for name, bad in (("feat_pool", [4, 6]), ("lookup_od", [5, 9])):
        for n in bad:
            with pytest.raises(RuntimeError, match=f"{name}: expected"):
                getattr(ops, name)([None], [2] * n)


# --------------------------------------------------------------- the tolerance is attainable
@pytest.mark.parametrize("h,w,C,r,L,kind", [(16, 20, 128, 3, 4, "special"), (17, 33, 256, 4, 4, "scattered"),
                                            (16, 32, 128, 3, 1, "smooth")])
def test_lookup_emulation_meets_the_gpu_tolerance(h, w, C, r, L, kind):
    """The fp32 torch emulation of ``lookup_od_kernel``'s operation order, on the GPU test's own
    cases, is within the GPU test's per-element tolerance."""
    f1, f2, coords, ref, tol = O.lookup_case(h, w, C, r, L, kind)
    got = O.lookup_emul(f1, f2, coords, r, L)
    ratio = O.ratio(got, ref, tol)
    print(f"[on-demand] emulation {h}x{w} C={C} r={r} L={L} {kind}: max err/tol = {ratio:.3f}")
    assert ratio <= 1.0
    assert float(ref.abs().max()) > 0.1


@pytest.mark.parametrize("h,w,C", [(16, 20, 128), (17, 33, 256), (16, 32, 128)])
def test_feat_pool_emulation_meets_the_gpu_tolerance(h, w, C):
    _, f2 = O.features(2, h, w, C, h * w + C)
    for (ref, tol), got in zip(O.feat_pool_ref(f2, 4), O.feat_pool_emul(f2, 4)):
        assert got.shape == ref.shape and O.ratio(got, ref, tol) <= 1.0
