"""On-demand correlation on the MI355X: the ``feat_pool`` and ``lookup_od`` kernels
(csrc/kernels/corr_od.hip) against fp64 references under derived per-element tolerances
(tests/_ondemand_refs.py), the fused flow update against the ``lookup`` op, repeatability, the
``corr="on_demand"`` engine against the fp32 golden model, and the host-side argument checks."""
import functools
import math

import pytest
import torch

import _ondemand_refs as O
from jax_raft_amd import raft_large, raft_small
from jax_raft_amd.models import reference as R
from jax_raft_amd.runtime.engine import RaftEngine

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(16, 20), (17, 33), (16, 32)]


def _nat():
    from jax_raft_amd.ops import native

    native.require()
    return native


def _dev_bf16(x):
    return x.to(DEV, torch.bfloat16).contiguous()


def _pooled_bufs(B, h, w, C, L, fill=float("nan")):
    return [torch.full((B, h >> l, w >> l, C), fill, device=DEV) for l in range(1, L)]


def _run_lookup_od(nat, f1, f2, coords, r, L, upd=(), extra=(), out=None):
    """feat_pool + lookup_od on device copies of the case; returns (out rows, pooled levels)."""
    B, h, w, C = f1.shape
    M = B * h * w
    S = 2 * r + 1
    ocs = nat.round_up(L * S * S, 8)
    g1, g2 = _dev_bf16(f1), _dev_bf16(f2)
    pooled = _pooled_bufs(B, h, w, C, L)
    nat.ops().feat_pool([g2] + pooled, [B, h, w, C, L])
    if out is None:
        out = torch.full((M, ocs), 5.0, dtype=torch.bfloat16, device=DEV)
    c = coords if coords.is_cuda else coords.reshape(M, 2).to(DEV).contiguous()
    nat.ops().lookup_od([c, out, g1, g2] + pooled + [None] * (4 - L) + list(upd), [L, B, h, w, r, C] + list(extra))
    torch.cuda.synchronize()
    return out, pooled


# ------------------------------------------------------------------------------- feat_pool
@pytest.mark.parametrize("C", [128, 256])
@pytest.mark.parametrize("h,w", SHAPES)
def test_feat_pool(h, w, C):
    """Pooled target features against fp64 pooling of the bf16-rounded features: every cell of
    every level written (NaN pre-fill), the error within the fp32 pooling's rounding (fp32
    storage adds none).  17 x 33: a row and a column dropped at every level."""
    nat = _nat()
    B, L = 2, 4
    _, f2 = O.features(B, h, w, C, h * w + C)
    pooled = _pooled_bufs(B, h, w, C, L)
    nat.ops().feat_pool([_dev_bf16(f2)] + pooled, [B, h, w, C, L])
    torch.cuda.synchronize()
    for l, ((ref, tol), got) in enumerate(zip(O.feat_pool_ref(f2, L), pooled), start=1):
        got = got.cpu()
        assert tuple(got.shape) == tuple(ref.shape) == (B, h >> l, w >> l, C)
        assert not torch.isnan(got).any(), f"level {l} has unwritten cells"
        ratio = O.ratio(got, ref, tol)
        print(f"[on-demand] feat_pool {h}x{w} C={C} level {l}: max err/tol = {ratio:.3f}")
        assert ratio <= 1.0, l
    # fewer levels: only those levels are written
    pooled = _pooled_bufs(B, h, w, C, L)
    nat.ops().feat_pool([_dev_bf16(f2)] + pooled[:1], [B, h, w, C, 2])
    torch.cuda.synchronize()
    assert not torch.isnan(pooled[0]).any() and torch.isnan(pooled[1]).all() and torch.isnan(pooled[2]).all()


# ------------------------------------------------------------------------------- lookup_od
@pytest.mark.parametrize("kind", ["smooth", "scattered", "special"])
@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("C,r", [(128, 3), (256, 4)])
@pytest.mark.parametrize("h,w", SHAPES)
def test_lookup_od(h, w, C, r, L, kind):
    """``lookup_od`` against the fp64 ``index_on_demand`` of the bf16-rounded feature maps.  Output
    pre-filled with 5.0: the padding channels up to the stride come back 0, the real channels are
    within the per-element tolerance (bf16 output rounding on |ref| + the fp32 accumulation and
    pooling terms on A; tests/_ondemand_refs.py).  Fields: smooth (overlapping windows), scattered
    (+-h jumps: disjoint windows, many partly or wholly off the map), special (integer-exact,
    +-1000 outside, each border)."""
    nat = _nat()
    f1, f2, coords, ref, tol = O.lookup_case(h, w, C, r, L, kind)
    out, _ = _run_lookup_od(nat, f1, f2, coords, r, L)
    got = out.float().cpu()
    n = L * (2 * r + 1) ** 2
    assert got.shape[1] % 8 == 0 and (got[:, n:] == 0).all()
    ratio = O.ratio(got[:, :n], ref, tol)
    print(f"[on-demand] lookup_od {h}x{w} C={C} r={r} L={L} {kind}: max err/tol = {ratio:.3f}")
    assert ratio <= 1.0
    assert float(ref.abs().max()) > 0.1
    if kind == "special":
        far = (coords.reshape(-1, 2).abs() >= 1000).any(-1)
        assert int(far.sum()) >= 3 and (got[far][:, : (2 * r + 1) ** 2] == 0).all()


@pytest.mark.parametrize("C,r", [(64, 1), (192, 2), (512, 4)])
def test_lookup_od_other_channel_counts(C, r):
    """C = 64 (half of each 16-lane group idle), 192 (a partial second chunk round) and 512 (four
    chunks per lane), radius 1 and 2."""
    nat = _nat()
    h, w, L = 17, 33, 3
    f1, f2, coords, ref, tol = O.lookup_case(h, w, C, r, L, "special")
    out, _ = _run_lookup_od(nat, f1, f2, coords, r, L)
    got = out.float().cpu()
    n = L * (2 * r + 1) ** 2
    assert (got[:, n:] == 0).all() and O.ratio(got[:, :n], ref, tol) <= 1.0


def test_lookup_od_is_repeatable():
    nat = _nat()
    f1, f2, coords, _, _ = O.lookup_case(17, 33, 256, 4, 4, "scattered")
    a, pa = _run_lookup_od(nat, f1, f2, coords, 4, 4)
    b, pb = _run_lookup_od(nat, f1, f2, coords, 4, 4)
    assert _bits_equal(a, b) and all(_bits_equal(x, y) for x, y in zip(pa, pb))


def _bits_equal(a, b):
    it = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ---------------------------------------------------------------------------- fused update
@pytest.mark.parametrize("w,C,parity", [(20, 128, False), (33, 256, True)])
def test_lookup_od_fused_update_matches_lookup(w, C, parity):
    """``lookup_od`` with the fused flow update (TapsUpd) against the ``lookup`` op with the same
    operands on a pyramid built by the ``corr`` op: coords, flow32 (and the odd-iteration buffer)
    and the hx / qx / flow8 flow channels bitwise (shared code, csrc/kernels/lookup_coords.h); the
    correlation rows within ``lookup_od``'s tolerance plus the volume path's (its bf16 level
    rounding), both against the fp64 reference at the updated coordinates."""
    nat = _nat()
    torch.manual_seed(19)
    B, h, L, r = 2, 16 + int(parity), 4, 4
    M = B * h * w
    f1, f2 = O.features(B, h, w, C, 31 * w + C)
    g1, g2 = _dev_bf16(f1), _dev_bf16(f2)
    lv, hl, wl = [], h, w
    for l in range(L):
        lv.append(torch.zeros((M, hl, wl), device=DEV, dtype=torch.bfloat16))
        hl //= 2
        wl //= 2
    nat.ops().corr([g1, g2] + lv, [B, h, w, C, L, h * w, 0], 1.0 / math.sqrt(C))
    taps = (torch.randn(M, 24) * 2).to(DEV)
    bias = torch.randn(2).to(DEV)
    coords0 = (R.make_coords_grid(B, h, w).reshape(M, 2) + torch.randn(M, 2) * 3).to(DEV)
    S = 2 * r + 1
    ocs = nat.round_up(L * S * S, 8)
    res = []
    for od in (False, True):
        coords = coords0.clone()
        f32 = torch.zeros(M, 2, device=DEV)
        f32b = torch.zeros(M, 2, device=DEV)
        hx = torch.zeros(M, 24, device=DEV, dtype=torch.bfloat16)
        qx = torch.zeros(M, 24, device=DEV, dtype=torch.bfloat16)
        f8 = torch.zeros(M, 2, device=DEV, dtype=torch.bfloat16)
        out = torch.full((M, ocs), 5.0, device=DEV, dtype=torch.bfloat16)
        upd = [taps, bias, f32, hx, qx, f8] + ([f32b] if parity else [])
        if od:
            _run_lookup_od(nat, f1, f2, coords, r, L, upd=upd, extra=[16, 8], out=out)
        else:
            nat.ops().lookup([coords, out] + lv + upd, [L, B, h, w, r, h * w, 0, 16, 8])
        torch.cuda.synchronize()
        res.append((coords, f32, f32b, hx, qx, f8, out))
    vol, new = res
    for a, b in zip(vol[:-1], new[:-1]):
        assert torch.equal(a, b)
    assert not torch.equal(new[0], coords0)                      # the update ran
    # eager ops run as iteration 1: with the parity buffer the odd-iteration flow32 is written
    assert (new[2].abs().sum() > 0) == parity and (new[1].abs().sum() > 0) == (not parity)
    ref, A, Vabs, level = O.lookup_ref(f1, f2, new[0].cpu().reshape(B, h, w, 2), r, L)
    n = L * S * S
    a, b = vol[-1].float().cpu(), new[-1].float().cpu()
    assert (a[:, n:] == 0).all() and (b[:, n:] == 0).all()
    r_od = O.ratio(b[:, :n], ref, O.lookup_tol(ref, A, level, C))
    r_vol = O.ratio(a[:, :n], ref, O.volume_tol(ref, A, Vabs, level, C))
    r_both = O.ratio(b[:, :n], a[:, :n], O.lookup_tol(ref, A, level, C) + O.volume_tol(ref, A, Vabs, level, C))
    print(f"[on-demand] fused update w={w} C={C}: err/tol on-demand {r_od:.3f}, volume {r_vol:.3f}, both {r_both:.3f}")
    assert r_od <= 1.0 and r_both <= 1.0


# ---------------------------------------------------------------------------------- engine
def _epe(a, b):
    return (a - b).norm(dim=-1).mean().item()


def _inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, H + 8, W + 8, 3, generator=g) * 2 - 1
    return base[:, 4:4 + H, 4:4 + W].contiguous(), base[:, 2:2 + H, 6:6 + W].contiguous()


# the volume engine's bounds (tests/test_engine_gpu.py): the on-demand path rounds no more than it
REL_EPE = {"raft_small": 0.065, "raft_large": 0.026}
ITERS = 4


@functools.lru_cache(maxsize=None)
def _golden(name, B, W):
    """(state dict, inputs, fp32 golden flows) of one engine case, computed once on the CPU."""
    torch.manual_seed(0)
    model, variables = {"raft_small": raft_small, "raft_large": raft_large}[name]()
    i1, i2 = _inputs(B, 128, W)
    ref = model.apply(variables, i1, i2, train=False, num_flow_updates=ITERS)
    return model.state_dict(), i1, i2, ref


def _model(name, B, W):
    sd, i1, i2, ref = _golden(name, B, W)
    model, _ = {"raft_small": raft_small, "raft_large": raft_large}[name]()
    model.load_state_dict(sd)
    return model.cuda(), i1.cuda(), i2.cuda(), ref


@pytest.mark.parametrize("name", ["raft_small", "raft_large"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B,W", [(2, 160), (2, 256), (4, 160), (4, 256)])
def test_on_demand_engine_matches_golden(name, use_graph, B, W):
    """The ``corr="on_demand"`` engine against the fp32 golden forward, under the volume engine's
    assertion and bounds (tests/test_engine_gpu.py:25-52) at every iteration; B = 4 at raft_large:
    the lane schedule.  The graph replay equals the first graph run bitwise."""
    model, i1, i2, ref = _model(name, B, W)
    out = model(i1, i2, num_flow_updates=ITERS, use_graph=use_graph, corr="on_demand")
    torch.cuda.synchronize()
    assert model.execution_path == "engine"
    eng = model.engine(i1.device, use_graph=use_graph, corr="on_demand")
    assert eng.corr_mode == "on_demand" and eng.num_plans() == 1
    assert out.shape == ref.shape == (ITERS, B, 128, W, 2)
    assert torch.isfinite(out).all()
    mag = ref.norm(dim=-1).mean().item()
    for it in range(ITERS):
        e = _epe(out[it].cpu(), ref[it])
        print(f"[on-demand] engine {name} B={B} W={W} graph={use_graph} it {it}: EPE / |flow| = {e / mag:.4f}")
        assert e < REL_EPE[name] * mag, (it, e, mag)
    if use_graph:
        again = model(i1, i2, num_flow_updates=ITERS, use_graph=True, corr="on_demand")
        torch.cuda.synchronize()
        assert torch.equal(again, out)


def test_on_demand_final_only():
    """The final-only plan (serving mode) under the same bound at the last iteration."""
    model, i1, i2, ref = _model("raft_small", 2, 160)
    last = model(i1, i2, num_flow_updates=ITERS, return_all_iters=False, corr="on_demand")
    torch.cuda.synchronize()
    assert last.shape == (1, 2, 128, 160, 2)
    mag = ref.norm(dim=-1).mean().item()
    assert _epe(last[0].cpu(), ref[-1]) < REL_EPE["raft_small"] * mag


@pytest.mark.parametrize("H0,W0,levels", [(100, 150, 3), (122, 150, 4)])
def test_on_demand_uint8_frames(H0, W0, levels):
    """uint8 frames of any size: normalised and padded by the plan's prep kernel, the flows cropped
    back to the frame.  100 x 150 pads to 104 x 152, a 13 x 19 feature map: below the 16 cells a
    four-level pyramid needs (volume or on demand), so that frame runs a three-level model (odd
    level sizes 13 x 19, 6 x 9, 3 x 4); 122 x 150 (16 x 19) runs the stock four levels."""
    from jax_raft_amd.models.layers import CorrBlock

    torch.manual_seed(0)
    model, _ = raft_small() if levels == 4 else raft_small(corr_block=CorrBlock(num_levels=levels, radius=3))
    model = model.cuda()
    g = torch.Generator().manual_seed(5)
    u1 = torch.randint(0, 256, (1, H0, W0, 3), generator=g, dtype=torch.uint8)
    u2 = torch.roll(u1, shifts=(1, 2), dims=(1, 2))
    flows = model(u1, u2, num_flow_updates=2, corr="on_demand")
    torch.cuda.synchronize()
    assert model.execution_path == "engine"
    assert flows.shape == (2, 1, H0, W0, 2) and torch.isfinite(flows).all() and flows.abs().max().item() > 0
    names = model.engine(flows.device, corr="on_demand").op_names(1, 104 if H0 == 100 else 128, 152, 2)
    assert "feat_pool" in names[0] and "lookup_od" in names[1]


def test_on_demand_warm_start():
    """``flow_init=0`` is bitwise the cold on-demand result (the warm plan differs in its seed
    only), ``return_flow_low`` returns the low-resolution flow and ``flow_init="previous"`` runs."""
    model, i1, i2, _ = _model("raft_small", 2, 160)
    cold = model(i1, i2, num_flow_updates=3, corr="on_demand")
    zero = torch.zeros(2, 16, 20, 2, device=DEV)
    warm, low = model(i1, i2, num_flow_updates=3, corr="on_demand", flow_init=zero, return_flow_low=True)
    torch.cuda.synchronize()
    assert torch.equal(warm, cold) and low.shape == (2, 16, 20, 2)
    prev = model(i1, i2, num_flow_updates=3, corr="on_demand", flow_init="previous")
    torch.cuda.synchronize()
    assert prev.shape == cold.shape and torch.isfinite(prev).all()
    seeded = model(i1, i2, num_flow_updates=3, corr="on_demand", flow_init=low)
    torch.cuda.synchronize()
    assert torch.isfinite(seeded).all() and not torch.equal(seeded, cold)


def test_volume_engine_is_untouched_by_an_on_demand_engine():
    """A ``"volume"`` engine on the same model in the same process returns bitwise what it returns
    with no on-demand engine present, before and after one has been built and run."""
    model, i1, i2, _ = _model("raft_large", 2, 256)
    before = model(i1, i2, num_flow_updates=3)
    od = model(i1, i2, num_flow_updates=3, corr="on_demand")
    after = model(i1, i2, num_flow_updates=3)
    fresh = RaftEngine(model, torch.device(DEV)).forward(i1, i2, 3)
    torch.cuda.synchronize()
    assert torch.equal(before, after) and torch.equal(before, fresh)
    assert not torch.equal(od, before)
    assert model.engine(i1.device) is not model.engine(i1.device, corr="on_demand")
    names = model.engine(i1.device).op_names(2, 128, 256, 3)
    assert "corr" in names[0] and "lookup" in names[1] and "lookup_od" not in names[1]
    od_names = model.engine(i1.device, corr="on_demand").op_names(2, 128, 256, 3)
    assert "feat_pool" in od_names[0] and "corr" not in od_names[0] and "lookup_od" in od_names[1]


# ------------------------------------------------------------------------------ host checks
def test_host_checks_raise_before_any_launch():
    nat = _nat()
    B, h, w, C, L, r = 1, 16, 20, 128, 4, 3
    M = B * h * w
    f = torch.zeros(B, h, w, C, device=DEV, dtype=torch.bfloat16)
    pooled = _pooled_bufs(B, h, w, C, L, fill=0.0)
    coords = torch.zeros(M, 2, device=DEV)
    out = torch.full((M, 200), 5.0, device=DEV, dtype=torch.bfloat16)
    good_t, good_i = [coords, out, f, f] + pooled, [L, B, h, w, r, C]
    nat.ops().lookup_od(good_t, good_i)                                   # the good call runs
    torch.cuda.synchronize()
    assert (out[:, :196] == 0).all()
    out.fill_(5.0)

    def bad(t, i, match, op="lookup_od"):
        with pytest.raises(RuntimeError, match=match):
            getattr(nat.ops(), op)(t, i)

    bad([coords, out, f.float(), f] + pooled, good_i, "bfloat16")                          # wrong dtype
    bad([coords.double(), out, f, f] + pooled, good_i, "float32")
    bad([coords, out, f, f] + [p.to(torch.bfloat16) for p in pooled], good_i, "float32")
    bad([coords, out.float(), f, f] + pooled, good_i, "bfloat16")
    bad([coords, out[:, :196].contiguous(), f, f] + pooled, good_i, "channel stride")     # 196 % 8 != 0
    bad([coords, out[:, :192].contiguous(), f, f] + pooled, good_i, "channel stride")     # < L * S * S
    small = torch.zeros(B, 8, 12, C, device=DEV, dtype=torch.bfloat16)
    bad([coords, out, small, small] + pooled, [L, B, 8, 12, r, C], "level too small")      # 8 >> 3 = 1
    bad([coords, out, f, f] + pooled[:2], good_i, "must be defined")                       # a level missing
    bad([coords, out, f, f] + pooled[:2] + [pooled[2][:, :1]], good_i, "contiguous|too small")
    bad(good_t, [L, B, h, w, 5, C], "radius")
    bad(good_t, [5, B, h, w, r, C], "levels")
    bad([coords, out, f[..., :96].contiguous(), f[..., :96].contiguous()] + pooled, [L, B, h, w, r, 96], "multiple of 64")
    bad(good_t + [torch.zeros(M, 24, device=DEV)], good_i, "fused")                        # taps without offsets
    bad([f] + pooled, [B, h, w, 96, L], "multiple of 64", op="feat_pool")
    bad([f.float()] + pooled, [B, h, w, C, L], "bfloat16", op="feat_pool")
    bad([small] + pooled, [B, 8, 12, C, L], "level too small", op="feat_pool")
    bad([f] + pooled[:1], [B, h, w, C, L], "must be defined", op="feat_pool")
    torch.cuda.synchronize()
    assert (out == 5.0).all()                                             # nothing was launched
