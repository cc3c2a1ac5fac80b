"""Warm start on the MI355X: the forward-projection and seed kernels (warm.hip)
against their golden definitions, bit for bit, and the engines' ``flow_init`` /
``return_flow_low`` / ``flow_init="previous"`` against the cold path and the fp32
golden forward (CPU semantics: tests/test_warm_start.py)."""
import functools

import pytest
import torch

from jax_raft_amd import raft_large, raft_small
from jax_raft_amd.models import reference as R
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime.engine import RaftEngine

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _epe(a, b):
    return (a - b).norm(dim=-1).mean().item()


def _inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, H + 8, W + 8, 3, generator=g) * 2 - 1
    # a translated pair so the flow is non-trivial
    i1 = base[:, 4:4 + H, 4:4 + W]
    i2 = base[:, 2:2 + H, 6:6 + W]
    return i1.contiguous(), i2.contiguous()


# the project's cold-start bf16 bounds (tests/test_engine_gpu.py: max over the iterations of
# EPE / mean |golden flow|, measured 0.048 / 0.017, with 1.3x / 1.5x headroom)
REL_EPE = {"raft_small": 0.065, "raft_large": 0.026}

# (factory, B, H, W): the ping-pong GRU; one lane with the merged grid; the lane schedule
CONFIGS = [(raft_small, 1, 128, 128), (raft_large, 2, 128, 256), (raft_large, 4, 128, 256)]
IDS = ["small-b1", "large-b2", "large-b4-lanes"]


def _smooth_init(B, h, w):
    """A smooth field of 1-3 cells magnitude."""
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    fx = 2.0 + torch.sin(xs / w * 3.0 + ys / h)            # 1 .. 3
    fy = -1.5 + 0.5 * torch.cos(ys / h * 2.0 - xs / w)     # -2 .. -1
    f = torch.stack([fx, fy], dim=-1).unsqueeze(0).repeat(B, 1, 1, 1)
    return f * (1.0 - 0.1 * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1))


# ------------------------------------------------------------------ the kernels
def _flow_field(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    f = torch.stack([1.5 * torch.sin(ys / 5.0) + 0.1 * xs / w, 1.2 * torch.cos(xs / 7.0)], dim=-1)
    f = f.unsqueeze(0).repeat(B, 1, 1, 1) + 0.3 * torch.randn(B, h, w, 2, generator=g)
    f[:, h // 4:h // 2, w // 4:w // 2] = torch.tensor([3.25, 2.0])     # an occluding patch
    f[:, :3, :4] = torch.tensor([-6.5, -5.0])                          # a patch leaving the frame
    f[-1, h - 3:, w - 3:] = torch.tensor([2.5, 3.5])                   # ... at the far corner too
    f[0, h // 2, w // 2, 0] = float("nan")
    f[0, 1, w - 2] = float("nan")
    f[-1, h - 1, 0, 1] = float("inf")
    f[:, 5, 5] = torch.tensor([0.5, -0.5])                             # landing exactly between cells
    return f


@pytest.mark.parametrize("radius", [0, 4, 7])
@pytest.mark.parametrize("B,h,w", [(1, 16, 20), (2, 17, 33), (1, 55, 128)])
def test_forward_project_kernel_is_bitwise_golden(B, h, w, radius):
    """Exact: every comparison the definition makes is on integers.  Three calls on ONE key
    buffer with alternating inputs: a key that a call leaves behind would win a later splat."""
    fa, fb = _flow_field(B, h, w, 1), _flow_field(B, h, w, 2).flip(2).contiguous()
    ga, gb = R.forward_project(fa, radius), R.forward_project(fb, radius)
    assert 0.5 < (ga != 0).any(-1).float().mean().item()   # (the case is not degenerate)
    keys = nat.project_keys(B, h, w, DEV)
    da, db = fa.to(DEV), fb.to(DEV)
    outs = [nat.forward_project(x, radius, keys=keys) for x in (da, db, da, da)]
    torch.cuda.synchronize()
    for o, gold in zip(outs, (ga, gb, ga, ga)):
        o = o.cpu()
        assert torch.equal(torch.isnan(o), torch.isnan(gold))
        assert torch.equal(torch.nan_to_num(o, nan=7.0), torch.nan_to_num(gold, nan=7.0))
    # a fresh buffer per call (keys=None) gives the same
    assert torch.equal(torch.nan_to_num(nat.forward_project(da, radius).cpu()), torch.nan_to_num(ga))


def test_forward_project_rejects_bad_arguments():
    f = torch.zeros(1, 16, 20, 2, device=DEV)
    with pytest.raises(RuntimeError, match="fill_radius"):
        nat.forward_project(f, 9)
    with pytest.raises(RuntimeError, match="keys"):
        nat.forward_project(f, 4, keys=nat.project_keys(1, 16, 21, DEV))
    with pytest.raises(ValueError):
        nat.forward_project(f[..., :1], 4)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_init_flow_kernel_is_bitwise(f32):
    """The seed vs a torch composition: coords = grid + flow_init, flow32 = flow_init, the flow
    channels of hx / qx / flow8 (flow4) in the buffers' dtype, every other channel untouched."""
    B, h, w, cs_, off = 2, 16, 20, 24, 14
    M = B * h * w
    g = torch.Generator().manual_seed(3)
    fi = ((torch.rand(B, h, w, 2, generator=g) - 0.5) * 7).to(DEV)
    dt = torch.float32 if f32 else torch.bfloat16
    hx = torch.randn(M, cs_, generator=g).to(DEV, dt)
    qx = torch.randn(M, cs_, generator=g).to(DEV, dt)
    fz = torch.randn(M, 4 if f32 else 8, generator=g).to(DEV, dt)
    coords = torch.full((M, 2), -1.0, device=DEV)
    flow32 = torch.full((M, 2), -1.0, device=DEV)
    hx0, qx0, fz0 = hx.clone(), qx.clone(), fz.clone()
    op = nat.ops().init_flow_f32 if f32 else nat.ops().init_flow
    op([fi, coords, flow32, hx, qx, fz], [B, h, w, off, off - 2])
    torch.cuda.synchronize()
    flat = fi.view(M, 2)
    assert torch.equal(coords.view(B, h, w, 2), R.make_coords_grid(B, h, w, device=DEV) + fi)
    assert torch.equal(flow32, flat)
    hx0[:, off:off + 2] = flat.to(dt)
    qx0[:, off - 2:off] = flat.to(dt)
    fz0[:, :2] = flat.to(dt)
    if f32:
        fz0[:, 2:] = 0     # flow4 rows are (fx, fy, 0, 0), as the fp32 flow update writes them
    assert torch.equal(hx, hx0) and torch.equal(qx, qx0) and torch.equal(fz, fz0)
    # qx / flow8 are optional
    hx1 = hx.clone().zero_()
    op([fi, coords, flow32, hx1, None, None], [B, h, w, off, off])
    torch.cuda.synchronize()
    assert torch.equal(hx1[:, off:off + 2], flat.to(dt))
    hx1[:, off:off + 2] = 0
    assert not hx1.any()


# ------------------------------------------------------------------- the engines
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("factory,B,H,W", CONFIGS, ids=IDS)
def test_zero_init_equals_cold(factory, B, H, W, use_graph):
    model = factory()[0].eval().to(DEV)
    i1, i2 = [t.to(DEV) for t in _inputs(B, H, W)]
    eng = RaftEngine(model, DEV, use_graph=use_graph)
    zeros = torch.zeros(B, H // 8, W // 8, 2, device=DEV)
    cold = eng.forward(i1, i2, 3)
    warm, low = eng.forward(i1, i2, 3, flow_init=zeros, return_flow_low=True)
    cold_low = eng.forward(i1, i2, 3, return_flow_low=True)[1]
    torch.cuda.synchronize()
    assert eng.num_plans() == 2
    assert torch.isfinite(cold).all() and torch.equal(warm, cold) and torch.equal(low, cold_low)
    if use_graph and B == 2:   # the serving mode once
        c1 = eng.forward(i1, i2, 3, return_all_iters=False)
        w1 = eng.forward(i1, i2, 3, return_all_iters=False, flow_init=zeros)
        torch.cuda.synchronize()
        assert c1.shape == (1, B, H, W, 2) and torch.equal(w1, c1)


@functools.lru_cache(maxsize=None)
def _golden_warm(name, B, H, W):
    """(flows, flow_low) of the fp32 golden forward from the smooth initial flow, 4 iterations."""
    model = {"raft_small": raft_small, "raft_large": raft_large}[name]()[0].eval()
    i1, i2 = _inputs(B, H, W)
    with torch.no_grad():
        return model(i1, i2, num_flow_updates=4, flow_init=_smooth_init(B, H // 8, W // 8), return_flow_low=True)


@pytest.mark.parametrize("factory,B,H,W", CONFIGS, ids=IDS)
def test_fp32_engine_warm_matches_golden(factory, B, H, W):
    """The project's fp32 bound (tests/test_engine_gpu.py: EPE < 1e-3 * (1 + mean |golden|)) per
    iteration, and on the low-resolution flow."""
    ref, ref_low = _golden_warm(factory.__name__, B, H, W)
    model = factory()[0].eval().to(DEV)
    i1, i2 = [t.to(DEV) for t in _inputs(B, H, W)]
    init = _smooth_init(B, H // 8, W // 8)
    eng = RaftEngine(model, DEV, precision="fp32")
    out, low = eng.forward(i1, i2, 4, flow_init=init.to(DEV), return_flow_low=True)
    cold = eng.forward(i1, i2, 4)
    zero = eng.forward(i1, i2, 4, flow_init=torch.zeros_like(init))   # a host tensor is copied in
    torch.cuda.synchronize()
    out, low = out.cpu(), low.cpu()
    assert out.shape == ref.shape and low.shape == ref_low.shape == (B, H // 8, W // 8, 2)
    mag = ref.norm(dim=-1).mean().item()
    assert (ref - cold.cpu()).abs().max().item() > 1.0   # the initial flow matters
    for it in range(4):
        e = _epe(out[it], ref[it])
        print(f"fp32 warm {factory.__name__} B={B} it={it}: epe {e:.3e} bound {1e-3 * (1 + mag):.3e}")
        assert e < 1e-3 * (1 + mag), (it, e, mag)
    mag_low = ref_low.norm(dim=-1).mean().item()
    assert _epe(low, ref_low) < 1e-3 * (1 + mag_low)
    assert torch.equal(zero, cold)


@pytest.mark.parametrize("factory,B,H,W", CONFIGS, ids=IDS)
def test_bf16_engine_warm_matches_golden(factory, B, H, W):
    """The project's cold-start bf16 bound per arch, on a warm start (measured on MI355X:
    profiles/warm_start_parity.txt)."""
    ref, ref_low = _golden_warm(factory.__name__, B, H, W)
    model = factory()[0].eval().to(DEV)
    i1, i2 = [t.to(DEV) for t in _inputs(B, H, W)]
    init = _smooth_init(B, H // 8, W // 8).to(DEV)
    out, low = model(i1, i2, num_flow_updates=4, flow_init=init, return_flow_low=True)   # through RAFT.forward
    torch.cuda.synchronize()
    assert model.execution_path == "engine"
    out = out.cpu()
    assert out.shape == ref.shape and torch.isfinite(out).all()
    mag = ref.norm(dim=-1).mean().item()
    for it in range(4):
        e = _epe(out[it], ref[it])
        print(f"bf16 warm {factory.__name__} B={B} it={it}: rel epe {e / mag:.4f} bound {REL_EPE[factory.__name__]}")
        assert e < REL_EPE[factory.__name__] * mag, (it, e, mag)
    # the low-resolution flow fed back through the golden projection: a usable next flow_init
    nxt = nat.forward_project(low.cpu())
    assert nxt.shape == (B, H // 8, W // 8, 2) and torch.isfinite(nxt).all()


def test_mixed_engine_zero_init_equals_cold():
    model = raft_small()[0].eval().to(DEV)
    i1, i2 = [t.to(DEV) for t in _inputs(1, 128, 128)]
    eng = RaftEngine(model, DEV, precision="mixed")
    cold = eng.forward(i1, i2, 3)
    warm = eng.forward(i1, i2, 3, flow_init=torch.zeros(1, 16, 16, 2, device=DEV))
    moved = eng.forward(i1, i2, 3, flow_init=_smooth_init(1, 16, 16).to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(warm, cold) and (moved - cold).abs().max().item() > 1.0


@pytest.mark.parametrize("factory,B,W,kw", [(raft_small, 1, 128, {}), (raft_large, 2, 256, {"split": 2}),
                                            (raft_small, 1, 128, {"precision": "fp32"})],
                         ids=["small-b1", "large-b2-split2", "small-fp32"])
def test_previous_equals_manual_projection(factory, B, W, kw):
    """flow_init="previous" == projecting the previous call's flow_low by hand; a replay of the
    same warm plan with new inputs carries nothing over; any previous iteration count / output
    mode of the same (B, H, W) qualifies."""
    model = factory()[0].eval().to(DEV)
    eng = RaftEngine(model, DEV, **kw)
    (a, b), (c, _) = [[t.to(DEV) for t in _inputs(B, 128, W, seed=s)] for s in (0, 1)]
    _, l1 = eng.forward(a, b, 3, return_flow_low=True)
    p2, l2 = eng.forward(b, c, 3, flow_init="previous", return_flow_low=True)
    m2 = eng.forward(b, c, 3, flow_init=nat.forward_project(l1))
    p3 = eng.forward(c, a, 3, flow_init="previous")        # the warm plan again, new inputs
    m3 = eng.forward(c, a, 3, flow_init=nat.forward_project(l2))
    _, l5 = eng.forward(a, b, 5, return_all_iters=False, return_flow_low=True)
    p4 = eng.forward(b, c, 3, flow_init="previous")
    m4 = eng.forward(b, c, 3, flow_init=nat.forward_project(l5))
    cold = eng.forward(b, c, 3)
    torch.cuda.synchronize()
    assert l1.shape == (B, 16, W // 8, 2) and torch.isfinite(p2).all()
    assert torch.equal(p2, m2) and torch.equal(p3, m3) and torch.equal(p4, m4)
    assert not torch.equal(p2, cold) and not torch.equal(p4, p2)
    # the projection ran on the device from the plan's own buffer: flow_low is a copy, not a view of it
    assert l1.data_ptr() != l2.data_ptr()


def test_previous_needs_a_previous_call():
    model = raft_small()[0].eval().to(DEV)
    eng = RaftEngine(model, DEV)
    a, b = [t.to(DEV) for t in _inputs(1, 128, 128)]
    with pytest.raises(ValueError, match="previous"):
        eng.forward(a, b, 3, flow_init="previous")
    eng.forward(a, b, 3)
    eng.forward(a, b, 3, flow_init="previous")
    a2, b2 = [t.to(DEV) for t in _inputs(1, 128, 160)]
    with pytest.raises(ValueError, match="previous"):     # another shape
        eng.forward(a2, b2, 3, flow_init="previous")
    eng.forward(a, b, 3)
    with torch.no_grad():
        model.update_block.flow_head.conv2.bias.add_(0.5)
    with pytest.raises(ValueError, match="previous"):     # the weights were repacked since
        eng.forward(a, b, 3, flow_init="previous")
    with pytest.raises(ValueError, match="shape"):
        eng.forward(a, b, 3, flow_init=torch.zeros(1, 16, 17, 2, device=DEV))
    with pytest.raises(ValueError):
        eng.forward(a, b, 3, flow_init="next")
    torch.cuda.synchronize()


def test_u8_frames_padded_flow_low():
    """A 436 x 1024-style odd size scaled down: flow_init / flow_low at the padded size / 8."""
    model = raft_small()[0].eval().to(DEV)
    g = torch.Generator().manual_seed(2)
    a = torch.randint(0, 256, (1, 122, 250, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (1, 122, 250, 3), generator=g, dtype=torch.uint8)
    cold = model(a, b, num_flow_updates=3)
    warm, low = model(a, b, num_flow_updates=3, flow_init=torch.zeros(1, 16, 32, 2), return_flow_low=True)
    nxt = model(a, b, num_flow_updates=3, flow_init="previous")
    torch.cuda.synchronize()
    assert cold.shape == (3, 1, 122, 250, 2) and low.shape == (1, 16, 32, 2)
    assert torch.equal(warm, cold) and torch.isfinite(nxt).all()
    with pytest.raises(ValueError, match=r"\(1, 16, 32, 2\)"):
        model(a, b, num_flow_updates=3, flow_init=torch.zeros(1, 15, 31, 2))


def test_guards_pipelined_cp_and_training():
    model = raft_large()[0].eval().to(DEV)
    a, b = [t.to(DEV) for t in _inputs(1, 128, 128)]
    z = torch.zeros(1, 16, 16, 2, device=DEV)
    eng = RaftEngine(model, DEV)
    with pytest.raises(NotImplementedError):
        eng.pipelined(a, b, 3, flow_init=z)
    with pytest.raises(NotImplementedError):
        eng.pipelined(a, b, 3, flow_init="previous")
    assert eng.flush() is None and eng.num_plans() == 0
    cp = RaftEngine(model, DEV, cp_group=True)
    with pytest.raises(NotImplementedError):
        cp.forward(a, b, 3, flow_init=z)
    with pytest.raises(NotImplementedError):
        model(a, b, train=True, num_flow_updates=2, flow_init=z)
    with pytest.raises(NotImplementedError):
        model(a, b, autograd=True, num_flow_updates=2, flow_init=z)
