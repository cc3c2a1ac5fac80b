"""The motion encoder's output conv inside the first fused ConvGRU stage (gru_fused.hip, op
``gru_fused_me``) against (a) the two launches it replaces -- the halo 3x3 conv, then the
``gru_fused`` row stage -- on the same buffers, and (b) the fp32 reference on the bf16-rounded
operands.  The fused kernel keeps the conv's K order (tap-major, channels in k16 steps, one
accumulator chain) and the stage is unchanged, so (a) is bitwise; against (b) the fused op's
error is then the pair's own error (asserted as "no larger", no absolute bound of its own)."""
import copy
import math

import pytest
import torch

from jax_raft_amd import raft_large
from jax_raft_amd.models import reference as R
from jax_raft_amd.runtime.engine import RaftEngine

pytestmark = pytest.mark.gpu

DEV = "cuda"
HD, CF, MOT = 128, 256, 126   # hidden, motion conv input, motion channels (+ 2 flow channels = x)


def _bf(x):
    return x.to(torch.bfloat16).float()


@pytest.fixture(scope="module")
def weights():
    """One set of weights for every shape: packed specs and their fp32 sources."""
    from jax_raft_amd.ops import native as nat

    nat.require()
    g = torch.Generator().manual_seed(11)
    km = torch.randn(3, 3, CF, MOT, generator=g) / math.sqrt(9 * CF)
    bm = torch.randn(MOT, generator=g) * 0.1
    kz, kr, kq = [torch.randn(1, 5, 2 * HD, HD, generator=g) / math.sqrt(5 * 2 * HD) for _ in range(3)]
    zero = torch.zeros(HD)
    return dict(
        km=km, bm=bm, kz=kz, kr=kr, kq=kq,
        me=nat.make_spec(km, bm, (1, 1), (1, 1), cin8=CF, device=DEV),
        sa=nat.make_spec(torch.cat([kz, kr], 3), torch.zeros(2 * HD), (1, 1), (0, 2), cin8=2 * HD, device=DEV),
        sb=nat.make_spec(kq, zero, (1, 1), (0, 2), cin8=2 * HD, device=DEV))


# (1, 1, 128): no neighbour rows; (2, 3, 24): short rows, both border rows and one interior row;
# (1, 5, 40): w not a multiple of 32; (2, 4, 128): full-width rows, batch crossing
@pytest.mark.parametrize("B,h,w", [(1, 1, 128), (2, 3, 24), (1, 5, 40), (2, 4, 128)])
def test_fused_op_equals_the_pair_bitwise(weights, B, h, w):
    from jax_raft_amd.ops import native as nat

    W = weights
    M = B * h * w
    g = torch.Generator().manual_seed(100 * B + 10 * h + w)
    cf = _bf(torch.randn(B, h, w, CF, generator=g))
    hs = _bf(torch.tanh(torch.randn(B, h, w, HD, generator=g)))
    flow = _bf(torch.randn(B, h, w, 2, generator=g) * 3)
    ctx = _bf(torch.randn(B, h, w, 3 * HD, generator=g) * 0.5)

    # (b) fp32 reference on the bf16-rounded operands (tests/test_kernels_gpu.py's construction)
    mot = _bf(torch.relu(R.conv2d_nhwc(cf, _bf(W["km"]), W["bm"], (1, 1), (1, 1))))
    xs = torch.cat([mot, flow], -1)
    hxr = torch.cat([hs, xs], -1)
    zero = torch.zeros(HD)
    z = torch.sigmoid(R.conv2d_nhwc(hxr, _bf(W["kz"]), zero, (1, 1), (0, 2)) + ctx[..., :HD])
    r = torch.sigmoid(R.conv2d_nhwc(hxr, _bf(W["kr"]), zero, (1, 1), (0, 2)) + ctx[..., HD:2 * HD])
    q = torch.tanh(R.conv2d_nhwc(torch.cat([_bf(r * hs), xs], -1), _bf(W["kq"]), zero, (1, 1), (0, 2))
                   + ctx[..., 2 * HD:])
    ref_h = ((1 - z) * hs + z * q).reshape(M, HD)
    ref_x = xs.reshape(M, HD)

    def buffers():
        hx = torch.full((M, 2 * HD), 5.0, dtype=torch.bfloat16, device=DEV)   # motion slots: a value no result has
        hx[:, :HD] = hs.reshape(M, HD).to(DEV, torch.bfloat16)
        hx[:, HD + MOT:] = flow.reshape(M, 2).to(DEV, torch.bfloat16)
        h32 = hs.reshape(M, HD).to(DEV).contiguous()
        hm = torch.full((M, HD), 7.0, dtype=torch.bfloat16, device=DEV)
        return hx, h32, hm

    cfg_ = cf.reshape(M, CF).to(DEV, torch.bfloat16).contiguous()
    bmap = ctx.reshape(M, 3 * HD).to(DEV, torch.bfloat16).contiguous()

    # (a) the pair: the halo conv in the loop's tile config, then the row stage
    hx_a, h32_a, hm_a = buffers()
    cfg = nat.HALO_CFG0 + nat.HALO_CFGS.index((256, 4, 1, 2, 4, 16))
    nat.ops().conv(*nat.conv_args(W["me"], cfg_, B, h, w, hx_a, y_coff=HD, act=nat.ACT_RELU, cfg=cfg))
    nat.ops().gru_fused([hx_a, W["sa"].w, W["sb"].w, bmap, h32_a, hx_a, hm_a], [B, h, w, 0])
    # the fused op
    hx_f, h32_f, hm_f = buffers()
    nat.ops().gru_fused_me([hx_f, W["sa"].w, W["sb"].w, bmap, h32_f, hx_f, hm_f, None, cfg_, W["me"].w, W["me"].b],
                           [B, h, w, MOT])
    torch.cuda.synchronize()

    assert torch.equal(hx_f[:, HD + MOT:].float().cpu(), flow.reshape(M, 2))   # the flow channels are intact
    assert torch.equal(hx_f, hx_a)       # all 256 channels: h', motion, flow
    assert torch.equal(h32_f, h32_a)
    assert torch.equal(hm_f, hm_a) and torch.equal(hm_f, hx_f[:, :HD])
    # (b): the fused op is no further from the reference than the pair (equal, as (a) is bitwise)
    for name, got_f, got_a, ref in (("h32", h32_f, h32_a, ref_h), ("h", hx_f[:, :HD], hx_a[:, :HD], ref_h),
                                    ("x", hx_f[:, HD:], hx_a[:, HD:], ref_x)):
        ef = (got_f.float().cpu() - ref).abs().max().item()
        ea = (got_a.float().cpu() - ref).abs().max().item()
        print(f"({B}, {h}, {w}) {name}: fused vs fp32 reference {ef:.3e}, pair {ea:.3e}")
        assert math.isfinite(ea) and ef <= ea, (name, ef, ea)


def test_engine_fused_motion_conv_is_bitwise(monkeypatch):
    """raft_large, batch 4, 136 x 264, 3 iterations, every iteration's flow: the lane schedule
    with the motion conv inside the first fused stage equals the two-launch lowering bitwise,
    and a second call on the same engine repeats it (no state carried over)."""
    model, _ = raft_large()
    g = torch.Generator().manual_seed(79)
    base = torch.rand(4, 144, 272, 3, generator=g) * 2 - 1
    i1 = base[:, 4:140, 4:268].contiguous().cuda()
    i2 = base[:, 2:138, 6:270].contiguous().cuda()
    m0 = copy.deepcopy(model).cuda()
    m1 = copy.deepcopy(model).cuda()
    monkeypatch.setattr(RaftEngine, "GRU", "fused")
    monkeypatch.setattr(RaftEngine, "GRU_ME", "off")
    off = m0(i1, i2, num_flow_updates=3, streams=True)
    monkeypatch.setattr(RaftEngine, "GRU_ME", "on")
    on = m1(i1, i2, num_flow_updates=3, streams=True)
    again = m1(i1, i2, num_flow_updates=3, streams=True)
    torch.cuda.synchronize()
    eng = m1.engine(torch.device("cuda", 0), streams=True)
    assert eng.gru_path == "fused" and eng._gru_me_ok(4, 17, 33)
    names = lambda m: [n for st in m.engine(torch.device("cuda", 0), streams=True)._states.values()
                       for n in st.plan.op_names(1)]   # the loop segment
    assert "gru_fused_me" in names(m1) and "gru_fused_me" not in names(m0)
    assert on.shape == (3, 4, 136, 264, 2) and torch.isfinite(on).all()
    assert torch.equal(on, off)
    assert torch.equal(again, on)
