"""The fused flow features (flowfeat.hip, op ``flow_features_fused``) against (a) the two launches
they replace -- ``conv_direct`` (7x7, 2 -> 128, relu), then the halo 3x3 conv (128 -> 64, relu) in
the tile config <128, 2, 2, 2, 8, 16> -- on the same buffers, and (b) the fp32 reference on the
bf16-rounded operands.  The fused kernel keeps both convs' accumulation order (kc = 0..3 for the
7x7; tap-major k16 steps in one accumulator chain for the 3x3) and rounds the intermediate to bf16
as the 7x7 conv stores it, so (a) is bitwise; against (b) the fused op's error is then the pair's
own error (asserted as "no larger", no absolute bound of its own)."""
import copy
import math

import pytest
import torch

from jax_raft_amd import raft_large
from jax_raft_amd.models import reference as R
from jax_raft_amd.runtime.engine import RaftEngine

pytestmark = pytest.mark.gpu

DEV = "cuda"
C1, C2, CS, COFF = 128, 64, 264, 192   # convflow1 / convflow2 channels; the wider ``cf`` rows and the slice written
SENTINEL = 5.0                          # a value no relu output of these weights takes exactly


def _bf(x):
    return x.to(torch.bfloat16).float()


def _pair_cfg():
    from jax_raft_amd.ops import native as nat

    return nat.HALO_CFG0 + nat.HALO_CFGS.index((128, 2, 2, 2, 8, 16))


@pytest.fixture(scope="module")
def weights():
    """One set of weights for every shape: the packed operands and their fp32 sources."""
    from jax_raft_amd.ops import native as nat

    nat.require()
    g = torch.Generator().manual_seed(23)
    k1 = torch.randn(7, 7, 2, C1, generator=g) / math.sqrt(49 * 2) / 8
    b1 = torch.randn(C1, generator=g) * 0.1
    k2 = torch.randn(3, 3, C1, C2, generator=g) / math.sqrt(9 * C1)
    b2 = torch.randn(C2, generator=g) * 0.1
    return dict(k1=k1, b1=b1, k2=k2, b2=b2, w1=nat.pack_direct_weight(k1).to(DEV), b1d=b1.to(DEV).contiguous(),
                sp2=nat.make_spec(k2, b2, (1, 1), (1, 1), cin8=C1, device=DEV))


# (1, 1, 16): one row -- top and bottom padding in the same tile, the 7x7 window mostly outside the
# image; (2, 3, 24): width not a multiple of 16, two images; (1, 9, 17): one row and one column past
# a tile edge; (2, 8, 16): exactly one tile per image (nothing may leak across the batch boundary);
# (1, 5, 40): several tiles across with a ragged last one
@pytest.mark.parametrize("B,h,w", [(1, 1, 16), (2, 3, 24), (1, 9, 17), (2, 8, 16), (1, 5, 40)])
def test_flow_features_fused_equals_the_pair_bitwise(weights, B, h, w):
    from jax_raft_amd.ops import native as nat

    W = weights
    M = B * h * w
    g = torch.Generator().manual_seed(1000 * B + 10 * h + w)
    flow = _bf(torch.randn(B, h, w, 2, generator=g) * 15)   # tens of pixels: the bf16 rounding of flow8 matters

    # (b) fp32 reference on the bf16-rounded operands (tests/test_kernels_gpu.py's construction)
    f1r = _bf(torch.relu(R.conv2d_nhwc(flow, _bf(W["k1"]), W["b1"], (1, 1), (3, 3))))
    ref = torch.relu(R.conv2d_nhwc(f1r, _bf(W["k2"]), W["b2"], (1, 1), (1, 1))).reshape(M, C2)

    flow8 = flow.reshape(M, 2).to(DEV, torch.bfloat16).contiguous()
    # (a) the pair on its own buffers
    f1 = torch.full((M, C1), SENTINEL, dtype=torch.bfloat16, device=DEV)
    cf_a = torch.full((M, CS), SENTINEL, dtype=torch.bfloat16, device=DEV)
    nat.ops().conv_direct([flow8, W["w1"], W["b1d"], f1], [B, h, w, 2, 7, 7, 3, 3, C1, 1, 0])
    nat.ops().conv(*nat.conv_args(W["sp2"], f1, B, h, w, cf_a, y_coff=COFF, act=nat.ACT_RELU, cfg=_pair_cfg()))
    # the fused op
    cf_f = torch.full((M, CS), SENTINEL, dtype=torch.bfloat16, device=DEV)
    nat.flow_features_fused(flow8, W["w1"], W["b1d"], W["sp2"], B, h, w, cf_f, COFF)
    torch.cuda.synchronize()

    for cf in (cf_f, cf_a):   # the channels beside the slice are untouched
        assert (cf[:, :COFF] == SENTINEL).all() and (cf[:, COFF + C2:] == SENTINEL).all()
    assert torch.equal(cf_f, cf_a)
    got_f, got_a = cf_f[:, COFF:COFF + C2].float().cpu(), cf_a[:, COFF:COFF + C2].float().cpu()
    ef, ea = (got_f - ref).abs().max().item(), (got_a - ref).abs().max().item()
    print(f"({B}, {h}, {w}) cf: fused vs fp32 reference {ef:.3e}, pair {ea:.3e}, max |ref| {ref.abs().max().item():.3e}")
    assert ref.abs().max().item() > 0.1 and math.isfinite(ea) and ef <= ea, (ef, ea)


def test_engine_fused_flow_features_are_bitwise(monkeypatch):
    """raft_large, batch 2, 136 x 264 (h = 17, w = 33), 3 iterations, every iteration's flow, on the
    lane schedule: the fused flow features equal the two-launch lowering bitwise (its 3x3 conv in
    the halo config the fused kernel is built on), and a second call into a fresh output tensor
    repeats the result."""
    model, _ = raft_large()
    g = torch.Generator().manual_seed(83)
    base = torch.rand(2, 144, 272, 3, generator=g) * 2 - 1
    i1 = base[:, 4:140, 4:268].contiguous().cuda()
    i2 = base[:, 2:138, 6:270].contiguous().cuda()
    m0 = copy.deepcopy(model).cuda()
    m1 = copy.deepcopy(model).cuda()
    kw = dict(num_flow_updates=3, streams=True)
    monkeypatch.setenv("JR_CFG_OVERRIDE", f"me.convflow2={_pair_cfg()}")   # (read when an engine is built)
    monkeypatch.setattr(RaftEngine, "FLOW_FUSED", "off")
    off = m0(i1, i2, **kw)
    monkeypatch.setattr(RaftEngine, "FLOW_FUSED", "on")
    on = m1(i1, i2, **kw)
    again = m1(i1, i2, **kw)
    torch.cuda.synchronize()
    names = lambda m: [n.split("@")[0] for st in m.engine(torch.device("cuda", 0), streams=True)._states.values()
                       for n in st.plan.op_names(1)]   # the loop segment ("op@lane" on the side lanes)
    assert "flow_features_fused" in names(m1) and "conv_direct" not in names(m1)
    assert "flow_features_fused" not in names(m0) and "conv_direct" in names(m0)
    assert on.shape == (3, 2, 136, 264, 2) and torch.isfinite(on).all()
    assert again.data_ptr() != on.data_ptr()
    assert torch.equal(on, off)
    assert torch.equal(again, on)
