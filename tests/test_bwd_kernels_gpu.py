"""Per-element fp64 reference tests of the HIP kernels that carry the fused training backward's
gradients to the feature maps and the weights: lookup_bwd (corr.hip), pyr_bwd_dc and
upsample_convex_bwd (train.hip), bgemm (bgemm.hip) and wgrad (wgrad.hip: the im2col tiles, the
3x3 halo path and the split reduction).

The references, cases, tolerances and assertions live in tests/_bwd_refs.py and are shared with
tests/test_bwd_kernel_refs.py, which checks the references against fp64 autograd, runs the same
assertions on an fp32 CPU emulation of the kernels and shows that mutants of it fail them.  Every
comparison is per element, |got - ref| <= tol everywhere and nothing excluded; exact results
(untouched lookup cells, the selection GEMM, sentinels) are compared bitwise.  Every output buffer
starts as NaN, or as the stated pre-fill (lookup_bwd accumulates into random fp32 maps; dmask
keeps a sentinel in columns 576..).

Not reachable: ``pyr_bwd_dc8_kernel``, the 64-bit-index form of the vector kernel, needs
M h w >= 2^34 elements (a 32 GB bf16 volume) and cannot be reached at test size; the scalar and the
32-bit vector kernels are.
"""
import pytest
import torch

import _bwd_refs as Bw

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


def _ops():
    from jax_raft_amd.ops import native

    native.require()
    return native.ops()


def _d(x, dtype=None):
    return x.to(DEV, dtype).contiguous() if dtype is not None else x.to(DEV).contiguous()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _wgrad_ints(case):
    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, (PH, PW) = case
    OH, OW = Bw.wgrad_out_hw(case)
    return [N, H, W, xoff, cin8, KH, KW, s, s, PH, PW, yoff, OH, OW, cout, cin]


class Gpu:
    """The HIP kernels behind the interface of tests/_bwd_refs.py: CPU tensors in and out."""

    def lookup_bwd(self, coords, g, gdt, dlevels, L, B, h, w, r):
        lv = [_d(v) for v in dlevels]
        _ops().lookup_bwd([_d(coords), _d(g, gdt)] + lv + [None] * (4 - L), [L, B, h, w, r])
        torch.cuda.synchronize()
        return [v.cpu() for v in lv]

    def pyr_bwd_dc(self, gs, L, M, h, w, scale):
        dc = _nan(M, h, w, dtype=BF16)
        _ops().pyr_bwd_dc([dc] + [_d(g) for g in gs] + [None] * (4 - L), [L, M, h, w], scale)
        torch.cuda.synchronize()
        return dc.float().cpu()

    def bgemm(self, a, b, M, N, K, a_kmajor, alpha, out_dtype):
        c = _nan(a.shape[0], M, N, dtype=out_dtype)
        _ops().bgemm([_d(a), _d(b), c], [M, N, K, a_kmajor], alpha)
        torch.cuda.synchronize()
        return c.cpu()

    def wgrad(self, x, dy, case, part=None, bpart=None):
        N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, pad = case
        dw, db = _nan(KH, KW, cin, cout), _nan(cout)
        # part = bpart = None: the op sizes its own workspace
        _ops().wgrad([_d(x), _d(dy), dw, db, part, bpart], _wgrad_ints(case))
        torch.cuda.synchronize()
        return dw.cpu(), db.cpu()

    def upsample_convex_bwd(self, mask, flow, g, B, h, w, alpha, dcs, sentinel):
        M = B * h * w
        dmask = _nan(M, dcs, dtype=BF16)
        dmask[:, 576:] = sentinel
        taps = _nan(M, 18)
        _ops().upsample_convex_bwd([_d(mask, BF16), _d(flow), _d(g), dmask, taps], [B, h, w], alpha)
        torch.cuda.synchronize()
        return dmask.float().cpu(), taps.cpu()


GPU = Gpu()
BGEMM_DTYPES = [torch.float32, BF16]


@pytest.mark.parametrize("case", Bw.LOOKUP_CASES, ids=str)
def test_lookup_bwd(case):
    Bw.check_lookup_bwd(GPU, case)


@pytest.mark.parametrize("scale", Bw.PYR_SCALES, ids=["s16", "s128"])
@pytest.mark.parametrize("case", Bw.PYR_CASES, ids=str)
def test_pyr_bwd_dc(case, scale):
    Bw.check_pyr_bwd_dc(GPU, case, scale)


@pytest.mark.parametrize("out_dtype", BGEMM_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("a_kmajor", [0, 1])
@pytest.mark.parametrize("case", Bw.BGEMM_CASES, ids=str)
def test_bgemm(case, a_kmajor, out_dtype):
    Bw.check_bgemm(GPU, case, a_kmajor, out_dtype)


@pytest.mark.parametrize("out_dtype", BGEMM_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("a_kmajor", [0, 1])
@pytest.mark.parametrize("case", Bw.BGEMM_SELECT_CASES, ids=str)
def test_bgemm_select(case, a_kmajor, out_dtype):
    Bw.check_bgemm_select(GPU, case, a_kmajor, out_dtype)


@pytest.mark.parametrize("case", Bw.WGRAD_CASES, ids=str)
def test_wgrad(case):
    Bw.check_wgrad(GPU, case)


def test_wgrad_halo_plan():
    """The ragged halo case is planned as 7 splits of 4 tiles (the last one 3): the op accepts a workspace
    of exactly 7 partial tiles, computes the same gradient in it, and refuses one element less."""
    case = Bw.WGRAD_HALO_CASES[1]
    plan = Bw.wgrad_plan(case)
    assert (plan.S, plan.tps, plan.ntiles) == (7, 4, 27)
    c = Bw.wgrad_inputs(case)
    x, dy = c.x.to(BF16), c.dy.to(BF16)
    n = plan.S * plan.cout_pad * plan.kpad
    dw, db = GPU.wgrad(x, dy, case, _nan(n), _nan(plan.S * plan.cout_pad))
    dw0, db0 = GPU.wgrad(x, dy, case)
    assert Bw.bits_equal(dw, dw0) and Bw.bits_equal(db, db0)
    with pytest.raises(RuntimeError, match="wgrad: workspace"):
        GPU.wgrad(x, dy, case, _nan(n - 1), _nan(plan.S * plan.cout_pad))
    with pytest.raises(RuntimeError, match="wgrad: workspace"):
        GPU.wgrad(x, dy, case, _nan(n), _nan(plan.S * plan.cout_pad - 1))


@pytest.mark.parametrize("variant", Bw.CONVEX_VARIANTS, ids=str)
def test_upsample_convex_bwd(variant):
    Bw.check_upsample_convex_bwd(GPU, variant)
