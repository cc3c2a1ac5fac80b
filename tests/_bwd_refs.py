"""Plain fp64 references of the five kernels that carry the fused training backward's gradients
to the feature maps and the weights -- lookup_bwd (corr.hip), pyr_bwd_dc and upsample_convex_bwd
(train.hip), bgemm (bgemm.hip) and wgrad (wgrad.hip: im2col tiles, 3x3 halo path, split
reduction) -- the cases they are tested at and the per-element checks.

Shaped like tests/_train_refs.py: each ``*_ref`` takes the rounded inputs the kernel sees,
computes in float64 and returns the expected value with, per element, the magnitude sum the
tolerance scales with.  Each ``check_*`` takes an implementation (CPU tensors in, CPU tensors
out): the HIP ops in tests/test_bwd_kernels_gpu.py, an fp32 emulation of the kernels' arithmetic
and its mutants in tests/test_bwd_kernel_refs.py.

Tolerances (the convention of tests/_train_refs.py, derived and not measured):

* fp32 result: ``tol = 2^-16 sum |terms|`` per element.
* bf16 result computed in fp32: ``tol = 2^-8 |ref| + 2^-16 bound``.
* Exact results are compared bitwise: a lookup_bwd cell outside every sampling window keeps its
  pre-fill, bgemm with a selection operand returns ``0.5 B[idx]``, sentinels survive.

One kernel needs a further term.  upsample_convex_bwd takes its softmax with ``__expf``, which is
``exp2(x log2(e))`` in fp32: the product's rounding (2^-24 relative, plus the rounded constant)
is an *absolute* error of the exponent of about ``|x| 2^-24``, i.e. a relative error of e_k =
exp(x_k) of up to ``|x_k| 2^-23`` with a factor 2 to spare, x_k = logit_k - max <= 0.  With
w_k = e_k / sum_j e_j the weight's relative error is at most

    d_k = 2^-23 (|x_k| + sum_j w_j |x_j|)

and, to first order in d, with A_j = |g_x u_jx| + |g_y u_jy|:

    dmask_k = alpha w_k (g.u_k - sum_j w_j g.u_j):  alpha w_k (d_k (A_k + sum_j w_j A_j) + sum_j w_j d_j A_j)
    taps[2k + c] = 8 sum_s w_k(s) g_c(s):           8 sum_s w_k(s) d_k(s) |g_c(s)|

These are added to the tolerances.  They vanish for near-uniform logits and reach the size of
the 2^-16 term at |x| ~ 64 (the 12 randn logits case reaches -76).  The hardware exponential returns zero
where exp(x_k) falls below the smallest normal fp32 (2^-126), so w_k also carries an absolute
error of 2^-126, and a bf16 result below 2^-126 may be flushed: ``2^-126 (1 + alpha (A_k + sum_j
w_j A_j))`` is added to dmask's tolerance and ``8 * 2^-126 sum_s |g_c|`` to taps'.

None of these kernels takes a sign decision, so no element is excluded from any check: the
excluded share is 0 by construction, and ``_check`` asserts it.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace as NS

import torch

from _train_refs import U_ACC, U_BF16, _gen, bf, bits_equal, flow_gather_ref, ratio, report  # noqa: F401

F64 = torch.float64
U_EXP = 2.0 ** -23
TINY = 2.0 ** -126
BF16 = torch.bfloat16


def round_up(a: int, b: int) -> int:
    return (a + b - 1) // b * b


def _check(name: str, got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """|got - ref| <= tol on every element: nothing is excluded."""
    assert got.shape == ref.shape == tol.shape, f"{name}: shapes {got.shape} {ref.shape} {tol.shape}"
    checked = got.numel()   # ratio() without a keep mask looks at every element
    excluded = 1.0 - checked / max(ref.numel(), 1)
    assert excluded == 0.0
    r = ratio(got, ref, tol)
    report(name, r, excluded)
    assert r <= 1.0, f"{name}: error / tolerance = {r}"
    return r


# ================================================================================ lookup_bwd
# (B, h, w, L, radius, g dtype, gcs)
LOOKUP_CASES = [
    (2, 9, 13, 4, 4, BF16, 328),          # odd maps down to 1x1, B h w % 4 == 2 (a half-idle last block)
    (1, 8, 16, 4, 4, torch.float32, 324),  # no padding channels
    (1, 7, 10, 2, 6, torch.float32, 344),  # radius 6: lane i = S is the 14th of 16
    (1, 7, 10, 3, 1, BF16, 32),
    (2, 6, 9, 1, 5, BF16, 128),
    (1, 12, 20, 4, 3, BF16, 200),
    (1, 6, 8, 2, 2, torch.float32, 56),
]
LOOKUP_PAD = 1e30   # the padding channels g[:, L S^2:]: must not matter


@functools.lru_cache(maxsize=None)
def lookup_inputs(case):
    B, h, w, L, r, gdt, gcs = case
    M, S = B * h * w, 2 * r + 1
    gen = _gen(800 + LOOKUP_CASES.index(case))
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys], -1).reshape(1, h * w, 2).repeat(B, 1, 1).reshape(M, 2)
    coords = grid + 3 * torch.randn(M, 2, generator=gen)
    coords[0] = torch.tensor([3.0, 2.0])              # exact integers: fx = fy = 0
    coords[1] = torch.tensor([-0.25, -0.25])          # windows straddling the border by a fraction
    coords[2] = torch.tensor([w - 0.75, h - 0.75])
    coords[3] = torch.tensor([-30.5, 3.25])           # off the map at level 0, partly on it at level 3
    coords[4] = torch.tensor([w + 40.0, h + 7.5])
    coords[5] = torch.tensor([float(w - 1), 0.0])
    g = torch.randn(M, gcs, generator=gen)
    if gdt == BF16:
        g = bf(g)
    g[:, L * S * S:] = LOOKUP_PAD
    pre = [torch.randn(M, h >> l, w >> l, generator=gen) for l in range(L)]
    return NS(B=B, h=h, w=w, L=L, r=r, gdt=gdt, gcs=gcs, M=M, S=S, coords=coords.contiguous(), g=g, pre=pre)


def lookup_bwd_ref(coords, g, L, r, h, w):
    """d_l[q] = sum_{i,j} g[q][l S^2 + i S + j] times the four bilinear weights at
    (cx / 2^l - r + i, cy / 2^l - r + j): i the column offset, j the row offset, cells off the map
    dropped.  Per level (value, sum |w g|, cells inside a sampling window), each [M, h_l, w_l]."""
    M, S = coords.shape[0], 2 * r + 1
    g64, q = g.double(), torch.arange(M)
    out = []
    for l in range(L):
        hl, wl = h >> l, w >> l
        c = coords.double() / float(2 ** l)
        fl = torch.floor(c)
        f = c - fl
        x0, y0 = fl[:, 0].long() - r, fl[:, 1].long() - r
        val = torch.zeros(M, hl, wl, dtype=F64)
        bound = torch.zeros_like(val)
        win = torch.zeros(M, hl, wl, dtype=torch.bool)
        for i in range(S):
            for j in range(S):
                gv = g64[:, l * S * S + i * S + j]
                for dx in (0, 1):
                    wx = f[:, 0] if dx else 1.0 - f[:, 0]
                    col = x0 + i + dx
                    for dy in (0, 1):
                        wy = f[:, 1] if dy else 1.0 - f[:, 1]
                        row = y0 + j + dy
                        ok = (col >= 0) & (col < wl) & (row >= 0) & (row < hl)
                        idx = (q[ok], row[ok], col[ok])
                        t = (wx * wy * gv)[ok]
                        val.index_put_(idx, t, accumulate=True)
                        bound.index_put_(idx, t.abs(), accumulate=True)
                        win[idx] = True
        out.append((val, bound, win))
    return out


@functools.lru_cache(maxsize=None)
def lookup_ref_of(case):
    c = lookup_inputs(case)
    return lookup_bwd_ref(c.coords, c.g, c.L, c.r, c.h, c.w)


def check_lookup_bwd(impl, case):
    """impl.lookup_bwd(coords fp32 [M, 2], g [M, gcs] (fp32 storage), g dtype, dlevels (list of fp32
    [M, h_l, w_l]), L, B, h, w, radius) -> the accumulated levels.  Called on the random pre-fill,
    then again on its own result."""
    c = lookup_inputs(case)
    ref = lookup_ref_of(case)
    assert any(bool((~win).any()) for _, _, win in ref) and all(bool(win.any()) for _, _, win in ref)
    one = impl.lookup_bwd(c.coords, c.g, c.gdt, [p.clone() for p in c.pre], c.L, c.B, c.h, c.w, c.r)
    two = impl.lookup_bwd(c.coords, c.g, c.gdt, [p.clone() for p in one], c.L, c.B, c.h, c.w, c.r)
    name = f"lookup_bwd{case[:5]}/{'bf16' if c.gdt == BF16 else 'fp32'}/gcs{c.gcs}"
    assert len(one) == len(two) == c.L
    for l, (val, bound, win) in enumerate(ref):
        p64 = c.pre[l].double()
        _check(f"{name} level {l}", one[l], p64 + val, U_ACC * (p64.abs() + bound))
        _check(f"{name} level {l} second call", two[l], p64 + 2 * val, U_ACC * (p64.abs() + 2 * bound))
        for got in (one[l], two[l]):
            assert got.dtype == torch.float32
            assert bits_equal(got[~win], c.pre[l][~win]), f"{name} level {l}: a cell outside every window changed"


# ================================================================================ pyr_bwd_dc
# (M, h, w, L): M need not be B h w
PYR_CASES = [
    (37, 9, 12, 4),    # scalar kernel; row 8 and columns 8..11 have no coarse terms
    (37, 9, 16, 4),    # vector kernel, odd h
    (5, 8, 8, 4),
    (70, 6, 24, 3),
    (3, 13, 40, 2),
    (11, 5, 16, 1),
]
PYR_SCALES = [1.0 / 16.0, 1.0 / math.sqrt(128.0)]


@functools.lru_cache(maxsize=None)
def pyr_inputs(case):
    M, h, w, L = case
    gen = _gen(900 + PYR_CASES.index(case))
    # g_l ~ 4^l randn: every level weighs the same in dC
    return [torch.randn(M, h >> l, w >> l, generator=gen) * float(4 ** l) for l in range(L)]


def pyr_bwd_dc_ref(gs, h, w, scale):
    """dC[q][y][x] = s sum_l g_l[q][y >> l][x >> l] / 4^l over y < h_l 2^l, x < w_l 2^l (the adjoint of
    the 2x2 floor average pooling chain); s at its fp32 value.  Returns (value, magnitude sum)."""
    s = float(torch.tensor(scale, dtype=torch.float32))
    M = gs[0].shape[0]
    val = torch.zeros(M, h, w, dtype=F64)
    bound = torch.zeros_like(val)
    for l, g in enumerate(gs):
        f = 2 ** l
        up = g.double().repeat_interleave(f, 1).repeat_interleave(f, 2) / float(4 ** l)
        val[:, :up.shape[1], :up.shape[2]] += up
        bound[:, :up.shape[1], :up.shape[2]] += up.abs()
    return s * val, s * bound


def check_pyr_bwd_dc(impl, case, scale):
    """impl.pyr_bwd_dc(gs (list of fp32 [M, h_l, w_l]), L, M, h, w, scale) -> fp32 [M, h, w] holding the
    bf16 result."""
    M, h, w, L = case
    gs = pyr_inputs(case)
    ref, bound = pyr_bwd_dc_ref(gs, h, w, scale)
    out = impl.pyr_bwd_dc(gs, L, M, h, w, scale)
    _check(f"pyr_bwd_dc{case} scale={scale:.5f}", out, ref, U_BF16 * ref.abs() + U_ACC * bound)


# ================================================================================ bgemm
# (batch, M, N, K)
BGEMM_CASES = [(1, 128, 128, 64), (2, 256, 128, 192), (3, 128, 256, 128), (1, 128, 128, 3072)]
BGEMM_SELECT_CASES = BGEMM_CASES[:2]
BGEMM_ALPHA = 0.37
BGEMM_SELECT_ALPHA = 0.5


@functools.lru_cache(maxsize=2)
def bgemm_inputs(case, select):
    batch, M, N, K = case
    gen = _gen(1000 + BGEMM_CASES.index(case))
    b = bf(torch.randn(batch, K, N, generator=gen))
    if select:   # row m of op(A[b]) has a single 1 at column (7 m + 3 b) mod K
        idx = (7 * torch.arange(M)[None, :] + 3 * torch.arange(batch)[:, None]) % K
        a = torch.zeros(batch, M, K)
        a.scatter_(2, idx[..., None], 1.0)
        return NS(a=a, b=b, idx=idx)
    return NS(a=bf(torch.randn(batch, M, K, generator=gen)), b=b, idx=None)


def bgemm_ref(a, b, alpha):
    """alpha op(A) B in fp64 with alpha at its fp32 value; a is op(A) [batch, M, K]."""
    al = float(torch.tensor(alpha, dtype=torch.float32))
    return al * torch.matmul(a.double(), b.double()), abs(al) * torch.matmul(a.double().abs(), b.double().abs())


def _bgemm_name(case, a_kmajor, out_dtype):
    return f"bgemm{case} a_kmajor={a_kmajor} {'fp32' if out_dtype == torch.float32 else 'bf16'}"


def check_bgemm(impl, case, a_kmajor, out_dtype):
    """impl.bgemm(A bf16 ([batch, M, K], or [batch, K, M] with a_kmajor), B bf16 [batch, K, N], M, N, K,
    a_kmajor, alpha, out_dtype) -> C of out_dtype [batch, M, N]."""
    batch, M, N, K = case
    c = bgemm_inputs(case, False)
    ref, bound = bgemm_ref(c.a, c.b, BGEMM_ALPHA)
    a = (c.a.transpose(1, 2) if a_kmajor else c.a).contiguous().to(BF16)
    out = impl.bgemm(a, c.b.to(BF16), M, N, K, a_kmajor, BGEMM_ALPHA, out_dtype)
    assert out.dtype == out_dtype and out.shape == (batch, M, N)
    tol = U_ACC * bound if out_dtype == torch.float32 else U_BF16 * ref.abs() + U_ACC * bound
    _check(_bgemm_name(case, a_kmajor, out_dtype), out.float(), ref, tol)


def check_bgemm_select(impl, case, a_kmajor, out_dtype):
    """A selection operand makes every output one element of B: C[m][n] = 0.5 B[idx[m]][n] bitwise, so a
    permutation inside K -- which a sum over random operands cannot see when both fragments share it --
    is an exact mismatch."""
    batch, M, N, K = case
    c = bgemm_inputs(case, True)
    a = (c.a.transpose(1, 2) if a_kmajor else c.a).contiguous().to(BF16)
    out = impl.bgemm(a, c.b.to(BF16), M, N, K, a_kmajor, BGEMM_SELECT_ALPHA, out_dtype)
    want = (BGEMM_SELECT_ALPHA * torch.gather(c.b, 1, c.idx[..., None].expand(batch, M, N))).to(out_dtype)
    assert out.dtype == out_dtype and out.shape == (batch, M, N)
    ok = bits_equal(out, want)
    report(_bgemm_name(case, a_kmajor, out_dtype) + " selection (bitwise)", 0.0 if ok else float("inf"), 0.0)
    assert ok, f"bgemm{case} a_kmajor={a_kmajor}: C is not 0.5 B[(7 m + 3 b) mod K] bitwise"


# ================================================================================ wgrad
# (N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, stride, (PH, PW))
_HALO = (3, 3, 1, (1, 1))
WGRAD_HALO_CASES = [
    (1, 8, 16, 64, 0, 64, 64, 64, 64, 0) + _HALO,          # one tile, S = 1
    (3, 17, 33, 72, 0, 72, 72, 70, 72, 0) + _HALO,         # 27 tiles ragged right and below, S = 7, last split 3
    (2, 9, 11, 512, 256, 256, 256, 64, 256, 192) + _HALO,  # slices at an offset
    (1, 10, 12, 8, 0, 2, 8, 128, 128, 0) + _HALO,
    (1, 10, 12, 256, 0, 256, 256, 2, 8, 0) + _HALO,
]
WGRAD_IM2COL_CASES = [
    (2, 25, 35, 64, 0, 64, 64, 96, 96, 0, 3, 3, 2, (1, 1)),       # M = 468: two splits, the second ends in 20 pixels
    (1, 10, 12, 328, 0, 324, 328, 256, 256, 0, 1, 1, 1, (0, 0)),
    (1, 13, 17, 8, 0, 3, 8, 64, 64, 0, 7, 7, 2, (3, 3)),
    (2, 7, 9, 256, 0, 256, 256, 192, 192, 0, 1, 5, 1, (0, 2)),    # 256 x 256 tile, partial cout tile
    (2, 7, 9, 256, 0, 256, 256, 192, 192, 0, 5, 1, 1, (2, 0)),
    (2, 13, 17, 32, 0, 32, 32, 64, 64, 0, 1, 1, 2, (0, 0)),       # 64 x 64 tile
]
WGRAD_CASES = WGRAD_HALO_CASES + WGRAD_IM2COL_CASES
WGRAD_PAD = 1e4   # channels cin..cin8 of x and cout..round_up(cout, 8) of dy
WPX, HTR, HTC = 64, 8, 16


def wgrad_out_hw(case):
    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, (PH, PW) = case
    return (H + 2 * PH - KH) // s + 1, (W + 2 * PW - KW) // s + 1


def wgrad_is_halo(case):
    return case[10:] == _HALO


def wgrad_plan(case):
    """What wgrad.hip plans for a case (jr_wgrad_plan, wgrad_halo_geom, jr_wgrad): the splits S, the
    workspace rows / columns (cout_pad, kpad), and per split the pixels (im2col path: px_split, a
    multiple of 64) or the 8 x 16 pixel tiles (halo path: tps) it reduces over."""
    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, (PH, PW) = case
    OH, OW = wgrad_out_hw(case)
    M, K = N * OH * OW, KH * KW * cin8
    if cout >= 192 and K >= 1024:
        bco, bkk, slots = 256, 256, 256
    else:
        bco, bkk, slots = (128 if cout > 64 else 64), (128 if K > 64 else 64), 512
    tiles = ((K + bkk - 1) // bkk) * ((cout + bco - 1) // bco)
    S = max(1, min(slots // tiles, (M + 4 * WPX - 1) // (4 * WPX)))
    plan = NS(M=M, K=K, bco=bco, bkk=bkk, cout_pad=round_up(cout, bco), kpad=round_up(K, bkk), halo=wgrad_is_halo(case))
    if plan.halo:
        tx, ty = (W + HTC - 1) // HTC, (H + HTR - 1) // HTR
        ntiles, nco, nci = N * tx * ty, (cout + 63) // 64, (cin8 + 63) // 64
        s_ = max(1, min(256 // (nco * nci), (ntiles + 3) // 4))
        plan.tps = (ntiles + s_ - 1) // s_
        plan.S = (ntiles + plan.tps - 1) // plan.tps
        plan.ntiles, plan.tiles_x, plan.tiles_y = ntiles, tx, ty
        plan.cout_pad = max(plan.cout_pad, nco * 64)
    else:
        plan.px_split = round_up((M + S - 1) // S, WPX)
        plan.S = (M + plan.px_split - 1) // plan.px_split
    return plan


@functools.lru_cache(maxsize=2)
def wgrad_inputs(case):
    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, pad = case
    OH, OW = wgrad_out_hw(case)
    cout8 = round_up(cout, 8)
    assert xoff + cin8 <= xcs and yoff + cout8 <= ycs
    gen = _gen(1100 + WGRAD_CASES.index(case))
    x = torch.full((N, H, W, xcs), float("nan"))
    dy = torch.full((N, OH, OW, ycs), float("nan"))
    x[..., xoff:xoff + cin8] = WGRAD_PAD
    dy[..., yoff:yoff + cout8] = WGRAD_PAD
    x[..., xoff:xoff + cin] = bf(torch.randn(N, H, W, cin, generator=gen))
    dy[..., yoff:yoff + cout] = bf(torch.randn(N, OH, OW, cout, generator=gen))
    return NS(x=x, dy=dy)


def wgrad_ref(x, dy, case):
    """fp64 autograd of models/reference.py:conv2d_nhwc on the slices: (dW [KH, KW, cin, cout], db [cout])
    and the same on |x|, |dy| (the sums of the terms' magnitudes)."""
    from jax_raft_amd.models import reference as R

    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, pad = case
    xs, ys = x[..., xoff:xoff + cin].double(), dy[..., yoff:yoff + cout].double()
    k = torch.zeros(KH, KW, cin, cout, dtype=F64, requires_grad=True)
    b = torch.zeros(cout, dtype=F64, requires_grad=True)
    dw, db = torch.autograd.grad(R.conv2d_nhwc(xs, k, b, (s, s), pad), (k, b), ys)
    bw, bb = torch.autograd.grad(R.conv2d_nhwc(xs.abs(), k, b, (s, s), pad), (k, b), ys.abs())
    return dw, db, bw, bb


@functools.lru_cache(maxsize=2)
def wgrad_ref_of(case):
    c = wgrad_inputs(case)
    return wgrad_ref(c.x, c.dy, case)


def _wgrad_name(case):
    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, pad = case
    return (f"wgrad {'halo' if wgrad_is_halo(case) else 'im2col'} {KH}x{KW}/s{s} ({N}, {H}, {W}) "
            f"{cin}/{cin8}@{xoff}/{xcs} -> {cout}@{yoff}/{ycs}")


def check_wgrad(impl, case):
    """impl.wgrad(x bf16 [N, H, W, xcs], dy bf16 [N, OH, OW, ycs], case) -> (dw fp32 [KH, KW, cin, cout],
    db fp32 [cout]).  Channels outside the 8-aligned slices are NaN, channels of the 8-padding 1e4."""
    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, pad = case
    c = wgrad_inputs(case)
    dw_ref, db_ref, dw_bound, db_bound = wgrad_ref_of(case)
    dw, db = impl.wgrad(c.x.to(BF16), c.dy.to(BF16), case)
    assert dw.dtype == torch.float32 and db.dtype == torch.float32
    _check(_wgrad_name(case) + " dw", dw, dw_ref, U_ACC * dw_bound)
    _check(_wgrad_name(case) + " db", db, db_ref, U_ACC * db_bound)


# ================================================================================ upsample_convex_bwd
CONVEX_CASES = [(1, 1, 1), (1, 2, 3), (2, 5, 7), (3, 6, 16)]   # (B, h, w)
# (case, alpha, logit scale): both alphas everywhere, near one-hot softmax once
CONVEX_VARIANTS = [(c, a, 2.0) for c in CONVEX_CASES for a in (0.25, 1.0)] + [((2, 5, 7), 0.25, 12.0)]
CONVEX_DCS = 584
CONVEX_SENTINEL = -7.0


@functools.lru_cache(maxsize=None)
def convex_inputs(case, logit_scale):
    B, h, w = case
    M = B * h * w
    gen = _gen(1200 + M + int(logit_scale))
    mask = bf(logit_scale * torch.randn(M, 576, generator=gen))
    flow = 3 * torch.randn(M, 2, generator=gen)
    g = torch.randn(B, 8 * h, 8 * w, 2, generator=gen)
    return NS(mask=mask, flow=flow, g=g)


def convex_neighbours(flow, B, h, w, clamp=False):
    """u_k = 8 flow(q + d_k), d_k = (k / 3 - 1, k % 3 - 1) (row, column), 0 off the map: [M, 9, 2]."""
    f = 8.0 * flow.reshape(B, h, w, 2)
    fp = torch.zeros(B, h + 2, w + 2, 2, dtype=flow.dtype)
    fp[:, 1:-1, 1:-1] = f
    if clamp:   # a mutant's neighbourhood: the border pixel instead of zero
        ys, xs = (torch.arange(h + 2) - 1).clamp(0, h - 1), (torch.arange(w + 2) - 1).clamp(0, w - 1)
        fp = f[:, ys][:, :, xs]
    u = torch.stack([fp[:, k // 3:k // 3 + h, k % 3:k % 3 + w] for k in range(9)], 3)   # [B, h, w, 9, 2]
    return u.reshape(B * h * w, 9, 2)


def convex_subpixels(g, B, h, w):
    """g [B, 8h, 8w, 2] -> [M, 64, 2]: sub-pixel s = a 8 + b of pixel (y, x) is (8 y + a, 8 x + b)."""
    return g.reshape(B, h, 8, w, 8, 2).permute(0, 1, 3, 2, 4, 5).reshape(B * h * w, 64, 2)


def upsample_convex_bwd_ref(mask, flow, g, B, h, w, alpha):
    """Closed form in fp64: dmask_k(s) = alpha w_k (g.u_k - g.up), taps[q][2k + c] = 8 sum_s w_k(s) g_c(s),
    w = softmax_k(mask[k 64 + s]), with the magnitude sums and the __expf terms of the module docstring."""
    M = B * h * w
    al = float(torch.tensor(alpha, dtype=torch.float32))
    logit = mask.double().reshape(M, 9, 64)
    x = logit - logit.max(1, keepdim=True).values
    wk = torch.softmax(logit, 1)                                   # [M, 9, 64]
    u = convex_neighbours(flow.double(), B, h, w)                  # [M, 9, 2]
    gs = convex_subpixels(g.double(), B, h, w)                     # [M, 64, 2]
    a = torch.einsum("mkc,msc->mks", u, gs)                        # g.u_k
    A = torch.einsum("mkc,msc->mks", u.abs(), gs.abs())            # |g_x u_kx| + |g_y u_ky|
    gup, Aup = (wk * a).sum(1, keepdim=True), (wk * A).sum(1, keepdim=True)
    d = U_EXP * (x.abs() + (wk * x.abs()).sum(1, keepdim=True))
    out = NS()
    out.dmask = (al * wk * (a - gup)).reshape(M, 576)
    out.dmask_bound = (al * wk * (A + Aup)).reshape(M, 576)
    out.dmask_extra = (al * wk * (d * (A + Aup) + (wk * d * A).sum(1, keepdim=True)) +
                       TINY * (1.0 + al * (A + Aup))).reshape(M, 576)
    out.taps = 8.0 * torch.einsum("mks,msc->mkc", wk, gs).reshape(M, 18)
    out.taps_bound = 8.0 * torch.einsum("mks,msc->mkc", wk, gs.abs()).reshape(M, 18)
    out.taps_extra = (8.0 * torch.einsum("mks,msc->mkc", wk * d, gs.abs()) +
                      8.0 * TINY * gs.abs().sum(1)[:, None, :]).reshape(M, 18)
    return out


def check_upsample_convex_bwd(impl, variant):
    """impl.upsample_convex_bwd(mask [M, 576] (bf16 values), flow fp32 [M, 2], g fp32 [B, 8h, 8w, 2], B, h, w,
    alpha, dcs, sentinel) -> (dmask fp32 [M, dcs] holding the bf16 result, columns 576.. pre-filled with the
    sentinel; taps fp32 [M, 18])."""
    case, alpha, logit_scale = variant
    B, h, w = case
    c = convex_inputs(case, logit_scale)
    ref = upsample_convex_bwd_ref(c.mask, c.flow, c.g, B, h, w, alpha)
    dmask, taps = impl.upsample_convex_bwd(c.mask, c.flow, c.g, B, h, w, alpha, CONVEX_DCS, CONVEX_SENTINEL)
    name = f"upsample_convex_bwd{case} alpha={alpha} logits x{logit_scale:g}"
    assert dmask.shape == (B * h * w, CONVEX_DCS)
    assert bool((dmask[:, 576:] == CONVEX_SENTINEL).all()), f"{name}: dmask written past column 576"
    _check(name + " dmask", dmask[:, :576], ref.dmask,
           U_BF16 * ref.dmask.abs() + U_ACC * ref.dmask_bound + ref.dmask_extra)
    _check(name + " taps", taps, ref.taps, U_ACC * ref.taps_bound + ref.taps_extra)
