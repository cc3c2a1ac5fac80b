"""Plain fp64 references of the training-only kernels (csrc/kernels/train.hip and the
statistics / norm_act kernels of elementwise.hip), the cases they are tested at and the
per-element checks.

Each ``*_ref`` takes the same rounded inputs the kernel sees (bf16-valued tensors, fp32
statistics), computes in float64 and returns the expected value together with, per element,
the magnitude sum that the tolerance scales with.

Each ``check_*`` takes an *implementation* -- an object with one method per kernel that maps
CPU tensors to CPU tensors -- and asserts it against the reference.  The GPU tests pass the
HIP kernels (tests/test_train_kernels_gpu.py); the CPU tests pass an fp32 emulation of the
kernels' arithmetic (tests/test_train_kernel_refs.py), which shows that the derived
tolerances are attainable, i.e. not vacuous and not too tight for correct fp32 code.

Tolerances (derived, not measured):

* bf16 output computed in fp32: ``tol = 2^-8 |ref| + 2^-16 bound``.  The first term is one
  bf16 round-to-nearest (half an ulp is at most 2^-8 relative); the second is 256 fp32 unit
  roundoffs of the operands' magnitude (rsqrt, contraction, summation order) and stays 256x
  below a bf16 ulp.
* fp32 reduction: ``tol = 2^-16 sum |terms|``.
* ReLU sign: an element is ambiguous iff ``0 < |z| <= 2^-18 (|gamma xhat| + |beta|)``.
"""
from __future__ import annotations

import functools
import struct
from types import SimpleNamespace as NS

import torch

EPS = 1e-5
U_BF16 = 2.0 ** -8
U_ACC = 2.0 ** -16
U_SIGN = 2.0 ** -18
U_BN = 2.0 ** -20
REPORT = []   # (name, largest error / tolerance, excluded share) of every check of this process


def bf(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep fp32 storage."""
    return x.to(torch.bfloat16).float()


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def ratio(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor, keep=None) -> float:
    """Largest |got - ref| / tol over the kept elements (a NaN or an error at tol = 0 is inf)."""
    err = (got.double() - ref.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol.double().expand_as(err))
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))
    if keep is not None:
        r = torch.where(keep.expand_as(r), r, torch.zeros_like(r))
    return float(r.max()) if r.numel() else 0.0


def report(name: str, r: float, excluded: float = 0.0) -> None:
    REPORT.append((name, r, excluded))
    print(f"[train-kernels] {name}: max err/tol = {r:.3f}, excluded = {100 * excluded:.3f} %")


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ----------------------------------------------------------------------------- normalisation
def norm_mean_rstd(st, mode: int, N: int, HW: int, C: int, eps: float = EPS):
    """fp64 (mean, rstd), each [N, 1, C], from the (sum, sumsq) statistics [N][C][2].
    mode 1: per (n, c), cnt = HW; mode 2: summed over n, cnt = N HW; mode 0: identity."""
    if mode == 0:
        return torch.zeros(N, 1, C, dtype=torch.float64), torch.ones(N, 1, C, dtype=torch.float64)
    s = st.double().reshape(N, C, 2)
    cnt = float(HW)
    if mode == 2:
        s = s.sum(0, keepdim=True).expand(N, C, 2)
        cnt = float(N) * float(HW)
    mean = s[..., 0] / cnt
    var = (s[..., 1] / cnt - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    return mean[:, None, :], rstd[:, None, :]


def norm_bwd_ref(g, om, y, st, mode, gamma, beta, relu, eps=EPS):
    """Backward of conv -> norm -> (relu) [+ residual] (comment block above the norm_bwd kernels).
    g, om, y: [N, HW, C]; st: [N, C, 2] or None (mode 0).  Returns dy, bound (per element), red and
    red_bound ([N, C, 2]: sum g, sum g xhat and the sums of the terms' magnitudes), gres, the
    ambiguous-ReLU element mask and the [N, C] mask of normalisation sets holding one."""
    N, HW, C = y.shape
    g64, y64 = g.double(), y.double()
    mean, rstd = norm_mean_rstd(st, mode, N, HW, C, eps)
    gam = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    bet = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    xh = (y64 - mean) * rstd
    z = gam * xh + bet
    zero = torch.zeros_like(g64)   # a masked element is +0, whatever the sign of g
    gres = g64 if om is None else torch.where(om > 0, g64, zero)
    amb = torch.zeros_like(z, dtype=torch.bool)
    gm = gres
    if relu & 1:
        gm = torch.where(z > 0, gres, zero)
        amb = (z.abs() > 0) & (z.abs() <= U_SIGN * ((gam * xh).abs() + bet.abs()))
    red = torch.stack([gm.sum(1), (gm * xh).sum(1)], -1)
    red_bound = torch.stack([gm.abs().sum(1), (gm * xh).abs().sum(1)], -1)
    if mode == 0:
        dy, bound = gm, gm.abs()
    else:
        S, cnt = red, float(HW)
        if mode == 2:
            S, cnt = red.sum(0, keepdim=True).expand(N, C, 2), float(N) * float(HW)
        m1, m2 = (S[..., 0] / cnt)[:, None, :], (S[..., 1] / cnt)[:, None, :]
        a = rstd * gam
        dy = a * (gm - m1 - xh * m2)
        bound = a.abs() * (gm.abs() + m1.abs() + (xh * m2).abs())
    sets = amb.any(1)
    if mode == 2:
        sets = sets.any(0, keepdim=True).expand(N, C)
    return NS(dy=dy, bound=bound, red=red, red_bound=red_bound, gres=gres, amb=amb, sets=sets)


def norm_coeff_ref(st, mode, gam, bet, N, HW, C, eps=EPS):
    """fp64 (a, b), each [N, 1, C], of elementwise.hip:norm_coeff: x -> a x + b."""
    mean, rstd = norm_mean_rstd(st, mode, N, HW, C, eps)
    a, b = rstd, -mean * rstd
    if gam is not None:
        a, b = a * gam.double(), b * gam.double()
    if bet is not None:
        b = b + bet.double()
    return a, b


def norm_act_ref(x, sx, mode_x, gx, bx, r, sr, mode_r, gr, br, relu, eps=EPS):
    """act2(act1(a_x x + b_x) + (a_r r + b_r)): relu bit 0 before the residual, bit 1 after.
    Returns (value, bound = |a_x x| + |b_x| + |a_r r| + |b_r|, ambiguous-ReLU mask)."""
    N, HW, C = x.shape
    ax, bx_ = norm_coeff_ref(sx, mode_x, gx, bx, N, HW, C, eps)
    x64 = x.double()
    z = ax * x64 + bx_
    bound = (ax * x64).abs() + bx_.abs()
    amb = torch.zeros_like(z, dtype=torch.bool)
    if relu & 1:
        amb = (z.abs() > 0) & (z.abs() <= U_SIGN * bound)
        z = z.clamp_min(0.0)
    if r is not None:
        ar, br_ = norm_coeff_ref(sr, mode_r, gr, br, N, HW, C, eps)
        r64 = r.double()
        z = z + (ar * r64 + br_)
        bound = bound + (ar * r64).abs() + br_.abs()
    if relu & 2:
        amb = amb | ((z.abs() > 0) & (z.abs() <= U_SIGN * bound))
        z = z.clamp_min(0.0)
    return z, bound, amb


def stats_ref(x):
    """fp64 (sum x, sum x^2) per (n, c): [N, C, 2], and the sums of the terms' magnitudes."""
    x64 = x.double()
    return (torch.stack([x64.sum(1), (x64 * x64).sum(1)], -1),
            torch.stack([x64.abs().sum(1), (x64 * x64).sum(1)], -1))


def bn_table_ref(src, count, mom, mode, a0=None, b0=None):
    """One row of bn_table.  src: fp32 [N, C, 2].  mode 0: the running statistics
    (mom a + (1 - mom) mean, mom b + (1 - mom) biased variance) and their magnitude sums;
    mode 1: (sum_n src[..., 1], sum_n src[..., 0]) and the sums of the terms' magnitudes.
    ``mom`` is taken at its fp32 value, as the table carries it."""
    s = src.double()
    if mode == 1:
        return (s[..., 1].sum(0), s[..., 0].sum(0)), (s[..., 1].abs().sum(0), s[..., 0].abs().sum(0))
    m32 = torch.tensor(mom, dtype=torch.float32)
    mo, om = float(m32), float(torch.tensor(1.0) - m32)
    S = s.sum(0)
    mean = S[:, 0] / float(count)
    var = (S[:, 1] / float(count) - mean * mean).clamp_min(0.0)
    a, b = a0.double(), b0.double()
    return ((mo * a + om * mean, mo * b + om * var),
            ((mo * a).abs() + (om * mean).abs(), (mo * b).abs() + (om * var).abs()))


def sum_iters_ref(a, b):
    """out[m] = cat(sum_t a[t][m], sum_t b[t][m]): fp32 adds in t order, one bf16 rounding."""
    outs = []
    for x in (a, b):
        acc = torch.zeros(x.shape[1:], dtype=torch.float32)
        for t in range(x.shape[0]):
            acc += x[t].float()
        outs.append(acc)
    return torch.cat(outs, -1).to(torch.bfloat16)


# ----------------------------------------------------------------------------- sequence loss
def seq_loss_ref(pred, gt, valid, max_flow, scale=None):
    """pred [N, P, 2], gt [P, 2], valid [P] or None (fp32 values).  fp64 per-iteration L1 sums over
    the valid pixels (valid * |d| over every pixel, so a NaN poisons its iteration), EPE sum, the
    <1 / <3 / <5 px counts and the valid count of the last prediction, the gradient
    scale_i valid sign(pred_i - gt) (fp32, sign(NaN) = 0), and the margins of the exact counts."""
    p, g = pred.double(), gt.double()
    mag = torch.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
    ok = mag < max_flow
    if valid is not None:
        ok = ok & (valid >= 0.5)
    d = p - g
    l1 = (ok.double()[None, :, None] * d.abs()).sum((1, 2))
    e = torch.sqrt(d[-1, :, 0] ** 2 + d[-1, :, 1] ** 2)[ok]
    out = NS(l1=l1, epe=e.sum(), c1=int((e < 1).sum()), c3=int((e < 3).sum()), c5=int((e < 5).sum()),
             cnt=int(ok.sum()), ok=ok)
    ef = e[torch.isfinite(e)]
    out.epe_margin = min(float((ef - k).abs().min()) for k in (1.0, 3.0, 5.0)) if ef.numel() else float("inf")
    out.mag_margin = float((mag - max_flow).abs().min())
    if scale is not None:
        sgn = (d > 0).float() - (d < 0).float()
        out.grad = (scale.float()[:, None, None] * ok.float()[None, :, None]) * sgn
    return out


# ----------------------------------------------------------------------------- upsampling adjoints
def flow_gather_ref(taps, N, h, w):
    """dflow(p)[c] = sum over the in-map q = p - d_k of taps[q][2k + c], d_k = (k / 3 - 1, k % 3 - 1).
    taps: [N h w, tcs >= 18]; channels 18.. are not read.  Returns (value, sum |taps read|), [N h w, 2]."""
    t = taps.reshape(N, h, w, -1)[..., :18].double().reshape(N, h, w, 9, 2)
    val = torch.zeros(N, h, w, 2, dtype=torch.float64)
    bound = torch.zeros_like(val)
    for kh in range(3):
        for kw in range(3):
            dy, dx = kh - 1, kw - 1
            y0, y1 = max(0, dy), min(h, h + dy)
            x0, x1 = max(0, dx), min(w, w + dx)
            if y0 >= y1 or x0 >= x1:
                continue
            src = t[:, y0 - dy:y1 - dy, x0 - dx:x1 - dx, kh * 3 + kw]
            val[:, y0:y1, x0:x1] += src
            bound[:, y0:y1, x0:x1] += src.abs()
    return val.reshape(-1, 2), bound.reshape(-1, 2)


def bilinear8_bwd_ref(g, B, h, w):
    """Adjoint of the x8 align-corners bilinear of models/reference.py:upsample_flow(flow, None), by
    fp64 autograd (the op accepts h = 1 and w = 1).  g: [B, 8h, 8w, 2].  Returns (value,
    bound = 8 sum w_y w_x |g|), [B h w, 2]; the weights are non-negative, so the bound is the same
    adjoint applied to |g|."""
    from jax_raft_amd.models import reference as R

    flow = torch.zeros(B, h, w, 2, dtype=torch.float64, requires_grad=True)
    up = R.upsample_flow(flow, None)
    g64 = g.double().reshape(B, 8 * h, 8 * w, 2)
    val, = torch.autograd.grad(up, flow, g64, retain_graph=True)
    bound, = torch.autograd.grad(up, flow, g64.abs())
    return val.reshape(-1, 2), bound.reshape(-1, 2)


# ============================================================================= cases and checks
# (N, HW, C, mode): see the table in tests/test_train_kernels_gpu.py
NORM_BWD_CASES = [(3, 1073, 96, 1), (2, 5, 24, 1), (1, 4801, 128, 1), (6, 37, 64, 2), (4, 300, 32, 2),
                  (512, 2100, 8, 1), (2, 333, 64, 0)]
# the three forms the encoder records (train/fused_encoder.py:_record_bwd)
NORM_BWD_VARIANTS = ["relu", "res", "ds"]
NORM_BWD_SET_CAP = 0.02
ZERO_CHANNEL = 3


@functools.lru_cache(maxsize=2)
def norm_bwd_inputs(case):
    N, HW, C, mode = case
    gen = _gen(100 + NORM_BWD_CASES.index(case))
    y = bf(2 * torch.randn(N, HW, C, generator=gen) + 0.5)
    y[:, :, ZERO_CHANNEL] = 0.0   # variance 0: the fmaxf / eps path
    g = bf(torch.randn(N, HW, C, generator=gen))
    om = bf(torch.randn(N, HW, C, generator=gen))
    st = stats_ref(y)[0].float() if mode else None
    gamma = beta = None
    if mode == 2:
        gamma = torch.rand(C, generator=gen) + 0.5
        beta = torch.randn(C, generator=gen) * 0.3
    return NS(N=N, HW=HW, C=C, mode=mode, g=g, om=om, y=y, st=st, gamma=gamma, beta=beta)


def check_norm_bwd(impl, case, variant):
    """impl.norm_bwd(g, om, y, st, mode, gamma, beta, relu, gres_dtype) -> (dy fp32 [N, HW, C] holding
    the bf16 result, red fp32 [N, C, 2] or None, gres (of gres_dtype) or None)."""
    c = norm_bwd_inputs(case)
    relu = 0 if variant == "ds" else 1
    om = None if variant == "relu" else c.om
    gres_dtype = None
    if variant == "res":   # fp32 on one shape, bf16 on the next
        gres_dtype = torch.float32 if NORM_BWD_CASES.index(case) % 2 == 0 else torch.bfloat16
    ref = norm_bwd_ref(c.g, om, c.y, c.st, c.mode, c.gamma, c.beta, relu)
    # asserted from the reference alone, before any result is looked at
    share = float(ref.sets.double().mean())
    assert share <= NORM_BWD_SET_CAP, f"{share:.4f} of the normalisation sets hold an ambiguous ReLU"
    args = (c.g, om, c.y, c.st, c.mode, c.gamma, c.beta, relu, gres_dtype)
    dy, red, gres = impl.norm_bwd(*args)
    dy2, red2, gres2 = impl.norm_bwd(*args)
    name = f"norm_bwd{case}/{variant}"
    assert dy.shape == ref.dy.shape
    if c.mode == 0:
        assert red is None
        assert bits_equal(dy.to(torch.bfloat16), ref.dy.to(torch.bfloat16)), "mode 0: dy must be g bitwise"
        report(name + " dy (bitwise)", 0.0, 0.0)
    else:
        keep = ~ref.sets
        r = ratio(dy, ref.dy, U_BF16 * ref.dy.abs() + U_ACC * ref.bound, keep[:, None, :])
        report(name + " dy", r, share)
        assert r <= 1.0, f"{name}: dy error / tolerance = {r}"
        r = ratio(red, ref.red, U_ACC * ref.red_bound, keep[:, :, None])
        report(name + " red", r, share)
        assert r <= 1.0, f"{name}: red error / tolerance = {r}"
        assert bits_equal(red, red2), "red differs between two identical calls"
    if gres_dtype is not None:
        assert gres.dtype == gres_dtype
        assert bits_equal(gres, ref.gres.to(gres_dtype)), "gres must be g [om > 0] bitwise"
        assert bits_equal(gres, gres2)
    else:
        assert gres is None
    assert bits_equal(dy, dy2), "dy differs between two identical calls"


# ------------------------------------------------------------------------ stats / norm_act
# (1, 4801, 128): 301 partial blocks and (2, 28160, 32): 440 -- the final kernel's second round
STATS_CASES = [(1, 4801, 128), (2, 28160, 32), (3, 1073, 96)]
NORM_ACT_CASES = [(3, 1073, 96), (2, 5, 24)]
NORM_ACT_FORMS = ["none", "raw", "in", "bn"]
NORM_ACT_AMB_CAP = 0.001


@functools.lru_cache(maxsize=2)
def stats_inputs(case):
    N, HW, C = case
    gen = _gen(200 + N + HW + C)
    x = bf(2 * torch.randn(N, HW, C, generator=gen) + 0.5)
    r = bf(torch.randn(N, HW, C, generator=gen) - 0.25)
    aff = [torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3,
           torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3]
    return NS(x=x, r=r, aff=aff)


def check_stats(impl, case):
    """impl.stats(x [N, HW, C]) -> fp32 [N, C, 2]."""
    x = stats_inputs(case).x
    ref, bound = stats_ref(x)
    st, st2 = impl.stats(x), impl.stats(x)
    r = ratio(st, ref, U_ACC * bound)
    report(f"stats{case}", r)
    assert r <= 1.0, f"stats{case}: error / tolerance = {r}"
    assert bits_equal(st, st2), "stats differ between two identical calls"


def check_norm_act(impl, case, form):
    """impl.norm_act(x, sx, mode_x, gx, bx, r, sr, mode_r, gr, br, relu) -> fp32 [N, HW, C] holding the
    bf16 result.  The reference is fed the implementation's own statistics."""
    c = stats_inputs(case)
    x, r, sx, sr, mode_x, mode_r = c.x, None, impl.stats(c.x), None, 1, 0
    gx = bx = gr = br = None
    if form == "raw":
        r = c.r
    elif form == "in":     # residual normalised with its own statistics, and an affine
        r, sr, mode_r = c.r, impl.stats(c.r), 1
        gr, br = c.aff[2], c.aff[3]
    elif form == "bn":
        r, sr, mode_x, mode_r = c.r, impl.stats(c.r), 2, 2
        gx, bx, gr, br = c.aff
    for relu in range(4):
        ref, bound, amb = norm_act_ref(x, sx, mode_x, gx, bx, r, sr, mode_r, gr, br, relu)
        share = float(amb.double().mean())
        assert share <= NORM_ACT_AMB_CAP
        y = impl.norm_act(x, sx, mode_x, gx, bx, r, sr, mode_r, gr, br, relu)
        rr = ratio(y, ref, U_BF16 * ref.abs() + U_ACC * bound, ~amb)
        name = f"norm_act{case}/{form}/relu{relu}"
        report(name, rr, share)
        assert rr <= 1.0, f"{name}: error / tolerance = {rr}"


# ------------------------------------------------------------------------ bn_table
BN_SENTINEL = -12345.0
BN_PAD = 8
BN_ROWS = [(64, 1, 0), (96, 6, 1), (300, 2, 0), (32, 12, 1)]   # (C, N, mode); one launch, max_c = 300
BN_HW = 50
BN_MOM = 0.9


def momentum_bits(mom: float) -> int:
    return struct.unpack("<i", struct.pack("<f", float(mom)))[0]


@functools.lru_cache(maxsize=1)
def bn_table_inputs():
    gen = _gen(300)
    rows = []
    for C, N, mode in BN_ROWS:
        if mode == 0:   # forward: per-(n, c) (sum, sumsq) of a conv output
            src = stats_ref(bf(2 * torch.randn(N, BN_HW, C, generator=gen) + 0.5))[0].float()
        else:           # backward: the norm backward's (sum g, sum g xhat)
            src = torch.randn(N, C, 2, generator=gen) * 10
        d0 = torch.full((C + BN_PAD,), BN_SENTINEL)
        d1 = torch.full((C + BN_PAD,), BN_SENTINEL)
        d0[:C] = torch.randn(C, generator=gen)          # running mean / stale gradient
        d1[:C] = torch.rand(C, generator=gen) + 0.5     # running variance
        rows.append(NS(src=src, d0=d0, d1=d1, N=N, C=C, count=N * BN_HW if mode == 0 else 1,
                       mom=BN_MOM if mode == 0 else 0.0, mode=mode))
    return rows


def check_bn_table(impl):
    """impl.bn_table(rows) -> [(dst0, dst1)] after one launch over all rows; every destination is
    C + BN_PAD floats long and must keep its sentinel tail."""
    rows = bn_table_inputs()
    outs = impl.bn_table(rows)
    assert len(outs) == len(rows)
    for k, (row, (o0, o1)) in enumerate(zip(rows, outs)):
        C = row.C
        (e0, e1), (b0, b1) = bn_table_ref(row.src, row.count, row.mom, row.mode, row.d0[:C], row.d1[:C])
        u = U_BN if row.mode == 0 else U_ACC
        for o, e, b, nm in ((o0, e0, b0, "dst0"), (o1, e1, b1, "dst1")):
            assert o.shape == (C + BN_PAD,)
            assert bool((o[C:] == BN_SENTINEL).all()), f"bn_table row {k}: {nm} written past C"
            r = ratio(o[:C], e, u * b)
            report(f"bn_table row {k} (C={C}, N={row.N}, mode {row.mode}) {nm}", r)
            assert r <= 1.0, f"bn_table row {k} {nm}: error / tolerance = {r}"


# ------------------------------------------------------------------------ sum_iters
SUM_ITERS_CASES = [(1, 5, 8, 8), (12, 777, 256, 128), (3, 33, 128, 256)]   # (T, M, Ca, Cb)


def check_sum_iters(impl, case):
    """impl.sum_iters(a bf16 [T, M, Ca], b bf16 [T, M, Cb]) -> bf16 [M, Ca + Cb]."""
    T, M, Ca, Cb = case
    gen = _gen(400 + T)
    a = torch.randn(T, M, Ca, generator=gen).to(torch.bfloat16)
    b = (torch.randn(T, M, Cb, generator=gen) * 3).to(torch.bfloat16)
    out = impl.sum_iters(a, b)
    assert bits_equal(out, sum_iters_ref(a, b)), "sum_iters must equal the fp32 t-order sum bitwise"
    report(f"sum_iters{case} (bitwise)", 0.0)


# ------------------------------------------------------------------------ sequence loss
LOSS_GRID = 1024 * 256   # pixels per grid-stride round of seq_loss_kernel
# (P, N, NaN?): two full rounds and a ragged third; a second round of 7 pixels; one partial round
SEQ_LOSS_CASES = [(2 * LOSS_GRID + 300, 12, True), (LOSS_GRID + 7, 32, False), (LOSS_GRID + 7, 1, False),
                  (1000, 5, False)]
MAX_FLOW = 400.0
EPE_MARGIN = 1e-5
MAG_MARGIN = 1e-3


@functools.lru_cache(maxsize=1)
def seq_loss_inputs(case, with_valid):
    P, N, nan = case
    gen = _gen(500 + N + (1 if with_valid else 0))
    gt = torch.randn(P, 2, generator=gen) * 20
    gt[::97] = torch.tensor([500.0, 3.0])          # beyond max_flow: invalid whatever the plane says
    pred = gt[None] + torch.randn(N, P, 2, generator=gen) * 2
    pred[:, 5::53, 0] = gt[5::53, 0]                # exact ties: sign 0
    valid = (torch.rand(P, generator=gen) > 0.3).float() if with_valid else None
    # keep the final EPE away from the bucket edges (the counts are compared exactly)
    d = pred[-1].double() - gt.double()
    e = torch.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    near = ((e - 1).abs() < 1e-3) | ((e - 3).abs() < 1e-3) | ((e - 5).abs() < 1e-3)
    pred[-1][near] = gt[near] + torch.tensor([0.5, 0.25])
    nan_at = None
    if nan:   # a valid pixel of the third grid-stride round, not in the last prediction
        nan_at = (1, 2 * LOSS_GRID + 123)
        gt[nan_at[1]] = torch.tensor([1.5, -2.0])
        if valid is not None:
            valid[nan_at[1]] = 1.0
        pred[:, nan_at[1]] = gt[nan_at[1]] + 0.75
        pred[nan_at[0], nan_at[1], 0] = float("nan")
    scale = (torch.arange(N, dtype=torch.float32) * 0.13 + 0.37) / 1024.0
    return NS(P=P, N=N, pred=pred.contiguous(), gt=gt.contiguous(), valid=valid, scale=scale, nan_at=nan_at)


def seq_loss_blocks_expected(P: int) -> int:
    return min(1024, (P + 255) // 256)


def check_seq_loss(impl, case, with_valid):
    """impl.seq_loss(pred, gt, valid, max_flow) -> fp32 part [blocks, 37];
    impl.seq_loss_bwd(pred, gt, valid, max_flow, scale) -> fp32 grad [N, P, 2]."""
    c = seq_loss_inputs(case, with_valid)
    ref = seq_loss_ref(c.pred, c.gt, c.valid, MAX_FLOW, c.scale)
    # preconditions of the exact counts, from the reference alone
    assert ref.epe_margin > EPE_MARGIN and ref.mag_margin > MAG_MARGIN
    assert 0 < ref.cnt < c.P and ref.c1 < ref.c3 < ref.c5 < ref.cnt
    part = impl.seq_loss(c.pred, c.gt, c.valid, MAX_FLOW)
    assert part.shape[1] == 37
    s = part.double().sum(0)
    name = f"seq_loss(P={c.P}, N={c.N}, valid={with_valid})"
    worst = 0.0
    for i in range(c.N):
        if torch.isnan(ref.l1[i]):
            assert c.nan_at is not None and i == c.nan_at[0]
            assert torch.isnan(s[i]), f"{name}: the NaN did not reach iteration {i}'s sum"
        else:
            worst = max(worst, ratio(s[i], ref.l1[i], U_ACC * ref.l1[i].abs()))
    if c.nan_at is not None:
        assert torch.isnan(ref.l1[c.nan_at[0]]) and int(torch.isnan(ref.l1).sum()) == 1
    worst = max(worst, ratio(s[32], ref.epe, U_ACC * ref.epe.abs()))
    report(name + " sums", worst)
    assert worst <= 1.0, f"{name}: error / tolerance = {worst}"
    assert bool((s[c.N:32] == 0).all())
    assert [float(s[33]), float(s[34]), float(s[35]), float(s[36])] == [ref.c1, ref.c3, ref.c5, ref.cnt]
    grad = impl.seq_loss_bwd(c.pred, c.gt, c.valid, MAX_FLOW, c.scale)
    assert bits_equal(grad, ref.grad), f"{name}: gradient is not scale valid sign(pred - gt) bitwise"
    if c.nan_at is not None:
        i, p = c.nan_at
        assert float(grad[i, p, 0]) == 0.0 and float(grad[i, p, 1]) == float(c.scale[i])


# ------------------------------------------------------------------------ upsampling adjoints
FLOW_GATHER_CASES = [(1, 1, 1), (2, 1, 5), (1, 3, 3), (3, 6, 16)]   # (N, h, w)
FLOW_GATHER_STRIDES = [(18, 2), (18, 8), (24, 2), (24, 8)]          # (tcs, dcs)
BILINEAR_CASES = [(1, 1, 9), (1, 9, 1), (2, 2, 3), (1, 55, 128)]    # (B, h, w)
BILINEAR_DCS = 8


def check_flow_gather(impl, case, strides):
    """impl.flow_gather_bwd(taps fp32 [M, tcs], N, h, w, dcs) -> fp32 [M, dcs] holding the bf16 result
    (the implementation pre-fills the output with NaN, so unwritten channels show)."""
    N, h, w = case
    tcs, dcs = strides
    M = N * h * w
    gen = _gen(600 + M + tcs)
    taps = torch.randn(M, tcs, generator=gen) * 2
    taps[:, 18:] = float("nan")   # must not be read
    ref, bound = flow_gather_ref(taps, N, h, w)
    out = impl.flow_gather_bwd(taps, N, h, w, dcs)
    assert out.shape == (M, dcs)
    r = ratio(out[:, :2], ref, U_BF16 * ref.abs() + U_ACC * bound)
    report(f"flow_gather_bwd{case} tcs={tcs} dcs={dcs}", r)
    assert r <= 1.0, f"flow_gather_bwd{case}: error / tolerance = {r}"
    assert bool((out[:, 2:] == 0).all()), "channels 2.. must be written as zero"


def check_bilinear(impl, case):
    """impl.upsample_bilinear_bwd(g fp32 [B, 8h, 8w, 2], B, h, w, dcs) -> fp32 [B h w, dcs]."""
    B, h, w = case
    gen = _gen(700 + h + w)
    g = torch.randn(B, 8 * h, 8 * w, 2, generator=gen)
    ref, bound = bilinear8_bwd_ref(g, B, h, w)
    out = impl.upsample_bilinear_bwd(g, B, h, w, BILINEAR_DCS)
    assert out.shape == (B * h * w, BILINEAR_DCS)
    r = ratio(out[:, :2], ref, U_BF16 * ref.abs() + U_ACC * bound)
    report(f"upsample_bilinear_bwd{case}", r)
    assert r <= 1.0, f"upsample_bilinear_bwd{case}: error / tolerance = {r}"
    assert bool((out[:, 2:] == 0).all()), "channels 2.. must be written as zero"
