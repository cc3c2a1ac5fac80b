"""The oracle of tests/test_bwd_kernels_gpu.py, checked without a GPU.

1. Every fp64 reference of tests/_bwd_refs.py equals fp64 ``torch.autograd`` of the plain forward
   expression (``R.index_pyramid``, the 2x2 floor average-pooling chain, the correlation volume,
   ``R.conv2d_nhwc`` against the explicit im2col sum, an fp64 transcription of
   ``R.upsample_flow``) to 1e-12 relative.
2. The tolerances are attainable: an fp32 emulation of each kernel's arithmetic -- the same
   inputs, fp32 throughout, one bf16 rounding where the kernel has one -- passes every ``check_*``
   that the GPU tests run.
3. The checks are not vacuous: each mutant of that emulation (a swapped index, a dropped border,
   a dropped split, a missing factor ...) fails its ``check_*`` on at least one of the listed cases.
"""
import pytest
import torch
import torch.nn.functional as F

import _bwd_refs as Bw
from jax_raft_amd.models import reference as R

F32 = torch.float32
F64 = torch.float64
BF16 = torch.bfloat16


def _close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


# ============================================================================ 1. the references
def _grid_sample64(img, grid):
    """models/reference.py:grid_sample without its ``H > 1`` assertion (the pyramids of the odd maps end
    in one-row levels): bilinear sampling at pixel coordinates, taps off the image contribute 0."""
    n, H, W, C = img.shape
    x, y = grid[..., 0], grid[..., 1]
    x0, y0 = torch.floor(x), torch.floor(y)
    flat = img.reshape(n, H * W, C)
    out = torch.zeros(grid.shape[:-1] + (C,), dtype=img.dtype)
    bidx = torch.arange(n).view(n, 1, 1)
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0.long() + dx, y0.long() + dy
            wx = (x - x0) if dx else 1.0 - (x - x0)
            wy = (y - y0) if dy else 1.0 - (y - y0)
            valid = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            lin = yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
            out = out + (wx * wy * valid.to(img.dtype)).unsqueeze(-1) * flat[bidx.expand_as(lin), lin]
    return out


def _index_pyramid64(pyramid, coords, radius):
    """models/reference.py:index_pyramid on _grid_sample64."""
    B, h, w, _ = coords.shape
    side = 2 * radius + 1
    delta = R.neighborhood_offsets(radius).reshape(1, side, side, 2)
    c = coords.reshape(B * h * w, 1, 1, 2)
    out = []
    for vol in pyramid:
        out.append(_grid_sample64(vol.unsqueeze(-1), c + delta).reshape(B, h, w, side * side))
        c = c / 2
    return torch.cat(out, dim=-1)


@pytest.mark.parametrize("case", Bw.LOOKUP_CASES, ids=str)
def test_lookup_bwd_ref_is_autograd(case):
    c = Bw.lookup_inputs(case)
    gen = torch.Generator().manual_seed(21)
    pyr = [torch.randn(c.M, c.h >> l, c.w >> l, generator=gen, dtype=F64).requires_grad_(True) for l in range(c.L)]
    coords = c.coords.double().reshape(c.B, c.h, c.w, 2)
    out = _index_pyramid64(pyr, coords, c.r)
    if all((c.h >> l) > 1 for l in range(c.L)):   # the library's own lookup accepts float64 and agrees
        lib = R.index_pyramid([p.detach() for p in pyr], coords, c.r)
        assert lib.dtype == F64 and _close(out.detach(), lib)
    n = c.L * c.S * c.S
    g = c.g.double()[:, :n].reshape(c.B, c.h, c.w, n)
    grads = torch.autograd.grad((out * g).sum(), pyr)
    for (val, bound, win), gr in zip(Bw.lookup_ref_of(case), grads):
        assert _close(val, gr)
        assert bool((bound >= val.abs() * (1 - 1e-12)).all())
        assert bool((val[~win] == 0).all()) and bool((bound[~win] == 0).all())


def test_lookup_cases_reach_the_planted_windows():
    """(-30.5, 3.25) is off the map at level 0 and on it at level 3; the integer coordinate has zero-weight
    cells inside its window; (w + 40, h + 7.5) touches nothing."""
    case = Bw.LOOKUP_CASES[0]
    c = Bw.lookup_inputs(case)
    ref = Bw.lookup_ref_of(case)
    assert not bool(ref[0][2][3].any()) and bool(ref[3][2][3].any())
    assert bool((ref[0][2][0] & (ref[0][1][0] == 0)).any())
    assert not any(bool(win[4].any()) for _, _, win in ref)
    assert c.M % 4 == 2


@pytest.mark.parametrize("case", Bw.PYR_CASES, ids=str)
def test_pyr_bwd_dc_ref_is_autograd(case):
    M, h, w, L = case
    gs = Bw.pyr_inputs(case)
    scale = Bw.PYR_SCALES[1]
    s32 = float(torch.tensor(scale, dtype=F32))
    vol = torch.randn(M, h, w, generator=torch.Generator().manual_seed(22), dtype=F64).requires_grad_(True)
    lv, loss = s32 * vol, 0.0
    for l in range(L):   # models/reference.py:build_pyramid_queries
        loss = loss + (lv * gs[l].double()).sum()
        hh, ww = lv.shape[-2] // 2, lv.shape[-1] // 2
        lv = lv[:, :2 * hh, :2 * ww].reshape(M, hh, 2, ww, 2).mean(dim=(2, 4))
    ref, bound = Bw.pyr_bwd_dc_ref(gs, h, w, scale)
    assert _close(ref, torch.autograd.grad(loss, vol)[0])
    assert bool((bound >= ref.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("case", Bw.BGEMM_CASES[:3], ids=str)
def test_bgemm_ref_is_the_volume_adjoint(case):
    """corr = alpha f1 f2^T: dfmap1 = alpha dC f2 (A row-major), dfmap2 = alpha dC^T f1 (A k-major)."""
    batch, M, N, K = case
    gen = torch.Generator().manual_seed(23)
    f1 = torch.randn(batch, M, N, generator=gen, dtype=F64).requires_grad_(True)
    f2 = torch.randn(batch, K, N, generator=gen, dtype=F64).requires_grad_(True)
    dC = torch.randn(batch, M, K, generator=gen, dtype=F64)
    al = float(torch.tensor(Bw.BGEMM_ALPHA, dtype=F32))
    d1, d2 = torch.autograd.grad((al * torch.matmul(f1, f2.transpose(1, 2)) * dC).sum(), (f1, f2))
    assert _close(Bw.bgemm_ref(dC, f2.detach(), Bw.BGEMM_ALPHA)[0], d1)
    # the k-major operand is dC itself, read as op(A) = dC^T
    assert _close(Bw.bgemm_ref(dC.transpose(1, 2), f1.detach(), Bw.BGEMM_ALPHA)[0], d2)
    sel = Bw.bgemm_inputs(case, True)
    assert bool((sel.a.sum(2) == 1).all()) and bool(((sel.a == 0) | (sel.a == 1)).all())


@pytest.mark.parametrize("case", [Bw.WGRAD_IM2COL_CASES[2], Bw.WGRAD_IM2COL_CASES[0], Bw.WGRAD_HALO_CASES[3]], ids=str)
def test_wgrad_ref_is_the_im2col_sum(case):
    """dW[kh][kw][ci][co] = sum_m x[n][oh s - p + kh][ow s - p + kw][ci] dy[m][co] (0 off the map)."""
    N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, (PH, PW) = case
    OH, OW = Bw.wgrad_out_hw(case)
    c = Bw.wgrad_inputs(case)
    dw, db, bw, bb = Bw.wgrad_ref_of(case)
    xs = torch.zeros(N, H + 2 * PH, W + 2 * PW, cin, dtype=F64)
    xs[:, PH:PH + H, PW:PW + W] = c.x[..., xoff:xoff + cin].double()
    ys = c.dy[..., yoff:yoff + cout].double()
    want = torch.zeros(KH, KW, cin, cout, dtype=F64)
    for kh in range(KH):
        for kw in range(KW):
            win = xs[:, kh:kh + (OH - 1) * s + 1:s, kw:kw + (OW - 1) * s + 1:s]
            want[kh, kw] = torch.einsum("nhwc,nhwo->co", win, ys)
    assert _close(dw, want) and _close(db, ys.sum((0, 1, 2)))
    assert bool((bw >= dw.abs() * (1 - 1e-12)).all()) and _close(bb, ys.abs().sum((0, 1, 2)))


def test_wgrad_plans():
    """The cases reach the code they name (the plan is transcribed from wgrad.hip; the GPU test checks the
    halo plan against the op's workspace check)."""
    p = Bw.wgrad_plan(Bw.WGRAD_HALO_CASES[0])
    assert (p.ntiles, p.S) == (1, 1)
    p = Bw.wgrad_plan(Bw.WGRAD_HALO_CASES[1])
    assert (p.ntiles, p.tiles_x, p.tiles_y, p.S, p.tps) == (27, 3, 3, 7, 4) and p.ntiles - 6 * p.tps == 3
    p = Bw.wgrad_plan(Bw.WGRAD_IM2COL_CASES[0])
    assert (p.M, p.S, p.px_split, (p.M - p.px_split) % Bw.WPX) == (468, 2, 256, 20)
    assert [Bw.wgrad_plan(c).bco for c in Bw.WGRAD_IM2COL_CASES] == [128, 128, 64, 256, 256, 64]
    assert [Bw.wgrad_plan(c).bkk for c in Bw.WGRAD_IM2COL_CASES] == [128, 128, 128, 256, 256, 64]
    assert all(Bw.wgrad_plan(c).halo for c in Bw.WGRAD_HALO_CASES)
    assert not any(Bw.wgrad_plan(c).halo for c in Bw.WGRAD_IM2COL_CASES)


def _upsample_flow64(flow, up_mask):
    """models/reference.py:upsample_flow (convex mode) without its casts to fp32."""
    B, h, w, C = flow.shape
    m = torch.softmax(up_mask.reshape(B, h, w, 9, 8, 8), dim=3)
    fp = F.pad((8 * flow).permute(0, 3, 1, 2), (1, 1, 1, 1))
    neigh = torch.stack([fp[:, :, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], dim=2)
    neigh = neigh.permute(0, 3, 4, 1, 2)   # (B, h, w, C, 9)
    up = (neigh.unsqueeze(-1) * m.reshape(B, h, w, 1, 9, 64)).sum(dim=4)
    return up.reshape(B, h, w, C, 8, 8).permute(0, 1, 4, 2, 5, 3).reshape(B, 8 * h, 8 * w, C)


@pytest.mark.parametrize("variant", Bw.CONVEX_VARIANTS, ids=str)
def test_upsample_convex_bwd_ref_is_autograd(variant):
    case, alpha, logit_scale = variant
    B, h, w = case
    c = Bw.convex_inputs(case, logit_scale)
    al = float(torch.tensor(alpha, dtype=F32))
    flow = c.flow.double().reshape(B, h, w, 2).requires_grad_(True)
    pre = (c.mask.double().reshape(B, h, w, 576) / al).requires_grad_(True)   # conv output before the multiplier
    up = _upsample_flow64(flow, pre * al)
    assert _close(up.detach(), R.upsample_flow(c.flow.reshape(B, h, w, 2), c.mask.reshape(B, h, w, 576)), 1e-6)
    dm, df = torch.autograd.grad((up * c.g.double()).sum(), (pre, flow))
    ref = Bw.upsample_convex_bwd_ref(c.mask, c.flow, c.g, B, h, w, alpha)
    assert _close(ref.dmask, dm.reshape(-1, 576))
    assert _close(Bw.flow_gather_ref(ref.taps, B, h, w)[0], df.reshape(-1, 2))
    assert bool((ref.dmask_bound >= ref.dmask.abs() * (1 - 1e-12)).all())
    assert bool((ref.taps_bound >= ref.taps.abs() * (1 - 1e-12)).all())
    # the __expf term is a correction: below the 2^-16 term for the 2 randn logits
    if logit_scale == 2.0:
        assert bool((ref.dmask_extra <= Bw.U_ACC * ref.dmask_bound + 1e-30).all())


# ============================================================================ 2. fp32 emulation
class Fp32:
    """The kernels' arithmetic on the CPU: fp32 for everything, one bf16 rounding where the kernel has one.
    ``mut`` names one deliberate error (part 3)."""

    def __init__(self, mut=None):
        self.mut = mut

    # ---------------------------------------------------------------- corr.hip: corr_lookup_bwd_kernel
    def lookup_bwd(self, coords, g, gdt, dlevels, L, B, h, w, r):
        mut = self.mut
        M, S = coords.shape[0], 2 * r + 1
        gflat = g.to(gdt).float().reshape(-1)
        stride = L * S * S if mut == "lookup_stride" else g.shape[1]
        q = torch.arange(M)
        out = []
        for l in range(L):
            hl, wl = h >> l, w >> l
            sc = torch.tensor(1.0 / float(1 << (l + 1 if mut == "lookup_scale" else l)), dtype=F32)
            c = coords * sc
            fl = torch.floor(c)
            fx, fy = c[:, 0] - fl[:, 0], c[:, 1] - fl[:, 1]
            x0, y0 = fl[:, 0].long() - r, fl[:, 1].long() - r
            acc = torch.zeros(M, hl, wl)
            hit = torch.zeros(M, hl, wl, dtype=torch.bool)
            for i in range(S):
                for j in range(S):
                    ch = l * S * S + (j * S + i if mut == "lookup_swap_ij" else i * S + j)
                    gv = gflat[q * stride + ch]
                    for dx, wx in ((0, 1.0 - fx), (1, fx)):
                        if mut == "lookup_drop_col" and dx == 1 and i == S - 1:
                            continue   # lane i = S never writes its column
                        for dy, wy in ((0, 1.0 - fy), (1, fy)):
                            col, row = x0 + i + dx, y0 + j + dy
                            ok = (col >= 0) & (col < wl) & (row >= 0) & (row < hl)
                            idx = (q[ok], row[ok], col[ok])
                            acc.index_put_(idx, (wx * wy * gv)[ok], accumulate=True)
                            hit[idx] = True
            assert acc.dtype == F32
            out.append(torch.where(hit, acc, dlevels[l]) if mut == "lookup_overwrite" else dlevels[l] + acc)
        return out

    # ---------------------------------------------------------------- train.hip: pyr_bwd_dc*
    def pyr_bwd_dc(self, gs, L, M, h, w, scale):
        mut = self.mut
        v = gs[0].clone()
        ys, xs = torch.arange(h), torch.arange(w)
        for l in range(1, L):
            if mut == "pyr_no_level3" and l == 3:
                continue
            hl, wl = h >> l, w >> l
            yy, xx = ys >> l, xs >> l
            if mut == "pyr_swap_level2" and l == 2 and w % 8 == 0:
                xx = xx ^ 1   # the vector kernel's float2: t.y for the first four outputs
            oky, okx = yy < hl, xx < wl
            if mut == "pyr_clamp_rows":
                oky = torch.ones_like(oky)
            f = torch.tensor(1.0 / float(1 << (l if mut == "pyr_half" else 2 * l)), dtype=F32)
            t = gs[l][:, yy.clamp(max=hl - 1)][:, :, xx.clamp(max=wl - 1)] * f
            v = v + t * (oky[:, None] & okx[None, :])
        assert v.dtype == F32
        return Bw.bf(v * torch.tensor(scale, dtype=F32))

    # ---------------------------------------------------------------- bgemm.hip
    def bgemm(self, a, b, M, N, K, a_kmajor, alpha, out_dtype):
        mut = self.mut
        batch = a.shape[0]
        op, bb = a.float(), b.float()
        if a_kmajor:
            op = op.reshape(batch, M, K) if mut == "bgemm_ignore_kmajor" else op.transpose(1, 2)
        if mut == "bgemm_swap_k":   # k = 5 and 6 of every 32-deep step exchanged in the A fragment
            idx = torch.arange(K)
            idx[5::32], idx[6::32] = torch.arange(K)[6::32], torch.arange(K)[5::32]
            op = op[:, :, idx]
        if mut == "bgemm_drop_stage":
            op, bb = op[:, :, :K - 64], bb[:, :K - 64]
        c = torch.matmul(op, bb) * torch.tensor(alpha, dtype=F32)
        assert c.dtype == F32
        return c.to(out_dtype)

    # ---------------------------------------------------------------- wgrad.hip
    def _pixels(self, case, plan):
        """The pixels m = (n, oh, ow) that reach the sum."""
        N, H, W = case[:3]
        OH, OW = Bw.wgrad_out_hw(case)
        m = torch.arange(plan.M)
        keep = torch.ones(plan.M, dtype=torch.bool)
        if plan.halo:
            n, y, x = m // (OH * OW), (m // OW) % OH, m % OW
            tile = n * plan.tiles_x * plan.tiles_y + (y // Bw.HTR) * plan.tiles_x + x // Bw.HTC
            if self.mut == "wgrad_drop_split" and plan.S > 1:
                keep = tile < (plan.S - 1) * plan.tps
            if self.mut == "wgrad_drop_ragged":   # the pixels of the partial tiles
                keep = (y < H // Bw.HTR * Bw.HTR) & (x < W // Bw.HTC * Bw.HTC)
        else:
            last = (plan.S - 1) * plan.px_split
            if self.mut == "wgrad_drop_split" and plan.S > 1:
                keep = m < last
            if self.mut == "wgrad_drop_ragged":   # the last split's final, partial 64-pixel stage
                keep = m < last + (plan.M - last) // Bw.WPX * Bw.WPX
        return keep

    def wgrad(self, x, dy, case):
        mut = self.mut
        N, H, W, xcs, xoff, cin, cin8, cout, ycs, yoff, KH, KW, s, (PH, PW) = case
        OH, OW = Bw.wgrad_out_hw(case)
        plan = Bw.wgrad_plan(case)
        xs = x[..., xoff:xoff + cin8].float().permute(0, 3, 1, 2)
        pad = (PH, PW)
        if mut == "wgrad_clamp_pad" and (PH or PW):
            xs, pad = F.pad(xs, (PW, PW, PH, PH), mode="replicate"), (0, 0)
        cols = F.unfold(xs, (KH, KW), padding=pad, stride=s)   # [N, cin8 KH KW, OH OW], rows (c, kh, kw)
        cols = cols.reshape(N, cin8, KH * KW, OH * OW).permute(0, 3, 2, 1).reshape(plan.M, KH * KW, cin8)
        ys = dy[..., yoff:yoff + cout].float().reshape(plan.M, cout)
        keep = self._pixels(case, plan)
        ys = ys * keep[:, None]
        dw8 = torch.einsum("mtc,mo->tco", cols, ys)            # the partials' k = tap cin8 + ci
        db = ys.sum(0)
        assert dw8.dtype == F32
        if mut == "wgrad_no_ci_guard" and cin < cin8:
            # the stray rows ci >= cin land on the next taps' rows; the stores race, here the strays land last
            flat = torch.zeros((KH * KW * cin + cin8) * cout)
            for t in reversed(range(KH * KW)):
                for ci in range(cin8):
                    flat[(t * cin + ci) * cout:(t * cin + ci + 1) * cout] = dw8[t, ci]
            dw = flat[:KH * KW * cin * cout].reshape(KH, KW, cin, cout)
        else:
            dw = dw8[:, :cin].reshape(KH, KW, cin, cout)
        if mut == "wgrad_flip_taps":
            dw = dw.flip(0, 1)
        return dw.contiguous(), db

    # ---------------------------------------------------------------- train.hip: upsample_convex_bwd_kernel
    def upsample_convex_bwd(self, mask, flow, g, B, h, w, alpha, dcs, sentinel):
        mut = self.mut
        M = B * h * w
        logit = mask.reshape(M, 9, 64)
        e = torch.exp(logit - logit.max(1, keepdim=True).values)
        wk = e * (1.0 / e.sum(1, keepdim=True))
        u = Bw.convex_neighbours(flow, B, h, w, clamp=mut == "convex_clamp")
        gs = Bw.convex_subpixels(g, B, h, w)
        a = torch.einsum("mkc,msc->mks", u, gs)
        gup = torch.zeros(M, 1, 64) if mut == "convex_no_up" else (wk * a).sum(1, keepdim=True)
        al = torch.tensor(1.0 if mut == "convex_no_alpha" else alpha, dtype=F32)
        dm = al * wk * (a - gup)
        taps = (1.0 if mut == "convex_no_8" else 8.0) * torch.einsum("mks,msc->mkc", wk, gs).reshape(M, 18)
        assert dm.dtype == F32 and taps.dtype == F32
        out = torch.full((M, dcs), sentinel)
        out[:, :576] = Bw.bf(dm.reshape(M, 576))
        return out, taps


EMU = Fp32()
BGEMM_DTYPES = [F32, BF16]


@pytest.mark.parametrize("case", Bw.LOOKUP_CASES, ids=str)
def test_emulated_lookup_bwd(case):
    Bw.check_lookup_bwd(EMU, case)


@pytest.mark.parametrize("scale", Bw.PYR_SCALES, ids=["s16", "s128"])
@pytest.mark.parametrize("case", Bw.PYR_CASES, ids=str)
def test_emulated_pyr_bwd_dc(case, scale):
    Bw.check_pyr_bwd_dc(EMU, case, scale)


@pytest.mark.parametrize("out_dtype", BGEMM_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("a_kmajor", [0, 1])
@pytest.mark.parametrize("case", Bw.BGEMM_CASES, ids=str)
def test_emulated_bgemm(case, a_kmajor, out_dtype):
    Bw.check_bgemm(EMU, case, a_kmajor, out_dtype)


@pytest.mark.parametrize("out_dtype", BGEMM_DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("a_kmajor", [0, 1])
@pytest.mark.parametrize("case", Bw.BGEMM_SELECT_CASES, ids=str)
def test_emulated_bgemm_select(case, a_kmajor, out_dtype):
    Bw.check_bgemm_select(EMU, case, a_kmajor, out_dtype)


@pytest.mark.parametrize("case", Bw.WGRAD_CASES, ids=str)
def test_emulated_wgrad(case):
    Bw.check_wgrad(EMU, case)


@pytest.mark.parametrize("variant", Bw.CONVEX_VARIANTS, ids=str)
def test_emulated_upsample_convex_bwd(variant):
    Bw.check_upsample_convex_bwd(EMU, variant)


# ============================================================================ 3. mutants
def _bgemm_runs(check, cases):
    return [(check, (c, ak, dt)) for c in cases for ak in (1, 0) for dt in BGEMM_DTYPES]


def _runs(check, cases):
    return [(check, (c,)) for c in cases]


MUTANTS = {
    "lookup_swap_ij": _runs(Bw.check_lookup_bwd, Bw.LOOKUP_CASES),
    "lookup_drop_col": _runs(Bw.check_lookup_bwd, Bw.LOOKUP_CASES),
    "lookup_overwrite": _runs(Bw.check_lookup_bwd, Bw.LOOKUP_CASES),
    "lookup_stride": _runs(Bw.check_lookup_bwd, Bw.LOOKUP_CASES),
    "lookup_scale": _runs(Bw.check_lookup_bwd, Bw.LOOKUP_CASES),
    "pyr_no_level3": [(Bw.check_pyr_bwd_dc, (c, s)) for c in Bw.PYR_CASES for s in Bw.PYR_SCALES],
    "pyr_clamp_rows": [(Bw.check_pyr_bwd_dc, (c, s)) for c in Bw.PYR_CASES for s in Bw.PYR_SCALES],
    "pyr_half": [(Bw.check_pyr_bwd_dc, (c, s)) for c in Bw.PYR_CASES for s in Bw.PYR_SCALES],
    "pyr_swap_level2": [(Bw.check_pyr_bwd_dc, (c, s)) for c in Bw.PYR_CASES for s in Bw.PYR_SCALES],
    "bgemm_drop_stage": _bgemm_runs(Bw.check_bgemm, Bw.BGEMM_CASES),
    "bgemm_ignore_kmajor": _bgemm_runs(Bw.check_bgemm, Bw.BGEMM_CASES),
    "bgemm_swap_k": _bgemm_runs(Bw.check_bgemm_select, Bw.BGEMM_SELECT_CASES),   # must fail the selection case
    "wgrad_drop_ragged": _runs(Bw.check_wgrad, Bw.WGRAD_CASES),
    "wgrad_drop_split": _runs(Bw.check_wgrad, Bw.WGRAD_CASES),
    "wgrad_flip_taps": _runs(Bw.check_wgrad, Bw.WGRAD_CASES),
    "wgrad_no_ci_guard": _runs(Bw.check_wgrad, Bw.WGRAD_CASES),
    "wgrad_clamp_pad": _runs(Bw.check_wgrad, Bw.WGRAD_CASES),
    "convex_clamp": _runs(Bw.check_upsample_convex_bwd, Bw.CONVEX_VARIANTS),
    "convex_no_up": _runs(Bw.check_upsample_convex_bwd, Bw.CONVEX_VARIANTS),
    "convex_no_alpha": _runs(Bw.check_upsample_convex_bwd, Bw.CONVEX_VARIANTS),
    "convex_no_8": _runs(Bw.check_upsample_convex_bwd, Bw.CONVEX_VARIANTS),
}
# where a mutant changes the result at all: everywhere, unless named here
MUTANT_MUST_FAIL = {
    "lookup_stride": [c for c in Bw.LOOKUP_CASES if c[6] != c[3] * (2 * c[4] + 1) ** 2],
    "pyr_no_level3": [c for c in Bw.PYR_CASES if c[3] == 4],
    "pyr_clamp_rows": [Bw.PYR_CASES[0], Bw.PYR_CASES[1]],
    "pyr_half": [c for c in Bw.PYR_CASES if c[3] > 1],
    "pyr_swap_level2": [c for c in Bw.PYR_CASES if c[3] > 2 and c[2] % 8 == 0],
    "wgrad_drop_ragged": [Bw.WGRAD_HALO_CASES[1], Bw.WGRAD_IM2COL_CASES[0]],
    "wgrad_drop_split": [Bw.WGRAD_HALO_CASES[1], Bw.WGRAD_IM2COL_CASES[0]],
    "wgrad_flip_taps": [c for c in Bw.WGRAD_CASES if c[10] * c[11] > 1],
    "wgrad_no_ci_guard": [c for c in Bw.WGRAD_CASES if c[5] < c[6] and c[10] * c[11] > 1],   # 1x1: past the end only
    "wgrad_clamp_pad": [c for c in Bw.WGRAD_CASES if c[13] != (0, 0)],
    "convex_no_alpha": [v for v in Bw.CONVEX_VARIANTS if v[1] != 1.0],
}


@pytest.mark.parametrize("mut", list(MUTANTS), ids=str)
def test_mutant_fails(mut):
    """A kernel with this error fails its check: on every case where the error changes the result (the
    named ones; all of them otherwise, a_kmajor = 1 for the ignored flag)."""
    impl = Fp32(mut)
    failed = []
    for check, args in MUTANTS[mut]:
        must = MUTANT_MUST_FAIL.get(mut)
        if must is not None and args[0] not in must:
            continue
        if mut == "bgemm_ignore_kmajor" and args[1] == 0:
            continue
        try:
            check(impl, *args)
        except AssertionError:
            failed.append(args)
            continue
        pytest.fail(f"mutant {mut} passed {check.__name__}{args}")
    assert failed
