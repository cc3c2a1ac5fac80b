"""Plain fp64 reference of the census kernels (csrc/kernels/census.hip), the cases they are tested
at and the per-element checks, in the style of ``_unsup_refs.py`` (whose inputs these cases use:
``unsup_inputs`` with the shapes below; the census scale of iteration i is ``scale[i, 0]``).

``census_ref`` computes the per-iteration sums, the coefficient plane and the gradient by the
explicit formulas of ``train/unsup.py`` (steps 2c-3c) -- no autograd; the gradient as the scatter
``grad_w[p + d] += s(p) kappa(p, d)``, ``grad_w[p] -= s(p) kappa(p, d)`` -- in float64.  The fp32 steps
(the landing point ``px = float(x) + f.x``, ``inside``, the clamp, the floor and ``wx = pxc - x0``) are
computed in fp32, exactly as the kernel sees them (each is ONE fp32 operation on fp32 inputs), and then
promoted: no pixel is ambiguous and nothing is excluded from any check.

Tolerances (derived, not measured), with U = 2^-16 = 256 fp32 unit roundoffs as in ``_train_refs``.
An error bound is written d(.), a magnitude bound (.)B; every stage adds U times the magnitude of
its own result for its own roundings (the kernels' quotients and roots are products with the
hardware's reciprocal and reciprocal square root, 1 ulp each: a few u per stage, like the rest).

* Grey: ``GB = 127.5 (0.299 |r| + 0.587 |g| + 0.114 |b|)``, ``dG <= U GB``.  Warped grey: the bilinear
  expression with every term replaced by its magnitude down to the taps' GB, ``tB = c00B + wx (c01B +
  c00B)``, ``bB`` alike, ``wB = tB + wy (bB + tB)``, ``dw <= U wB``; its derivatives ``dwxB = (1 - wy)
  (c01B + c00B) + wy (c11B + c10B)``, ``dwyB = bB + tB``.
* Differences: ``dD1 <= U (GB(n) + GB(p))``, ``dD2 <= U (wB(n) + wB(p))``.
* ``tau(D) = D / sqrt(0.81 + D^2)``: ``tau' = 0.81 / (0.81 + D^2)^1.5`` is positive and decreasing in
  |D|, so over the interval the computed D can lie in ``tau' <= tau'(max(|D| - dD, 0)) <= 1 / 0.9``:
  ``dtau <= tau'(max(|D| - dD, 0)) dD + U |tau|``.  With ``diff = tau(D2) - tau(D1)``:
  ``ddiff <= dtau1 + dtau2 + U |diff|``; ``e = diff^2``: ``de <= 2 |diff| ddiff + ddiff^2 + U e``.
* ``k(e) = e / (0.1 + e)``: ``k' = 0.1 / (0.1 + e)^2`` is decreasing in e >= 0, at most 10:
  ``dk <= k'(max(e - de, 0)) de + U k``; ``dh <= sum_d dk + U h``.
* ``cen = (h + 0.01)^0.4``: its derivative ``0.4 (h + 0.01)^-0.6`` is decreasing in h, at most
  ``0.4 * 0.01^-0.6``: ``dcen <= 0.4 (max(h - dh, 0) + 0.01)^-0.6 dh + U cen``.  A sum of terms:
  ``sum mask dcen`` over the valid pixels ``+ U sum mask |term|``.  Counts are integers of at most
  256 per partial row: exact.
* The coefficient ``s = 0.4 (h + 0.01)^-0.6`` (valid masked pixels, 0 elsewhere): ``|s'| = 0.24 (h +
  0.01)^-1.6``, decreasing: ``ds <= 0.24 (max(h - dh, 0) + 0.01)^-1.6 dh + U s``.
* ``kappa = k'(e) 2 diff tau'(D2)``.  Both derivatives may be evaluated by the quotient rule, as
  autograd through the golden op does: ``k' = 1 / (0.1 + e) - e / (0.1 + e)^2`` and ``tau' = 1 / sqrt(q) -
  D^2 / q^1.5``, ``q = 0.81 + D^2``, whose roundings are U times the terms' magnitudes, not times the
  (smaller) difference.  ``|k''| = 0.2 / (0.1 + e)^3`` is decreasing: ``dk' <= |k''|(max(e - de, 0)) de +
  U (1 / (0.1 + e) + e / (0.1 + e)^2)``.  ``|tau''| = 2.43 |D| / (0.81 + D^2)^2.5`` rises up to |D| = 0.45
  and falls after it, so its supremum over ``[|D| - dD, |D| + dD]`` is its value at the end nearer to
  0.45, or at 0.45 if that lies inside: ``dtau' <= sup |tau''| dD + U (1 / sqrt(q) + D^2 / q^1.5)``.  The
  product of three factors, each taken at its upper end: ``dkappa <= 2 [(k' + dk') (|diff| + ddiff) (tau' + dtau') - k' |diff| tau'] + U
  |kappa|``.
* ``A(q) = -sum_d (s(q) + s(q+d)) kappa(q, d)`` (the kernel's gather; the same number as the scatter):
  ``dA <= sum_d [(ds(q) + ds(q+d)) |kappa| + (s(q) + s(q+d) + ds(q) + ds(q+d)) dkappa] + U sum_d (s(q) +
  s(q+d)) |kappa|``.
* A gradient element ``scale A dw`` (dw one of dw/dwx, dw/dwy) where inside, exactly 0 elsewhere:
  ``tol = |scale| [dA (|dw| + U dwB) + |A| U dwB] + U |scale A dw|``.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from _train_refs import U_ACC, bits_equal, ratio, report
from _unsup_refs import NAN_AT, unsup_inputs

R, C_TAU, C_K, C_H, C_POW = 3, 0.81, 0.1, 0.01, 0.4
PEN = 0.5
CENSUS_TILE, CENSUS_ITERS = (32, 8), 4      # the kernels' pixel tile (x, y) and iterations per block
# three tiles and a ragged remainder on both axes, a ragged second group of iterations (no grid-stride loop)
TILE_CASE = (CENSUS_ITERS + 1, 1, 3 * CENSUS_TILE[1] + 5, 3 * CENSUS_TILE[0] + 7, False)
# (N, B, H, W, NaN?)
CENSUS_CASES = [(1, 1, 1, 1, False), (1, 1, 6, 9, False), (1, 1, 7, 7, False), (2, 1, 7, 8, False), (2, 1, 8, 7, False),
                (3, 2, 13, 37, False), (12, 2, 40, 72, False), (12, 2, 40, 72, True), (32, 1, 24, 40, False), TILE_CASE]
VALID_GEOM = {(1, 1, 1, 1, False): 0, (1, 1, 6, 9, False): 0, (1, 1, 7, 7, False): 1}   # pixels whose patch is in the frame


def tiles_expected(B: int, H: int, W: int) -> int:
    tx, ty = CENSUS_TILE
    return B * ((H + ty - 1) // ty) * ((W + tx - 1) // tx)


def census_inputs(case, with_mask):
    """``unsup_inputs`` of the case; in the one-valid-pixel case the centre's flow is kept inside
    the frame, so that the pixel is valid."""
    c = unsup_inputs(case, with_mask)
    if case == (1, 1, 7, 7, False) and not getattr(c, "centred", False):
        c.pred[:, :, 3, 3] = c.pred[:, :, 3, 3].clamp(-2.0, 2.0)
        if c.mask is not None:
            c.mask[:, 3, 3] = 1.0
        c.centred = True
    return c


def gray64(img: torch.Tensor):
    i = img.double()
    g = 127.5 * ((0.299 * i[..., 0] + 0.587 * i[..., 1]) + 0.114 * i[..., 2])
    a = i.abs()
    return g, 127.5 * ((0.299 * a[..., 0] + 0.587 * a[..., 1]) + 0.114 * a[..., 2])


def landing32c(f: torch.Tensor):
    """Step 2c in fp32 for flows (B, H, W, 2): inside, the four tap indices and fp64 (wx, wy)."""
    H, W = f.shape[-3], f.shape[-2]
    px = torch.arange(W, dtype=torch.float32).view(1, W) + f[..., 0]
    py = torch.arange(H, dtype=torch.float32).view(H, 1) + f[..., 1]
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    zero = torch.zeros((), dtype=torch.float32)
    pxc = torch.where(px >= 0, px, zero).clamp(max=W - 1)
    pyc = torch.where(py >= 0, py, zero).clamp(max=H - 1)
    x0f, y0f = torch.floor(pxc), torch.floor(pyc)
    wx, wy = pxc - x0f, pyc - y0f                      # fp32, as the kernel computes them
    x0, y0 = x0f.long(), y0f.long()
    return inside, x0, (x0 + 1).clamp(max=W - 1), y0, (y0 + 1).clamp(max=H - 1), wx.double(), wy.double()


def warp64(f32: torch.Tensor, G2: torch.Tensor, G2B: torch.Tensor):
    """(inside, w, wB, dwx, dwy, dwxB, dwyB) of one prediction, fp64."""
    B, H, W, _ = f32.shape
    inside, x0, x1, y0, y1, wx, wy = landing32c(f32)

    def taps(plane):
        flat = plane.reshape(B, H * W)
        tap = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).reshape(B, H * W)).view(B, H, W)
        return tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)

    c00, c01, c10, c11 = taps(G2)
    b00, b01, b10, b11 = taps(G2B)
    t, b = c00 + wx * (c01 - c00), c10 + wx * (c11 - c10)
    tB, bB = b00 + wx * (b01 + b00), b10 + wx * (b11 + b10)
    return (inside, t + wy * (b - t), tB + wy * (bB + tB), (1.0 - wy) * (c01 - c00) + wy * (c11 - c10), b - t,
            (1.0 - wy) * (b01 + b00) + wy * (b11 + b10), bB + tB)


def offsets(radius=R):
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def shifted(padded: torch.Tensor, dy: int, dx: int, H: int, W: int):
    """plane(p + d) of a plane zero-padded by R."""
    return padded[:, R + dy:R + dy + H, R + dx:R + dx + W]


def tau_d2_sup(D, dD):
    """sup |tau''| over [|D| - dD, |D| + dD]."""
    f = lambda x: 2.43 * x / (C_TAU + x * x) ** 2.5
    lo, hi = (D.abs() - dD).clamp_min(0.0), D.abs() + dD
    peak = torch.full_like(D, 0.45)
    return torch.where((lo <= 0.45) & (hi >= 0.45), f(peak), torch.maximum(f(lo), f(hi)))


@functools.lru_cache(maxsize=None)
def census_ref(case, with_mask):
    """The reference of ``census_inputs(case, with_mask)``: fp64 per-iteration sums (N, 4) with the
    tolerances of columns 0 and 3, the coefficient plane (N, B, H, W) and the gradient for the
    case's scale (N, B, H, W, 2), each with its tolerance."""
    c = census_inputs(case, with_mask)
    N, B, H, W = c.N, c.B, c.H, c.W
    U = U_ACC
    pad = lambda t: F.pad(t, (R, R, R, R))
    G1, G1B = gray64(c.img1)
    G2, G2B = gray64(c.img2)
    on = torch.ones(B, H, W, dtype=torch.bool) if c.mask is None else c.mask >= 0.5
    m = on.double()
    geom = torch.zeros(B, H, W, dtype=torch.bool)
    if H > 2 * R and W > 2 * R:
        geom[:, R:H - R, R:W - R] = True
    G1p, G1Bp = pad(G1), pad(G1B)
    sums, sum_tol = torch.zeros(N, 4, dtype=torch.float64), torch.zeros(N, 4, dtype=torch.float64)
    coef, coef_tol = torch.zeros(N, B, H, W, dtype=torch.float64), torch.zeros(N, B, H, W, dtype=torch.float64)
    grad, tol = torch.zeros(N, B, H, W, 2, dtype=torch.float64), torch.zeros(N, B, H, W, 2, dtype=torch.float64)
    clamp_seen = []
    for i in range(N):
        f32 = c.pred[i]
        f = f32.double()
        inside, w, wB, dwx, dwy, dwxB, dwyB = warp64(f32, G2, G2B)
        wp, wBp = pad(w), pad(wB)
        valid = inside & geom
        per = []                                            # per offset: what the backward needs
        h, dh = torch.zeros_like(w), torch.zeros_like(w)
        for dy, dx in offsets():
            D1, D2 = shifted(G1p, dy, dx, H, W) - G1, shifted(wp, dy, dx, H, W) - w
            dD1, dD2 = U * (shifted(G1Bp, dy, dx, H, W) + G1B), U * (shifted(wBp, dy, dx, H, W) + wB)
            t1, t2 = D1 / torch.sqrt(C_TAU + D1 * D1), D2 / torch.sqrt(C_TAU + D2 * D2)
            tp_sup = lambda D, dD: C_TAU / (C_TAU + (D.abs() - dD).clamp_min(0.0) ** 2) ** 1.5
            diff = t2 - t1
            ddiff = tp_sup(D1, dD1) * dD1 + U * t1.abs() + tp_sup(D2, dD2) * dD2 + U * t2.abs() + U * diff.abs()
            e = diff * diff
            de = 2.0 * diff.abs() * ddiff + ddiff * ddiff + U * e
            k = e / (C_K + e)
            elo = (e - de).clamp_min(0.0)
            h = h + k
            dh = dh + C_K / (C_K + elo) ** 2 * de + U * k
            per.append((dy, dx, D2, dD2, diff, ddiff, e, de, elo))
        dh = dh + U * h
        hlo = (h - dh).clamp_min(0.0)
        cen = (h + C_H) ** C_POW
        dcen = C_POW * (hlo + C_H) ** (C_POW - 1.0) * dh + U * cen
        zero = torch.zeros_like(cen)
        term = torch.where(valid, cen, torch.where(inside, zero, zero + PEN)) + 0.0 * (f[..., 0] + f[..., 1])
        sel = on & valid
        last = i == N - 1
        sums[i] = torch.stack([(m * term).sum(), (on & ~inside).sum().double(), (on & inside & ~geom).sum().double(),
                               cen[sel].sum() if last else zero.sum()])
        sum_tol[i, 0] = dcen[sel].sum() + U * (m * torch.where(valid, cen, torch.where(inside, zero, zero + PEN))).sum()
        sum_tol[i, 3] = dcen[sel].sum() + U * cen[sel].sum() if last else 0.0
        s = sel.double() * C_POW * (h + C_H) ** (C_POW - 1.0)
        ds = sel.double() * (C_POW * (1.0 - C_POW) * (hlo + C_H) ** (C_POW - 2.0) * dh + U * s)
        coef[i], coef_tol[i] = s, ds
        sp, dsp = pad(s), pad(ds)
        gw = torch.zeros(B, H + 2 * R, W + 2 * R, dtype=torch.float64)      # the scatter, padded
        dA = torch.zeros_like(w)
        touched = torch.zeros(B, H, W, dtype=torch.bool)
        for dy, dx, D2, dD2, diff, ddiff, e, de, elo in per:
            q2 = C_TAU + D2 * D2
            tp = C_TAU / q2 ** 1.5
            dtp = tau_d2_sup(D2, dD2) * dD2 + U * (1.0 / q2.sqrt() + D2 * D2 / q2 ** 1.5)
            kp = C_K / (C_K + e) ** 2
            dkp = 2.0 * C_K / (C_K + elo) ** 3 * de + U * (1.0 / (C_K + e) + e / (C_K + e) ** 2)
            kappa = kp * 2.0 * diff * tp
            dkappa = 2.0 * ((kp + dkp) * (diff.abs() + ddiff) * (tp + dtp) - kp * diff.abs() * tp) + U * kappa.abs()
            contrib = s * kappa                                              # of pixel p to its neighbour p + d
            gw[:, R + dy:R + dy + H, R + dx:R + dx + W] += contrib
            gw[:, R:R + H, R:R + W] -= contrib
            S, dS = s + shifted(sp, dy, dx, H, W), ds + shifted(dsp, dy, dx, H, W)
            dA = dA + dS * kappa.abs() + (S + dS) * dkappa + U * S * kappa.abs()
            # a valid pixel whose patch holds a neighbour that lands outside the frame (the clamp path)
            touched |= sel & (shifted(pad((~inside).double()), dy, dx, H, W) > 0)
        clamp_seen.append(bool(touched.any()))
        assert float(gw[:, :R].abs().sum() + gw[:, -R:].abs().sum() + gw[:, :, :R].abs().sum() + gw[:, :, -R:].abs().sum()) == 0.0
        A = gw[:, R:R + H, R:R + W]
        sc = float(c.scale[i, 0])
        ins = inside.double()
        for ch, (dw, dwB) in enumerate(((dwx, dwxB), (dwy, dwyB))):
            grad[i, ..., ch] = sc * ins * A * dw
            tol[i, ..., ch] = ins * (abs(sc) * (dA * (dw.abs() + U * dwB) + A.abs() * U * dwB) + U * (sc * A * dw).abs())
    return NS(sums=sums, sum_tol=sum_tol, coef=coef, coef_tol=coef_tol, grad=grad, tol=tol, clamp_seen=clamp_seen,
              n_valid=int((geom & on).sum()))


def check_census_loss(impl, case, with_mask):
    """impl.census_loss(pred, img1, img2, mask, out_penalty) -> (fp32 part [tiles, N, 4], fp32 coef
    [N, B, H, W] or None); the implementation pre-fills its outputs with NaN, so unwritten elements show."""
    c, ref = census_inputs(case, with_mask), census_ref(case, with_mask)
    name = f"census_loss{case} mask={with_mask}"
    part, coef = impl.census_loss(c.pred, c.img1, c.img2, c.mask, PEN)
    assert part.dtype == torch.float32 and part.shape[1:] == (c.N, 4), part.shape
    if getattr(impl, "tiles", True):
        assert part.shape[0] == tiles_expected(c.B, c.H, c.W)
    part2, coef2 = impl.census_loss(c.pred, c.img1, c.img2, c.mask, PEN)
    assert bits_equal(part, part2), f"{name}: two identical calls differ"
    s = part.double().sum(0)
    worst = 0.0
    for i in range(c.N):
        if c.nan and i == NAN_AT[0]:
            assert torch.isnan(ref.sums[i, 0]) and torch.isnan(s[i, 0]), f"{name}: the NaN did not reach iteration {i}'s sum"
            continue
        assert bool(torch.isfinite(ref.sums[i]).all()) and bool(torch.isfinite(s[i]).all()), f"{name}: iteration {i}"
        for q in (0, 3):
            worst = max(worst, ratio(s[i, q], ref.sums[i, q], ref.sum_tol[i, q]))
    assert int(torch.isnan(ref.sums[:, 0]).sum()) == (1 if c.nan else 0)
    assert torch.equal(s[:, 1:3], ref.sums[:, 1:3]), f"{name}: counts {s[:, 1:3].tolist()} != {ref.sums[:, 1:3].tolist()}"
    assert bool(torch.isfinite(part[:, :, 1:]).all()), f"{name}: unwritten or non-finite partials"
    assert bool((part[:, :-1, 3] == 0).all()), f"{name}: the cen sum belongs to the last iteration only"
    if case in VALID_GEOM:
        assert int(c.B * max(c.H - 2 * R, 0) * max(c.W - 2 * R, 0)) == VALID_GEOM[case]
        if VALID_GEOM[case] == 0:                       # no valid pixel: penalties only, exactly
            assert torch.equal(s[:, 0], PEN * ref.sums[:, 1]) and not s[:, 3].any()
    report(name + " sums", worst)
    assert worst <= 1.0, f"{name}: error / tolerance = {worst}"
    if coef is not None:
        assert coef.dtype == torch.float32 and coef.shape == c.pred.shape[:-1] and bits_equal(coef, coef2)
        assert bool(torch.isfinite(coef).all()), f"{name}: unwritten or non-finite coefficients"
        assert torch.equal(coef != 0, ref.coef != 0), f"{name}: the coefficient's support"
        r = ratio(coef, ref.coef, ref.coef_tol)
        report(name + " coef", r)
        assert r <= 1.0, f"{name}: coefficient error / tolerance = {r}"


def check_census_loss_bwd(impl, case, with_mask):
    """impl.census_loss_bwd(pred, img1, img2, mask, out_penalty, scale (N,)) -> fp32 grad [N, B, H, W, 2]."""
    c, ref = census_inputs(case, with_mask), census_ref(case, with_mask)
    name = f"census_loss_bwd{case} mask={with_mask}"
    scale = c.scale[:, 0].contiguous()
    grad = impl.census_loss_bwd(c.pred, c.img1, c.img2, c.mask, PEN, scale)
    assert grad.dtype == torch.float32 and grad.shape == c.pred.shape
    again = impl.census_loss_bwd(c.pred, c.img1, c.img2, c.mask, PEN, scale)
    assert bits_equal(grad, again), f"{name}: two identical calls differ"
    # the census term's gradient is finite everywhere: a non-finite flow is not inside and has none
    assert bool(torch.isfinite(ref.grad).all()) and bool(torch.isfinite(grad).all()), f"{name}: non-finite gradient"
    r = ratio(grad, ref.grad, ref.tol)
    report(name, r)
    assert r <= 1.0, f"{name}: error / tolerance = {r}"
    # not vacuous: the tolerance is far below the gradient itself
    big = ref.grad.abs() > 0
    if c.P >= 1000:
        assert float((ref.tol[big] / ref.grad.abs()[big]).median()) < 0.05
