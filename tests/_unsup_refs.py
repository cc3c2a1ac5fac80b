"""Plain fp64 reference of the label-free loss kernels (csrc/kernels/unsup.hip), the cases they
are tested at and the per-element checks, in the style of ``_train_refs.py``.

``unsup_ref`` computes the block-partial sums and the gradient by the explicit formulas of
``train/unsup.py`` / the kernel's header -- no autograd -- in float64.  Steps 1-2 (the landing
point ``px = float(x) + f.x``, ``inside``, the floor and ``wx = px - x0``) are computed in fp32,
exactly as the kernel sees them (each is ONE fp32 operation on fp32 inputs, so there is no order to
differ in), and then promoted: no pixel is ambiguous and nothing is excluded from any check.

Each ``check_*`` takes an *implementation* -- an object whose methods map CPU tensors to CPU
tensors.  The GPU tests pass the HIP kernels (tests/test_unsup_gpu.py); the CPU tests pass the
fp32 golden op and an fp32 emulation of the kernels' operation order (tests/test_unsup.py), which
shows that the tolerances are attainable, and wrong variants, which shows they are not vacuous.

Tolerances (derived, not measured), with U = 2^-16 = 256 fp32 unit roundoffs as in ``_train_refs``:

* Magnitude bounds are the same expressions with every term replaced by its magnitude, down to
  the texels: ``tB = |c00| + wx (|c01| + |c00|)``, ``bB`` alike, ``vB = tB + wy (bB + tB)``,
  ``dB_c = vB_c + |image1_c|``, ``pixB = mean_c sqrt(dB_c^2 + eps^2)`` (rho is 1-Lipschitz, so an
  error of a few u dB in d moves rho by no more), ``out_penalty`` outside.
* An edge weight ``a = exp(-kappa m)``, ``m = mean_c |image1' - image1|``: m carries a few u of
  ``mB = mean_c (|image1'| + |image1|)``, the product with kappa one more, exp two ulps, so
  ``|da| <= a (kappa mB + 1) * (a few u)``; the bound of a is ``aB = a (1 + kappa mB)``.
* A sum: ``tol = U * sum |terms|`` with the terms' bounds above (``aB sum_k sqrt((|f'_k| + |f_k|)^2
  + eps_s^2)`` for a smoothness pair).
* A gradient element.  Photometric, per channel: ``rho'(d) = d / sqrt(d^2 + eps^2)`` has
  ``|rho'| <= 1`` and ``|d rho'/dd| = eps^2 / (d^2 + eps^2)^1.5 <= 1 / eps``, so the error of d,
  ``|dd| <= U dB_c``, is amplified to ``|d rho'| <= U dB_c / eps`` -- the term that matters at
  eps = 0.01 -- and ``rho' dv`` is off by at most ``(U dB_c / eps) |dv_c| + U dvB_c`` (the second
  term: ``|rho'| <= 1`` times the error of ``dv_c``, a few u of its bound ``dvB_c``, and every
  rounding of the products and sums).  Smoothness, per neighbour: ``D`` is one exact fp32
  subtraction (relative error u), ``|d rho_s'/dD| |D| u <= 0.385 u`` (the maximum of
  ``x / (1 + x^2)^1.5``), the root and the quotient add a few u of ``|rho_s'| <= 1``: at most
  ``U aB`` per neighbour, the weight's own error included.  With the scales
  (s_p, s_s): ``tol = |s_p| / 3 sum_c [(U dB_c / eps) |dv_c| + U dvB_c] + |s_s| U sum_nb aB``.
* Counts are integers below 2^24 per block: exact.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace as NS

import torch

from _train_refs import U_ACC, _gen, bf, bits_equal, ratio, report

UNSUP_GRID = 1024 * 256   # pixels per grid-stride round of unsup_loss_kernel (GRID_X * BLOCK)
UNSUP_BLOCK = 256
PRM = (0.01, 0.001, 10.0, 0.5)   # eps, eps_s, edge_kappa, out_penalty
# (N, B, H, W, NaN?): the issue's shapes; then the NaN case; then more than one grid-stride round
# (and a ragged second group of iterations: the kernels take 4 per block)
UNSUP_CASES = [(1, 1, 1, 1, False), (2, 1, 1, 9, False), (2, 1, 9, 1, False), (3, 2, 13, 37, False),
               (12, 2, 40, 72, False), (32, 1, 24, 40, False), (12, 2, 40, 72, True), (5, 1, 516, 512, False)]
assert 516 * 512 > UNSUP_GRID
NAN_AT = (5, 1, 17, 33)   # (iteration, b, y, x) of the NaN case: a middle iteration, an interior pixel


def blocks_expected(P: int) -> int:
    return min(UNSUP_GRID // UNSUP_BLOCK, (P + UNSUP_BLOCK - 1) // UNSUP_BLOCK)


@functools.lru_cache(maxsize=None)
def unsup_inputs(case, with_mask):
    N, B, H, W, nan = case
    gen = _gen(900 + N + 7 * H + W + (1 if with_mask else 0))
    P = B * H * W
    ys = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    it = torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1)
    # smooth + scattered
    fx = 2.5 * torch.sin(0.11 * xs + 0.07 * ys + 0.3 * it) + 0.8 * torch.randn(N, B, H, W, generator=gen)
    fy = 1.5 * torch.cos(0.05 * xs - 0.13 * ys + 0.2 * it) + 0.8 * torch.randn(N, B, H, W, generator=gen)
    pred = torch.stack([fx, fy], -1).contiguous()
    flat = pred.view(N, P, 2)
    px = xs.expand(N, B, H, W).reshape(N, P)
    py = ys.expand(N, B, H, W).reshape(N, P)
    idx = torch.arange(P)
    sel = lambda k: idx % 13 == k
    flat[:, sel(1)] = torch.round(flat[:, sel(1)])                                   # exact-integer landings
    flat[:, sel(2), 0] = (W - 1) - px[:, sel(2)]                                      # exactly on W - 1
    flat[:, sel(3), 1] = (H - 1) - py[:, sel(3)]                                      # exactly on H - 1
    flat[:, sel(4), 0] = -px[:, sel(4)] - 1e-3                                        # just outside
    flat[:, sel(5), 1] = (H - 1) - py[:, sel(5)] + 1e-3
    flat[:, idx % 53 == 6] = torch.tensor([1e6, -1e6])                                # far outside
    if W > 1:                                                                         # exact ties with a neighbour
        t = (idx % 13 == 8) & (idx % W > 0)
        flat[:, t] = flat[:, torch.nonzero(t).squeeze(1) - 1]
    if H > 1:
        t = (idx % 13 == 10) & ((idx // W) % H > 0)
        flat[:, t, 1] = flat[:, torch.nonzero(t).squeeze(1) - W, 1]
    img1 = bf(0.6 * torch.sin(0.3 * xs + 0.2 * ys).squeeze(0).unsqueeze(-1)
              + 0.15 * torch.randn(B, H, W, 3, generator=gen)).contiguous()          # bf16-valued
    img2 = (0.6 * torch.sin(0.3 * xs + 0.2 * ys + 0.4).squeeze(0).unsqueeze(-1)
            + 0.3 * torch.randn(B, H, W, 3, generator=gen)).contiguous()             # arbitrary fp32
    mask = None
    if with_mask:
        mask = (torch.rand(B, H, W, generator=gen) > 0.3).float()
        mask.view(-1)[idx % 17 == 3] = 0.5      # on
        mask.view(-1)[idx % 17 == 4] = 0.49     # off
    if nan:
        i, b, y, x = NAN_AT
        pred[:, b, y - 1:y + 2, x - 1:x + 2] = pred[:, b, y - 1:y + 2, x - 1:x + 2].clamp(-1.0, 1.0)   # finite, inside
        pred[i, b, y, x, 0] = float("nan")
        if mask is not None:
            mask[b, y, x] = 1.0
    scale = torch.stack([(torch.arange(N, dtype=torch.float32) * 0.13 + 0.37) / 1024.0,
                         (torch.arange(N, dtype=torch.float32) * 0.05 + 0.21) / 64.0], -1).contiguous()
    return NS(N=N, B=B, H=H, W=W, P=P, pred=pred, img1=img1, img2=img2, mask=mask, scale=scale, nan=nan)


def landing32(f: torch.Tensor):
    """Steps 1-2 in fp32 for flows (..., H, W, 2): inside, the four tap indices and fp64 (wx, wy)."""
    H, W = f.shape[-3], f.shape[-2]
    px = torch.arange(W, dtype=torch.float32).view(1, W) + f[..., 0]
    py = torch.arange(H, dtype=torch.float32).view(H, 1) + f[..., 1]
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    zero = torch.zeros((), dtype=torch.float32)
    pxs, pys = torch.where(inside, px, zero), torch.where(inside, py, zero)
    x0f, y0f = torch.floor(pxs), torch.floor(pys)
    wx, wy = pxs - x0f, pys - y0f                      # fp32, as the kernel computes them
    x0, y0 = x0f.long(), y0f.long()
    return inside, x0, (x0 + 1).clamp(max=W - 1), y0, (y0 + 1).clamp(max=H - 1), wx.double(), wy.double()


def edge_ref(img1: torch.Tensor, kappa: float):
    """fp64 (a, aB) between horizontal neighbours (B, H, W-1) and vertical ones (B, H-1, W)."""
    i = img1.double()

    def pair(p, q):
        a = torch.exp(-kappa * (q - p).abs().mean(-1))
        return a, a * (1.0 + kappa * (q.abs() + p.abs()).mean(-1))

    return pair(i[:, :, :-1], i[:, :, 1:]), pair(i[:, :-1], i[:, 1:])


@functools.lru_cache(maxsize=None)
def unsup_ref(case, with_mask):
    """The reference of ``unsup_inputs(case, with_mask)``: fp64 per-iteration sums (N, 4) with
    their bounds, and the gradient for the case's scale with its tolerance, (N, B, H, W, 2)."""
    c = unsup_inputs(case, with_mask)
    eps, eps_s, kappa, pen = PRM
    N, B, H, W = c.N, c.B, c.H, c.W
    i1, i2 = c.img1.double(), c.img2.double().reshape(B, H * W, 3)
    on = torch.ones(B, H, W, dtype=torch.bool) if c.mask is None else c.mask >= 0.5
    m = on.double()
    (ax, axB), (ay, ayB) = edge_ref(c.img1, kappa)
    sums = torch.zeros(N, 4, dtype=torch.float64)
    bounds = torch.zeros(N, 4, dtype=torch.float64)
    grad = torch.zeros(N, B, H, W, 2, dtype=torch.float64)
    tol = torch.zeros(N, B, H, W, 2, dtype=torch.float64)
    for i in range(N):
        f32 = c.pred[i]
        f = f32.double()
        inside, x0, x1, y0, y1, wx, wy = landing32(f32)
        wx, wy = wx.unsqueeze(-1), wy.unsqueeze(-1)

        def tap(yy, xx):
            idx = (yy * W + xx).reshape(B, H * W, 1).expand(-1, -1, 3)
            return torch.gather(i2, 1, idx).view(B, H, W, 3)

        c00, c01, c10, c11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
        t, b = c00 + wx * (c01 - c00), c10 + wx * (c11 - c10)
        tB, bB = c00.abs() + wx * (c01.abs() + c00.abs()), c10.abs() + wx * (c11.abs() + c10.abs())
        d = t + wy * (b - t) - i1
        dB = tB + wy * (bB + tB) + i1.abs()
        r = torch.sqrt(d * d + eps * eps)
        pix = torch.where(inside, r.mean(-1), pen + 0.0 * (f[..., 0] + f[..., 1]))
        pixB = torch.where(inside, torch.sqrt(dB * dB + eps * eps).mean(-1), torch.full_like(pix, pen))
        # smoothness: the pairs to the right of and below every pixel
        dx, dy = f[:, :, 1:] - f[:, :, :-1], f[:, 1:] - f[:, :-1]
        rx, ry = torch.sqrt(dx * dx + eps_s ** 2), torch.sqrt(dy * dy + eps_s ** 2)
        rxB = torch.sqrt((f[:, :, 1:].abs() + f[:, :, :-1].abs()) ** 2 + eps_s ** 2)
        ryB = torch.sqrt((f[:, 1:].abs() + f[:, :-1].abs()) ** 2 + eps_s ** 2)
        sel = on & inside
        sums[i] = torch.stack([(m * pix).sum(), (ax.unsqueeze(-1) * rx).sum() + (ay.unsqueeze(-1) * ry).sum(),
                               (on & ~inside).sum().double(), pix[sel].sum() if i == N - 1 else pix.new_zeros(())])
        bounds[i] = torch.stack([(m * pixB).sum(), (axB.unsqueeze(-1) * rxB).sum() + (ayB.unsqueeze(-1) * ryB).sum(),
                                 pix.new_zeros(()), pixB[sel].sum() if i == N - 1 else pix.new_zeros(())])
        # gradient: photometric part
        sp, ss = float(c.scale[i, 0]), float(c.scale[i, 1])
        dr = d / r
        dvx = (1.0 - wy) * (c01 - c00) + wy * (c11 - c10)
        dvy = b - t
        dvxB = (1.0 - wy) * (c01.abs() + c00.abs()) + wy * (c11.abs() + c10.abs())
        dvyB = bB + tB
        k = (sel.double() * sp / 3.0).unsqueeze(-1)
        amp = U_ACC * dB / eps
        grad[i] = torch.stack([(k * dr * dvx).sum(-1), (k * dr * dvy).sum(-1)], -1)
        tol[i] = abs(sp) / 3.0 * sel.double().unsqueeze(-1) * torch.stack(
            [(amp * dvx.abs() + U_ACC * dvxB).sum(-1), (amp * dvy.abs() + U_ACC * dvyB).sum(-1)], -1)
        # ... and the four-neighbour stencil
        gx, gy = ax.unsqueeze(-1) * dx / rx, ay.unsqueeze(-1) * dy / ry        # a rho_s'(D) of each pair
        grad[i, :, :, :-1] -= ss * gx
        grad[i, :, :, 1:] += ss * gx
        grad[i, :, :-1] -= ss * gy
        grad[i, :, 1:] += ss * gy
        tol[i, :, :, :-1] += abs(ss) * U_ACC * axB.unsqueeze(-1)
        tol[i, :, :, 1:] += abs(ss) * U_ACC * axB.unsqueeze(-1)
        tol[i, :, :-1] += abs(ss) * U_ACC * ayB.unsqueeze(-1)
        tol[i, :, 1:] += abs(ss) * U_ACC * ayB.unsqueeze(-1)
    return NS(sums=sums, bounds=bounds, grad=grad, tol=tol)


def check_unsup_loss(impl, case, with_mask):
    """impl.unsup_loss(pred, img1, img2, mask, prm) -> fp32 part [blocks, N, 4] (the implementation
    pre-fills its output with NaN, so unwritten elements show)."""
    c, ref = unsup_inputs(case, with_mask), unsup_ref(case, with_mask)
    name = f"unsup_loss{case} mask={with_mask}"
    part = impl.unsup_loss(c.pred, c.img1, c.img2, c.mask, PRM)
    assert part.dtype == torch.float32 and part.shape[1:] == (c.N, 4), part.shape
    if getattr(impl, "blocks", True):
        assert part.shape[0] == blocks_expected(c.P)
    again = impl.unsup_loss(c.pred, c.img1, c.img2, c.mask, PRM)
    assert bits_equal(part, again), f"{name}: two identical calls differ"
    s = part.double().sum(0)
    worst = 0.0
    for i in range(c.N):
        if c.nan and i == NAN_AT[0]:
            assert torch.isnan(ref.sums[i, 0]) and torch.isnan(ref.sums[i, 1])
            assert torch.isnan(s[i, 0]) and torch.isnan(s[i, 1]), f"{name}: the NaN did not reach iteration {i}'s sums"
            continue
        assert bool(torch.isfinite(ref.sums[i]).all()) and bool(torch.isfinite(s[i]).all()), f"{name}: iteration {i}"
        for q in (0, 1, 3):
            worst = max(worst, ratio(s[i, q], ref.sums[i, q], U_ACC * ref.bounds[i, q]))
    assert int(torch.isnan(ref.sums[:, 0]).sum()) == (1 if c.nan else 0)
    assert torch.equal(s[:, 2], ref.sums[:, 2]), f"{name}: counts {s[:, 2].tolist()} != {ref.sums[:, 2].tolist()}"
    assert bool((part[:, :-1, 3] == 0).all()), f"{name}: the inside sum belongs to the last iteration only"
    report(name + " sums", worst)
    assert worst <= 1.0, f"{name}: error / tolerance = {worst}"


def check_unsup_loss_bwd(impl, case, with_mask):
    """impl.unsup_loss_bwd(pred, img1, img2, mask, prm, scale) -> fp32 grad [N, B, H, W, 2]."""
    c, ref = unsup_inputs(case, with_mask), unsup_ref(case, with_mask)
    name = f"unsup_loss_bwd{case} mask={with_mask}"
    grad = impl.unsup_loss_bwd(c.pred, c.img1, c.img2, c.mask, PRM, c.scale)
    assert grad.dtype == torch.float32 and grad.shape == c.pred.shape
    again = impl.unsup_loss_bwd(c.pred, c.img1, c.img2, c.mask, PRM, c.scale)
    assert bits_equal(grad, again), f"{name}: two identical calls differ"
    finite = torch.isfinite(ref.grad)
    if c.nan:
        i, b, y, x = NAN_AT
        # the NaN is in the flow's x component: by propagation through the smoothness stencil
        assert not bool(finite[i, b, y, x, 0]), "the reference's gradient at the NaN pixel must be non-finite"
        assert bool(finite[:i].all()) and bool(finite[i + 1:].all())
        assert not bool(torch.isfinite(grad[i, b, y, x, 0])), f"{name}: finite gradient at the NaN pixel"
    else:
        assert bool(finite.all())
    assert torch.equal(torch.isfinite(grad), finite), f"{name}: non-finite elements differ from the reference's"
    r = ratio(grad, ref.grad, ref.tol, finite)
    report(name, r)
    assert r <= 1.0, f"{name}: error / tolerance = {r}"
    # not vacuous: the tolerance is far below the gradient itself
    big = finite & (ref.grad.abs() > 0)
    if c.P >= 1000:
        assert float((ref.tol[big] / ref.grad.abs()[big]).median()) < 0.05
