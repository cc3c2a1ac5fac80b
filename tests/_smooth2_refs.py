"""Plain fp64 reference of the second-order smoothness kernels (csrc/kernels/smooth2.hip), the cases
they are tested at and the per-element checks, in the style of ``_unsup_refs.py``.

``smooth2_ref`` computes the per-iteration sums and the gradient by the explicit formulas of
``train/unsup.py`` step 4b -- no autograd -- in float64, by shifted slices of the (B, H, W) grid, so
that no triple can cross a row end, a frame end or a sample boundary.

Each ``check_*`` takes an *implementation* -- an object whose methods map CPU tensors to CPU tensors.
The GPU tests pass the HIP kernels (tests/test_smooth2_gpu.py); the CPU tests pass the fp32 golden op
and an fp32 emulation of the kernels' operation order (tests/test_smooth2.py), which shows that the
tolerances are attainable, and wrong variants, which shows they are not vacuous.

Tolerances (derived, not measured), with U = 2^-16 = 256 fp32 unit roundoffs as in ``_unsup_refs``:

* An edge weight ``a = exp(-kappa m)``, ``m = mean_c |image1'' - image1|`` over the stride-2 pair: as in
  ``_unsup_refs``, ``|da| <= a (kappa mB + 1) * (a few u)`` with ``mB = mean_c (|image1''| + |image1|)``;
  the bound of a is ``aB = a (1 + kappa mB)``.
* A sum: ``tol = U * sum |term bounds|``, a triple's bound being ``aB sum_k sqrt(MB_k^2 + eps_s^2)`` with
  ``MB = |f0| + 2 |f1| + |f2|``, the magnitude bound of ``D = (f2 - f1) - (f1 - f0)``.
* A gradient element.  Unlike the first-order difference, D is not one exact subtraction: its fp32 value is
  off by up to a few ``u MB``, and ``psi(D) = D / sqrt(D^2 + eps_s^2)`` amplifies that by its slope
  ``eps_s^2 / (D^2 + eps_s^2)^1.5``, which is ``1 / eps_s`` at D = 0 and falls monotonically in ``|D|``.  A
  uniform ``1 / eps_s`` would make the check vacuous at eps_s = 0.001, so the bound is local: with
  ``delta = U MB`` the computed D lies within delta of the reference's, and the slope anywhere on that
  interval is at most the slope at ``max(|D_ref| - delta, 0)``.  Per triple and component:
  ``aB (delta slope + U)`` -- the second term covers the root, the quotient (``|psi| <= 1``) and the
  weight's own error.  A pixel is the left end, the centre and the right end of up to three triples per
  axis, with coefficients 1, 2, 1: the tolerance is the sum of the triples' bounds with those coefficients,
  times ``|scale|``.
* Nothing is excluded from any check.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import torch

from _train_refs import U_ACC, _gen, bf, bits_equal, ratio, report

GRID = 1024 * 256    # pixels per grid-stride round of smooth2_loss_kernel (GRID_X * BLOCK)
BLOCK = 256
EPS_S, KAPPA = 0.001, 10.0
PRM = (0.01, EPS_S, KAPPA, 0.5)   # the kernels' parameter tensor: eps, eps_s, edge_kappa, out_penalty
# (N, B, H, W, NaN?): axes without triples; exactly one triple per row and column; odd width and two samples;
# several blocks and a ragged iteration group (the kernels take 4 per block); the most iterations; the NaN
# case; more than one grid-stride round
CASES = [(1, 1, 1, 1, False), (2, 1, 1, 2, False), (2, 1, 2, 9, False), (2, 1, 9, 2, False), (1, 1, 3, 3, False),
         (3, 2, 13, 37, False), (5, 2, 40, 72, False), (32, 1, 24, 40, False), (12, 2, 40, 72, True),
         (5, 1, 516, 512, False)]
assert 516 * 512 > GRID
NAN_AT = (5, 1, 17, 33)   # (iteration, b, y, x) of the NaN case: a middle iteration, an interior pixel; component x


def blocks_expected(P: int) -> int:
    return min(GRID // BLOCK, (P + BLOCK - 1) // BLOCK)


@functools.lru_cache(maxsize=None)
def inputs(case):
    N, B, H, W, nan = case
    gen = _gen(1700 + N + 7 * H + W)
    ys = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    it = torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1)
    # smooth + scattered, as _unsup_refs.unsup_inputs builds it
    fx = 2.5 * torch.sin(0.11 * xs + 0.07 * ys + 0.3 * it) + 0.8 * torch.randn(N, B, H, W, generator=gen)
    fy = 1.5 * torch.cos(0.05 * xs - 0.13 * ys + 0.2 * it) + 0.8 * torch.randn(N, B, H, W, generator=gen)
    pred = torch.stack([fx, fy], -1).contiguous()
    # an integer-valued linear ramp: every second difference inside it is exactly 0 in fp32 and in fp64, the
    # pixels where psi's slope is 1 / eps_s ...
    y0, y1, x0, x1 = H // 4, H // 2, W // 4, (3 * W) // 4
    ramp = torch.stack([2.0 * xs + 3.0 * ys - 5.0 + it, 2.0 * ys - xs + 1.0 - it], -1).expand(N, B, H, W, 2)
    pred[:, :, y0:y1, x0:x1] = ramp[:, :, y0:y1, x0:x1]
    # ... and a constant region
    pred[:, :, H // 2:(3 * H) // 4, :W // 2] = torch.tensor([1.25, -0.75])
    img1 = bf(0.6 * torch.sin(0.3 * xs + 0.2 * ys).squeeze(0).unsqueeze(-1)
              + 0.15 * torch.randn(B, H, W, 3, generator=gen)).contiguous()          # bf16-valued
    if nan:
        i, b, y, x = NAN_AT
        pred[i, b, y, x, 0] = float("nan")
    scale = ((torch.arange(N, dtype=torch.float32) * 0.05 + 0.21) / 64.0).contiguous()
    return NS(N=N, B=B, H=H, W=W, P=B * H * W, pred=pred, img1=img1, scale=scale, nan=nan)


def edge_ref(img1: torch.Tensor, kappa: float):
    """fp64 (a, aB) across the triples along x (B, H, W-2) and along y (B, H-2, W); an axis shorter than 3 has none."""
    i = img1.double()

    def pair(p, q):
        a = torch.exp(-kappa * (q - p).abs().mean(-1))
        return a, a * (1.0 + kappa * (q.abs() + p.abs()).mean(-1))

    return pair(i[:, :, :-2], i[:, :, 2:]), pair(i[:, :-2], i[:, 2:])


def _ends(t: torch.Tensor, axis: int):
    """The (left end, centre, right end) views of a (B, H, W, 2) tensor along H (axis 1) or W (axis 2)."""
    n = t.shape[axis]
    cut = lambda lo, hi: t.narrow(axis, lo, max(hi - lo, 0)) if n >= 3 else t.narrow(axis, 0, 0)
    return cut(0, n - 2), cut(1, n - 1), cut(2, n)


@functools.lru_cache(maxsize=None)
def smooth2_ref(case):
    """The reference of ``inputs(case)``: fp64 per-iteration sums (N, 2) = (x axis, y axis) with their bounds, and
    the gradient for the case's scale with its tolerance, (N, B, H, W, 2)."""
    c = inputs(case)
    N, B, H, W = c.N, c.B, c.H, c.W
    es2 = EPS_S ** 2
    edges = edge_ref(c.img1, KAPPA)
    sums = torch.zeros(N, 2, dtype=torch.float64)
    bounds = torch.zeros(N, 2, dtype=torch.float64)
    grad = torch.zeros(N, B, H, W, 2, dtype=torch.float64)
    tol = torch.zeros(N, B, H, W, 2, dtype=torch.float64)
    for i in range(N):
        f = c.pred[i].double()
        s = float(c.scale[i])
        for q, axis in ((0, 2), (1, 1)):
            a, aB = (e.unsqueeze(-1) for e in edges[q])
            f0, f1, f2 = _ends(f, axis)
            D = (f2 - f1) - (f1 - f0)
            MB = f0.abs() + 2.0 * f1.abs() + f2.abs()
            r = torch.sqrt(D * D + es2)
            sums[i, q] = (a * r).sum()
            bounds[i, q] = (aB * torch.sqrt(MB * MB + es2)).sum()
            t = a * D / r                                              # a psi(D) of each triple
            delta = U_ACC * MB
            near = (D.abs() - delta).clamp_min(0.0)                    # the steepest point of psi within delta of D
            tt = aB * (delta * es2 / (near * near + es2) ** 1.5 + U_ACC)
            for view, coef in zip(_ends(grad[i], axis), (1.0, -2.0, 1.0)):
                view += coef * s * t
            for view, coef in zip(_ends(tol[i], axis), (1.0, 2.0, 1.0)):
                view += coef * abs(s) * tt
    return NS(sums=sums, bounds=bounds, grad=grad, tol=tol)


def check_partials(impl, case):
    """impl.smooth2_loss(pred, img1, prm) -> fp32 part [blocks, N, 4] (the implementation pre-fills its output
    with NaN, so unwritten elements show)."""
    c, ref = inputs(case), smooth2_ref(case)
    name = f"smooth2_loss{case}"
    part = impl.smooth2_loss(c.pred, c.img1, PRM)
    assert part.dtype == torch.float32 and part.shape[1:] == (c.N, 4), part.shape
    if getattr(impl, "blocks", True):
        assert part.shape[0] == blocks_expected(c.P)
    again = impl.smooth2_loss(c.pred, c.img1, PRM)
    assert bits_equal(part, again), f"{name}: two identical calls differ"
    assert bool((part[:, :, 2:] == 0).all()), f"{name}: words 2 and 3 of a row are 0"
    s = part.double().sum(0)[:, :2]
    worst = 0.0
    for i in range(c.N):
        if c.nan and i == NAN_AT[0]:
            assert not bool(torch.isfinite(ref.sums[i]).any())
            assert not bool(torch.isfinite(s[i]).any()), f"{name}: the NaN did not reach iteration {i}'s sums"
            continue
        assert bool(torch.isfinite(ref.sums[i]).all()) and bool(torch.isfinite(s[i]).all()), f"{name}: iteration {i}"
        worst = max(worst, ratio(s[i], ref.sums[i], U_ACC * ref.bounds[i]))
    if c.W < 3:
        assert not s[:, 0].any(), f"{name}: W < 3 has no triples along x"
    if c.H < 3:
        assert not s[:, 1].any(), f"{name}: H < 3 has no triples along y"
    report(name + " sums", worst)
    assert worst <= 1.0, f"{name}: error / tolerance = {worst}"


def check_grad(impl, case):
    """impl.smooth2_loss_bwd(pred, img1, prm, scale) -> fp32 grad [N, B, H, W, 2]."""
    c, ref = inputs(case), smooth2_ref(case)
    name = f"smooth2_loss_bwd{case}"
    grad = impl.smooth2_loss_bwd(c.pred, c.img1, PRM, c.scale)
    assert grad.dtype == torch.float32 and grad.shape == c.pred.shape
    again = impl.smooth2_loss_bwd(c.pred, c.img1, PRM, c.scale)
    assert bits_equal(grad, again), f"{name}: two identical calls differ"
    finite = torch.isfinite(ref.grad)
    if c.nan:
        i, b, y, x = NAN_AT
        # the x component of the pixels that share a triple with the NaN pixel: two to each side in its row and column
        want = torch.ones_like(finite)
        want[i, b, y, x - 2:x + 3, 0] = False
        want[i, b, y - 2:y + 3, x, 0] = False
        assert torch.equal(finite, want), "the reference's non-finite elements are the triples that touch the NaN"
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
