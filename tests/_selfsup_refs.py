"""Plain fp64 references of the self-supervision ops (train/selfsup.py, csrc/kernels/selfsup.hip), the
cases they are tested at and the per-element checks, in the style of ``_unsup_refs.py``.

``crop_ref`` resamples by the explicit formula in float64 from the fp32 coordinates (``xs = (float(u) +
0.5) * rx - 0.5`` is computed in fp32 exactly as the op sees it and then promoted, so no tap is
ambiguous).  ``loss_ref`` computes the per-iteration sums and the gradient by the explicit formulas --
no autograd -- in float64.  ``step_ref`` composes the trainer's target, weight and loss from a teacher
flow, the teacher's plane T, the student's plane S and the student's predictions.

Each ``check_*`` takes an *implementation*: an object whose methods map CPU tensors to CPU tensors.
The GPU tests pass the HIP kernels, the CPU tests the fp32 golden op and an fp32 emulation of the
kernels' operation order (the tolerances are attainable) and wrong variants (they are not vacuous).

Tolerances (derived, not measured), u = 2^-24 the fp32 unit roundoff, U = 2^-16 = 256 u as in
``_train_refs``:

* ``d = pred - target`` is ONE correctly rounded fp32 subtraction of fp32 inputs: ``|dd| <= u |d|``,
  relative to d itself, whatever the magnitudes of pred and target.
* ``rho(d) = sqrt(d^2 + eps^2)`` is 1-Lipschitz in d, so the error of d moves it by at most
  ``u |d| <= u rho``; the square, the sum and the root add a relative u, u and u / 2 + u, and
  ``eps^2`` (fp32 eps, one product: relative 3 u against the fp64 eps) moves rho by at most
  ``1.5 u rho``: ``|d rho| <= 6 u rho``, and for ``e = rho(d.x) + rho(d.y)``: ``|de| <= 7 u e``.
  A term ``weight * e`` adds one product: ``8 u weight e``.  A sum of terms is accumulated in fp32 per
  thread, wave and block and in fp64 after that; every term is >= 0, so ``tol = U sum(terms)``
  covers the accumulation's few-hundred-term fp32 chains with a wide margin.
* ``rho'(d) = d / sqrt(d^2 + eps^2)``: ``|rho'| <= 1`` and ``|d| |d rho'/dd| = x / (1 + x^2)^1.5 <=
  0.385`` (x = d / eps), so the relative error u of d moves rho' by at most ``0.385 u``; eps^2's
  relative 3 u moves it by ``1.5 u x / (1 + x^2)^1.5 <= 0.58 u``; the root's operand, the root and
  the quotient add ``(u + u) / 2 + u + u = 3 u`` relative to ``|rho'|``; the products with the
  weight and the scale two more: ``|d grad| <= |scale| weight u (0.97 + 5 |rho'|)``.  The tolerance
  is ``|scale| weight 8 u (0.25 + |rho'|)``, which is at least that bound.  Where ``d = 0`` the
  gradient is exactly 0, where ``weight = 0`` exactly 0 (checked bitwise).
* Counts and the sum of 0/1 weights are integers below 2^24 per block: exact.
* ``crop_resize`` is checked bitwise between the kernel and the golden op; against ``crop_ref`` the
  blend ``t + wy (b - t)`` carries a few u of ``tB + wy (bB + tB)``, ``tB = |c00| + wx (|c01| + |c00|)``
  (every term replaced by its magnitude), times ``|scale|``: ``tol = U`` times that bound.
* ``step_ref``: the target's error ``dt <= U tB`` moves a term by at most ``weight (dt.x + dt.y)`` (rho is
  1-Lipschitz), the weight's error ``dw <= U T'B (1 - S)`` by ``dw e``; with the term's own ``8 u
  weight e``: ``tol = U sum_i gamma^(N-1-i) sum [weight (tB.x + tB.y + e) + T'B (1 - S) e] / P``.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

from _train_refs import U_ACC, _gen, bits_equal, ratio, report

U32 = 2.0 ** -24
U_GRAD = 8 * U32
SELFSUP_ROUND = 1024 * 256 * 2   # pixels per grid-stride round of selfsup_loss_kernel (GRID_X * BLOCK * 2)
SELFSUP_BLOCK = 256
EPS = 0.001
NAN = float("nan")

# (B, H, W, c): the issue's two CPU cases; the GPU adds one with several blocks per row
CROP_CASES = [(1, 5, 7, 1), (2, 37, 53, 4)]
CROP_CASES_GPU = CROP_CASES + [(1, 130, 259, 16)]
# (N, B, H, W, weight, Btot, B0): weight in none | frac | zero; N = 5 is a ragged group of iterations (4 per
# block); odd and even pixel counts (the 16-byte and the 8-byte path); a window inside a larger stack; more
# than one grid-stride round
LOSS_CASES = [(1, 1, 1, 1, "frac", 1, 0), (1, 1, 1, 1, "none", 1, 0), (5, 1, 37, 53, "frac", 1, 0),
              (5, 2, 37, 53, "none", 2, 0), (32, 3, 12, 10, "frac", 3, 0), (5, 2, 37, 53, "zero", 2, 0),
              (5, 2, 12, 10, "frac", 5, 2), (3, 1, 37, 53, "frac", 4, 3), (1, 1, 600, 900, "frac", 1, 0)]
assert 600 * 900 > SELFSUP_ROUND
LOSS_CASES_CPU = LOSS_CASES[:-1]
ZERO_AT = (0, 0, 0)        # (b, y, x): pred == target there in every iteration, weight > 0
NAN_CASE = (5, 2, 12, 10, "frac", 2, 0)
NAN_TARGET_AT = (1, 3, 4)  # weight 0 and a NaN target: contributes nothing
NAN_PRED_AT = (2, 0, 7, 5)  # (iteration, b, y, x): weight 0 and a NaN prediction: a NaN sum, a NaN gradient there only


def blocks_expected(P: int) -> int:
    return min(SELFSUP_ROUND // (2 * SELFSUP_BLOCK), ((P + 1) // 2 + SELFSUP_BLOCK - 1) // SELFSUP_BLOCK)


# ------------------------------------------------------------------ crop_resize
def ratios(H, W, c):
    return np.float32((W - 2 * c) / W), np.float32((H - 2 * c) / H)


def axis32(n: int, nc: int, r):
    """One axis in fp32 as the op computes it: tap indices (inside the crop) and the fp64 weight."""
    s = (torch.arange(n, dtype=torch.float32) + 0.5) * float(r) - 0.5
    s = s.clamp(0.0, float(nc - 1))
    f = torch.floor(s)
    i0 = f.long()
    return i0, (i0 + 1).clamp(max=nc - 1), (s - f).double()


def crop_ref(x: torch.Tensor, c: int, scale=None):
    """fp64 (value, magnitude bound) of crop_resize(x, c, scale)."""
    B, H, W, C = x.shape
    rx, ry = ratios(H, W, c)
    x0, x1, wx = axis32(W, W - 2 * c, rx)
    y0, y1, wy = axis32(H, H - 2 * c, ry)
    wx, wy = wx.view(1, 1, W, 1), wy.view(1, H, 1, 1)
    X = x.double()
    tap = lambda yy, xx: X[:, c + yy][:, :, c + xx]
    c00, c01, c10, c11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    t, b = c00 + wx * (c01 - c00), c10 + wx * (c11 - c10)
    tB, bB = c00.abs() + wx * (c01.abs() + c00.abs()), c10.abs() + wx * (c11.abs() + c10.abs())
    v, vB = t + wy * (b - t), tB + wy * (bB + tB)
    if scale is not None:
        s = torch.tensor([float(np.float32(k)) for k in scale], dtype=torch.float64)
        v, vB = v * s, vB * s.abs()
    return v, vB


def crop_input(case, C, seed=0):
    B, H, W, c = case
    return torch.randn(B, H, W, C, generator=_gen(4100 + H + 3 * W + C + seed)) * 3.0


# ------------------------------------------------------------------ the loss
@functools.lru_cache(maxsize=None)
def loss_inputs(case, nan=False):
    N, B, H, W, wkind, Btot, B0 = case
    gen = _gen(5200 + 3 * N + 7 * H + W + Btot + B0)
    stack = (4.0 * torch.randn(N, Btot, H, W, 2, generator=gen)).contiguous()
    target = (4.0 * torch.randn(B, H, W, 2, generator=gen)).contiguous()
    idx = torch.arange(B * H * W)
    # near the target (|d| around eps, where rho' is steep), far from it, and exactly on it
    win = stack[:, B0:B0 + B]
    near = (idx % 3 == 1).view(B, H, W)
    win[:, near] = target[near] + 0.003 * torch.randn(N, int(near.sum()), 2, generator=gen)
    win[:, idx.view(B, H, W) % 11 == 5] *= 100.0
    b, y, x = ZERO_AT
    win[:, b, y, x] = target[b, y, x]
    weight = None
    if wkind == "frac":
        weight = torch.rand(B, H, W, generator=gen)
        weight.view(-1)[idx % 5 == 2] = 0.0
        weight.view(-1)[idx % 7 == 3] = 1.0
        weight[b, y, x] = 0.75
    elif wkind == "zero":
        weight = torch.zeros(B, H, W)
    if nan:
        tb, ty, tx = NAN_TARGET_AT
        target[tb, ty, tx, 1] = NAN
        weight[tb, ty, tx] = 0.0
        i, pb, py, px = NAN_PRED_AT
        stack[i, B0 + pb, py, px, 0] = NAN
        weight[pb, py, px] = 0.0
    scale = ((torch.arange(N, dtype=torch.float32) * 0.13 + 0.37) / 1024.0).contiguous()
    return NS(N=N, B=B, H=H, W=W, P=B * H * W, Btot=Btot, B0=B0, stack=stack, target=target, weight=weight,
              scale=scale, nan=nan)


def loss_formulas(pred, target, weight, eps, scale=None):
    """fp64 by the explicit formulas: sums (N, 4), and with ``scale`` the gradient and |rho'| per component."""
    N, B, H, W, _ = pred.shape
    p = pred.double()
    w = torch.ones(B, H, W, dtype=torch.float64) if weight is None else weight.double()
    on = w > 0
    t = torch.where(on.unsqueeze(-1), target.double(), torch.zeros((), dtype=torch.float64))
    d = p - t
    r = torch.sqrt(d * d + eps * eps)
    term = torch.where(on, w * (r[..., 0] + r[..., 1]), 0.0 * (p[..., 0] + p[..., 1]))
    sums = torch.zeros(N, 4, dtype=torch.float64)
    sums[:, 0] = term.flatten(1).sum(1)
    sums[-1, 1], sums[-1, 2], sums[-1, 3] = sums[-1, 0], w[on].sum(), float(on.sum())
    if scale is None:
        return sums
    dr = d / r
    s = scale.double().view(N, 1, 1, 1, 1)
    grad = torch.where(on.unsqueeze(-1), s * w.unsqueeze(-1) * dr, 0.0 * p)
    tol = torch.where(on.unsqueeze(-1), s.abs() * w.unsqueeze(-1) * U_GRAD * (0.25 + dr.abs()), torch.zeros_like(p))
    return sums, grad, tol


@functools.lru_cache(maxsize=None)
def loss_ref(case, nan=False):
    c = loss_inputs(case, nan)
    sums, grad, tol = loss_formulas(c.stack[:, c.B0:c.B0 + c.B], c.target, c.weight, EPS, c.scale)
    return NS(sums=sums, grad=grad, tol=tol)


def check_loss(impl, case, nan=False):
    """impl.selfsup_loss(stack, target, weight, eps, B0) -> fp32 part [blocks, N, 4] (the implementation
    pre-fills its output with NaN, so unwritten elements show)."""
    c, ref = loss_inputs(case, nan), loss_ref(case, nan)
    name = f"selfsup_loss{case} nan={nan}"
    part = impl.selfsup_loss(c.stack, c.target, c.weight, EPS, c.B0)
    assert part.dtype == torch.float32 and part.shape[1:] == (c.N, 4), part.shape
    if getattr(impl, "blocks", True):
        assert part.shape[0] == blocks_expected(c.P)
    assert bits_equal(part, impl.selfsup_loss(c.stack, c.target, c.weight, EPS, c.B0)), f"{name}: two identical calls differ"
    s = part.double().sum(0)
    worst = 0.0
    for i in range(c.N):
        if nan and i == NAN_PRED_AT[0]:
            assert torch.isnan(ref.sums[i, 0]) and torch.isnan(s[i, 0]), f"{name}: the NaN did not reach iteration {i}'s sum"
            continue
        assert bool(torch.isfinite(ref.sums[i]).all()) and bool(torch.isfinite(s[i]).all()), f"{name}: iteration {i}"
        for q in (0, 1, 2):
            worst = max(worst, ratio(s[i, q], ref.sums[i, q], U_ACC * ref.sums[i, q].abs()))
    assert int(torch.isnan(ref.sums[:, 0]).sum()) == (1 if nan else 0)
    assert torch.equal(s[:, 3], ref.sums[:, 3]), f"{name}: counts {s[:, 3].tolist()} != {ref.sums[:, 3].tolist()}"
    assert bool((part[:, :-1, 1:] == 0).all()), f"{name}: columns 1-3 belong to the last iteration only"
    assert bits_equal(part[:, -1, 1], part[:, -1, 0])
    report(name + " sums", worst)
    assert worst <= 1.0, f"{name}: error / tolerance = {worst}"


def check_loss_bwd(impl, case, nan=False):
    """impl.selfsup_loss_bwd(stack, target, weight, eps, scale, B0) -> fp32 grad [N, B, H, W, 2]."""
    c, ref = loss_inputs(case, nan), loss_ref(case, nan)
    name = f"selfsup_loss_bwd{case} nan={nan}"
    grad = impl.selfsup_loss_bwd(c.stack, c.target, c.weight, EPS, c.scale, c.B0)
    assert grad.dtype == torch.float32 and grad.shape == (c.N, c.B, c.H, c.W, 2)
    assert bits_equal(grad, impl.selfsup_loss_bwd(c.stack, c.target, c.weight, EPS, c.scale, c.B0)), f"{name}: two calls differ"
    finite = torch.isfinite(ref.grad)
    if nan:
        i, b, y, x = NAN_PRED_AT
        assert not bool(finite[i, b, y, x, 0]) and int((~finite).sum()) == 1     # that component only
        assert not bool(torch.isfinite(grad[i, b, y, x, 0])), f"{name}: finite gradient at the NaN prediction"
    else:
        assert bool(finite.all())
    assert torch.equal(torch.isfinite(grad), finite), f"{name}: non-finite elements differ from the reference's"
    r = ratio(grad, ref.grad, ref.tol, finite)
    report(name, r)
    assert r <= 1.0, f"{name}: error / tolerance = {r}"
    # exact zeros: without weight, and where the prediction is the target
    if c.weight is not None:
        off = (c.weight <= 0).unsqueeze(0).unsqueeze(-1).expand_as(grad) & finite
        assert bool((grad[off] == 0).all()), f"{name}: a gradient under weight 0"
    b, y, x = ZERO_AT
    if c.weight is None or float(c.weight[b, y, x]) > 0:
        assert bool((grad[:, b, y, x] == 0).all()), f"{name}: d = 0 must give gradient 0"
    big = finite & (ref.grad.abs() > 0)
    if c.P >= 1000 and bool(big.any()):   # not vacuous: the tolerance is far below the gradient itself
        assert float((ref.tol[big] / ref.grad.abs()[big]).median()) < 1e-5


# ------------------------------------------------------------------ the step's composition
STEP_CASE = (3, 2, 37, 53, 4)   # N, B2 (= 2B stacked pairs), H, W, c
GAMMA = 0.8


@functools.lru_cache(maxsize=None)
def step_inputs():
    N, B2, H, W, c = STEP_CASE
    gen = _gen(6300)
    ys, xs = torch.arange(H, dtype=torch.float32).view(1, H, 1), torch.arange(W, dtype=torch.float32).view(1, 1, W)
    teacher = torch.stack([3.0 * torch.sin(0.1 * xs + 0.05 * ys) + 0.3 * torch.randn(B2, H, W, generator=gen),
                           2.0 * torch.cos(0.07 * xs - 0.09 * ys) + 0.3 * torch.randn(B2, H, W, generator=gen)], -1)
    T = (torch.rand(B2, H, W, generator=gen) > 0.25).float()
    S = (torch.rand(B2, H, W, generator=gen) > 0.5).float()
    preds = 3.0 * torch.randn(N, B2, H, W, 2, generator=gen)
    return NS(N=N, B2=B2, H=H, W=W, c=c, teacher=teacher.contiguous(), T=T, S=S, preds=preds.contiguous())


@functools.lru_cache(maxsize=None)
def step_ref():
    """fp64 (loss, tolerance, target, weight) of the trainer's composition."""
    s = step_inputs()
    H, W, c = s.H, s.W, s.c
    scale = (np.float32(W / (W - 2 * c)), np.float32(H / (H - 2 * c)))
    target, tB = crop_ref(s.teacher, c, scale)
    Tc, TcB = crop_ref(s.T.unsqueeze(-1), c)
    Tc, TcB = Tc.squeeze(-1), TcB.squeeze(-1)
    weight = Tc * (1.0 - s.S.double())
    on = weight > 0
    P = s.B2 * H * W
    loss, tol = 0.0, 0.0
    for i in range(s.N):
        d = s.preds[i].double() - target
        e = torch.sqrt(d * d + EPS * EPS).sum(-1)
        g = GAMMA ** (s.N - 1 - i)
        loss += g * float((weight * e)[on].sum()) / P
        tol += U_ACC * g * float((weight * (tB.sum(-1) + e) + TcB * (1.0 - s.S.double()) * e).sum()) / P
    return NS(loss=loss, tol=tol, target=target, weight=weight)


def check_step(impl):
    """impl.step_loss(teacher, T, S, preds, c, gamma, eps) -> the self-supervision loss, a scalar."""
    s, ref = step_inputs(), step_ref()
    got = float(impl.step_loss(s.teacher, s.T, s.S, s.preds, s.c, GAMMA, EPS))
    r = abs(got - ref.loss) / ref.tol
    report("selfsup step", r)
    assert ref.tol < 1e-3 * abs(ref.loss)                  # not vacuous
    assert r <= 1.0, f"selfsup step: loss {got} vs {ref.loss}, error / tolerance = {r}"
