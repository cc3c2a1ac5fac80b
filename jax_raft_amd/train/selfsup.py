"""Self-supervision for label-free training (UFlow, Jonschkowski et al. 2020; SMURF, Stone et al. 2021):
the model's own flow on the full frame (the "teacher", no gradient) supervises the same model on a
centre crop of the frames (the "student").  The student cannot see what lies beyond the crop, so it
learns to extrapolate flows that leave the frame -- the pixels where the photometric term of
``train/unsup.py`` has nothing to compare and pays only ``out_penalty``.

Golden ops (plain torch ops, the CPU path and every test's oracle; the kernels of
``csrc/kernels/selfsup.hip`` equal ``crop_resize`` bit for bit and the sums up to their order):

``crop_resize(x, c, scale)``, x (B, H, W, C), the centre crop ``[c, H-c) x [c, W-c)`` resampled
bilinearly back to H x W (the student's view of an image, a flow or a mask), fp32 operations each
rounded on its own:

1. ``Wc = W - 2c``, ``Hc = H - 2c``; ``rx = fp32(Wc / W)``, ``ry = fp32(Hc / H)``, computed in fp64
   and rounded once (:func:`crop_ratios`).
2. Output column u: ``xs = (float(u) + 0.5) * rx - 0.5``, clamped to ``[0, Wc - 1]``;
   ``x0 = floor(xs)``, ``x1 = min(x0 + 1, Wc - 1)``, ``wx = xs - x0``; the taps are the columns
   ``c + x0`` and ``c + x1``.  Rows alike with ry, Hc.  Nothing outside the crop is read.
3. ``v = t + wy (b - t)``, ``t = c00 + wx (c01 - c00)``, ``b = c10 + wx (c11 - c10)`` (so a plane of
   ones gives exactly 1.0).
4. Channel k is multiplied by ``scale[k]`` (fp32) after the blend.  For a flow the scale is
   :func:`flow_scale` ``= (fp32(W / Wc), fp32(H / Hc))``: a displacement in the student's pixels.

``selfsup_sums(flow_preds, target, weight, eps)``, flow_preds (N, B, H, W, 2), target (B, H, W, 2)
without gradient, weight (B, H, W) >= 0 or None (all ones); per iteration i and pixel:

1. ``d = pred - target``, ``e = sqrt(d.x^2 + eps^2) + sqrt(d.y^2 + eps^2)`` (the Charbonnier function
   per component).
2. The term is ``weight * e`` where ``weight > 0`` and ``0 * (pred.x + pred.y)`` elsewhere: a
   non-finite prediction poisons the sum whatever the weight, a non-finite target under weight 0
   contributes nothing.  The zero term is written ``(0 * p.x) p.x + (0 * p.y) p.y`` with the first
   factors detached: the same value, and a gradient ``0 * p`` that is exactly 0 at a finite prediction
   and NaN at a non-finite one (the trainer's guard reads the gradient norm, not the loss).
3. Row i of the result: ``(sum term, the same for i = N-1 else 0, sum weight for i = N-1, count of
   weight > 0 for i = N-1)``.

``selfsup_loss_reference``: ``loss = sum_i gamma^(N-1-i) sum(term_i) / P`` with ``P = B H W``, the count
of ALL pixels (not the weight sum: few selected pixels must mean a small loss, as in UFlow).
Metrics (detached, last iteration): ``selfsup`` = ``sum term / sum weight`` (NaN when that is 0),
``selfsup_w`` = the share of pixels with ``weight > 0``.

``selfsup_loss`` is the front end for training: GPU fp32 predictions with N <= 32 run the two loss
kernels behind an autograd function (a batch window ``preds[:, k:]`` of a contiguous stack is read in
place, without a copy), everything else the golden op.  No host synchronisation.

Not built, on purpose: a student with fewer iterations than the teacher, a separate (EMA or frozen)
teacher, a ramped weight, a "teacher only" mask or a thresholded teacher plane, random crop offsets,
SMURF's full-image warping and multi-frame training.  The default parameter values are placeholders.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_NATIVE_N = 32
MAX_CHANNELS = 4


def crop_ratios(H: int, W: int, c: int) -> Tuple[float, float]:
    """``(rx, ry) = (fp32(Wc / W), fp32(Hc / H))``: the division in fp64, rounded once."""
    return float(np.float32((W - 2 * c) / W)), float(np.float32((H - 2 * c) / H))


def flow_scale(H: int, W: int, c: int) -> Tuple[float, float]:
    """``(fp32(W / Wc), fp32(H / Hc))``: what a flow's channels are multiplied by in the student's frame."""
    return float(np.float32(W / (W - 2 * c))), float(np.float32(H / (H - 2 * c)))


def check_crop(x, c, scale=None) -> Tuple[int, int, int, int]:
    """The host checks of ``crop_resize`` -> (B, H, W, C)."""
    if not isinstance(x, torch.Tensor) or x.ndim != 4 or not x.is_floating_point():
        raise ValueError(f"crop_resize: x must be (B, H, W, C) floating point, got "
                         f"{tuple(x.shape) if isinstance(x, torch.Tensor) else x} {getattr(x, 'dtype', '')}")
    B, H, W, C = x.shape
    if B < 1 or H < 1 or W < 1 or not 1 <= C <= MAX_CHANNELS:
        raise ValueError(f"crop_resize: x must be (B, H, W, C) with 1 <= C <= {MAX_CHANNELS}, got {tuple(x.shape)}")
    if isinstance(c, bool) or not isinstance(c, int):
        raise ValueError(f"crop_resize: the margin c must be an int, got {c!r}")
    if c < 1 or 2 * c >= min(H, W):
        raise ValueError(f"crop_resize: the margin c = {c} must be at least 1 and 2 c below min(H, W) = {min(H, W)}")
    if scale is not None and len(scale) != C:
        raise ValueError(f"crop_resize: scale must hold C = {C} floats, got {len(scale)}")
    return B, H, W, C


def _axis(n: int, nc: int, r: float, device):
    s = (torch.arange(n, device=device, dtype=torch.float32) + 0.5) * r - 0.5     # every op rounded in fp32
    s = s.clamp(0.0, float(nc - 1))
    f = torch.floor(s)
    i0 = f.long()
    return i0, torch.clamp(i0 + 1, max=nc - 1), s - f


def crop_resize(x: torch.Tensor, c: int, scale: Optional[Sequence[float]] = None) -> torch.Tensor:
    """The golden op (module docstring): x (B, H, W, C) -> (B, H, W, C) in x's dtype."""
    B, H, W, C = check_crop(x, c, scale)
    rx, ry = crop_ratios(H, W, c)
    x0, x1, wx = _axis(W, W - 2 * c, rx, x.device)
    y0, y1, wy = _axis(H, H - 2 * c, ry, x.device)
    wx, wy = wx.to(x.dtype).view(1, 1, W, 1), wy.to(x.dtype).view(1, H, 1, 1)
    top, bot = x[:, c + y0], x[:, c + y1]                  # (B, H, W, C): rows of the crop
    c00, c01, c10, c11 = top[:, :, c + x0], top[:, :, c + x1], bot[:, :, c + x0], bot[:, :, c + x1]
    t = c00 + wx * (c01 - c00)
    b = c10 + wx * (c11 - c10)
    v = t + wy * (b - t)
    if scale is not None:
        v = v * torch.tensor([float(np.float32(s)) for s in scale], dtype=x.dtype, device=x.device)
    return v


def _check(flow_preds, target, weight) -> Tuple[int, int, int, int]:
    if (not isinstance(flow_preds, torch.Tensor) or flow_preds.ndim != 5 or flow_preds.shape[-1] != 2
            or not flow_preds.is_floating_point()):
        raise ValueError(f"selfsup_loss: flow_preds must be (N, B, H, W, 2) floating point, got "
                         f"{tuple(flow_preds.shape) if isinstance(flow_preds, torch.Tensor) else flow_preds} "
                         f"{getattr(flow_preds, 'dtype', '')}")
    N, B, H, W, _ = flow_preds.shape
    if N < 1 or B < 1 or H < 1 or W < 1:
        raise ValueError(f"selfsup_loss: empty flow_preds {tuple(flow_preds.shape)}")
    if not isinstance(target, torch.Tensor) or tuple(target.shape) != (B, H, W, 2) or not target.is_floating_point():
        raise ValueError(f"selfsup_loss: target must be {(B, H, W, 2)} floating point, got "
                         f"{tuple(target.shape) if isinstance(target, torch.Tensor) else target} {getattr(target, 'dtype', '')}")
    if target.requires_grad:
        raise ValueError("selfsup_loss: the target takes no gradient (detach the teacher's flow)")
    if target.device != flow_preds.device:
        raise ValueError(f"selfsup_loss: target is on {target.device}, flow_preds on {flow_preds.device}")
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or tuple(weight.shape) != (B, H, W) or not weight.is_floating_point():
            raise ValueError(f"selfsup_loss: weight must be {(B, H, W)} floating point, got "
                             f"{tuple(weight.shape) if isinstance(weight, torch.Tensor) else weight}")
        if weight.device != flow_preds.device:
            raise ValueError(f"selfsup_loss: weight is on {weight.device}, flow_preds on {flow_preds.device}")
    return N, B, H, W


def selfsup_sums(flow_preds, target, weight=None, eps: float = 0.001) -> torch.Tensor:
    """The sums the loss is assembled from, (N, 4), differentiable in ``flow_preds`` (column 0; module
    docstring).  fp64 predictions are computed in fp64."""
    N, B, H, W = _check(flow_preds, target, weight)
    cdt = torch.float64 if flow_preds.dtype == torch.float64 else torch.float32
    dev = flow_preds.device
    w = torch.ones((B, H, W), dtype=cdt, device=dev) if weight is None else weight.detach().to(cdt)
    on = w > 0
    zero = torch.zeros((), dtype=cdt, device=dev)
    # a target without weight is never used (it may be non-finite: torch.where alone would still pass
    # its NaN into the gradient)
    tgt = torch.where(on.unsqueeze(-1), target.detach().to(cdt), zero)
    wsum, cnt = torch.where(on, w, zero).sum(), on.sum().to(cdt)
    rows = []
    for i in range(N):
        p = flow_preds[i].to(cdt)
        d = p - tgt
        e = torch.sqrt(d[..., 0] ** 2 + eps * eps) + torch.sqrt(d[..., 1] ** 2 + eps * eps)
        off = ((0.0 * p.detach()) * p).sum(-1)             # 0 * (p.x + p.y), gradient 0 * p
        total = torch.where(on, w * e, off).sum()
        last = i == N - 1
        rows.append(torch.stack([total, total.detach() if last else zero, wsum if last else zero, cnt if last else zero]))
    return torch.stack(rows)


def _assemble(s: torch.Tensor, P: int, gamma: float):
    """(N, 4) sums -> (loss, [selfsup, selfsup_w], weights (N,))."""
    n = s.shape[0]
    w = (gamma ** torch.arange(n - 1, -1, -1, device=s.device, dtype=torch.float64)).to(s.dtype)
    loss = (w * (s[:, 0] / P)).sum()
    nan = torch.full((), float("nan"), dtype=s.dtype, device=s.device)
    wsum = s[-1, 2].detach()
    mean = torch.where(wsum > 0, s[-1, 1].detach() / torch.where(wsum > 0, wsum, torch.ones_like(wsum)), nan)
    return loss, torch.stack([mean, s[-1, 3].detach() / P]), w


def selfsup_loss_reference(flow_preds, target, weight=None, gamma: float = 0.8,
                           eps: float = 0.001) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The golden op (module docstring): ``(loss, {"selfsup", "selfsup_w"})``."""
    s = selfsup_sums(flow_preds, target, weight, eps)
    loss, mets, _ = _assemble(s, flow_preds[0].numel() // 2, gamma)
    return loss, {"selfsup": mets[0], "selfsup_w": mets[1]}


def batch_window(x: torch.Tensor):
    """``(stack, B0)`` when the (N, B, H, W, 2) tensor x is the batches ``[B0, B0 + B)`` of a contiguous
    stack (N, Btot, H, W, 2) -- itself, or the tensor it is a view of -- so that the kernels can read it
    in place; None otherwise (the caller then copies)."""
    if x.is_contiguous():
        return x, 0
    N, B, H, W, _ = x.shape
    base = x._base
    if base is None or base.ndim != 5 or not base.is_contiguous() or base.dtype != x.dtype:
        return None
    if base.shape[0] != N or tuple(base.shape[2:]) != (H, W, 2) or x.stride() != base.stride():
        return None
    off, per = x.storage_offset() - base.storage_offset(), H * W * 2
    if off < 0 or off % per or off // per + B > base.shape[1]:
        return None
    return base.detach(), off // per


class _SelfsupLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, target, weight, gamma, eps):
        from ..ops import native as nat

        N, B, H, W, _ = preds.shape
        P = B * H * W
        win = batch_window(preds)
        stack, b0 = win if win is not None else (preds.contiguous(), 0)
        prm = nat.selfsup_params(eps, preds.device)
        part = nat.selfsup_loss_partials(stack, target, weight, prm=prm, batch0=b0)
        s = part.double().sum(0)                           # block order; the counts stay exact
        loss, mets, w = _assemble(s, P, gamma)
        ctx.save_for_backward(stack, target, weight, prm, w / P)
        ctx.b0 = b0
        mets = mets.float()
        ctx.mark_non_differentiable(mets)
        return loss.float(), mets

    @staticmethod
    def backward(ctx, gl, _gm):
        from ..ops import native as nat

        stack, target, weight, prm, scale = ctx.saved_tensors
        grad = nat.selfsup_loss_grad(stack, target, weight, (scale * gl.double()).float().contiguous(), prm=prm,
                                     batch0=ctx.b0)
        return grad, None, None, None, None


def selfsup_loss(flow_preds, target, weight=None, gamma: float = 0.8,
                 eps: float = 0.001) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``selfsup_loss_reference`` for training: GPU fp32 predictions with N <= 32 run the native kernels
    (csrc/kernels/selfsup.hip: the partial sums in one pass over the predictions, the gradient in one
    more; no host synchronisation, bitwise repeatable); everything else runs the golden op."""
    if not (flow_preds.is_cuda and flow_preds.dtype == torch.float32 and flow_preds.shape[0] <= MAX_NATIVE_N):
        return selfsup_loss_reference(flow_preds, target, weight, gamma, eps)
    _check(flow_preds, target, weight)
    w = None if weight is None else weight.detach().float().contiguous()
    loss, mets = _SelfsupLoss.apply(flow_preds, target.detach().float().contiguous(), w, float(gamma), float(eps))
    return loss, {"selfsup": mets[0], "selfsup_w": mets[1]}
