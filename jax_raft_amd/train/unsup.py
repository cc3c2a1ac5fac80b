"""Label-free training loss: photometric + edge-aware smoothness on every iteration's prediction
(SMURF, Stone et al. 2021: the sequence weights ``gamma^(N-i-1)`` applied to an unsupervised loss;
the constant penalty on pixels without a photometric term is UnFlow's, Meister et al. 2018).

``unsup_loss_reference`` is the golden op: plain differentiable torch ops, the CPU path and every
test's oracle.  ``unsup_loss`` is the front end: GPU tensors with N <= 32 run the two kernels of
``csrc/kernels/unsup.hip`` behind an autograd function, everything else the golden op.

For iteration i and pixel (y, x) with ``f = flow_preds[i, b, y, x]`` (P = B H W):

1. Coordinates, in fp32 whatever the input's precision, as ``models/reference.py:warp_frames``
   steps 1-2: ``px = float(x) + f.x``, ``py = float(y) + f.y``; ``inside`` iff ``0 <= px <= W-1``
   and ``0 <= py <= H-1`` (NaN fails); ``x0 = floor(px)``, ``x1 = min(x0+1, W-1)``,
   ``wx = px - x0``, y likewise.  The gradient flows through ``wx`` and ``wy`` (d wx / d f.x = 1),
   not through the floor.
2. ``v_c = t + wy (b - t)``, ``t = c00 + wx (c01 - c00)``, ``b = c10 + wx (c11 - c10)`` on image2's
   four texels per channel.
3. ``d_c = v_c - image1_c``, ``rho(d) = sqrt(d^2 + eps^2)``, ``pix = mean_c rho(d_c)`` where inside;
   elsewhere the pixel pays the constant ``out_penalty`` and gives no gradient (a flow that points
   off the frame must not be free).  A non-finite f makes its pixel's term NaN, whatever the mask.
   ``photo_i = sum(mask pix) / P``.
4. ``a_x(y, x) = exp(-edge_kappa mean_c |image1(y, x+1) - image1(y, x)|)`` for x < W-1, ``a_y``
   likewise between rows; ``smooth_i = [sum a_x sum_k rho_s(f_k(y, x+1) - f_k(y, x)) + sum a_y
   sum_k rho_s(f_k(y+1, x) - f_k(y, x))] / (2P)`` over all pixels whatever the mask,
   ``rho_s(d) = sqrt(d^2 + eps_s^2)``.  H = 1 or W = 1 has no pairs on that axis.
5. ``loss = sum_i gamma^(N-i-1) (photo_i + smooth_weight smooth_i)``.  Metrics (detached, last
   iteration): ``photo`` the mean of pix over the inside masked pixels (NaN without any),
   ``smooth`` = smooth_{N-1}, ``inside`` the share of the masked pixels (all pixels without a
   mask) that are inside.

The default parameter values are placeholders: this repository ships no data to tune them on.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

DEFAULTS = dict(gamma=0.8, eps=0.01, eps_s=0.001, edge_kappa=10.0, smooth_weight=0.05, out_penalty=0.5)
MAX_NATIVE_N = 32


def _check(flow_preds, image1, image2, mask):
    if flow_preds.ndim != 5 or flow_preds.shape[-1] != 2 or not flow_preds.is_floating_point():
        raise ValueError(f"unsup_loss: flow_preds must be (N, B, H, W, 2) floating point, got {tuple(flow_preds.shape)} "
                         f"{flow_preds.dtype}")
    N, B, H, W, _ = flow_preds.shape
    if N < 1 or B < 1 or H < 1 or W < 1:
        raise ValueError(f"unsup_loss: empty flow_preds {tuple(flow_preds.shape)}")
    for name, t in (("image1", image1), ("image2", image2)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, H, W, 3) or not t.is_floating_point():
            raise ValueError(f"unsup_loss: {name} must be {(B, H, W, 3)} floating point, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else t} {getattr(t, 'dtype', '')}")
        if t.device != flow_preds.device:
            raise ValueError(f"unsup_loss: {name} is on {t.device}, flow_preds on {flow_preds.device}")
    if mask is not None:
        if tuple(mask.shape) != (B, H, W):
            raise ValueError(f"unsup_loss: mask must be {(B, H, W)}, got {tuple(mask.shape)}")
        if mask.device != flow_preds.device:
            raise ValueError(f"unsup_loss: mask is on {mask.device}, flow_preds on {flow_preds.device}")
    return N, B, H, W


def edge_weights(image1: torch.Tensor, edge_kappa: float):
    """``(a_x (B, H, W-1), a_y (B, H-1, W))`` of step 4."""
    ax = torch.exp(-edge_kappa * (image1[:, :, 1:] - image1[:, :, :-1]).abs().mean(-1))
    ay = torch.exp(-edge_kappa * (image1[:, 1:] - image1[:, :-1]).abs().mean(-1))
    return ax, ay


def sample_image(flow: torch.Tensor, image2: torch.Tensor):
    """Steps 1-2 for one prediction (B, H, W, 2): ``(inside (B, H, W) bool, v (B, H, W, 3))`` in
    image2's dtype; v is differentiable in the flow through wx and wy, and finite where not inside
    (it is sampled at the origin there)."""
    B, H, W, _ = flow.shape
    dev = flow.device
    f = flow.detach().float()                          # the coordinates are fp32 whatever the input is
    px = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W) + f[..., 0]
    py = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1) + f[..., 1]
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)   # NaN fails
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    pxs, pys = torch.where(inside, px, zero), torch.where(inside, py, zero)
    x0f, y0f = torch.floor(pxs), torch.floor(pys)
    # the fp32 values, and d wx / d f.x = d wy / d f.y = 1 where inside, in the flow's own precision
    # (the added term is an exact zero; a gradient routed through the fp32 cast would be rounded)
    g = flow.to(image2.dtype)
    slope = torch.where(inside.unsqueeze(-1), g - g.detach(), torch.zeros((), dtype=image2.dtype, device=dev))
    wx = ((pxs - x0f).to(image2.dtype) + slope[..., 0]).unsqueeze(-1)
    wy = ((pys - y0f).to(image2.dtype) + slope[..., 1]).unsqueeze(-1)
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    flat = image2.reshape(B, H * W, 3)

    def tap(yy, xx):
        idx = (yy * W + xx).reshape(B, H * W, 1).expand(-1, -1, 3)
        return torch.gather(flat, 1, idx).view(B, H, W, 3)

    c00, c01, c10, c11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    t = c00 + wx * (c01 - c00)
    b = c10 + wx * (c11 - c10)
    return inside, t + wy * (b - t)


def unsup_sums(flow_preds, image1, image2, mask=None, eps: float = 0.01, eps_s: float = 0.001, edge_kappa: float = 10.0,
               out_penalty: float = 0.5) -> torch.Tensor:
    """The sums the loss is assembled from, (N, 4), differentiable in ``flow_preds`` (columns 0, 1):
    ``sum(mask pix)``, the smoothness sum (before the division by 2P), the count of masked pixels
    that are not inside, and -- last iteration only, 0 elsewhere -- the sum of pix over the inside
    masked pixels.  fp64 inputs are computed in fp64 (the coordinates of step 1 stay fp32)."""
    N, B, H, W = _check(flow_preds, image1, image2, mask)
    cdt = torch.float64 if flow_preds.dtype == torch.float64 else torch.float32
    i1, i2 = image1.to(cdt), image2.to(cdt)
    on = torch.ones((B, H, W), dtype=torch.bool, device=flow_preds.device) if mask is None else mask >= 0.5
    m = on.to(cdt)
    ax, ay = edge_weights(i1, edge_kappa)
    rows = []
    for i in range(N):
        f = flow_preds[i].to(cdt)
        inside, v = sample_image(f, i2)
        pix_in = torch.sqrt((v - i1) ** 2 + eps * eps).mean(-1)
        pix = torch.where(inside, pix_in, out_penalty + 0.0 * (f[..., 0] + f[..., 1]))
        smooth = ((ax.unsqueeze(-1) * torch.sqrt((f[:, :, 1:] - f[:, :, :-1]) ** 2 + eps_s * eps_s)).sum()
                  + (ay.unsqueeze(-1) * torch.sqrt((f[:, 1:] - f[:, :-1]) ** 2 + eps_s * eps_s)).sum())
        sel = on & inside
        last = pix.detach()[sel].sum() if i == N - 1 else pix.new_zeros(())
        rows.append(torch.stack([(m * pix).sum(), smooth, (on & ~inside).sum().to(cdt), last]))
    return torch.stack(rows)


def _assemble(s: torch.Tensor, cnt, P: int, gamma: float, smooth_weight: float):
    """(N, 4) sums and the number of masked pixels -> (loss, [photo, smooth, inside], weights (N,))."""
    n = s.shape[0]
    w = (gamma ** torch.arange(n - 1, -1, -1, device=s.device, dtype=torch.float64)).to(s.dtype)
    loss = (w * (s[:, 0] / P + smooth_weight * (s[:, 1] / (2.0 * P)))).sum()
    nan = torch.full((), float("nan"), dtype=s.dtype, device=s.device)
    ins = cnt - s[-1, 2].detach()
    photo = torch.where(ins > 0, s[-1, 3].detach() / ins.clamp_min(1.0), nan)
    inside = torch.where(cnt > 0, ins / cnt.clamp_min(1.0), nan)
    return loss, torch.stack([photo, s[-1, 1].detach() / (2.0 * P), inside]), w


def _count(mask, P: int, device, dtype):
    if mask is None:
        return torch.full((), float(P), dtype=dtype, device=device)
    return (mask >= 0.5).sum().to(dtype)


def unsup_loss_reference(flow_preds, image1, image2, mask=None, gamma: float = 0.8, eps: float = 0.01,
                         eps_s: float = 0.001, edge_kappa: float = 10.0, smooth_weight: float = 0.05,
                         out_penalty: float = 0.5) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The golden op (module docstring).  flow_preds (N, B, H, W, 2), channel 0 = x, in pixels;
    image1 / image2 (B, H, W, 3) in [-1, 1]; mask (B, H, W), used where >= 0.5, or None."""
    s = unsup_sums(flow_preds, image1, image2, mask, eps, eps_s, edge_kappa, out_penalty)
    P = flow_preds[0].numel() // 2
    loss, mets, _ = _assemble(s, _count(mask, P, s.device, s.dtype), P, gamma, smooth_weight)
    return loss, {"photo": mets[0], "smooth": mets[1], "inside": mets[2]}


class _UnsupLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, image1, image2, mask, gamma, eps, eps_s, edge_kappa, smooth_weight, out_penalty):
        from ..ops import native as nat

        P = preds[0].numel() // 2
        prm = nat.unsup_params(eps, eps_s, edge_kappa, out_penalty, preds.device)
        part = nat.unsup_loss_partials(preds, image1, image2, mask, prm=prm)
        s = part.double().sum(0)                       # block order; the counts stay exact
        loss, mets, w = _assemble(s, _count(mask, P, preds.device, torch.float64), P, gamma, smooth_weight)
        scale = torch.stack([w / P, w * (smooth_weight / (2.0 * P))], dim=-1)
        ctx.save_for_backward(preds, image1, image2, mask, prm, scale)
        mets = mets.float()
        ctx.mark_non_differentiable(mets)
        return loss.float(), mets

    @staticmethod
    def backward(ctx, gl, _gm):
        from ..ops import native as nat

        preds, image1, image2, mask, prm, scale = ctx.saved_tensors
        grad = nat.unsup_loss_grad(preds, image1, image2, mask, (scale * gl.double()).float().contiguous(), prm=prm)
        return (grad,) + (None,) * 9


def unsup_loss(flow_preds, image1, image2, mask=None, gamma: float = 0.8, eps: float = 0.01, eps_s: float = 0.001,
               edge_kappa: float = 10.0, smooth_weight: float = 0.05,
               out_penalty: float = 0.5) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``unsup_loss_reference`` for training: GPU tensors with N <= 32 run the native kernels
    (csrc/kernels/unsup.hip: the partial sums in one pass over the predictions, the gradient in one
    more, no host synchronisation, bitwise repeatable); everything else runs the golden op."""
    if not (flow_preds.is_cuda and flow_preds.shape[0] <= MAX_NATIVE_N and flow_preds.dtype != torch.float64):
        return unsup_loss_reference(flow_preds, image1, image2, mask, gamma, eps, eps_s, edge_kappa, smooth_weight,
                                    out_penalty)
    _check(flow_preds, image1, image2, mask)
    m = None if mask is None else mask.float().contiguous()
    loss, mets = _UnsupLoss.apply(flow_preds.float().contiguous(), image1.float().contiguous(),
                                  image2.float().contiguous(), m, float(gamma), float(eps), float(eps_s),
                                  float(edge_kappa), float(smooth_weight), float(out_penalty))
    return loss, {"photo": mets[0], "smooth": mets[1], "inside": mets[2]}
