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
4b. ``smooth_order=2`` (UFlow's and SMURF's choice on KITTI: a first-order penalty pulls slanted surfaces
   towards piecewise-constant flow, a second-order one leaves affine flow free) replaces step 4's sums:
   ``a2_x(y, x) = exp(-edge_kappa mean_c |image1(y, x+2) - image1(y, x)|)`` for x < W-2, the stride-2
   image difference across the triple, ``a2_y`` likewise between rows y and y+2;
   ``D2x_k(y, x) = (f_k(y, x+2) - f_k(y, x+1)) - (f_k(y, x+1) - f_k(y, x))``, ``D2y_k`` likewise down a
   column; ``smooth_i = [sum a2_x sum_k rho_s(D2x_k) + sum a2_y sum_k rho_s(D2y_k)] / (2P)`` over all
   pixels whatever the mask, with step 4's ``rho_s``, normalisation and ``smooth_weight``.  A triple never
   crosses a row end, a frame end or a sample boundary: W < 3 has no triples on the x axis, H < 3 none on
   the y axis.
5. ``loss = sum_i gamma^(N-i-1) (photo_i + smooth_weight smooth_i)``.  Metrics (detached, last
   iteration): ``photo`` the mean of pix over the inside masked pixels (NaN without any),
   ``smooth`` = smooth_{N-1} of the order in use, ``inside`` the share of the masked pixels (all pixels without a
   mask) that are inside.

``photo="census"`` replaces steps 2-3 by the soft census term of UnFlow / SMURF (SMURF's constants,
module constants here: a 7x7 patch, 0.81, 0.1, 0.01, 0.4), which compares the local ordering of
intensities, not the colours, and so survives exposure, shadow and compression changes:

2c. Grey planes in 8-bit levels, once per call: ``g(img) = 127.5 ((0.299 r + 0.587 g) + 0.114 b)``,
    ``G1 = g(image1)``, ``G2 = g(image2)``.  The landing point is clamped instead of tested:
    ``pxc = min(px >= 0 ? px : 0, W-1)`` (NaN becomes 0), ``x0 = floor(pxc)``, ``x1 = min(x0+1, W-1)``,
    ``wx = pxc - x0``, y alike, and ``w = t + wy (b - t)`` as in step 2 on G2: a pixel that lands outside
    has the border's grey.  The gradient flows through wx and wy only where ``inside``.
3c. ``tau(D) = D / sqrt(0.81 + D^2)``; over the 48 offsets d != 0 of the patch
    ``e_d = (tau(G1(p+d) - G1(p)) - tau(w(p+d) - w(p)))^2``, ``h(p) = sum_d e_d / (0.1 + e_d)``,
    ``cen(p) = (h(p) + 0.01)^0.4``.  ``valid(p)`` = inside(p) and the patch lies in the frame
    (3 <= x < W-3, 3 <= y < H-3).  The pixel's term is ``cen`` where valid, ``out_penalty`` where not
    inside (no gradient), 0 inside but in the border band; every pixel adds ``0 (f.x + f.y)``.
    ``photo_i = sum(mask term) / P``; the ``photo`` metric is the mean of cen over the valid masked
    pixels of the last iteration.  ``eps`` is not used.

The default parameter values are placeholders: this repository ships no data to tune them on.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

DEFAULTS = dict(gamma=0.8, eps=0.01, eps_s=0.001, edge_kappa=10.0, smooth_weight=0.05, out_penalty=0.5)
MAX_NATIVE_N = 32
PHOTO = ("charbonnier", "census")
SMOOTH_ORDERS = (1, 2)   # step 4 | step 4b
# the soft census term: SMURF's published constants, not configuration
CENSUS_R = 3           # 7x7 patch, 48 offsets
CENSUS_TAU = 0.81      # tau(D) = D / sqrt(0.81 + D^2)
CENSUS_K = 0.1         # k(e) = e / (0.1 + e)
CENSUS_H = 0.01        # cen = (h + 0.01)^0.4
CENSUS_POW = 0.4


def _check_photo(photo):
    if photo not in PHOTO:
        raise ValueError(f"unsup_loss: unknown photo {photo!r} (charbonnier or census)")


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


def census_gray(img: torch.Tensor) -> torch.Tensor:
    """Step 2c's grey plane (B, H, W) of an image (B, H, W, 3) in [-1, 1], in 8-bit levels."""
    return 127.5 * ((0.299 * img[..., 0] + 0.587 * img[..., 1]) + 0.114 * img[..., 2])


def sample_gray(flow: torch.Tensor, G2: torch.Tensor):
    """Step 2c for one prediction (B, H, W, 2): ``(inside (B, H, W) bool, w (B, H, W))`` in G2's dtype;
    w is differentiable in the flow through wx and wy where inside."""
    B, H, W, _ = flow.shape
    dev = flow.device
    f = flow.detach().float()                          # the coordinates are fp32 whatever the input is
    px = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W) + f[..., 0]
    py = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1) + f[..., 1]
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)   # NaN fails
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    pxc = torch.where(px >= 0, px, zero).clamp(max=W - 1)            # NaN -> 0
    pyc = torch.where(py >= 0, py, zero).clamp(max=H - 1)
    x0f, y0f = torch.floor(pxc), torch.floor(pyc)
    g = flow.to(G2.dtype)
    slope = torch.where(inside.unsqueeze(-1), g - g.detach(), torch.zeros((), dtype=G2.dtype, device=dev))
    wx = (pxc - x0f).to(G2.dtype) + slope[..., 0]
    wy = (pyc - y0f).to(G2.dtype) + slope[..., 1]
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    flat = G2.reshape(B, H * W)
    tap = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).reshape(B, H * W)).view(B, H, W)
    c00, c01, c10, c11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    t = c00 + wx * (c01 - c00)
    b = c10 + wx * (c11 - c10)
    return inside, t + wy * (b - t)


def census_patch(G1: torch.Tensor, w: torch.Tensor, radius: int = CENSUS_R) -> torch.Tensor:
    """Step 3c's ``cen`` on the pixels whose patch lies in the frame, (B, H - 2 radius, W - 2 radius)
    (H, W > 2 radius), by shifted slices."""
    B, H, W = G1.shape
    r = radius
    tau = lambda D: D / torch.sqrt(CENSUS_TAU + D * D)
    c1, cw = G1[:, r:H - r, r:W - r], w[:, r:H - r, r:W - r]
    h = torch.zeros_like(cw)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            n1, nw = G1[:, r + dy:H - r + dy, r + dx:W - r + dx], w[:, r + dy:H - r + dy, r + dx:W - r + dx]
            e = (tau(n1 - c1) - tau(nw - cw)) ** 2
            h = h + e / (CENSUS_K + e)
    return (h + CENSUS_H) ** CENSUS_POW


def census_sums(flow_preds, image1, image2, mask=None, out_penalty: float = 0.5) -> torch.Tensor:
    """The sums the census term is assembled from, (N, 4), differentiable in ``flow_preds`` (column
    0): ``sum(mask term)``, the count of masked pixels that are not inside, the count of masked
    pixels inside but in the border band and -- last iteration only, 0 elsewhere -- the sum of cen
    over the valid masked pixels.  fp64 inputs are computed in fp64 (the coordinates stay fp32)."""
    N, B, H, W = _check(flow_preds, image1, image2, mask)
    cdt = torch.float64 if flow_preds.dtype == torch.float64 else torch.float32
    G1, G2 = census_gray(image1.to(cdt)), census_gray(image2.to(cdt))
    dev = flow_preds.device
    on = torch.ones((B, H, W), dtype=torch.bool, device=dev) if mask is None else mask >= 0.5
    m = on.to(cdt)
    r = CENSUS_R
    geom = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
    if H > 2 * r and W > 2 * r:
        geom[:, r:H - r, r:W - r] = True
    zero = torch.zeros((), dtype=cdt, device=dev)
    rows = []
    for i in range(N):
        f = flow_preds[i].to(cdt)
        inside, w = sample_gray(f, G2)
        if H > 2 * r and W > 2 * r:
            cen = torch.nn.functional.pad(census_patch(G1, w), (r, r, r, r))
        else:
            cen = torch.zeros((B, H, W), dtype=cdt, device=dev)
        valid = inside & geom
        term = torch.where(valid, cen, torch.where(inside, zero, zero + out_penalty)) + 0.0 * (f[..., 0] + f[..., 1])
        sel = on & valid
        last = cen.detach()[sel].sum() if i == N - 1 else cen.new_zeros(())
        rows.append(torch.stack([(m * term).sum(), (on & ~inside).sum().to(cdt), (on & inside & ~geom).sum().to(cdt), last]))
    return torch.stack(rows)


def smooth_sums(flow_preds, image1, eps_s: float = 0.001, edge_kappa: float = 10.0) -> torch.Tensor:
    """Step 4's sums (before the division by 2P), (N,), differentiable in ``flow_preds``."""
    cdt = torch.float64 if flow_preds.dtype == torch.float64 else torch.float32
    ax, ay = edge_weights(image1.to(cdt), edge_kappa)
    rows = []
    for i in range(flow_preds.shape[0]):
        f = flow_preds[i].to(cdt)
        rows.append((ax.unsqueeze(-1) * torch.sqrt((f[:, :, 1:] - f[:, :, :-1]) ** 2 + eps_s * eps_s)).sum()
                    + (ay.unsqueeze(-1) * torch.sqrt((f[:, 1:] - f[:, :-1]) ** 2 + eps_s * eps_s)).sum())
    return torch.stack(rows)


def edge_weights2(image1: torch.Tensor, edge_kappa: float):
    """``(a2_x (B, H, W-2), a2_y (B, H-2, W))`` of step 4b; an axis shorter than 3 has none."""
    ax = torch.exp(-edge_kappa * (image1[:, :, 2:] - image1[:, :, :-2]).abs().mean(-1))
    ay = torch.exp(-edge_kappa * (image1[:, 2:] - image1[:, :-2]).abs().mean(-1))
    return ax, ay


def smooth2_sums(flow_preds, image1, eps_s: float = 0.001, edge_kappa: float = 10.0) -> torch.Tensor:
    """Step 4b's sums (before the division by 2P), (N, 2): over the triples along x and over the triples
    along y; differentiable in ``flow_preds``, computed in fp64 for fp64 input."""
    cdt = torch.float64 if flow_preds.dtype == torch.float64 else torch.float32
    ax, ay = edge_weights2(image1.to(cdt), edge_kappa)
    rows = []
    for i in range(flow_preds.shape[0]):
        f = flow_preds[i].to(cdt)
        dx = (f[:, :, 2:] - f[:, :, 1:-1]) - (f[:, :, 1:-1] - f[:, :, :-2])
        dy = (f[:, 2:] - f[:, 1:-1]) - (f[:, 1:-1] - f[:, :-2])
        rows.append(torch.stack([(ax.unsqueeze(-1) * torch.sqrt(dx ** 2 + eps_s * eps_s)).sum(),
                                 (ay.unsqueeze(-1) * torch.sqrt(dy ** 2 + eps_s * eps_s)).sum()]))
    return torch.stack(rows)


def _check_order(smooth_order):
    if isinstance(smooth_order, bool) or not isinstance(smooth_order, int) or smooth_order not in SMOOTH_ORDERS:
        raise ValueError(f"unsup_loss: unknown smooth_order {smooth_order!r} (1 or 2)")


def _census_columns(c: torch.Tensor, smooth: torch.Tensor):
    """Census sums (N, 4) and smoothness sums (N,) -> the (N, 4) layout of ``_assemble`` and the band count."""
    return torch.stack([c[:, 0], smooth, c[:, 1], c[:, 3]], dim=-1), c[-1, 2].detach()


def _assemble(s: torch.Tensor, cnt, P: int, gamma: float, smooth_weight: float, band=None):
    """(N, 4) sums and the number of masked pixels -> (loss, [photo, smooth, inside], weights (N,)).
    ``band`` (census): the last iteration's masked pixels inside but without a term of their own,
    left out of the photo metric's mean."""
    n = s.shape[0]
    w = (gamma ** torch.arange(n - 1, -1, -1, device=s.device, dtype=torch.float64)).to(s.dtype)
    loss = (w * (s[:, 0] / P + smooth_weight * (s[:, 1] / (2.0 * P)))).sum()
    nan = torch.full((), float("nan"), dtype=s.dtype, device=s.device)
    ins = cnt - s[-1, 2].detach()
    den = ins if band is None else ins - band
    photo = torch.where(den > 0, s[-1, 3].detach() / den.clamp_min(1.0), nan)
    inside = torch.where(cnt > 0, ins / cnt.clamp_min(1.0), nan)
    return loss, torch.stack([photo, s[-1, 1].detach() / (2.0 * P), inside]), w


def _count(mask, P: int, device, dtype):
    if mask is None:
        return torch.full((), float(P), dtype=dtype, device=device)
    return (mask >= 0.5).sum().to(dtype)


def unsup_loss_reference(flow_preds, image1, image2, mask=None, gamma: float = 0.8, eps: float = 0.01,
                         eps_s: float = 0.001, edge_kappa: float = 10.0, smooth_weight: float = 0.05,
                         out_penalty: float = 0.5, photo: str = "charbonnier",
                         smooth_order: int = 1) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The golden op (module docstring).  flow_preds (N, B, H, W, 2), channel 0 = x, in pixels;
    image1 / image2 (B, H, W, 3) in [-1, 1]; mask (B, H, W), used where >= 0.5, or None;
    photo: "charbonnier" (steps 2-3) | "census" (steps 2c-3c); smooth_order: 1 (step 4) | 2 (step 4b)."""
    _check_photo(photo)
    _check_order(smooth_order)
    P = flow_preds[0].numel() // 2
    band = None
    second = None if smooth_order == 1 else smooth2_sums(flow_preds, image1, eps_s, edge_kappa).sum(-1)
    if photo == "census":
        c = census_sums(flow_preds, image1, image2, mask, out_penalty)
        s, band = _census_columns(c, smooth_sums(flow_preds, image1, eps_s, edge_kappa) if second is None else second)
    else:
        s = unsup_sums(flow_preds, image1, image2, mask, eps, eps_s, edge_kappa, out_penalty)
        if second is not None:
            s = torch.stack([s[:, 0], second, s[:, 2], s[:, 3]], dim=-1)
    loss, mets, _ = _assemble(s, _count(mask, P, s.device, s.dtype), P, gamma, smooth_weight, band)
    return loss, {"photo": mets[0], "smooth": mets[1], "inside": mets[2]}


class _UnsupLoss(torch.autograd.Function):
    """Smoothness from the two kernels of csrc/kernels/unsup.hip; the photometric term from the same launches
    (``photo="charbonnier"``) or from csrc/kernels/census.hip, unsup.hip's then called with a zero photometric scale.
    ``smooth_order=2``: the smoothness from the two kernels of csrc/kernels/smooth2.hip, unsup.hip's called with a zero
    smoothness scale -- and not at all with ``photo="census"``, where they would carry nothing."""

    @staticmethod
    def forward(ctx, preds, image1, image2, mask, photo, smooth_order, gamma, eps, eps_s, edge_kappa, smooth_weight,
                out_penalty):
        from ..ops import native as nat

        P = preds[0].numel() // 2
        prm = nat.unsup_params(eps, eps_s, edge_kappa, out_penalty, preds.device)
        census, second = photo == "census", smooth_order == 2
        # sums in block (census: tile) order; the counts stay exact
        if not (census and second):
            s = nat.unsup_loss_partials(preds, image1, image2, mask, prm=prm).double().sum(0)
            smooth = s[:, 1]
        if second:
            smooth = nat.smooth2_loss_partials(preds, image1, prm=prm).double().sum(0)[:, :2].sum(-1)
            if not census:
                s = torch.stack([s[:, 0], smooth, s[:, 2], s[:, 3]], dim=-1)
        band = gray = coef = None
        if census:
            gray = nat.census_gray_planes(image1, image2)
            part, coef = nat.census_loss_partials(preds, image1, image2, mask, prm=prm, gray=gray)
            s, band = _census_columns(part.double().sum(0), smooth)
        loss, mets, w = _assemble(s, _count(mask, P, preds.device, torch.float64), P, gamma, smooth_weight, band)
        zero = torch.zeros_like(w)
        ws = w * (smooth_weight / (2.0 * P))
        # the backward's scales: unsup.hip's photometric and smoothness terms, census.hip's term, smooth2.hip's term
        scale = torch.stack([zero if census else w / P, zero if second else ws, w / P if census else zero], dim=-1)
        ctx.photo, ctx.smooth_order = photo, smooth_order
        ctx.save_for_backward(preds, image1, image2, mask, prm, scale, gray, coef, ws if second else None)
        mets = mets.float()
        ctx.mark_non_differentiable(mets)
        return loss.float(), mets

    @staticmethod
    def backward(ctx, gl, _gm):
        from ..ops import native as nat

        preds, image1, image2, mask, prm, scale, gray, coef, scale2 = ctx.saved_tensors
        scale = (scale * gl.double()).float()
        census, second = ctx.photo == "census", ctx.smooth_order == 2
        grad = None
        if not (census and second):
            grad = nat.unsup_loss_grad(preds, image1, image2, mask, scale[:, :2].contiguous(), prm=prm)
        if census:
            grad = nat.census_loss_grad(preds, image1, image2, mask, scale[:, 2].contiguous(), prm=prm, gray=gray, coef=coef,
                                        out=grad)
        if second:
            nat.smooth2_loss_grad(preds, image1, (scale2 * gl.double()).float(), prm=prm, out=grad)
        return (grad,) + (None,) * 11


def unsup_loss(flow_preds, image1, image2, mask=None, gamma: float = 0.8, eps: float = 0.01, eps_s: float = 0.001,
               edge_kappa: float = 10.0, smooth_weight: float = 0.05,
               out_penalty: float = 0.5, photo: str = "charbonnier",
               smooth_order: int = 1) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``unsup_loss_reference`` for training: GPU tensors with N <= 32 run the native kernels
    (csrc/kernels/unsup.hip: the partial sums in one pass over the predictions, the gradient in one
    more; ``photo="census"``: the tiled stencil kernels of csrc/kernels/census.hip for the
    photometric term; ``smooth_order=2``: the two kernels of csrc/kernels/smooth2.hip for the smoothness
    term; no host synchronisation, bitwise repeatable); everything else runs the golden op."""
    _check_photo(photo)
    _check_order(smooth_order)
    if not (flow_preds.is_cuda and flow_preds.shape[0] <= MAX_NATIVE_N and flow_preds.dtype != torch.float64):
        return unsup_loss_reference(flow_preds, image1, image2, mask, gamma, eps, eps_s, edge_kappa, smooth_weight,
                                    out_penalty, photo, smooth_order)
    _check(flow_preds, image1, image2, mask)
    m = None if mask is None else mask.float().contiguous()
    loss, mets = _UnsupLoss.apply(flow_preds.float().contiguous(), image1.float().contiguous(), image2.float().contiguous(), m,
                                  photo, int(smooth_order), float(gamma), float(eps), float(eps_s), float(edge_kappa),
                                  float(smooth_weight), float(out_penalty))
    return loss, {"photo": mets[0], "smooth": mets[1], "inside": mets[2]}
