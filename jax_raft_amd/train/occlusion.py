"""Occlusion estimates for label-free training: which pixels of one frame have a counterpart in the
other, from a forward and a backward flow.  A pixel covered in the other frame has no counterpart,
and a photometric term on it pulls its flow towards whatever happens to look similar, so the loss
(``train/unsup.py``, its ``mask`` argument) leaves such pixels out.

Two estimates, both golden ops -- fixed sequences of operations that the kernels equal bit for bit:

* ``kind="fb"``: forward-backward consistency (UnFlow, Meister et al. 2018; ``models/reference.py:
  fb_consistency``).  It needs flows that are already good.
* ``kind="range"``: the range map of Wang et al. 2018 -- splat every pixel of the other frame along
  its flow and count how much lands on each pixel; a pixel that nothing maps onto is occluded.  UFlow
  (Jonschkowski et al. 2020) and SMURF use it early in training, when forward-backward consistency
  does not mean anything yet.

``range_map`` for the source pixel (y, x) with ``f = flow[b, y, x]``:

1. ``px = float(x) + f.x``, ``py = float(y) + f.y``, one fp32 add each.  The source contributes iff
   ``-1 < px < W`` and ``-1 < py < H`` (float comparisons: NaN and +-inf fail).
2. ``x0 = floor(px)``, ``qx = int(rint((px - x0) * 16))`` (ties to even, in [0, 16]); y likewise.
3. The four taps ``(x0 + dx, y0 + dy)``, dx, dy in {0, 1}, have the integer weights
   ``(dx ? qx : 16 - qx) * (dy ? qy : 16 - qy)``: 256 per source, units of 1/256 of a pixel.
4. A tap is added to ``acc[b, ty, tx]`` iff ``0 <= tx < W`` and ``0 <= ty < H``.

The sums are integers, so the order of the additions does not matter.  The 1/16 quantisation per
axis keeps a cell inside an int32 whatever the flow is, as long as ``H * W <= 2**23`` (every source
on one cell: 256 H W); a rigid translation by any fraction still gives exactly 256 in the covered
interior.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

KINDS = ("range", "fb")
UNIT = 256                  # one source pixel, in acc's units
MAX_PIXELS = 1 << 23        # H * W: 256 * 2^23 = 2^31 is the first sum an int32 cannot hold


def _check_flow(name: str, flow) -> Tuple[int, int, int]:
    if not isinstance(flow, torch.Tensor) or flow.ndim != 4 or flow.shape[-1] != 2 or flow.dtype != torch.float32:
        raise ValueError(f"{name}: flows must be (B, H, W, 2) fp32, got "
                         f"{tuple(flow.shape) if isinstance(flow, torch.Tensor) else flow} {getattr(flow, 'dtype', '')}")
    B, H, W, _ = flow.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{name}: empty flow {tuple(flow.shape)}")
    return B, H, W


def check_pixels(name: str, H: int, W: int) -> None:
    if H * W > MAX_PIXELS:
        raise ValueError(f"{name}: H * W = {H * W} is above 2^23, an int32 cell could overflow")


def range_threshold(thr: float) -> int:
    """The integer ``T = ceil(thr * 256)`` that ``acc >= T`` is tested with."""
    return int(math.ceil(float(thr) * UNIT))


def _landing(flow: torch.Tensor):
    B, H, W, _ = flow.shape
    f = flow.detach()
    px = torch.arange(W, device=f.device, dtype=torch.float32).view(1, 1, W) + f[..., 0]
    py = torch.arange(H, device=f.device, dtype=torch.float32).view(1, H, 1) + f[..., 1]
    return px, py


def range_map(flow: torch.Tensor) -> torch.Tensor:
    """The range map (B, H, W) int32 of a flow (B, H, W, 2) fp32 (module docstring): how much of the
    flow's own frame lands on each pixel of the other frame, in 1/256 of a source pixel."""
    B, H, W = _check_flow("range_map", flow)
    check_pixels("range_map", H, W)
    px, py = _landing(flow)
    ok = (px > -1) & (px < W) & (py > -1) & (py < H)            # NaN, +-inf fail
    zero = torch.zeros((), dtype=torch.float32, device=flow.device)
    pxs, pys = torch.where(ok, px, zero), torch.where(ok, py, zero)
    x0f, y0f = torch.floor(pxs), torch.floor(pys)
    qx = torch.round((pxs - x0f) * 16.0).to(torch.int64)        # torch.round: ties to even
    qy = torch.round((pys - y0f) * 16.0).to(torch.int64)
    x0, y0 = x0f.to(torch.int64), y0f.to(torch.int64)
    base = (torch.arange(B, device=flow.device, dtype=torch.int64) * (H * W)).view(B, 1, 1)
    acc = torch.zeros(B * H * W, dtype=torch.int32, device=flow.device)
    for dy in (0, 1):
        for dx in (0, 1):
            tx, ty = x0 + dx, y0 + dy
            w = (qx if dx else 16 - qx) * (qy if dy else 16 - qy)
            sel = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            acc.index_add_(0, (base + ty * W + tx)[sel], w[sel].to(torch.int32))
    return acc.view(B, H, W)


def lands_inside(flow: torch.Tensor) -> torch.Tensor:
    """(B, H, W) bool: step 1 of ``fb_consistency`` -- ``0 <= px <= W-1`` and ``0 <= py <= H-1`` for the
    pixel's own landing point (a non-finite flow is not inside)."""
    B, H, W = _check_flow("lands_inside", flow)
    px, py = _landing(flow)
    return (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)


def visibility_masks(flow_fw: torch.Tensor, flow_bw: torch.Tensor, kind: str, thr: float = 0.5, alpha: float = 0.01,
                     beta: float = 0.5) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(vis_fw, vis_bw)``, fp32 (B, H, W), 1.0 = use the pixel in the loss, 0.0 = leave it out, of a
    flow pair (B, H, W, 2) fp32 (fw: 1 -> 2, bw: 2 -> 1).  The inputs are detached: no gradient.

    ``kind="range"``: ``vis_fw = !lands_inside(flow_fw) | (range_map(flow_bw) >= ceil(thr * 256))`` -- a
    pixel of frame 1 is visible in frame 2 iff enough of frame 2 maps back onto it.  ``kind="fb"``:
    ``vis_fw = !lands_inside(flow_fw) | !occ_fw`` with ``occ`` from ``fb_consistency(flow_fw, flow_bw,
    alpha, beta)``.  ``vis_bw`` is symmetric.  A pixel whose own flow lands outside the frame (a
    non-finite flow included) keeps mask 1 under both kinds: it has to go on paying the loss's
    ``out_penalty``, or flows that point off the frame would be free."""
    if kind not in KINDS:
        raise ValueError(f"visibility_masks: unknown kind {kind!r} (range or fb)")
    _check_flow("visibility_masks", flow_fw)
    _check_flow("visibility_masks", flow_bw)
    if flow_fw.shape != flow_bw.shape or flow_fw.device != flow_bw.device:
        raise ValueError("visibility_masks: flow_fw and flow_bw must have the same shape and device")
    fw, bw = flow_fw.detach(), flow_bw.detach()
    out_fw, out_bw = ~lands_inside(fw), ~lands_inside(bw)
    if kind == "range":
        T = range_threshold(thr)
        vis_fw, vis_bw = out_fw | (range_map(bw) >= T), out_bw | (range_map(fw) >= T)
    else:
        from ..models.reference import fb_consistency

        occ_fw, occ_bw = fb_consistency(fw.contiguous(), bw.contiguous(), alpha, beta)
        vis_fw, vis_bw = out_fw | ~occ_fw, out_bw | ~occ_bw
    return vis_fw.float(), vis_bw.float()
