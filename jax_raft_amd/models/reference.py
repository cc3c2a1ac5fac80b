"""Golden pure-PyTorch RAFT primitives (exact reference semantics, NHWC, fp32).

This module is the numerical oracle for every HIP kernel in ``csrc/`` and the
whole CPU execution path (BASELINE config 1).  Each function reproduces the
behaviour of one primitive of the reference JAX/Flax model; the reference
line ranges are cited per function.  Implementations deliberately use plain
PyTorch indexing / ``F.conv2d`` so they can be cross-checked against
independent PyTorch primitives (``F.grid_sample``, ``F.avg_pool2d``,
``F.unfold``, ``F.interpolate``) in ``tests/test_reference.py``.

All tensors are channels-last (NHWC), like the reference.
"""
from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

__all__ = [
    "grid_sample",
    "make_coords_grid",
    "resize_with_aligned_corners",
    "upsample_flow",
    "conv2d_nhwc",
    "instance_norm_nhwc",
    "batch_norm_nhwc",
    "corr_volume",
    "build_pyramid",
    "index_pyramid",
    "index_on_demand",
    "neighborhood_offsets",
    "forward_project",
    "fill_offsets",
    "fb_consistency",
    "BidirectionalFlow",
    "warp_frames",
    "BidirectionalWarp",
    "interpolate_frames",
    "interp_params",
    "interp_times",
    "BidirectionalInterp",
    "CONSISTENT",
]


def grid_sample(img: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
    """Bilinear sampling at *pixel* coordinates with zero padding.

    Reference: ``jax_raft/model.py:24-34`` (``map_coordinates(order=1,
    mode='constant')`` vmapped over batch and channel).  ``grid[..., 0]`` is
    x (column) and ``grid[..., 1]`` is y (row).  Each of the 4 taps that falls
    outside the image contributes 0; in-bounds taps keep their weight (no
    renormalisation).

    img: (N, H, W, C); grid: (N, h, w, 2) -> (N, h, w, C)
    """
    assert img.shape[-3] > 1
    assert grid.ndim == 4 and grid.shape[-1] == 2
    n, H, W, C = img.shape
    x = grid[..., 0]
    y = grid[..., 1]
    x0 = torch.floor(x)
    y0 = torch.floor(y)
    wx1 = x - x0
    wy1 = y - y0
    wx0 = 1.0 - wx1
    wy0 = 1.0 - wy1
    x0i = x0.long()
    y0i = y0.long()
    flat = img.reshape(n, H * W, C)
    out = torch.zeros(grid.shape[:-1] + (C,), dtype=img.dtype, device=img.device)
    bidx = torch.arange(n, device=img.device).view(n, 1, 1)
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            xi = x0i + dx
            yi = y0i + dy
            valid = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            lin = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1))
            vals = flat[bidx.expand_as(lin), lin]  # (n, h, w, C)
            wgt = (wx * wy * valid.to(img.dtype)).unsqueeze(-1)
            out = out + wgt * vals
    return out


def make_coords_grid(batch_size: int, h: int, w: int, device=None) -> torch.Tensor:
    """``coords[b, y, x] = (x, y)`` float32.  Reference ``model.py:37-40``."""
    ys, xs = torch.meshgrid(
        torch.arange(h, device=device, dtype=torch.float32),
        torch.arange(w, device=device, dtype=torch.float32),
        indexing="ij",
    )
    coords = torch.stack([xs, ys], dim=-1)
    return coords.unsqueeze(0).repeat(batch_size, 1, 1, 1)


def _linear_resize_axis(x: torch.Tensor, axis: int, out_size: int) -> torch.Tensor:
    in_size = x.shape[axis]
    if in_size == out_size:
        return x
    # x_in = x_out * (in - 1) / (out - 1)   (align_corners=True)
    pos = torch.arange(out_size, dtype=torch.float64, device=x.device) * (
        (in_size - 1.0) / (out_size - 1.0)
    )
    i0 = torch.floor(pos).long().clamp(0, in_size - 1)
    i1 = (i0 + 1).clamp(max=in_size - 1)
    w1 = (pos - i0.double()).to(x.dtype)
    w0 = 1.0 - w1
    shape = [1] * x.ndim
    shape[axis] = out_size
    a = x.index_select(axis, i0)
    b = x.index_select(axis, i1)
    return a * w0.view(shape) + b * w1.view(shape)


def resize_with_aligned_corners(
    image: torch.Tensor, shape: Tuple[int, ...], method: str = "bilinear", antialias: bool = True
) -> torch.Tensor:
    """Bilinear resize emulating ``align_corners=True``.

    Reference ``model.py:43-66`` (``jax.image.scale_and_translate`` with
    ``scale=(out-1)/(in-1)``, ``translation=0.5-scale/2``).  Only the dims whose
    size changes are resized.  Only upsampling is exercised by RAFT; with
    ``antialias`` the triangle kernel is identical to plain linear
    interpolation for upsampling, so the flag does not change the result.
    """
    assert method == "bilinear", "currently only bilinear interpolation is supported"
    assert len(shape) == image.ndim
    out = image
    for axis in range(image.ndim):
        if image.shape[axis] != shape[axis]:
            out = _linear_resize_axis(out, axis, shape[axis])
    return out


def upsample_flow(flow: torch.Tensor, up_mask: Optional[torch.Tensor] = None, factor: int = 8) -> torch.Tensor:
    """x8 flow upsampling (bilinear when ``up_mask is None``, else convex).

    Reference ``model.py:69-98``.  Convex mode: mask channel index is
    ``k*64 + a*8 + b`` (k = 3x3 neighbour, row-major; a = sub-row; b = sub-col),
    softmax over k, weighted sum of the zero-padded 3x3 neighbourhood of
    ``factor*flow``, then pixel shuffle to (B, 8h, 8w, C).
    """
    B, h, w, C = flow.shape
    nh, nw = h * factor, w * factor
    if up_mask is None:
        up = resize_with_aligned_corners(flow, (B, nh, nw, C), method="bilinear", antialias=False)
        return factor * up
    assert up_mask.shape == (B, h, w, 9 * factor * factor)
    flow = flow.float()
    m = up_mask.float().reshape(B, h, w, 9, factor, factor)
    m = torch.softmax(m, dim=3)
    fp = F.pad((factor * flow).permute(0, 3, 1, 2), (1, 1, 1, 1))  # (B, C, h+2, w+2)
    neigh = []
    for ky in range(3):
        for kx in range(3):
            neigh.append(fp[:, :, ky:ky + h, kx:kx + w])
    neigh = torch.stack(neigh, dim=2)  # (B, C, 9, h, w)
    neigh = neigh.permute(0, 3, 4, 1, 2)  # (B, h, w, C, 9)
    # out[n,y,x,c,a,b] = sum_k m[n,y,x,k,a,b] * neigh[n,y,x,c,k]
    # as broadcast multiply + reduction: the einsum lowers to B*h*w tiny
    # (C x 9) @ (9 x 64) batched GEMMs, which the GPU library runs ~5x slower
    # than this memory-bound form (training profile, profiles/r1_train_kernel_breakdown_v1.txt)
    mm = m.reshape(B, h, w, 1, 9, factor * factor)
    up = (neigh.unsqueeze(-1) * mm).sum(dim=4)  # (B, h, w, C, 64)
    up = up.reshape(B, h, w, C, factor, factor).permute(0, 1, 4, 2, 5, 3).reshape(B, nh, nw, C)
    return up


def conv2d_nhwc(
    x: torch.Tensor,
    kernel: torch.Tensor,
    bias: Optional[torch.Tensor],
    stride: Tuple[int, int] = (1, 1),
    padding: Tuple[int, int] = (0, 0),
) -> torch.Tensor:
    """NHWC conv with an HWIO kernel (Flax layout), symmetric explicit padding.

    Reference: ``flax.linen.Conv`` as used by ``model.py:101-159`` (padding
    ``(k-1)//2`` per dim from ``model.py:137-141``) and the plain convs at
    ``model.py:304-310,347-349,394``.
    """
    w = kernel.permute(3, 2, 0, 1)  # HWIO -> OIHW
    y = F.conv2d(x.permute(0, 3, 1, 2), w, bias, stride=stride, padding=padding)
    return y.permute(0, 2, 3, 1)


def conv2d_nhwc_gemm(
    x: torch.Tensor,
    kernel: torch.Tensor,
    bias: Optional[torch.Tensor],
    stride: Tuple[int, int] = (1, 1),
    padding: Tuple[int, int] = (0, 0),
) -> torch.Tensor:
    """:func:`conv2d_nhwc` as explicit im2col + one fp32 GEMM (the same sum, no
    convolution library): the golden conv of GPU-side references (ops/functional.py
    ``golden_ops``), which must not depend on a conv library's algorithm search."""
    N, H, W, C = x.shape
    kh, kw, _, co = kernel.shape
    cols = F.unfold(x.permute(0, 3, 1, 2), (kh, kw), padding=padding, stride=stride)   # (N, C*kh*kw, L)
    OH = (H + 2 * padding[0] - kh) // stride[0] + 1
    OW = (W + 2 * padding[1] - kw) // stride[1] + 1
    w = kernel.permute(2, 0, 1, 3).reshape(C * kh * kw, co)          # unfold order: (c, i, j)
    y = torch.matmul(cols.transpose(1, 2), w)                        # (N, L, co)
    if bias is not None:
        y = y + bias
    return y.reshape(N, OH, OW, co)


def instance_norm_nhwc(x: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    """Flax ``nn.InstanceNorm(epsilon=1e-5, use_bias=False, use_scale=False)``
    (``model.py:706-707``): per (n, c) over H, W, biased variance.  Statistics
    in fp32 whatever the input dtype."""
    if torch.is_grad_enabled() and x.requires_grad:
        return _InstanceNormNHWC.apply(x, eps)
    xf = x.to(torch.promote_types(x.dtype, torch.float32))
    var, mean = torch.var_mean(xf, dim=(1, 2), unbiased=False, keepdim=True)
    return ((xf - mean) * torch.rsqrt(var + eps)).to(x.dtype)


class _InstanceNormNHWC(torch.autograd.Function):
    """Instance norm with a closed-form backward: saves only the input and the
    per-(n, c) statistics (no fp32 copies of the activation), and computes
    dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) in one expression chain
    instead of autograd's trace through the mean / square / rsqrt graph."""

    @staticmethod
    def forward(ctx, x, eps: float):
        xf = x.to(torch.promote_types(x.dtype, torch.float32))
        var, mean = torch.var_mean(xf, dim=(1, 2), unbiased=False, keepdim=True)
        rstd = torch.rsqrt(var + eps)
        ctx.save_for_backward(x, mean, rstd)
        return ((xf - mean) * rstd).to(x.dtype)

    @staticmethod
    def backward(ctx, gy):
        x, mean, rstd = ctx.saved_tensors
        ft = torch.promote_types(x.dtype, torch.float32)
        g = gy.to(ft)
        xhat = (x.to(ft) - mean) * rstd
        gm = g.mean(dim=(1, 2), keepdim=True)
        gxm = (g * xhat).mean(dim=(1, 2), keepdim=True)
        return (rstd * (g - gm - xhat * gxm)).to(x.dtype), None


def batch_norm_nhwc(
    x: torch.Tensor,
    scale: torch.Tensor,
    bias: torch.Tensor,
    mean: torch.Tensor,
    var: torch.Tensor,
    train: bool,
    eps: float = 1e-5,
    momentum: float = 0.99,
    sync_group=None,
):
    """Flax ``nn.BatchNorm`` (defaults: momentum 0.99, eps 1e-5) as used by the
    raft_large context encoder (``model.py:147,157,711``).

    Returns ``(y, new_mean, new_var)``; in eval mode the running statistics are
    used and returned unchanged.  ``sync_group`` (a torch.distributed group, or
    ``True`` for the default group) makes it a synchronised BatchNorm over the
    data-parallel ranks (Flax ``axis_name=`` semantics): the batch statistics
    come from one differentiable all-reduce of (sum x, sum x^2, count) per
    layer, so every rank normalises with -- and back-propagates through -- the
    global-batch mean/variance.
    """
    dt = x.dtype
    x = x.float()
    if train:
        if sync_group is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            from torch.distributed.nn.functional import all_reduce as _ar

            n = torch.full((1,), float(x.numel() // x.shape[-1]), device=x.device)
            packed = torch.cat([x.sum(dim=(0, 1, 2)), (x * x).sum(dim=(0, 1, 2)), n])
            packed = _ar(packed) if sync_group is True else _ar(packed, group=sync_group)
            C = x.shape[-1]
            tot = packed[2 * C]
            bmean = packed[:C] / tot
            bvar = packed[C:2 * C] / tot - bmean * bmean
        else:
            bmean = x.mean(dim=(0, 1, 2))
            bvar = (x * x).mean(dim=(0, 1, 2)) - bmean * bmean
        bvar = bvar.clamp_min(0.0)
        new_mean = momentum * mean + (1.0 - momentum) * bmean.detach()
        new_var = momentum * var + (1.0 - momentum) * bvar.detach()
        m, v = bmean, bvar
    else:
        new_mean, new_var = mean, var
        m, v = mean, var
    y = (x - m) * torch.rsqrt(v + eps) * scale + bias
    return y.to(dt), new_mean, new_var


def corr_volume(fmap1: torch.Tensor, fmap2: torch.Tensor) -> torch.Tensor:
    """All-pairs correlation ``fmap1 @ fmap2^T / sqrt(C)`` -> (B, h, w, h, w).

    Reference ``CorrBlock._compute_corr_volume``, ``model.py:472-481``.
    """
    B, h, w, C = fmap1.shape
    f1 = fmap1.reshape(B, h * w, C)
    f2 = fmap2.reshape(B, h * w, C)
    corr = torch.matmul(f1, f2.transpose(1, 2))
    return corr.reshape(B, h, w, h, w) / math.sqrt(C)


def build_pyramid(fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int) -> List[torch.Tensor]:
    """Correlation pyramid: level 0 is the (B*h*w, h, w) volume, each further
    level a 2x2/stride-2 VALID (floor) average pool.  Reference
    ``CorrBlock.build_pyramid``, ``model.py:418-446``.  Levels are returned as
    (B*h*w, h_l, w_l) (channel dim of size 1 squeezed)."""
    assert fmap1.shape == fmap2.shape, "Input feature maps should have the same shapes"
    min_fmap_size = 2 * (2 ** (num_levels - 1))
    assert not any(s < min_fmap_size for s in fmap1.shape[-3:-1]), (
        "Feature maps are too small to be down-sampled by the correlation pyramid. "
        f"H and W of feature maps should be at least {min_fmap_size}; got: {tuple(fmap1.shape[-3:-1])}. "
        f"Input image dimensions should be at least 8 * {min_fmap_size} = {8 * min_fmap_size}."
    )
    return build_pyramid_queries(fmap1, fmap2, num_levels)


def build_pyramid_queries(fmap1: torch.Tensor, fmap2: torch.Tensor, num_levels: int) -> List[torch.Tensor]:
    """:func:`build_pyramid` for a subset of query pixels: ``fmap1`` (B, hq, wq, C)
    holds the queries (e.g. a slab of query rows, context parallelism), ``fmap2``
    (B, h, w, C) every target pixel.  Levels are (B*hq*wq, h_l, w_l); each query's
    maps are exactly its rows of the full pyramid (pooling acts on target dims only)."""
    B, hq, wq, C = fmap1.shape
    _, h, w, _ = fmap2.shape
    f1 = fmap1.reshape(B, hq * wq, C)
    f2 = fmap2.reshape(B, h * w, C)
    vol = (torch.matmul(f1, f2.transpose(1, 2)) / math.sqrt(C)).reshape(B * hq * wq, h, w)
    pyr = [vol]
    for _ in range(num_levels - 1):
        hh, ww = vol.shape[-2] // 2, vol.shape[-1] // 2
        vol = vol[:, : 2 * hh, : 2 * ww].reshape(vol.shape[0], hh, 2, ww, 2).mean(dim=(2, 4))
        pyr.append(vol)
    return pyr


def neighborhood_offsets(radius: int, device=None) -> torch.Tensor:
    """``delta[i, j] = (i - r, j - r)`` -- x gets the slow index.  ``model.py:451-455``."""
    d = torch.linspace(-radius, radius, 2 * radius + 1, device=device)
    di, dj = torch.meshgrid(d, d, indexing="ij")
    return torch.stack([di, dj], dim=-1)  # (2r+1, 2r+1, 2)


def index_pyramid(pyramid: Sequence[torch.Tensor], coords: torch.Tensor, radius: int) -> torch.Tensor:
    """Radius-r bilinear lookup of every pyramid level around ``coords / 2^l``.

    Reference ``CorrBlock.index_pyramid``, ``model.py:448-470``.  Output
    channel = ``l*(2r+1)^2 + i*(2r+1) + j`` with x-offset ``i-r`` and y-offset
    ``j-r``.  coords: (B, h, w, 2) -> (B, h, w, L*(2r+1)^2)
    """
    B, h, w, _ = coords.shape
    side = 2 * radius + 1
    delta = neighborhood_offsets(radius, coords.device).reshape(1, side, side, 2)
    c = coords.reshape(B * h * w, 1, 1, 2)
    out = []
    for vol in pyramid:
        sc = c + delta
        s = grid_sample(vol.unsqueeze(-1), sc).reshape(B, h, w, side * side)
        out.append(s)
        c = c / 2
    return torch.cat(out, dim=-1)


def pool_features(fmap: torch.Tensor, num_levels: int) -> List[torch.Tensor]:
    """The target features of every pyramid level: level 0 is ``fmap`` (B, h, w, C), level l+1 the
    2x2/stride-2 VALID (floor) mean of level l, sizes ``h >> l, w >> l`` -- what
    :func:`build_pyramid` does to the volume's target dims, applied to the features."""
    levels = [fmap]
    for _ in range(num_levels - 1):
        B, h, w, C = fmap.shape
        hh, ww = h // 2, w // 2
        fmap = fmap[:, : 2 * hh, : 2 * ww].reshape(B, hh, 2, ww, 2, C).mean(dim=(2, 4))
        levels.append(fmap)
    return levels


def index_on_demand(fmap1: torch.Tensor, fmap2: torch.Tensor, coords: torch.Tensor, radius: int,
                    num_levels: int) -> torch.Tensor:
    """On-demand correlation lookup (original RAFT's ``alternate_corr``; no counterpart in the
    reference): what ``index_pyramid(build_pyramid(fmap1, fmap2, L), coords, r)`` returns, computed
    from the two feature maps without the all-pairs volume.  Memory O(P * C) instead of O(P^2).

    Pooling is linear, so the level-l volume cell ``(q; y, x)`` equals the correlation of query
    ``q`` with the level-l pooled target features (:func:`pool_features`):
    ``sum_c fmap1[q, c] * f2_l[y, x, c] / sqrt(C)``, and 0 outside the level map.  Per level the
    ``(2r+2)^2`` integer cells around ``floor(coords / 2^l) - r`` are formed and blended to the
    ``(2r+1)^2`` samples with :func:`grid_sample`'s weights (all samples of a level share one
    fractional offset); the channel order ``l*S^2 + i*S + j`` (x offset ``i - r`` slow) is
    :func:`index_pyramid`'s.  A fixed sequence of fp32 operations; equal to the volume path up
    to fp32 rounding.

    fmap1, fmap2: (B, h, w, C); coords: (B, h, w, 2) -> (B, h, w, L*(2r+1)^2)"""
    assert fmap1.shape == fmap2.shape, "Input feature maps should have the same shapes"
    B, h, w, C = fmap1.shape
    min_fmap_size = 2 * (2 ** (num_levels - 1))
    assert h >= min_fmap_size and w >= min_fmap_size, (
        f"Feature maps are too small for {num_levels} pyramid levels: H and W should be at least "
        f"{min_fmap_size}; got: {(h, w)}.")
    assert tuple(coords.shape) == (B, h, w, 2), "coords: (B, h, w, 2)"
    S = 2 * radius + 1
    W1 = S + 1
    dev = coords.device
    q = fmap1.reshape(B, h * w, 1, C)
    c = coords.reshape(B, h * w, 2)
    bidx = torch.arange(B, device=dev).view(B, 1, 1)
    win = torch.arange(W1, device=dev)
    out = []
    for f2 in pool_features(fmap2, num_levels):
        hl, wl = f2.shape[1:3]
        x0f = torch.floor(c[..., 0])
        y0f = torch.floor(c[..., 1])
        wx = (c[..., 0] - x0f).view(B, h * w, 1, 1)
        wy = (c[..., 1] - y0f).view(B, h * w, 1, 1)
        # the integer window base, clamped before it becomes an index (far-outside coordinates)
        bx = x0f.clamp(-2.0 ** 20, 2.0 ** 20).long() - radius
        by = y0f.clamp(-2.0 ** 20, 2.0 ** 20).long() - radius
        xs = (bx.unsqueeze(-1) + win).view(B, h * w, 1, W1)      # window columns
        ys = (by.unsqueeze(-1) + win).view(B, h * w, W1, 1)      # window rows
        valid = (xs >= 0) & (xs < wl) & (ys >= 0) & (ys < hl)    # (B, hw, W1, W1) [row, column]
        lin = (ys.clamp(0, hl - 1) * wl + xs.clamp(0, wl - 1)).view(B, h * w, W1 * W1)
        feats = f2.reshape(B, hl * wl, C)[bidx.expand_as(lin), lin]              # (B, hw, W1*W1, C)
        cells = (feats * q).sum(-1) / math.sqrt(C)
        cells = (cells * valid.view(B, h * w, W1 * W1).to(cells.dtype)).view(B, h * w, W1, W1)
        v = (1.0 - wy) * cells[:, :, :-1, :] + wy * cells[:, :, 1:, :]           # vertical: rows j, j + 1
        s = (1.0 - wx) * v[..., :-1] + wx * v[..., 1:]                           # horizontal: columns i, i + 1
        out.append(s.transpose(2, 3).reshape(B, h, w, S * S))                   # [i (x)][j (y)]
        c = c / 2
    return torch.cat(out, dim=-1)


# ------------------------------------------------------------------ warm start
# (no counterpart in the reference: original RAFT's ``forward_interpolate``, defined
# here with single fp32 operations and integers only so that the HIP kernel,
# csrc/kernels/warm.hip, matches bit for bit)

def fill_offsets(fill_radius: int) -> List[Tuple[int, int]]:
    """The hole search's neighbour offsets ``(dy, dx)``, ``|dy|, |dx| <= fill_radius``,
    ascending by ``(dy*dy + dx*dx, dy, dx)``."""
    r = range(-fill_radius, fill_radius + 1)
    return sorted(((dy, dx) for dy in r for dx in r), key=lambda o: (o[0] * o[0] + o[1] * o[1], o[0], o[1]))


def forward_project(flow: torch.Tensor, fill_radius: int = 4) -> torch.Tensor:
    """Project a flow field forward in time: the initial flow of pair t + 1 from the
    (1/8-resolution) flow of pair t.  flow, result: (B, h, w, 2) fp32, channel 0 = x.

    1. A source cell (x, y) with flow (fx, fy) lands at ``x1 = float(x) + fx``,
       ``y1 = float(y) + fy``; its target cell is ``tx = floor(x1 + 0.5)``,
       ``ty = floor(y1 + 0.5)``.  It is valid iff ``0 <= tx <= w-1`` and ``0 <= ty <= h-1``
       (float comparisons: NaN / inf are invalid).
    2. Key of a valid source: ``ix = rint((x1 - tx) * 256)``, ``iy`` likewise (half to even),
       ``d2 = ix*ix + iy*iy`` (integer), key = ``(d2 << 32) | (y*w + x)``.
    3. A target cell takes the flow of the valid source with the minimum key that lands in
       it: the nearest landing, ties to the lower source index.
    4. A cell nothing landed in takes the value of the first hit cell among
       :func:`fill_offsets` (out-of-map neighbours skipped), else (0, 0); holes are filled
       from hit cells only, never from other filled holes.
    """
    assert flow.ndim == 4 and flow.shape[-1] == 2 and flow.dtype == torch.float32, "flow: (B, h, w, 2) fp32"
    assert 0 <= fill_radius <= 8, "fill_radius must be in [0, 8]"
    B, h, w, _ = flow.shape
    dev = flow.device
    grid = make_coords_grid(1, h, w, device=dev)
    x1 = grid[..., 0] + flow[..., 0]
    y1 = grid[..., 1] + flow[..., 1]
    tx = torch.floor(x1 + 0.5)
    ty = torch.floor(y1 + 0.5)
    valid = (tx >= 0) & (tx <= w - 1) & (ty >= 0) & (ty <= h - 1)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    ix = torch.where(valid, torch.round((x1 - tx) * 256.0), zero).long()
    iy = torch.where(valid, torch.round((y1 - ty) * 256.0), zero).long()
    src = torch.arange(h * w, device=dev).view(1, h, w)
    empty = torch.iinfo(torch.int64).max
    key = torch.where(valid, ((ix * ix + iy * iy) << 32) | src, torch.full((), empty, device=dev))
    tgt = torch.where(valid, ty * w + tx, zero).long()
    keys = torch.full((B, h * w), empty, dtype=torch.int64, device=dev)
    keys.scatter_reduce_(1, tgt.reshape(B, -1), key.reshape(B, -1), "amin", include_self=True)
    hit = keys != empty
    win = torch.where(hit, keys & 0xFFFFFFFF, torch.zeros((), dtype=torch.int64, device=dev))
    splat = torch.gather(flow.reshape(B, h * w, 2), 1, win.unsqueeze(-1).expand(-1, -1, 2))
    hit = hit.view(B, h, w)
    splat = torch.where(hit.unsqueeze(-1), splat.view(B, h, w, 2), zero)
    R = fill_radius
    hit_p = F.pad(hit.to(torch.uint8), (R, R, R, R)).bool()
    splat_p = F.pad(splat, (0, 0, R, R, R, R))
    out = torch.zeros_like(flow)
    done = torch.zeros_like(hit)
    for dy, dx in fill_offsets(R):
        nb_hit = hit_p[:, R + dy:R + dy + h, R + dx:R + dx + w]
        take = nb_hit & ~done
        out = torch.where(take.unsqueeze(-1), splat_p[:, R + dy:R + dy + h, R + dx:R + dx + w], out)
        done = done | take
    return out


class BidirectionalFlow(NamedTuple):
    """What a ``bidirectional=True`` forward returns: the flows 1 -> 2 and 2 -> 1, each
    (N or 1, B, H, W, 2), and the (B, H, W) bool occlusion masks (True = occluded) of the
    forward-backward check of the two final flows (:func:`fb_consistency`)."""
    flows_fw: torch.Tensor
    flows_bw: torch.Tensor
    occ_fw: torch.Tensor
    occ_bw: torch.Tensor


def _fb_one(a: torch.Tensor, b: torch.Tensor, alpha: torch.Tensor, beta: torch.Tensor):
    """One direction of :func:`fb_consistency` on whole (B, H, W, 2) maps: (occluded, err)."""
    B, H, W, _ = a.shape
    grid = make_coords_grid(1, H, W, device=a.device)
    fx, fy = a[..., 0], a[..., 1]
    px = grid[..., 0] + fx
    py = grid[..., 1] + fy
    inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)   # NaN fails
    zero = torch.zeros((), dtype=torch.float32, device=a.device)
    pxs = torch.where(inside, px, zero)
    pys = torch.where(inside, py, zero)
    x0f, y0f = torch.floor(pxs), torch.floor(pys)
    wx, wy = (pxs - x0f).unsqueeze(-1), (pys - y0f).unsqueeze(-1)
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = torch.clamp(x0 + 1, max=W - 1), torch.clamp(y0 + 1, max=H - 1)
    bf = b.reshape(B, H * W, 2)

    def tap(yy, xx):
        idx = (yy * W + xx).reshape(B, H * W, 1).expand(-1, -1, 2)
        return torch.gather(bf, 1, idx).view(B, H, W, 2)

    b00, b01, b10, b11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    top = b00 + wx * (b01 - b00)
    bot = b10 + wx * (b11 - b10)
    g = top + wy * (bot - top)
    d = a + g
    err = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    mag = (fx * fx + fy * fy) + (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1])
    thr = alpha * mag + beta
    occ = ~inside | ~(err <= thr)
    return occ, torch.where(inside, err, torch.full((), float("inf"), device=a.device))


def fb_consistency(flow_fw: torch.Tensor, flow_bw: torch.Tensor, alpha: float = 0.01, beta: float = 0.5,
                   window: Optional[Tuple[int, int, int, int]] = None, return_err: bool = False):
    """Forward-backward consistency check (UnFlow, Meister et al. 2018): the occlusion masks of
    a flow pair.  flow_fw (1 -> 2), flow_bw (2 -> 1): (B, H, W, 2) fp32, channel 0 = x, in
    pixels; returns ``(occ_fw, occ_bw)``, (B, H, W) bool, True = occluded; with
    ``return_err`` also the two fp32 error maps ``(occ_fw, occ_bw, err_fw, err_bw)``.

    ``window = (H0, W0, top, left)``: the frame is that rectangle of the map (uint8 frames that
    were padded); coordinates are relative to it, pixels outside it get False (err 0).

    A fixed sequence of fp32 operations, every product and sum rounded on its own (the kernel
    csrc/kernels/fbcheck.hip equals it bit for bit).  For a frame pixel (y, x) with flow
    ``f = a[y, x]`` (``a`` this direction's flow, ``b`` the opposite one):

    1. ``px = float(x) + f.x``, ``py = float(y) + f.y``; ``inside`` iff ``0 <= px <= W0-1`` and
       ``0 <= py <= H0-1`` (NaN fails).
    2. ``x0 = floor(px)``, ``x1 = min(x0+1, W0-1)``, ``wx = px - float(x0)``; y likewise.
    3. Bilinear per channel: ``top = b00 + wx*(b01 - b00)``, ``bot = b10 + wx*(b11 - b10)``,
       ``g = top + wy*(bot - top)``.
    4. ``d = f + g``, ``err = d.x*d.x + d.y*d.y``,
       ``mag = (f.x*f.x + f.y*f.y) + (g.x*g.x + g.y*g.y)``, ``thr = alpha*mag + beta``.
    5. ``occluded = !inside || !(err <= thr)``; the err map holds ``err``, ``inf`` where ``!inside``.

    ``alpha = 0.01``, ``beta = 0.5`` are UnFlow's published defaults."""
    for f in (flow_fw, flow_bw):
        assert f.ndim == 4 and f.shape[-1] == 2 and f.dtype == torch.float32, "flows: (B, H, W, 2) fp32"
    assert flow_fw.shape == flow_bw.shape, "flow_fw and flow_bw must have the same shape"
    B, H, W, _ = flow_fw.shape
    H0, W0, top, left = (H, W, 0, 0) if window is None else map(int, window)
    assert H0 >= 1 and W0 >= 1 and top >= 0 and left >= 0 and top + H0 <= H and left + W0 <= W, \
        "window (H0, W0, top, left) must lie inside the map"
    dev = flow_fw.device
    al = torch.tensor(alpha, dtype=torch.float32, device=dev)
    be = torch.tensor(beta, dtype=torch.float32, device=dev)
    fw = flow_fw[:, top:top + H0, left:left + W0]
    bw = flow_bw[:, top:top + H0, left:left + W0]
    res = []
    for a, b in ((fw, bw), (bw, fw)):
        o, e = _fb_one(a, b, al, be)
        occ = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
        err = torch.zeros((B, H, W), dtype=torch.float32, device=dev)
        occ[:, top:top + H0, left:left + W0] = o
        err[:, top:top + H0, left:left + W0] = e
        res.append((occ, err))
    if return_err:
        return res[0][0], res[1][0], res[0][1], res[1][1]
    return res[0][0], res[1][0]


class BidirectionalWarp(NamedTuple):
    """What ``bidirectional=True, warp=True`` returns: :class:`BidirectionalFlow`'s four fields,
    the motion-compensated frames (B, H0, W0, 3) uint8 -- ``warped_fw`` is frame 2 sampled with the
    flow 1 -> 2 (it reproduces frame 1), ``warped_bw`` frame 1 sampled with the flow 2 -> 1 -- and
    ``photo`` (2, B, 2) int64: per direction and sample (sum of ``|warped - own|`` over kept pixels
    and channels, kept pixels) (:func:`warp_frames`)."""
    flows_fw: torch.Tensor
    flows_bw: torch.Tensor
    occ_fw: torch.Tensor
    occ_bw: torch.Tensor
    warped_fw: torch.Tensor
    warped_bw: torch.Tensor
    photo: torch.Tensor


def warp_frames(src: torch.Tensor, flow: torch.Tensor, occ: Optional[torch.Tensor] = None,
                own: Optional[torch.Tensor] = None, window: Optional[Tuple[int, int, int, int]] = None):
    """Motion-compensated frame and masked photometric error: ``src`` sampled at ``x + flow(x)``,
    the occluded pixels and those that land outside replaced.  Returns ``(warped, photo)``.

    src: (B, H0, W0, 3) uint8, the frame that is sampled; flow: (B, H, W, 2) fp32, channel 0 = x;
    ``window = (H0, W0, top, left)``: the frame's rectangle inside the flow map (default: the
    whole map); occ: (B, H, W) bool or None (True = occluded, :func:`fb_consistency`); own:
    (B, H0, W0, 3) uint8 or None, the frame ``warped`` should reproduce.

    A fixed sequence of fp32 operations, every product and sum rounded on its own (the kernel
    csrc/kernels/framewarp.hip equals it bit for bit).  Steps 1 and 2 are :func:`fb_consistency`'s,
    so the two ops agree on what "outside" means.  For a frame pixel (y, x) with
    ``f = flow[top + y, left + x]``:

    1. ``px = float(x) + f.x``, ``py = float(y) + f.y``; ``inside`` iff ``0 <= px <= W0-1`` and
       ``0 <= py <= H0-1`` (NaN fails).
    2. ``x0 = floor(px)``, ``x1 = min(x0+1, W0-1)``, ``wx = px - float(x0)``; y likewise.
    3. Per channel, the texels converted to fp32: ``t = c00 + wx*(c01 - c00)``,
       ``b = c10 + wx*(c11 - c10)``, ``v = t + wy*(b - t)`` (in [0, 255]: every step is monotone
       under rounding).
    4. ``w = uint8(rint(v))``, ties to even.
    5. ``keep = inside && !occ``; ``warped = keep ? w : own`` (0 without ``own``).
    6. ``photo[b] = (sum over kept pixels and the 3 channels of |w - own|, kept pixels)``, int64
       (B, 2); ``None`` without ``own``."""
    assert flow.ndim == 4 and flow.shape[-1] == 2 and flow.dtype == torch.float32, "flow: (B, H, W, 2) fp32"
    B, H, W, _ = flow.shape
    H0, W0, top, left = (H, W, 0, 0) if window is None else map(int, window)
    assert H0 >= 1 and W0 >= 1 and top >= 0 and left >= 0 and top + H0 <= H and left + W0 <= W, \
        "window (H0, W0, top, left) must lie inside the map"
    for name, t in (("src", src), ("own", own)):
        assert t is None or (tuple(t.shape) == (B, H0, W0, 3) and t.dtype == torch.uint8), \
            f"{name}: (B, H0, W0, 3) uint8"
    assert occ is None or (tuple(occ.shape) == (B, H, W) and occ.dtype == torch.bool), "occ: (B, H, W) bool"
    dev = flow.device
    f = flow[:, top:top + H0, left:left + W0]
    grid = make_coords_grid(1, H0, W0, device=dev)
    px = grid[..., 0] + f[..., 0]
    py = grid[..., 1] + f[..., 1]
    inside = (px >= 0) & (px <= W0 - 1) & (py >= 0) & (py <= H0 - 1)   # NaN fails
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    pxs = torch.where(inside, px, zero)
    pys = torch.where(inside, py, zero)
    x0f, y0f = torch.floor(pxs), torch.floor(pys)
    wx, wy = (pxs - x0f).unsqueeze(-1), (pys - y0f).unsqueeze(-1)
    x0, y0 = x0f.long(), y0f.long()
    x1, y1 = torch.clamp(x0 + 1, max=W0 - 1), torch.clamp(y0 + 1, max=H0 - 1)
    sf = src.reshape(B, H0 * W0, 3).to(torch.float32)

    def tap(yy, xx):
        idx = (yy * W0 + xx).reshape(B, H0 * W0, 1).expand(-1, -1, 3)
        return torch.gather(sf, 1, idx).view(B, H0, W0, 3)

    c00, c01, c10, c11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    t = c00 + wx * (c01 - c00)
    b = c10 + wx * (c11 - c10)
    v = t + wy * (b - t)
    w = torch.round(v).to(torch.uint8)
    keep = inside if occ is None else inside & ~occ[:, top:top + H0, left:left + W0]
    fill = own if own is not None else torch.zeros_like(src)
    warped = torch.where(keep.unsqueeze(-1), w, fill)
    if own is None:
        return warped, None
    d = (w.to(torch.int64) - own.to(torch.int64)).abs().sum(-1)
    photo = torch.stack([(d * keep).sum((1, 2)), keep.sum((1, 2))], dim=-1)
    return warped, photo


class BidirectionalInterp(NamedTuple):
    """What ``bidirectional=True, interpolate=t`` returns: :class:`BidirectionalFlow`'s four fields,
    then ``frames`` (K, B, H0, W0, 3) uint8, the frames at the K times ``t`` between frame 1
    (``t = 0``) and frame 2 (``t = 1``), and ``holes`` (K, B, H0, W0) bool, the pixels nothing was
    splatted onto, which hold the nearer input frame's pixel (:func:`interpolate_frames`)."""
    flows_fw: torch.Tensor
    flows_bw: torch.Tensor
    occ_fw: torch.Tensor
    occ_bw: torch.Tensor
    frames: torch.Tensor
    holes: torch.Tensor


CONSISTENT = 16             # the splat confidence of a pixel its own mask does not call occluded (occluded: 1); untuned
INTERP_COVER_UNIT = 1 << 20   # D of a cell covered fully by consistent pixels of both directions
INTERP_MAX_TIMES = 8          # times per model / engine call (each adds a clear and two kernels to the plan)
INTERP_MAX_MAPS = 65535       # directions * B of one splat launch (its grid's second dimension)
INTERP_MAX_PIXELS = 1 << 30   # H0 * W0 (warp_frames' limit): keeps every sum inside an int64


def interp_params(t: float, min_cover: float = 1.0 / 64) -> Tuple[int, int]:
    """Step 0 of :func:`interpolate_frames`: ``(tq, Dmin)`` of one time -- ``tq = int(rint(t * 256))``
    in [1, 255] and ``Dmin = max(1, ceil(min_cover * 2**20))``; ``ValueError`` otherwise (a NaN, 0 or
    1 for ``t``; a ``min_cover`` outside [0, 1])."""
    t, min_cover = float(t), float(min_cover)
    tq = int(round(t * 256.0)) if math.isfinite(t) else -1     # Python's round: ties to even, as rint
    if not 1 <= tq <= 255:
        raise ValueError(f"interpolate_frames: t = {t} must round to a 256th in [1/256, 255/256] (strictly between "
                         "the two frames)")
    if not 0.0 <= min_cover <= 1.0:   # NaN fails
        raise ValueError(f"interpolate_frames: min_cover = {min_cover} must lie in [0, 1]")
    return tq, max(1, int(math.ceil(min_cover * INTERP_COVER_UNIT)))


def interp_times(t, min_cover: float = 1.0 / 64, max_times: Optional[int] = None):
    """``(rows, many)`` of ``t``, a float or a sequence of floats: ``rows`` the :func:`interp_params` of
    every time (``ValueError`` for a time or ``min_cover`` out of range, or an empty or too long
    sequence), ``many`` whether ``t`` was a sequence."""
    many = not isinstance(t, (int, float)) and getattr(t, "ndim", 1) != 0   # a numpy / tensor scalar is one time
    ts = list(t) if many else [t]
    if not ts or (max_times is not None and len(ts) > max_times):
        raise ValueError(f"interpolate_frames: t must be a float or a sequence of 1 to {max_times or 'any number of'} "
                         f"floats, got {len(ts)}")
    return [interp_params(v, min_cover) for v in ts], many


def interpolate_frames(frame1: torch.Tensor, frame2: torch.Tensor, flow_fw: torch.Tensor, flow_bw: torch.Tensor,
                       t: float, occ_fw: Optional[torch.Tensor] = None, occ_bw: Optional[torch.Tensor] = None,
                       window: Optional[Tuple[int, int, int, int]] = None, min_cover: float = 1.0 / 64,
                       return_acc: bool = False):
    """The frame at time ``t`` between frame 1 (``t = 0``) and frame 2 (``t = 1``) by forward
    splatting: every pixel of both frames is pushed along a fraction of its own flow, and what meets
    in a cell is normalised.  Returns ``(frame_t, holes)``: (B, H0, W0, 3) uint8 and (B, H0, W0) bool.

    frame1 / frame2: (B, H0, W0, 3) uint8; flow_fw (1 -> 2) / flow_bw (2 -> 1): (B, H, W, 2) fp32,
    channel 0 = x; occ_fw / occ_bw: (B, H, W) bool or None, as :func:`fb_consistency` returns them;
    ``window = (H0, W0, top, left)``: the frame's rectangle inside the flow map (default: the whole
    map), as in :func:`warp_frames`.

    Exact integer arithmetic after two fp32 operations per axis, so neither the order of a scatter
    nor the order of atomics can change a bit (the kernels csrc/kernels/interp.hip equal it bit for
    bit, the accumulator included):

    0. ``tq, Dmin = interp_params(t, min_cover)``.  Direction 0 is (frame1, flow_fw, occ_fw) with
       the step ``s = fp32(tq) / 256`` and the temporal weight ``a0 = 256 - tq``; direction 1 is
       (frame2, flow_bw, occ_bw) with ``s = fp32(256 - tq) / 256`` and ``a1 = tq`` (``s`` is exact).
    1. For the frame pixel (y, x) of direction d with ``f = flow_d[top + y, left + x]``:
       ``px = float(x) + s * f.x``, ``py = float(y) + s * f.y`` -- the product rounded on its own,
       then the sum.  The pixel contributes iff ``-1 < px < W0`` and ``-1 < py < H0`` (float
       comparisons: NaN and +-inf fail).
    2. ``x0 = floor(px)``, ``qx = int(rint((px - x0) * 16))`` (ties to even, in [0, 16]); y likewise
       (``train/occlusion.py:range_map``'s steps 2 and 3).
    3. The four taps ``(x0 + dx, y0 + dy)`` have the integer weights ``w = (dx ? qx : 16 - qx) *
       (dy ? qy : 16 - qy)``: 256 per source.
    4. Confidence ``k = 1`` where the pixel's own mask calls it occluded, else ``CONSISTENT = 16``
       (no mask: 16).  A tap inside the frame adds ``(w*k, w*k*R, w*k*G, w*k*B)`` to the int64 cell
       ``acc[d, b, ty, tx, 0:4]``: a consistent pixel dominates an occluded one that lands on the
       same cell, and occluded pixels still fill what nothing else reaches.
    5. Per frame pixel: ``D = a0 * acc[0].w + a1 * acc[1].w``, ``N_c = a0 * acc[0].c + a1 *
       acc[1].c``, ``hole = D < Dmin``, ``v_c = (2 * N_c + D) // (2 * D)`` (round half up; in
       [0, 255] since ``N_c <= 255 * D``), and ``frame_t = hole ? (tq <= 128 ? frame1 : frame2)[y, x]
       : v``.  A cell covered fully by consistent pixels of both directions has ``D = 2**20``, the
       unit of ``min_cover``.

    Bound: one contribution is below 2^20 (256 * 16 * 255) and ``H0 * W0 <= 2**30`` is required, so
    a cell stays below 2^50 and step 5 below 2^61, whatever the flow.  ``CONSISTENT`` and the default
    ``min_cover`` are placeholders, untuned.  ``return_acc`` appends ``acc`` (2, B, H0, W0, 4) int64."""
    tq, dmin = interp_params(t, min_cover)
    assert flow_fw.ndim == 4 and flow_fw.shape[-1] == 2 and flow_fw.dtype == torch.float32, "flow_fw: (B, H, W, 2) fp32"
    assert flow_bw.shape == flow_fw.shape and flow_bw.dtype == torch.float32, "flow_bw: like flow_fw"
    B, H, W, _ = flow_fw.shape
    H0, W0, top, left = (H, W, 0, 0) if window is None else map(int, window)
    assert H0 >= 1 and W0 >= 1 and top >= 0 and left >= 0 and top + H0 <= H and left + W0 <= W, \
        "window (H0, W0, top, left) must lie inside the map"
    assert H0 * W0 <= INTERP_MAX_PIXELS, "H0 * W0 must be at most 2^30 (an int64 cell could overflow)"
    for name, fr in (("frame1", frame1), ("frame2", frame2)):
        assert tuple(fr.shape) == (B, H0, W0, 3) and fr.dtype == torch.uint8, f"{name}: (B, H0, W0, 3) uint8"
    for name, o in (("occ_fw", occ_fw), ("occ_bw", occ_bw)):
        assert o is None or (tuple(o.shape) == (B, H, W) and o.dtype == torch.bool), f"{name}: (B, H, W) bool"
    dev = flow_fw.device
    P = H0 * W0
    acc = torch.zeros((2, B * P, 4), dtype=torch.int64, device=dev)
    xs = torch.arange(W0, device=dev, dtype=torch.float32).view(1, 1, W0)
    ys = torch.arange(H0, device=dev, dtype=torch.float32).view(1, H0, 1)
    base = (torch.arange(B, device=dev, dtype=torch.int64) * P).view(B, 1, 1)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    one = torch.ones((), dtype=torch.int64, device=dev)
    for d, (frame, flow, occ, step) in enumerate(((frame1, flow_fw, occ_fw, tq), (frame2, flow_bw, occ_bw, 256 - tq))):
        s = torch.tensor(float(step), dtype=torch.float32, device=dev) / 256.0
        f = flow[:, top:top + H0, left:left + W0]
        px = xs + s * f[..., 0]
        py = ys + s * f[..., 1]
        ok = (px > -1) & (px < W0) & (py > -1) & (py < H0)          # NaN, +-inf fail
        pxs, pys = torch.where(ok, px, zero), torch.where(ok, py, zero)
        x0f, y0f = torch.floor(pxs), torch.floor(pys)
        qx = torch.round((pxs - x0f) * 16.0).to(torch.int64)        # torch.round: ties to even
        qy = torch.round((pys - y0f) * 16.0).to(torch.int64)
        x0, y0 = x0f.to(torch.int64), y0f.to(torch.int64)
        k = CONSISTENT * one if occ is None else torch.where(occ[:, top:top + H0, left:left + W0], one, CONSISTENT * one)
        rgb1 = torch.cat([torch.ones((B, H0, W0, 1), dtype=torch.int64, device=dev), frame.to(torch.int64)], -1)
        for dy in (0, 1):
            for dx in (0, 1):
                tx, ty = x0 + dx, y0 + dy
                w = (qx if dx else 16 - qx) * (qy if dy else 16 - qy) * k
                sel = ok & (tx >= 0) & (tx < W0) & (ty >= 0) & (ty < H0)
                acc[d].index_add_(0, (base + ty * W0 + tx)[sel], w[sel].unsqueeze(-1) * rgb1[sel])
    acc = acc.view(2, B, H0, W0, 4)
    tot = (256 - tq) * acc[0] + tq * acc[1]
    D = tot[..., :1]
    holes = D[..., 0] < dmin
    Ds = torch.where(holes.unsqueeze(-1), one, D)                   # a hole's quotient is not used
    v = torch.div(2 * tot[..., 1:] + Ds, 2 * Ds, rounding_mode="floor").clamp_(0, 255).to(torch.uint8)
    frame_t = torch.where(holes.unsqueeze(-1), frame1 if tq <= 128 else frame2, v)
    return (frame_t, holes, acc) if return_acc else (frame_t, holes)
