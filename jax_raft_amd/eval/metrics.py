"""Flow validation metrics as an accumulating op: the golden definition.

``flow_metrics`` reduces a batch of predictions against ground truth to six sums per sample and
adds them to the running total ``acc`` of a split; ``metrics_from`` turns that total into EPE, the
1 / 3 / 5 px rates, KITTI's F1-all and the per-image mean EPE.  This module is torch ops on CPU
tensors and is the definition; ``ops/native.py:flow_metrics`` runs it on CPU tensors and the HIP
kernels of ``csrc/kernels/metrics.hip`` on GPU tensors (counts bitwise equal, fp64 sums equal up to
the order of their additions).

Per pixel of a sample's rectangle that counts (no valid plane, or its valid byte != 0), in fp32 with
every product and sum rounded on its own and correctly rounded square roots::

    dx = pred.x - gt.x; dy = pred.y - gt.y; epe = sqrt(dx*dx + dy*dy)
    mag = sqrt(gt.x*gt.x + gt.y*gt.y)
    buckets: epe < 1, epe < 3, epe < 5            (on epe, not on its square)
    outlier: epe > 3 and double(epe) / double(mag) > 0.05

A NaN ``epe`` falls in no bucket, is no outlier and makes the sample's sum NaN.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

ROW = 6     # [sum of epe, valid pixels, epe < 1, epe < 3, epe < 5, outliers]
ACC = 8     # ROW totals, the sum of per-image mean epe, images


def _sqrt(x: torch.Tensor) -> torch.Tensor:
    """The correctly rounded fp32 square root.  ``torch.sqrt`` on fp32 CPU tensors is not (its
    vectorised kernel is off by one ulp on about 0.6 % of random arguments, against numpy's and the
    GPU's), so the root is taken in fp64 and rounded to fp32: the square root of a 24-bit number
    lies at least 2^-49 (relative) from every fp32 rounding boundary, far more than the error of an
    fp64 root, so the second rounding decides as the exact root would."""
    return torch.sqrt(x.double()).float()


def check_args(pred, gt, valid, sizes, acc) -> List[Tuple[int, int]]:
    """The host checks of both implementations -> ``sizes`` as a list of (Hs, Ws) ints."""
    for name, t in (("pred", pred), ("gt", gt)):
        if t.ndim != 4 or t.shape[-1] != 2 or t.dtype != torch.float32:
            raise ValueError(f"flow_metrics: {name} must be (B, H, W, 2) fp32, got {tuple(t.shape)} {t.dtype}")
    B, Hp, Wp, _ = pred.shape
    if gt.shape[0] != B or B < 1:
        raise ValueError(f"flow_metrics: pred holds {B} samples, gt {gt.shape[0]}")
    Hg, Wg = int(gt.shape[1]), int(gt.shape[2])
    if valid is not None and (valid.dtype != torch.uint8 or tuple(valid.shape) != (B, Hg, Wg)):
        raise ValueError(f"flow_metrics: valid must be ({B}, {Hg}, {Wg}) uint8, got {tuple(valid.shape)} {valid.dtype}")
    for name, t in (("gt", gt), ("valid", valid), ("acc", acc)):
        if t is not None and t.device != pred.device:
            raise ValueError(f"flow_metrics: {name} is on {t.device}, pred on {pred.device}")
    Hm, Wm = min(Hp, Hg), min(Wp, Wg)
    if sizes is None:
        sizes = [(Hm, Wm)] * B
    sizes = [(int(h), int(w)) for h, w in sizes]
    if len(sizes) != B:
        raise ValueError(f"flow_metrics: {len(sizes)} sizes for a batch of {B}")
    for h, w in sizes:
        if not (1 <= h <= Hm and 1 <= w <= Wm):
            raise ValueError(f"flow_metrics: sample size {(h, w)} does not fit pred {(Hp, Wp)} and gt {(Hg, Wg)}")
    if acc is not None and (acc.dtype != torch.float64 or tuple(acc.shape) != (ACC,)):
        raise ValueError(f"flow_metrics: acc must be ({ACC},) fp64, got {tuple(acc.shape)} {acc.dtype}")
    return sizes


def flow_metrics(pred: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor] = None,
                 sizes: Optional[Sequence[Tuple[int, int]]] = None, acc: Optional[torch.Tensor] = None):
    """``pred`` (B, Hp, Wp, 2) fp32, ``gt`` (B, Hg, Wg, 2) fp32, ``valid`` (B, Hg, Wg) uint8 or None,
    ``sizes`` a host list of (Hs, Ws) per sample (default: the whole of the smaller map): sample
    ``n`` is the top-left Hs x Ws rectangle of both maps and nothing outside it is read.

    -> ``(rows, acc)``: ``rows`` (B, 6) fp64 ``[sum of double(epe), n_valid, n<1, n<3, n<5,
    n_outlier]``; ``acc`` (8,) fp64, the running total (a new one of zeros when None), updated in
    place and returned: ``acc[0:6] += rows.sum(0)`` with the samples added in order, ``acc[6] +=``
    the sum of the per-image means ``rows[n, 0] / max(rows[n, 1], 1)``, ``acc[7] += B``."""
    sizes = check_args(pred, gt, valid, sizes, acc)
    B, dev = pred.shape[0], pred.device
    rows = torch.zeros((B, ROW), dtype=torch.float64, device=dev)
    three, ratio = torch.tensor(3.0, dtype=torch.float32, device=dev), torch.tensor(0.05, dtype=torch.float64, device=dev)
    for n, (Hs, Ws) in enumerate(sizes):
        p, g = pred[n, :Hs, :Ws], gt[n, :Hs, :Ws]
        dx, dy = p[..., 0] - g[..., 0], p[..., 1] - g[..., 1]
        epe = _sqrt(dx * dx + dy * dy)
        mag = _sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1])
        if valid is not None:
            on = valid[n, :Hs, :Ws] != 0
            epe, mag = epe[on], mag[on]
        epe, mag = epe.reshape(-1), mag.reshape(-1)
        e64 = epe.double()
        out = (epe > three) & (e64 / mag.double() > ratio)        # x / 0 = inf: an outlier; 0 / 0 = nan: none
        rows[n] = torch.stack([e64.sum(), torch.tensor(float(epe.numel()), dtype=torch.float64)]
                              + [(epe < b).sum().double() for b in (1.0, 3.0, 5.0)] + [out.sum().double()])
    if acc is None:
        acc = torch.zeros(ACC, dtype=torch.float64)
    tot = torch.zeros(ACC, dtype=torch.float64)
    for n in range(B):                                            # the samples in order
        tot[:ROW] += rows[n]
        tot[6] += rows[n, 0] / rows[n, 1].clamp(min=1.0)
    tot[7] = float(B)
    acc += tot
    return rows, acc


def metrics_from(acc) -> Dict[str, float]:
    """The metrics of a split from its total ``acc`` (a tensor or any sequence of 8 numbers): ``epe``
    over all counted pixels, the ``1px`` / ``3px`` / ``5px`` rates, ``f1`` (KITTI's F1-all, per cent),
    ``epe_image_mean`` (the mean of the per-image mean EPE, which RAFT reports for KITTI) and ``pixels``."""
    a = [float(v) for v in (acc.tolist() if isinstance(acc, torch.Tensor) else acc)]
    if len(a) != ACC:
        raise ValueError(f"metrics_from: {ACC} totals wanted, got {len(a)}")
    n = max(a[1], 1.0)
    return {"epe": a[0] / n, "1px": a[2] / n, "3px": a[3] / n, "5px": a[4] / n, "f1": 100.0 * a[5] / n,
            "epe_image_mean": a[6] / max(a[7], 1.0), "pixels": int(a[1])}


def photometric_error(photo: torch.Tensor, size: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(mae, coverage)`` of ``models/reference.py:warp_frames``' ``photo`` (..., 2) int64 = (sum of
    ``|warped - own|`` over kept pixels and channels, kept pixels) for frames of ``size = (H0, W0)``:
    ``mae = sum / (3 * count)`` in 8-bit levels, NaN where nothing was kept, and ``coverage = count /
    (H0 * W0)``; both fp64 of shape ``photo.shape[:-1]``.  A label-free check of a flow field, not an
    accuracy figure."""
    if photo.shape[-1] != 2 or photo.dtype != torch.int64:
        raise ValueError(f"photometric_error: photo must be (..., 2) int64, got {tuple(photo.shape)} {photo.dtype}")
    H0, W0 = (int(v) for v in size)
    if H0 < 1 or W0 < 1:
        raise ValueError(f"photometric_error: size must be (H0, W0) >= 1, got {tuple(size)}")
    s, n = photo[..., 0].to(torch.float64), photo[..., 1].to(torch.float64)
    return s / (3.0 * n), n / float(H0 * W0)
