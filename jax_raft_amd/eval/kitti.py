"""KITTI-2015 validation (training split): EPE and F1-all over the valid pixels.

RAFT's ``validate_kitti`` protocol: 24 iterations, per pair the end-point error ``||flow - gt||``
at the pixels whose ground truth is valid; a pixel is an outlier iff its error is above 3 px AND
above 5 % of the ground truth's magnitude.  RAFT averages the EPE per image and then over images,
and takes F1 over all valid pixels of the split; so does this module.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ..utils.flow_io import InputPadder, normalize_image


def kitti_metrics(flow: np.ndarray, gt: np.ndarray, valid: np.ndarray) -> Dict[str, float]:
    """``flow``, ``gt`` (H, W, 2), ``valid`` (H, W) -> ``epe`` (mean over the valid pixels) and ``f1``
    (the percentage of valid pixels with ``epe > 3`` and ``epe / |gt| > 0.05``)."""
    sums = _pair_sums(flow, gt, valid)
    n = max(sums[2], 1.0)
    return {"epe": sums[0] / n, "f1": 100.0 * sums[1] / n}


def _pair_sums(flow, gt, valid) -> np.ndarray:
    """(sum of epe, outliers, valid pixels) of one pair, float64."""
    flow, gt = np.asarray(flow, dtype=np.float32), np.asarray(gt, dtype=np.float32)
    on = np.asarray(valid).reshape(gt.shape[:2]) != 0
    epe = np.sqrt(((flow - gt) ** 2).sum(-1))[on].astype(np.float64)
    mag = np.sqrt((gt ** 2).sum(-1))[on].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (epe > 3.0) & (epe / mag > 0.05)
    return np.array([epe.sum(), out.sum(), on.sum()], dtype=np.float64)


@torch.no_grad()
def validate_kitti(model, data_root: str, iters: int = 24, device: Optional[torch.device] = None,
                   max_pairs: Optional[int] = None, verbose: bool = True, **engine_kw) -> Dict[str, float]:
    """EPE / F1 of ``model`` on ``<data_root>/training`` (``train/datasets.py:FlowPairs.kitti``).

    On a GPU device the model gets the raw uint8 frames, one pair per forward (the frames differ in
    size): the engine normalises and replicate-pads to a multiple of 8 on the device and returns
    the flow cropped back.  That padding is CENTRED (the 'sintel' mode), not the bottom-only
    padding RAFT uses for KITTI; on the CPU device the host pads the same way.

    Data parallel (an initialised process group): each rank takes every world-th pair and the sums
    are all-reduced, as in ``validate_sintel``."""
    from ..train.datasets import FlowPairs

    dist = torch.distributed if torch.distributed.is_available() and torch.distributed.is_initialized() else None
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
    device = device or (torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
    model = model.to(device).eval()
    ds = FlowPairs.kitti(data_root)
    n = len(ds) if max_pairs is None else min(len(ds), max_pairs)
    sums = np.zeros(5, dtype=np.float64)      # sum of per-image epe, images, outliers, valid pixels, sum of epe
    for i in range(rank, n, world):
        a, b, gt, valid = ds[i]
        if device.type == "cuda":
            i1, i2, padder = torch.from_numpy(a)[None], torch.from_numpy(b)[None], None
        else:
            i1, i2 = normalize_image(a), normalize_image(b)
            padder = InputPadder(i1.shape, channels_last=True)
            i1, i2 = padder.pad(i1, i2)
        pred = model(i1.to(device), i2.to(device), num_flow_updates=iters, **engine_kw)[-1].float().cpu()
        flow = (pred if padder is None else padder.unpad(pred))[0].numpy()
        s = _pair_sums(flow, gt, valid)
        sums += [s[0] / max(s[2], 1.0), 1.0, s[1], s[2], s[0]]
    if dist:
        st = torch.tensor(sums, dtype=torch.float64, device=device)
        dist.all_reduce(st)
        sums = st.cpu().numpy()
    res = {"epe": sums[0] / max(sums[1], 1.0), "f1": 100.0 * sums[2] / max(sums[3], 1.0), "pairs": int(n), "world": world}
    if verbose and rank == 0:
        print("Validation KITTI: EPE %f, F1-all %f" % (res["epe"], res["f1"]))
    return res
