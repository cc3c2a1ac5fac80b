"""Streaming validation: a held-out split evaluated without leaving the device.

``evaluate`` walks a split in order (``train/datasets.py:SequentialLoader``: the next batch is
decoded on the decode threads into pinned staging buffers while the current one runs), hands the
raw uint8 frames to the model -- the engine normalises, pads and crops on the GPU and returns the
final flow only -- and reduces every batch against its ground truth with ``flow_metrics`` into one
running ``acc`` on the device.  A split costs each rank ONE device-to-host read, at its end, and one
fp64 ``all_reduce`` when a process group exists.  On a CPU device the same code runs with the
golden op and the golden model.

The stand-alone validators ``eval/sintel.py:validate_sintel`` and ``eval/kitti.py:validate_kitti``
follow the reference's per-pair host protocol and are the comparison: the counts of both are
equal, the EPE up to the order of an fp64 sum.  As in ``validate_kitti``, the padding of KITTI
frames is the centred 'sintel' mode.

CLI, one JSON line per split::

    python -m jax_raft_amd.eval.validate --model raft_large [--weights W] name=root [name=root ...]
"""
from __future__ import annotations

import argparse
import inspect
import json
import time
from typing import Dict, List, Optional, Tuple

import torch

from .metrics import ACC, metrics_from

# name -> (dataset name of train/datasets.py:FlowPairs.open, RAFT's iteration count for the split)
SPLITS = {"chairs-val": ("chairs-val", 24), "sintel-clean": ("sintel-clean", 32), "sintel-final": ("sintel-final", 32),
          "kitti": ("kitti", 24)}


def parse_val(entries) -> List[Tuple[str, str]]:
    """``"name=root"`` strings -> ``[(name, root)]``; an unknown name or a missing root is a ``ValueError``."""
    out = []
    for e in entries:
        name, sep, root = str(e).partition("=")
        if not sep or not root or name not in SPLITS:
            raise ValueError(f"validation split {e!r}: name=root wanted, name one of {sorted(SPLITS)}")
        out.append((name, root))
    return out


def _dist():
    d = torch.distributed
    return d if d.is_available() and d.is_initialized() else None


@torch.no_grad()
def evaluate(model, name: str, root: str, iters: Optional[int] = None, batch: int = 4, max_pairs: Optional[int] = None,
             device: Optional[torch.device] = None, **engine_kw) -> Dict[str, float]:
    """The metrics of ``model`` on split ``name`` (``chairs-val``, ``sintel-clean``, ``sintel-final``,
    ``kitti``) under ``root``: ``metrics_from`` of the split's total plus ``pairs``, ``world`` and
    ``seconds``.  ``iters`` defaults to RAFT's (24 chairs, 32 Sintel, 24 KITTI).  Sequential, not
    shuffled: rank ``r`` of ``world`` takes items ``r, r + world, ...`` of the first ``max_pairs``;
    batches of up to ``batch`` consecutive pairs of one frame size, the tail as a smaller batch, a
    sparse list (KITTI) one pair at a time.  The model's mode flags and weights are left as they are."""
    from ..ops import native as nat
    from ..train.datasets import FlowPairs, SequentialLoader

    if name not in SPLITS:
        raise ValueError(f"unknown validation split {name!r} (one of {sorted(SPLITS)})")
    dataset, default_iters = SPLITS[name]
    iters = int(iters) if iters else default_iters
    dist = _dist()
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    device = torch.device(device)
    model = model.to(device)
    kw = dict(engine_kw)
    if kw.get("cp_group") is not None:
        raise NotImplementedError("evaluate: not under context parallelism (cp_group)")
    split_file = kw.pop("chairs_split", None)      # the trainer's own split file (name == "chairs-val")
    if "return_all_iters" in inspect.signature(model.forward).parameters:
        kw["return_all_iters"] = False             # the final flow only
    t0 = time.perf_counter()
    ds = FlowPairs.chairs(root, "validation", split_file) if split_file and name == "chairs-val" else FlowPairs.open(root, dataset)
    loader = SequentialLoader(ds, batch=batch, rank=rank, world=world, device=device,
                              max_pairs=max_pairs)
    acc = torch.zeros(ACC, dtype=torch.float64, device=device)
    try:
        for img1, img2, flow, valid, _ in loader:
            pred = model(img1, img2, num_flow_updates=iters, **kw)[-1]
            nat.flow_metrics(pred.float(), flow, valid, None, acc)
    finally:
        loader.close()
    if dist:
        dist.all_reduce(acc)
    total = acc.cpu()                               # the split's one device-to-host read
    res = metrics_from(total)
    res.update(pairs=int(loader.pairs), world=world, seconds=time.perf_counter() - t0)
    return res


def main(argv=None):
    from .. import raft_large, raft_small

    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="raft_large", choices=("raft_large", "raft_small"))
    ap.add_argument("--weights", default=None, help="a checkpoint that the model factory loads")
    ap.add_argument("--iters", type=int, default=0, help="0: the protocol's default of each split")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--max-pairs", type=int, default=None)
    ap.add_argument("splits", nargs="+", metavar="name=root")
    a = ap.parse_args(argv)
    splits = parse_val(a.splits)
    factory = raft_large if a.model == "raft_large" else raft_small
    model, _ = factory(weights=a.weights) if a.weights else factory()
    for name, root in splits:
        res = evaluate(model, name, root, iters=a.iters or None, batch=a.batch, max_pairs=a.max_pairs)
        print(json.dumps({"split": name, **res}), flush=True)


if __name__ == "__main__":
    main()
