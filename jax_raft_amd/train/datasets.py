"""Real flow datasets for training: the file lists and a prefetching pair loader.

:class:`FlowPairs` is a list of ``(image1 path, image2 path, flow path)`` with constructors for
the FlyingChairs layout and the Sintel training layout.  :class:`PairLoader` turns it into
batches of the frames AS THEY ARE ON DISK -- uint8 images and the fp32 flow, all of one size --
and uploads them; the crop and every augmentation happen afterwards on the device
(``ops/native.py:augment_pairs``).  A worker thread decodes batch ``step + 1`` into a ring of
pinned staging buffers while batch ``step`` trains.

Not covered (``NotImplementedError`` or absent): the sparse KITTI / HD1K augmentor and ``.png``
flow, mixed-dataset sampling for the Sintel stage, datasets with more than one frame size,
FlyingThings' ``.pfm`` flow.
"""
from __future__ import annotations

import os
import os.path as osp
import re
import threading
import time
from concurrent.futures import Future, ThreadPoolExecutor
from glob import glob
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..utils.flow_io import read_flo, read_image

MAX_THREADS = 16
_PPM_HEADER = re.compile(rb"P6\s+(\d+)\s+(\d+)\s+255\s")


def decode_threads() -> int:
    """Decoder threads of a loader: ``OMP_NUM_THREADS`` when set, at most 16 (a job's CPU share is
    far below the machine's core count, so the count is never taken from ``os.cpu_count()``)."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", ""))
    except ValueError:
        n = MAX_THREADS
    return max(1, min(n, MAX_THREADS))


def read_frame(path: str) -> np.ndarray:
    """``read_image``, with a direct read of binary 8-bit PPM (FlyingChairs' format: a short header,
    then the RGB bytes): one ``fromfile`` that releases the GIL, where the generic decoder holds it
    for most of ~0.5 ms per frame and so serialises the decode threads against the training loop.
    Anything else (PNG, a PPM with comments or 16-bit samples) goes through ``read_image``."""
    if path.endswith(".ppm"):
        with open(path, "rb") as f:
            m = _PPM_HEADER.match(f.read(32))
            if m is not None:
                w, h = int(m.group(1)), int(m.group(2))
                f.seek(m.end())                    # exactly one whitespace byte follows maxval
                data = np.fromfile(f, np.uint8, count=h * w * 3)
                if data.size == h * w * 3:
                    return data.reshape(h, w, 3)
    return read_image(path)


class FlowPairs:
    """``ds[i] -> (image1 uint8 (H, W, 3), image2, flow fp32 (H, W, 2))`` over a list of file triples."""

    def __init__(self, items: Sequence[Tuple[str, str, str]]):
        self.items: List[Tuple[str, str, str]] = [tuple(t) for t in items]
        if not self.items:
            raise ValueError("FlowPairs: no pairs")

    @classmethod
    def chairs(cls, root: str) -> "FlowPairs":
        """FlyingChairs: ``NNNNN_img1.ppm``, ``NNNNN_img2.ppm``, ``NNNNN_flow.flo`` in one directory."""
        firsts = sorted(glob(osp.join(root, "*_img1.ppm")))
        if not firsts:
            raise FileNotFoundError(f"no *_img1.ppm under {root}")
        items = []
        for a in firsts:
            stem = a[:-len("_img1.ppm")]
            b, f = stem + "_img2.ppm", stem + "_flow.flo"
            for p in (b, f):
                if not osp.isfile(p):
                    raise FileNotFoundError(p)
            items.append((a, b, f))
        return cls(items)

    @classmethod
    def sintel(cls, root: str, dstype: str = "clean") -> "FlowPairs":
        """The MPI-Sintel training split, ``clean`` or ``final`` pass (the tree ``eval/sintel.py`` walks)."""
        from ..eval.sintel import MpiSintel

        if dstype not in ("clean", "final"):
            raise ValueError(f"Sintel pass {dstype!r}: clean or final")
        ds = MpiSintel(root, "training", dstype)
        return cls([(a, b, f) for (a, b), f in zip(ds.image_list, ds.flow_list)])

    @classmethod
    def open(cls, root: str, dataset: str = "chairs") -> "FlowPairs":
        if dataset == "chairs":
            return cls.chairs(root)
        if dataset in ("sintel-clean", "sintel-final"):
            return cls.sintel(root, dataset.split("-")[1])
        if dataset in ("things", "kitti", "hd1k"):
            raise NotImplementedError(f"dataset {dataset!r}: .pfm / sparse .png flow readers are not implemented")
        raise ValueError(f"unknown dataset {dataset!r} (chairs, sintel-clean, sintel-final)")

    def __len__(self) -> int:
        return len(self.items)

    def __getitem__(self, i: int):
        a, b, f = self.items[i]
        try:
            flow = read_flo(f)
        except (ValueError, IndexError) as e:   # a truncated file: short header or short data
            raise ValueError(f"unreadable .flo file {f}: {e}") from None
        if flow is None:
            raise ValueError(f"unreadable .flo file {f}: bad magic")
        return read_frame(a), read_frame(b), flow


class PairLoader:
    """Batches of raw frames, a pure function of the step.

    ``indices_for(step)``: epoch ``step // steps_per_epoch`` permutes the dataset with a generator
    seeded by ``(seed, epoch)``; the ranks take disjoint slices of it, ``batch`` indices each per
    step (the tail of an epoch that does not fill a batch on every rank is dropped).
    ``fetch(step)`` returns the batch on ``device`` -- ``(image1 uint8 (B, H, W, 3), image2,
    flow fp32 (B, H, W, 2))`` -- uploaded ``non_blocking`` on the current stream from pinned
    staging buffers, and starts decoding ``step + 1`` on the worker thread.  Fetching steps in
    order therefore overlaps decode with training; any other step is decoded on the spot.
    """

    def __init__(self, dataset: FlowPairs, batch: int, seed: int = 0, rank: int = 0, world: int = 1,
                 device=None, depth: int = 3):
        self.ds, self.batch, self.seed, self.rank, self.world = dataset, int(batch), int(seed), int(rank), int(world)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.steps_per_epoch = len(dataset) // (self.batch * self.world)
        if self.steps_per_epoch < 1:
            raise ValueError(f"{len(dataset)} pairs do not fill one batch of {self.batch} on {self.world} rank(s)")
        a, _, f = dataset[0]
        self.frame = tuple(a.shape[:2])
        if tuple(f.shape[:2]) != self.frame:
            raise ValueError(f"{dataset.items[0][2]}: flow {f.shape[:2]} does not match its frame {self.frame}")
        self.depth = max(2, int(depth))
        self._pin = self.device.type == "cuda"
        self._slots = [None] * self.depth          # staging buffers, allocated on first use
        self._events = [None] * self.depth         # the upload that last read a slot
        self._pending = {}                         # step -> Future of its decode
        self._pool = ThreadPoolExecutor(decode_threads(), thread_name_prefix="pair-decode")
        self._worker = ThreadPoolExecutor(1, thread_name_prefix="pair-loader")
        self._lock = threading.Lock()
        self._perm = (None, None)

    # ------------------------------------------------------------------ order
    def indices_for(self, step: int) -> List[int]:
        epoch, k = divmod(int(step), self.steps_per_epoch)
        if self._perm[0] != epoch:
            self._perm = (epoch, np.random.default_rng([self.seed, epoch]).permutation(len(self.ds)))
        at = (k * self.world + self.rank) * self.batch
        return [int(i) for i in self._perm[1][at:at + self.batch]]

    # ----------------------------------------------------------------- decode
    def _staging(self, slot: int):
        if self._slots[slot] is None:
            H, W = self.frame
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=self._pin)
            self._slots[slot] = (mk((self.batch, H, W, 3), torch.uint8), mk((self.batch, H, W, 3), torch.uint8),
                                 mk((self.batch, H, W, 2), torch.float32))
        return self._slots[slot]

    def _decode_one(self, bufs, n: int, index: int) -> None:
        a, b, f = self.ds[index]
        for arr, path in zip((a, b, f), self.ds.items[index]):
            if tuple(arr.shape[:2]) != self.frame:
                raise ValueError(f"{path}: frame size {tuple(arr.shape[:2])} differs from the dataset's {self.frame} "
                                 "(datasets with more than one frame size are not supported)")
        for buf, arr in zip(bufs, (a, b, f)):      # numpy views of the staging tensors: a plain memcpy, GIL released
            np.copyto(buf[n].numpy(), arr)

    def _decode(self, step: int, indices: List[int]):
        slot = step % self.depth
        ev = self._events[slot]
        while ev is not None and not ev.query():   # the upload that read this slot must have finished (it long
            time.sleep(2e-4)                       # has: it was queued depth - 1 steps ago); polled, not a blocking wait
        bufs = self._staging(slot)
        for r in [self._pool.submit(self._decode_one, bufs, n, i) for n, i in enumerate(indices)]:
            r.result()
        return bufs

    def host_batch(self, step: int):
        """The staging buffers of ``step`` (valid until ``depth - 1`` further steps were fetched)."""
        idx = self.indices_for(step)
        with self._lock:
            fut: Optional[Future] = self._pending.pop(step, None)
            stale = list(self._pending.values())
            self._pending.clear()
        for s in stale:                            # a jump (resume, a test): no decode may still write a slot
            s.exception()
        bufs = fut.result() if fut is not None else self._worker.submit(self._decode, step, idx).result()
        return bufs

    def prefetch(self, step: int) -> None:
        idx = self.indices_for(step)
        with self._lock:
            if step not in self._pending:
                self._pending[step] = self._worker.submit(self._decode, step, idx)

    def fetch(self, step: int):
        bufs = self.host_batch(step)
        if self.device.type == "cuda":
            out = tuple(torch.empty(b.shape, dtype=b.dtype, device=self.device).copy_(b, non_blocking=True) for b in bufs)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._events[step % self.depth] = ev
        else:
            out = tuple(b.clone() for b in bufs)
        self.prefetch(step + 1)
        return out

    def close(self) -> None:
        self._worker.shutdown(wait=True)
        self._pool.shutdown(wait=True)
