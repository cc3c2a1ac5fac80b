"""Real flow datasets for training: the file lists and a prefetching pair loader.

:class:`FlowPairs` is a list of ``(image1 path, image2 path, flow path)`` with constructors for
the FlyingChairs layout and the Sintel training layout.  :class:`PairLoader` turns it into
batches of the frames AS THEY ARE ON DISK -- uint8 images and the fp32 flow, all of one size --
and uploads them; the crop and every augmentation happen afterwards on the device
(``ops/native.py:augment_pairs``).  A worker thread decodes batch ``step + 1`` into a ring of
pinned staging buffers while batch ``step`` trains.

Sparse ground truth: :class:`SparseFlowPairs` lists KITTI-2015 and HD1K, whose flow is a 16-bit
PNG with a validity channel (``utils/flow_io.py:read_flow_png``) and whose frames come in several
sizes.  The loader then stages every sample in the top-left corner of buffers of the largest
size, adds a uint8 valid plane and the list of sizes, and the device op is
``ops/native.py:augment_pairs_sparse``.

Not covered (``NotImplementedError`` or absent): mixed-dataset sampling for the Sintel stage,
dense and sparse samples in one batch, FlyingThings' ``.pfm`` flow.
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

from ..utils.flow_io import png_size, read_flo, read_flow_png, read_image

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


class SparseLayoutNotFound(FileNotFoundError, NotImplementedError):
    """``root`` does not hold the KITTI / HD1K layout that was asked for.  A ``FileNotFoundError``;
    also a ``NotImplementedError``, which is what ``FlowPairs.open`` raised for these two names
    whatever the root held while they had no reader, so callers that catch that keep working."""


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
        if dataset == "kitti":
            return cls.kitti(root)
        if dataset == "hd1k":
            return cls.hd1k(root)
        if dataset == "things":
            raise NotImplementedError(f"dataset {dataset!r}: the .pfm flow reader is not implemented")
        raise ValueError(f"unknown dataset {dataset!r} (chairs, sintel-clean, sintel-final, kitti, hd1k)")

    @classmethod
    def kitti(cls, root: str) -> "SparseFlowPairs":
        """KITTI-2015 training: ``training/image_2/NNNNNN_10.png``, ``NNNNNN_11.png`` and the flow
        ``training/flow_occ/NNNNNN_10.png``."""
        firsts = sorted(glob(osp.join(root, "training", "image_2", "*_10.png")))
        if not firsts:
            raise SparseLayoutNotFound(f"no training/image_2/*_10.png under {root}")
        items = []
        for a in firsts:
            b = a[:-len("_10.png")] + "_11.png"
            f = osp.join(root, "training", "flow_occ", osp.basename(a))
            for p in (b, f):
                if not osp.isfile(p):
                    raise FileNotFoundError(p)
            items.append((a, b, f))
        return SparseFlowPairs(items)

    @classmethod
    def hd1k(cls, root: str) -> "SparseFlowPairs":
        """HD1K: ``hd1k_input/image_2/SSSSSS_NNNN.png`` with the flow
        ``hd1k_flow_gt/flow_occ/SSSSSS_NNNN.png``; consecutive frames of one sequence are a pair."""
        flows = sorted(glob(osp.join(root, "hd1k_flow_gt", "flow_occ", "*_*.png")))
        if not flows:
            raise SparseLayoutNotFound(f"no hd1k_flow_gt/flow_occ/*.png under {root}")
        image = lambda f: osp.join(root, "hd1k_input", "image_2", osp.basename(f))
        items = []
        for f, nxt in zip(flows, flows[1:]):
            if osp.basename(f).split("_")[0] != osp.basename(nxt).split("_")[0]:
                continue                            # the last frame of a sequence has no successor
            for p in (image(f), image(nxt)):
                if not osp.isfile(p):
                    raise FileNotFoundError(p)
            items.append((image(f), image(nxt), f))
        return SparseFlowPairs(items)

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


class SparseFlowPairs(FlowPairs):
    """``ds[i] -> (image1, image2, flow fp32 (H, W, 2), valid uint8 (H, W))`` over PNG frames and
    KITTI-coded flow PNG; the pairs may differ in size."""

    sparse = True

    def __getitem__(self, i: int):
        a, b, f = self.items[i]
        flow, valid = read_flow_png(f)
        return read_image(a), read_image(b), flow, valid

    def sizes(self) -> List[Tuple[int, int]]:
        """(H, W) of every pair's first image, from the files' IHDR chunks (24 bytes each)."""
        return [png_size(a) for a, _, _ in self.items]


class PairLoader:
    """Batches of raw frames, a pure function of the step.

    ``indices_for(step)``: epoch ``step // steps_per_epoch`` permutes the dataset with a generator
    seeded by ``(seed, epoch)``; the ranks take disjoint slices of it, ``batch`` indices each per
    step (the tail of an epoch that does not fill a batch on every rank is dropped).
    ``fetch(step)`` returns the batch on ``device`` -- ``(image1 uint8 (B, H, W, 3), image2,
    flow fp32 (B, H, W, 2))`` -- uploaded ``non_blocking`` on the current stream from pinned
    staging buffers, and starts decoding ``step + 1`` on the worker thread.  Fetching steps in
    order therefore overlaps decode with training; any other step is decoded on the spot.

    Over a :class:`SparseFlowPairs` the frames may differ in size: ``frame_max`` / ``frame_min`` are
    the largest / smallest height and width in the list, the buffers are (B, Hmax, Wmax, ...) with
    every sample in the top-left corner, and ``fetch`` returns ``(image1, image2, flow, valid uint8
    (B, Hmax, Wmax), sizes)``, ``sizes`` a host-side list of (Hs, Ws).  The bytes outside a
    sample's own region are whatever an earlier batch left there: nothing may depend on them.
    """

    def __init__(self, dataset: FlowPairs, batch: int, seed: int = 0, rank: int = 0, world: int = 1,
                 device=None, depth: int = 3):
        self.ds, self.batch, self.seed, self.rank, self.world = dataset, int(batch), int(seed), int(rank), int(world)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.steps_per_epoch = len(dataset) // (self.batch * self.world)
        if self.steps_per_epoch < 1:
            raise ValueError(f"{len(dataset)} pairs do not fill one batch of {self.batch} on {self.world} rank(s)")
        self.sparse = bool(getattr(dataset, "sparse", False))
        if self.sparse:
            self._sizes = dataset.sizes()
            self.frame_max = (max(s[0] for s in self._sizes), max(s[1] for s in self._sizes))
            self.frame_min = (min(s[0] for s in self._sizes), min(s[1] for s in self._sizes))
            self.frame = self.frame_max            # the buffers' size
        else:
            a, _, f = dataset[0]
            self.frame = self.frame_max = self.frame_min = tuple(a.shape[:2])
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
            if self.sparse:
                self._slots[slot] += (mk((self.batch, H, W), torch.uint8),)
        return self._slots[slot]

    def _decode_one(self, bufs, n: int, index: int) -> None:
        if self.sparse:
            arrs = self.ds[index]
            Hs, Ws = self._sizes[index]
            for arr, path in zip(arrs, self.ds.items[index] + (self.ds.items[index][2],)):
                if tuple(arr.shape[:2]) != (Hs, Ws):
                    raise ValueError(f"{path}: size {tuple(arr.shape[:2])} differs from the pair's first image {(Hs, Ws)}")
            for buf, arr in zip(bufs, arrs):       # into the top-left corner; the rest of the buffer stays as it is
                np.copyto(buf[n].numpy()[:Hs, :Ws], arr)
            return
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

    def sizes_for(self, step: int) -> List[Tuple[int, int]]:
        """(Hs, Ws) of every sample of ``step`` (all ``frame`` for a dense list)."""
        return [self._sizes[i] if self.sparse else self.frame for i in self.indices_for(step)]

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
        if self.sparse:
            out += (self.sizes_for(step),)
        return out

    def close(self) -> None:
        self._worker.shutdown(wait=True)
        self._pool.shutdown(wait=True)
