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

FlyingThings3D (:meth:`FlowPairs.things`) is a dense list whose flow is ``.pfm``.

The Sintel stage of RAFT's schedule trains on a weighted mixture of dense and sparse lists:
:class:`MixedFlowPairs` (``FlowPairs.open(root, "mix")``).  Over one the loader uses PACKED SLOTS:
buffers ``(B, S, ...)`` with ``S`` the largest ``Hs * Ws`` of the list, sample ``n`` in the first
``Hs * Ws`` pixels of slot ``n`` with row pitch ``Ws``; only that prefix is uploaded, and the device op is
``ops/native.py:augment_pairs_mixed``.

Validation: ``FlowPairs.chairs(root, split=...)`` lists FlyingChairs' training or validation pairs
by its split file, and :class:`SequentialLoader` walks a list in order, unshuffled and with its
tail, for ``eval/validate.py:evaluate``.
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

from ..utils.flow_io import png_size, read_flo, read_flow_png, read_image, read_pfm

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


def frame_size(path: str) -> Tuple[int, int]:
    """(H, W) of an image file from its header: a PNG's IHDR, a binary PPM's first line; anything
    else is decoded."""
    if path.endswith(".png"):
        return png_size(path)
    if path.endswith(".ppm"):
        with open(path, "rb") as f:
            m = _PPM_HEADER.match(f.read(32))
        if m is not None:
            return int(m.group(2)), int(m.group(1))
    return tuple(read_frame(path).shape[:2])


class ThingsLayoutNotFound(FileNotFoundError, NotImplementedError):
    """``root`` does not hold the FlyingThings3D layout.  A ``FileNotFoundError``; also a
    ``NotImplementedError``, which ``FlowPairs.open`` raised for ``things`` whatever the root held
    while ``.pfm`` had no reader, so callers that catch that keep working."""


# RAFT's Sintel-stage mixture, and the directory of each part under the mixture's root
MIX_DEFAULT = (("sintel-clean", 100), ("sintel-final", 100), ("kitti", 200), ("hd1k", 5), ("things-clean", 1))
MIX_DIRS = {"sintel-clean": "Sintel", "sintel-final": "Sintel", "kitti": "KITTI", "hd1k": "HD1K",
            "things-clean": "FlyingThings3D", "things-final": "FlyingThings3D", "things": "FlyingThings3D"}


class SparseLayoutNotFound(FileNotFoundError, NotImplementedError):
    """``root`` does not hold the KITTI / HD1K layout that was asked for.  A ``FileNotFoundError``;
    also a ``NotImplementedError``, which is what ``FlowPairs.open`` raised for these two names
    whatever the root held while they had no reader, so callers that catch that keep working."""


CHAIRS_SPLITS = {"training": 1, "validation": 2}
CHAIRS_SPLIT_FILES = ("FlyingChairs_train_val.txt", "chairs_split.txt")


def read_chairs_split(root: str, pairs: int, split_file: Optional[str] = None) -> List[int]:
    """The labels of FlyingChairs' split file: one integer per pair in sorted order, 1 = training,
    2 = validation.  A missing file is a ``FileNotFoundError`` naming the paths tried; a wrong line
    count or any other label is a ``ValueError`` naming the file."""
    tried = ([split_file] if split_file is not None else
             [osp.join(d, n) for d in (root, osp.dirname(osp.abspath(root))) for n in CHAIRS_SPLIT_FILES])
    path = next((p for p in tried if osp.isfile(p)), None)
    if path is None:
        raise FileNotFoundError("no FlyingChairs split file: tried " + ", ".join(tried))
    with open(path) as f:
        words = f.read().split()
    if len(words) != pairs:
        raise ValueError(f"{path}: {len(words)} labels for {pairs} pairs")
    if any(w not in ("1", "2") for w in words):
        bad = next(w for w in words if w not in ("1", "2"))
        raise ValueError(f"{path}: label {bad!r} (1 = training or 2 = validation wanted)")
    return [int(w) for w in words]


class FlowPairs:
    """``ds[i] -> (image1 uint8 (H, W, 3), image2, flow fp32 (H, W, 2))`` over a list of file triples."""

    labelled = True     # the flow is ground truth (False: FramePairs, whose flow is a placeholder)

    def __init__(self, items: Sequence[Tuple[str, str, str]]):
        self.items: List[Tuple[str, str, str]] = [tuple(t) for t in items]
        if not self.items:
            raise ValueError("FlowPairs: no pairs")

    @classmethod
    def chairs(cls, root: str, split: Optional[str] = None, split_file: Optional[str] = None) -> "FlowPairs":
        """FlyingChairs: ``NNNNN_img1.ppm``, ``NNNNN_img2.ppm``, ``NNNNN_flow.flo`` in one directory.

        ``split``: ``"training"`` / ``"validation"`` keep the pairs whose line in the split file is
        1 / 2 (one integer per pair, in sorted order); None: every pair.  ``split_file`` defaults to
        ``FlyingChairs_train_val.txt``, then ``chairs_split.txt``, in ``root`` and then its parent."""
        if split is not None:
            if split not in CHAIRS_SPLITS:
                raise ValueError(f"FlyingChairs split {split!r}: one of {sorted(CHAIRS_SPLITS)}, or None")
            full = cls.chairs(root)
            labels = read_chairs_split(root, len(full), split_file)
            return cls([t for t, lab in zip(full.items, labels) if lab == CHAIRS_SPLITS[split]])
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
    def things(cls, root: str, dstype: str = "clean") -> "FlowPairs":
        """FlyingThings3D's training split, left camera, RAFT's listing: the image directories
        ``<pass>/TRAIN/*/*/left`` (``clean`` / ``final``: ``frames_cleanpass`` / ``frames_finalpass``) against the
        flow directories ``optical_flow/TRAIN/*/*/{into_future,into_past}/left``; ``into_future`` pairs
        ``(img[i], img[i+1], flow[i])`` and ``into_past`` pairs ``(img[i+1], img[i], flow[i+1])``."""
        frames = {"clean": "frames_cleanpass", "final": "frames_finalpass"}.get(dstype, dstype)
        image_dirs = sorted(osp.join(d, "left") for d in glob(osp.join(root, frames, "TRAIN", "*", "*")))
        if not image_dirs:
            raise ThingsLayoutNotFound(f"no {frames}/TRAIN/*/* under {root}")
        scenes = sorted(glob(osp.join(root, "optical_flow", "TRAIN", "*", "*")))
        if len(scenes) != len(image_dirs):
            raise FileNotFoundError(f"{root}: {len(image_dirs)} scenes under {frames}/TRAIN, {len(scenes)} under optical_flow/TRAIN")
        items = []
        for direction in ("into_future", "into_past"):
            for idir, scene in zip(image_dirs, scenes):
                images = sorted(glob(osp.join(idir, "*.png")))
                flows = sorted(glob(osp.join(scene, direction, "left", "*.pfm")))
                if len(images) != len(flows):
                    raise FileNotFoundError(f"{osp.join(scene, direction, 'left')}: {len(flows)} flows for {len(images)} frames of {idir}")
                for i in range(len(flows) - 1):
                    if direction == "into_future":
                        items.append((images[i], images[i + 1], flows[i]))
                    else:
                        items.append((images[i + 1], images[i], flows[i + 1]))
        return cls(items)

    @classmethod
    def frames(cls, root: str) -> "FramePairs":
        """Video without ground truth, for label-free training: every directory under ``root`` (``root``
        itself included) that holds image files is one sequence, its files in sorted order; consecutive
        frames of a sequence are a pair and no pair crosses sequences.  ``labelled`` is False and
        the flow of every item is a shared all-zero array."""
        if not osp.isdir(root):
            raise FileNotFoundError(f"{root}: not a directory")
        items = []
        for d, subdirs, files in os.walk(root):
            subdirs.sort()                          # os.walk then visits them in this order
            seq = sorted(osp.join(d, f) for f in files if f.lower().endswith(FRAME_EXTENSIONS))
            items += [(a, b, "") for a, b in zip(seq, seq[1:])]
        if not items:
            raise FileNotFoundError(f"no two consecutive image files in one directory under {root}")
        return FramePairs(items)

    @classmethod
    def open(cls, root: str, dataset: str = "chairs", parts=None):
        """The list of ``dataset`` under ``root``.  ``mix``: RAFT's Sintel-stage mixture, ``parts`` a
        sequence of names or ``(name, weight)`` (default :data:`MIX_DEFAULT`), each part in its
        directory ``Sintel``, ``KITTI``, ``HD1K`` or ``FlyingThings3D`` under ``root``; a named part
        whose directory is missing is a ``FileNotFoundError``."""
        if dataset == "mix":
            named = [(p, 1) if isinstance(p, str) else (p[0], int(p[1])) for p in (parts or MIX_DEFAULT)]
            opened = []
            for name, weight in named:
                if name not in MIX_DIRS:
                    raise ValueError(f"unknown part {name!r} of a mixture (one of {sorted(MIX_DIRS)})")
                d = osp.join(root, MIX_DIRS[name])
                if not osp.isdir(d):
                    raise FileNotFoundError(f"{d}: the directory of part {name!r} is missing")
                opened.append((cls.open(d, name), weight))
            return MixedFlowPairs(opened)
        if parts is not None:
            raise ValueError("FlowPairs.open: parts belong to dataset 'mix'")
        if dataset == "frames":
            return cls.frames(root)
        if dataset == "chairs":
            return cls.chairs(root)
        if dataset in ("chairs-train", "chairs-val"):
            return cls.chairs(root, "training" if dataset == "chairs-train" else "validation")
        if dataset in ("sintel-clean", "sintel-final"):
            return cls.sintel(root, dataset.split("-")[1])
        if dataset == "kitti":
            return cls.kitti(root)
        if dataset == "hd1k":
            return cls.hd1k(root)
        if dataset == "things":                      # both passes, as RAFT's things stage uses them
            return cls(cls.things(root, "clean").items + cls.things(root, "final").items)
        if dataset in ("things-clean", "things-final"):
            return cls.things(root, dataset.split("-")[1])
        raise ValueError(f"unknown dataset {dataset!r} (chairs, chairs-train, chairs-val, sintel-clean, sintel-final, kitti, hd1k, things, "
                         "things-clean, things-final, mix, frames)")

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
        if f.endswith(".pfm"):                      # a view of the file's bytes: the caller's copy is the only one
            return read_frame(a), read_frame(b), read_pfm(f)[..., :2]
        try:
            flow = read_flo(f)
        except (ValueError, IndexError) as e:   # a truncated file: short header or short data
            raise ValueError(f"unreadable .flo file {f}: {e}") from None
        if flow is None:
            raise ValueError(f"unreadable .flo file {f}: bad magic")
        return read_frame(a), read_frame(b), flow


FRAME_EXTENSIONS = (".png", ".ppm", ".jpg", ".jpeg", ".bmp")


class FramePairs(FlowPairs):
    """Consecutive frames of video, without ground truth (``FlowPairs.frames``): ``ds[i] -> (image1,
    image2, zeros fp32 (H, W, 2))``.  The flow is ONE shared all-zero array of the first frame's
    size, there only so that the loader and the augmentation ops stay as they are; nothing may
    write to it or read a label out of it (``labelled`` is False).  The loader rejects a frame of
    another size."""

    labelled = False

    def __init__(self, items):
        super().__init__(items)
        self._zero = None

    def __getitem__(self, i: int):
        a, b, _ = self.items[i]
        if self._zero is None:
            zero = np.zeros(frame_size(self.items[0][0]) + (2,), dtype=np.float32)
            zero.setflags(write=False)
            self._zero = zero
        return read_frame(a), read_frame(b), self._zero


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


class MixedFlowPairs:
    """A weighted mixture of lists, dense and sparse: ``parts`` is a sequence of ``(FlowPairs |
    SparseFlowPairs, weight)``.  The index space is the concatenation of every part repeated
    ``weight`` times -- ``len`` is the sum of ``weight * len(part)`` -- and item ``i`` maps to
    ``(part, i mod len(part))`` inside its part's stretch; nothing is materialised.  Per item:
    ``dense(i)`` and ``size(i)`` = (Hs, Ws), read from the files' headers once per part here.  A dense
    part has one frame size (another is a ``ValueError`` naming the file); a sparse part may have several."""

    mixed = True

    def __init__(self, parts):
        self.parts = [(p, int(w)) for p, w in parts]
        if not self.parts:
            raise ValueError("MixedFlowPairs: no parts")
        self._ends, self._sizes, total = [], [], 0
        for part, weight in self.parts:
            if weight < 1:
                raise ValueError(f"MixedFlowPairs: weight {weight} (a positive integer wanted)")
            sizes = [frame_size(t[0]) for t in part.items]
            if not getattr(part, "sparse", False):
                for t, s in zip(part.items, sizes):
                    if s != sizes[0]:
                        raise ValueError(f"{t[0]}: frame size {s} differs from the part's {sizes[0]} "
                                         "(a dense part has one frame size)")
                sizes = sizes[:1]
            self._sizes.append(sizes)
            total += weight * len(part)
            self._ends.append(total)
        self.slot_pixels = max(h * w for sizes in self._sizes for h, w in sizes)

    def __len__(self) -> int:
        return self._ends[-1]

    def locate(self, i: int) -> Tuple[int, int]:
        """Item ``i`` -> (index of its part, index inside the part)."""
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        k = int(np.searchsorted(self._ends, i, side="right"))
        return k, (i - (self._ends[k - 1] if k else 0)) % len(self.parts[k][0])

    def dense(self, i: int) -> bool:
        return not getattr(self.parts[self.locate(i)[0]][0], "sparse", False)

    def size(self, i: int) -> Tuple[int, int]:
        k, j = self.locate(i)
        return self._sizes[k][j if len(self._sizes[k]) > 1 else 0]

    def paths(self, i: int) -> Tuple[str, str, str]:
        k, j = self.locate(i)
        return self.parts[k][0].items[j]

    def sizes(self) -> List[Tuple[int, int]]:
        """Every frame size that occurs (not one per item)."""
        return sorted({s for sizes in self._sizes for s in sizes})

    def __getitem__(self, i: int):
        k, j = self.locate(i)
        return self.parts[k][0][j]


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

    Over a :class:`MixedFlowPairs` the slots are packed: buffers ``(B, S, 3)`` uint8 x 2, ``(B, S, 2)``
    fp32 and ``(B, S)`` uint8 with ``S = slot_pixels``, the largest ``Hs * Ws`` of the list; sample
    ``n`` is the first ``Hs * Ws`` pixels of slot ``n`` with row pitch ``Ws``.  ``fetch`` uploads only
    those prefixes (the valid prefix of sparse samples only), returns ``(image1, image2, flow, valid,
    sizes, dense_flags)`` and leaves the bytes it queued in ``last_upload_bytes``.  A dense sample's
    valid bytes and everything past a prefix are unspecified.
    """

    def __init__(self, dataset: FlowPairs, batch: int, seed: int = 0, rank: int = 0, world: int = 1,
                 device=None, depth: int = 3):
        self.ds, self.batch, self.seed, self.rank, self.world = dataset, int(batch), int(seed), int(rank), int(world)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.steps_per_epoch = len(dataset) // (self.batch * self.world)
        if self.steps_per_epoch < 1:
            raise ValueError(f"{len(dataset)} pairs do not fill one batch of {self.batch} on {self.world} rank(s)")
        self.sparse = bool(getattr(dataset, "sparse", False))
        self.mixed = bool(getattr(dataset, "mixed", False))
        self.last_upload_bytes = 0
        if self.mixed:
            sizes = dataset.sizes()
            self.slot_pixels = dataset.slot_pixels
            self.frame_max = (max(s[0] for s in sizes), max(s[1] for s in sizes))
            self.frame_min = (min(s[0] for s in sizes), min(s[1] for s in sizes))
            self.frame = None                      # there is no one frame: the slots are packed
        elif self.sparse:
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
        if self._slots[slot] is None and self.mixed:
            B, S = self.batch, self.slot_pixels
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=self._pin)
            self._slots[slot] = (mk((B, S, 3), torch.uint8), mk((B, S, 3), torch.uint8), mk((B, S, 2), torch.float32),
                                 mk((B, S), torch.uint8))
        if self._slots[slot] is None:
            H, W = self.frame
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=self._pin)
            self._slots[slot] = (mk((self.batch, H, W, 3), torch.uint8), mk((self.batch, H, W, 3), torch.uint8),
                                 mk((self.batch, H, W, 2), torch.float32))
            if self.sparse:
                self._slots[slot] += (mk((self.batch, H, W), torch.uint8),)
        return self._slots[slot]

    def _decode_one(self, bufs, n: int, index: int) -> None:
        if self.mixed:
            arrs = self.ds[index]                  # 3 arrays of a dense item, 4 of a sparse one
            Hs, Ws = self.ds.size(index)
            paths = self.ds.paths(index)
            for arr, path in zip(arrs, paths + (paths[2],)):
                if tuple(arr.shape[:2]) != (Hs, Ws):
                    raise ValueError(f"{path}: size {tuple(arr.shape[:2])} differs from the frame size {(Hs, Ws)} of its list")
            for buf, arr in zip(bufs, arrs):       # the slot's prefix, row pitch Ws; the rest stays as it is
                np.copyto(buf[n].numpy()[:Hs * Ws].reshape((Hs, Ws) + arr.shape[2:]), arr)
            return
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
        if self.mixed:
            return [self.ds.size(i) for i in self.indices_for(step)]
        return [self._sizes[i] if self.sparse else self.frame for i in self.indices_for(step)]

    def dense_for(self, step: int) -> List[bool]:
        """Whether each sample of ``step`` has dense ground truth (a mixed list)."""
        return [self.ds.dense(i) for i in self.indices_for(step)]

    def _fetch_mixed(self, step: int):
        bufs = self.host_batch(step)
        sizes, dense = self.sizes_for(step), self.dense_for(step)
        cuda = self.device.type == "cuda"
        out = tuple(torch.empty(b.shape, dtype=b.dtype, device=self.device) for b in bufs)
        queued = 0
        for n, ((Hs, Ws), d) in enumerate(zip(sizes, dense)):
            for dst, src in zip(out[:3 if d else 4], bufs):
                dst[n, :Hs * Ws].copy_(src[n, :Hs * Ws], non_blocking=cuda)
                queued += Hs * Ws * src[n, :1].numel() * src.element_size()
        self.last_upload_bytes = queued
        if cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._events[step % self.depth] = ev
        self.prefetch(step + 1)
        return out + (sizes, dense)

    def fetch(self, step: int):
        if self.mixed:
            return self._fetch_mixed(step)
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


class SequentialLoader:
    """The pairs of a list in order, for validation: rank ``r`` of ``world`` takes items ``r, r + world,
    ...`` of the first ``max_pairs`` (all by default); consecutive items of one frame size form
    batches of up to ``batch`` and the tail is kept as a smaller batch.  A sparse list (several frame
    sizes) runs batch 1.

    Iterating yields ``(image1 uint8 (k, H, W, 3), image2, flow fp32 (k, H, W, 2), valid uint8 (k, H, W)
    or None, indices)`` on ``device``, each batch at its own frame size.  The next batch is decoded
    by at most ``decode_threads()`` threads into a ring of pinned staging buffers -- the items
    through the dataset's own ``__getitem__``, as :class:`PairLoader` reads them -- while the
    caller works on the current one; the uploads are ``non_blocking`` on the current stream."""

    def __init__(self, dataset: FlowPairs, batch: int = 4, rank: int = 0, world: int = 1, device=None,
                 max_pairs: Optional[int] = None, depth: int = 3):
        self.ds = dataset
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.sparse = bool(getattr(dataset, "sparse", False))
        if getattr(dataset, "mixed", False):
            raise ValueError("SequentialLoader: a mixture is a training list, not a validation split")
        self.pairs = len(dataset) if max_pairs is None else max(0, min(len(dataset), int(max_pairs)))
        self.indices = list(range(int(rank), self.pairs, int(world)))
        sizes = {i: frame_size(dataset.items[i][0]) for i in self.indices}
        bs = 1 if self.sparse else max(1, int(batch))
        self.batches: List[List[int]] = []
        for i in self.indices:
            last = self.batches[-1] if self.batches else None
            if last is not None and len(last) < bs and sizes[last[0]] == sizes[i]:
                last.append(i)
            else:
                self.batches.append([i])
        self._sizes = sizes
        self._cap = bs * max((h * w for h, w in sizes.values()), default=0)   # pixels of the largest batch
        self.depth = max(2, int(depth))
        self._pin = self.device.type == "cuda"
        self._slots = [None] * self.depth
        self._events = [None] * self.depth
        self._pool = ThreadPoolExecutor(decode_threads(), thread_name_prefix="val-decode")
        self._worker = ThreadPoolExecutor(1, thread_name_prefix="val-loader")

    def __len__(self) -> int:
        return len(self.batches)

    def _staging(self, slot: int, k: int, size: Tuple[int, int]):
        """Views (k, H, W, C) of the slot's flat pinned buffers."""
        if self._slots[slot] is None:
            mk = lambda n, dt: torch.empty(n, dtype=dt, pin_memory=self._pin)
            self._slots[slot] = (mk(self._cap * 3, torch.uint8), mk(self._cap * 3, torch.uint8),
                                 mk(self._cap * 2, torch.float32)) + ((mk(self._cap, torch.uint8),) if self.sparse else ())
        H, W = size
        return tuple(buf[:k * H * W * c].view((k, H, W) + ((c,) if c > 1 else ()))
                     for buf, c in zip(self._slots[slot], (3, 3, 2, 1)))

    def _decode_one(self, views, n: int, index: int, size: Tuple[int, int]) -> None:
        arrs = self.ds[index]                      # 3 arrays of a dense item, 4 of a sparse one
        paths = self.ds.items[index] + (self.ds.items[index][2],)
        for arr, path in zip(arrs, paths):
            if tuple(arr.shape[:2]) != size:
                raise ValueError(f"{path}: size {tuple(arr.shape[:2])} differs from the pair's first image {size}")
        for view, arr in zip(views, arrs):
            np.copyto(view[n].numpy(), arr)

    def _decode(self, k: int):
        slot, idx = k % self.depth, self.batches[k]
        ev = self._events[slot]
        while ev is not None and not ev.query():   # the upload that read this slot (depth - 1 batches ago)
            time.sleep(2e-4)
        size = self._sizes[idx[0]]
        views = self._staging(slot, len(idx), size)
        for r in [self._pool.submit(self._decode_one, views, n, i, size) for n, i in enumerate(idx)]:
            r.result()
        return views

    def __iter__(self):
        cuda = self.device.type == "cuda"
        fut = self._worker.submit(self._decode, 0) if self.batches else None
        for k, idx in enumerate(self.batches):
            views = fut.result()
            fut = self._worker.submit(self._decode, k + 1) if k + 1 < len(self.batches) else None
            if cuda:
                out = tuple(torch.empty(v.shape, dtype=v.dtype, device=self.device).copy_(v, non_blocking=True) for v in views)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(self.device))
                self._events[k % self.depth] = ev
            else:
                out = tuple(v.clone() for v in views)
            yield out[0], out[1], out[2], (out[3] if self.sparse else None), list(idx)

    def close(self) -> None:
        self._worker.shutdown(wait=True)
        self._pool.shutdown(wait=True)
