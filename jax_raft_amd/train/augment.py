"""RAFT's dense flow augmentation as one gather: the golden op and its host-side sampler.

``augment_pairs`` is this project's own definition of the dense ``FlowAugmentor`` of the
original RAFT recipe (photometric jitter, an eraser occlusion on image 2, random scale and
stretch, flips, a random crop), written as ONE gather over the uint8 source frames: every
output pixel is computed from 4 source taps, nothing is resized or cropped in between.  The
semantics are fixed here as a sequence of fp32 operations, each product and sum rounded on its
own; ``csrc/kernels/augment.hip`` equals this op bit for bit (``ops/native.py:augment_pairs``
runs this op on CPU tensors and the kernels on GPU tensors).

Per sample the host draws one record (:class:`AugmentParams`): the resized size (Hr, Wr), the
fp32 ratios Ws/Wr, Hs/Hr and their inverses, the crop origin (y0, x0) in the resized image, the
flip flags, per image brightness b, contrast k, saturation s and a 3x3 hue matrix (the YIQ
rotation, rounded to fp32), and up to two eraser rectangles in source pixels of image 2.  The
host computes every ratio, reciprocal and matrix once: golden and kernel only add, multiply,
compare, floor and divide by 255.

Per output pixel (y, x) of sample n:

1. u = x + x0, mirrored to Wr - 1 - u on an h-flip; src_x = (u + 0.5) * (Ws/Wr) - 0.5 clamped
   to [0, Ws - 1]; x_lo = floor(src_x), x_hi = min(x_lo + 1, Ws - 1), wx = src_x - x_lo.  The
   same in y.  Tap coordinates are clamped whatever the record says.
2. Each of the 4 taps of each image is transformed as a texel (r, g, b) in [0, 255], clamped to
   [0, 255] after every step: eraser (image 2: a tap whose integer source coordinate lies in a
   rectangle becomes the image's mean colour, ``(sum + N // 2) // N`` per channel from the
   exact integer sums), brightness ``c * b``, contrast ``(c - m) * k + m`` with
   ``m = min(255, b * L)`` and L the luma of that image's mean colour, saturation
   ``(c - g) * s + g`` with g the texel's own luma, hue ``M c``.  Luma is
   ``(0.299 r + 0.587 g) + 0.114 b``; a matrix row is ``(M0 r + M1 g) + M2 b``.
   A contrast or saturation factor of exactly 1 leaves the texel as it is (``(c - m) + m`` is
   not c in fp32): that is what makes the identity record a plain crop.
3. The image value is the bilinear blend ``top = t00 + wx (t01 - t00)``, ``bot`` alike,
   ``top + wy (bot - top)``, then ``v / 255 * 2 - 1`` (``utils/flow_io.py:normalize_image``).
4. The flow is the same blend of the 4 flow taps, times (Wr/Ws, Hr/Hs), negated on a flipped
   axis; valid = 1 iff |fx| < 1000 and |fy| < 1000 (false for NaN), and the flow written where
   valid = 0 is 0 (the sequence loss multiplies by the mask, and 0 * NaN would poison it).

An identity record (Hr, Wr = Hs, Ws, no flips, factors 1, identity hue, no rectangles) is a
plain crop plus normalisation: the ``augment=False`` path is this op with such records.

Sparse ground truth (KITTI, HD1K) has an op of its own, :func:`augment_pairs_sparse`, with records
that also carry each sample's size (:class:`SparseAugmentParams`, :func:`sample_sparse`): the
images as above, the flow moved point by point (its docstring; ``augment.hip``'s sparse layout).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

# record layout (one sample: 16 int32 words + 32 fp32 words; csrc/kernels/augment.hip reads the same)
N_INTS, N_FLOATS = 16, 32
I_HR, I_WR, I_Y0, I_X0, I_HFLIP, I_VFLIP, I_NRECT, I_RECT = 0, 1, 2, 3, 4, 5, 6, 8   # rect: (x0, y0, x1, y1) x 2
F_SX, F_SY, F_ISX, F_ISY, F_COL1, F_COL2 = 0, 1, 2, 3, 4, 16                         # colour: b, k, s, M[9]
MAX_RESIZED = 1 << 16
MAX_FLOW = 1000.0


@dataclass(frozen=True)
class Stage:
    min_scale: float
    max_scale: float
    crop: Tuple[int, int]


# RAFT's dense-augmentor presets per training stage
STAGES = {
    "chairs": Stage(-0.1, 1.0, (368, 496)),
    "things": Stage(-0.4, 0.8, (400, 720)),
    "sintel": Stage(-0.2, 0.6, (368, 768)),
}

_YIQ = np.array([[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523, 0.312]], dtype=np.float64)
_YIQ_INV = np.linalg.inv(_YIQ)


def hue_matrix(theta: float) -> np.ndarray:
    """The RGB matrix of a rotation by ``theta`` radians in the IQ plane of YIQ, rounded to fp32."""
    if theta == 0.0:
        return np.eye(3, dtype=np.float32)
    c, s = math.cos(theta), math.sin(theta)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]], dtype=np.float64)
    return (_YIQ_INV @ rot @ _YIQ).astype(np.float32)


def _colour_words(colour) -> np.ndarray:
    b, k, s, theta = (1.0, 1.0, 1.0, 0.0) if colour is None else colour
    return np.concatenate([np.array([b, k, s], dtype=np.float32), hue_matrix(float(theta)).reshape(9)])


def _draw_dense(g, st: Stage, src, h: int, w: int, augment: bool):
    """The draws of one dense sample from generator ``g``, in RAFT's order: the arguments of
    ``AugmentParams.record`` after ``src``."""
    Hs, Ws = src
    sx = sy = 1.0
    if augment and g.random() < 0.8:            # spatial augmentation
        floor_ = max((h + 8) / Hs, (w + 8) / Ws)
        sx = sy = 2.0 ** g.uniform(st.min_scale, st.max_scale)
        if g.random() < 0.8:                    # stretch
            sx *= 2.0 ** g.uniform(-0.2, 0.2)
            sy *= 2.0 ** g.uniform(-0.2, 0.2)
        sx, sy = max(sx, floor_), max(sy, floor_)
    Hr, Wr = max(h, int(round(Hs * sy))), max(w, int(round(Ws * sx)))
    hflip = bool(augment and g.random() < 0.5)
    vflip = bool(augment and g.random() < 0.1)
    y0, x0 = int(g.integers(0, Hr - h + 1)), int(g.integers(0, Wr - w + 1))
    c1 = c2 = None
    rects = []
    if augment:
        def colour():
            b, k, s = g.uniform(0.6, 1.4, 3)
            return float(b), float(k), float(s), 2.0 * math.pi * g.uniform(-0.5 / 3.14, 0.5 / 3.14)
        c1 = colour()
        c2 = colour() if g.random() < 0.2 else c1          # asymmetric
        if g.random() < 0.5:                               # eraser
            for _ in range(int(g.integers(1, 3))):
                rx, ry = int(g.integers(0, Ws)), int(g.integers(0, Hs))
                dx, dy = int(g.integers(50, 101)), int(g.integers(50, 101))
                rects.append((rx, ry, rx + dx, ry + dy))
    return (Hr, Wr), (y0, x0), hflip, vflip, c1, c2, rects


def _draw_sparse(g, st: Stage, p_hflip: float, src, h: int, w: int, augment: bool):
    """The draws of one sparse sample (``sample_sparse``), as :func:`_draw_dense` returns them."""
    Hs, Ws = src
    scale = 1.0
    if augment and g.random() < 0.8:                # spatial augmentation
        scale = max(2.0 ** g.uniform(st.min_scale, st.max_scale), (h + 1) / Hs, (w + 1) / Ws)
    Hr, Wr = max(h, int(round(Hs * scale))), max(w, int(round(Ws * scale)))
    hflip = bool(augment and g.random() < p_hflip)
    y0 = int(np.clip(g.integers(0, Hr - h + 20), 0, Hr - h))
    x0 = int(np.clip(g.integers(-50, Wr - w + 50), 0, Wr - w))
    colour, rects = None, []
    if augment:
        b, k, s = g.uniform(0.6, 1.4, 3)
        colour = (float(b), float(k), float(s), 2.0 * math.pi * g.uniform(-0.5 / 3.14, 0.5 / 3.14))
        if g.random() < 0.5:                        # eraser
            for _ in range(int(g.integers(1, 3))):
                rx, ry = int(g.integers(0, Ws)), int(g.integers(0, Hs))
                dx, dy = int(g.integers(50, 101)), int(g.integers(50, 101))
                rects.append((rx, ry, rx + dx, ry + dy))
    return (Hr, Wr), (y0, x0), hflip, False, colour, colour, rects


def _constancy_safe(draws):
    """The same draws with what breaks brightness constancy taken out (label-free training,
    train/unsup.py): image 2 gets image 1's colour and no eraser rectangle.  Every draw has
    been consumed, so every other word of the record is that of the unrestricted one."""
    size, origin, hflip, vflip, c1, _c2, _rects = draws
    return size, origin, hflip, vflip, c1, c1, []


class AugmentParams:
    """The records of one batch, on the host: ``ints`` (B, 16) int32 and ``floats`` (B, 32) fp32."""

    def __init__(self, ints: np.ndarray, floats: np.ndarray):
        self.ints = np.ascontiguousarray(ints, dtype=np.int32).reshape(-1, N_INTS)
        self.floats = np.ascontiguousarray(floats, dtype=np.float32).reshape(-1, N_FLOATS)
        if len(self.ints) != len(self.floats):
            raise ValueError("AugmentParams: ints and floats of different batch sizes")

    def __len__(self) -> int:
        return len(self.ints)

    def __eq__(self, other) -> bool:
        return (isinstance(other, AugmentParams) and np.array_equal(self.ints, other.ints)
                and np.array_equal(self.floats.view(np.int32), other.floats.view(np.int32)))

    # ------------------------------------------------------------ construction
    @classmethod
    def record(cls, src: Tuple[int, int], resized: Optional[Tuple[int, int]] = None, origin: Tuple[int, int] = (0, 0),
               hflip: bool = False, vflip: bool = False, colour1=None, colour2=None,
               rects: Sequence[Tuple[int, int, int, int]] = ()) -> "AugmentParams":
        """One record.  ``colour``: (b, k, s, hue angle in radians) or None for none;
        ``rects``: up to two (x0, y0, x1, y1), upper bounds exclusive, in source pixels."""
        Hs, Ws = src
        Hr, Wr = resized or src
        if len(rects) > 2:
            raise ValueError("AugmentParams: at most two eraser rectangles")
        ints = np.zeros(N_INTS, dtype=np.int32)
        ints[[I_HR, I_WR, I_Y0, I_X0, I_HFLIP, I_VFLIP, I_NRECT]] = [Hr, Wr, origin[0], origin[1], bool(hflip),
                                                                    bool(vflip), len(rects)]
        for j, r in enumerate(rects):
            ints[I_RECT + 4 * j:I_RECT + 4 * j + 4] = r
        floats = np.zeros(N_FLOATS, dtype=np.float32)
        floats[[F_SX, F_SY, F_ISX, F_ISY]] = [Ws / Wr, Hs / Hr, Wr / Ws, Hr / Hs]
        floats[F_COL1:F_COL1 + 12] = _colour_words(colour1)
        floats[F_COL2:F_COL2 + 12] = _colour_words(colour2)
        return cls(ints[None], floats[None])

    @classmethod
    def cat(cls, records: Sequence["AugmentParams"]) -> "AugmentParams":
        return cls(np.concatenate([r.ints for r in records]), np.concatenate([r.floats for r in records]))

    @classmethod
    def identity(cls, batch: int, src: Tuple[int, int], origin: Tuple[int, int] = (0, 0)) -> "AugmentParams":
        return cls.cat([cls.record(src, origin=origin)] * batch)

    @classmethod
    def sample(cls, batch: int, src: Tuple[int, int], stage: str = "chairs", crop: Optional[Tuple[int, int]] = None,
               seed: int = 0, step: int = 0, rank: int = 0, augment: bool = True,
               constancy: bool = False) -> "AugmentParams":
        """``batch`` records drawn from RAFT's dense-augmentor distributions, a pure function of
        (seed, step, rank, sample index).  ``augment=False``: identity records with a random crop.
        ``constancy=True``: the same draws, but colour 2 = colour 1 and no eraser rectangles."""
        if stage not in STAGES:
            raise ValueError(f"unknown augmentation stage {stage!r} (one of {sorted(STAGES)})")
        st = STAGES[stage]
        h, w = crop or st.crop
        Hs, Ws = src
        if Hs < h or Ws < w:
            raise ValueError(f"source {Hs}x{Ws} is smaller than the crop {h}x{w}")
        safe = _constancy_safe if constancy else (lambda d: d)
        return cls.cat([AugmentParams.record(src, *safe(_draw_dense(np.random.default_rng([int(seed), int(step), int(rank), n]),
                                                                    st, src, h, w, augment))) for n in range(batch)])

    # -------------------------------------------------------------- validation
    def validate(self, src: Tuple[int, int], crop: Tuple[int, int]) -> None:
        """Host-side check of every record before it is uploaded; ``ValueError`` on the first bad one."""
        Hs, Ws = src
        h, w = crop
        if h < 1 or w < 1 or Hs < 1 or Ws < 1:
            raise ValueError("augment: empty source or crop")
        if Hs < h or Ws < w:
            raise ValueError(f"augment: source {Hs}x{Ws} is smaller than the crop {h}x{w}")
        i, f = self.ints.astype(np.int64), self.floats
        Hr, Wr, y0, x0 = i[:, I_HR], i[:, I_WR], i[:, I_Y0], i[:, I_X0]
        checks = (
            ("the crop is larger than the resized size", (Hr < h) | (Wr < w)),
            ("the resized size is out of range", (Hr > MAX_RESIZED) | (Wr > MAX_RESIZED)),
            ("the crop origin lies outside the resized image", (y0 < 0) | (x0 < 0) | (y0 > Hr - h) | (x0 > Wr - w)),
            ("flip flags must be 0 or 1", (i[:, I_HFLIP] & ~1 != 0) | (i[:, I_VFLIP] & ~1 != 0)),
            ("0..2 eraser rectangles", (i[:, I_NRECT] < 0) | (i[:, I_NRECT] > 2)),
            ("non-finite parameter", ~np.isfinite(f).all(axis=1)),
            ("negative colour factor", (f[:, F_COL1:F_COL1 + 3] < 0).any(axis=1) | (f[:, F_COL2:F_COL2 + 3] < 0).any(axis=1)),
            ("the ratios do not belong to the resized size",
             (f[:, F_SX] != (Ws / Wr).astype(np.float32)) | (f[:, F_SY] != (Hs / Hr).astype(np.float32))
             | (f[:, F_ISX] != (Wr / Ws).astype(np.float32)) | (f[:, F_ISY] != (Hr / Hs).astype(np.float32))),
        )
        for what, bad in checks:
            if bad.any():
                raise ValueError(f"augment: record {int(np.argmax(bad))}: {what}")

    def packed(self, pin: bool = False) -> torch.Tensor:
        """(B, 48) int32 words (the fp32 words bit-cast), the form the kernel reads."""
        words = torch.from_numpy(np.concatenate([self.ints, self.floats.view(np.int32)], axis=1))
        if pin:
            buf = torch.empty(words.shape, dtype=torch.int32, pin_memory=True)
            buf.copy_(words)
            return buf
        return words


# ---------------------------------------------------------------------- golden
def colour_sums(img_u8: torch.Tensor) -> torch.Tensor:
    """Exact per-channel integer sums of (B, Hs, Ws, 3) uint8 frames -> (B, 3) int64."""
    return img_u8.to(torch.int64).sum((1, 2))


def _luma(r, g, b):
    return (r * 0.299 + g * 0.587) + b * 0.114


def _clamp(c):
    return c.clamp(0.0, 255.0)


def _texel(c, col, m):
    """Brightness, contrast, saturation, hue of texels c = (r, g, b); col (B, 12) fp32, m (B,) fp32."""
    v = lambda j: col[:, j].view(-1, 1, 1)
    b_, k_, s_ = v(0), v(1), v(2)
    m = m.view(-1, 1, 1)
    c = [_clamp(x * b_) for x in c]
    c = [_clamp(torch.where(k_ == 1.0, x, (x - m) * k_ + m)) for x in c]
    g = _luma(*c)
    c = [_clamp(torch.where(s_ == 1.0, x, (x - g) * s_ + g)) for x in c]
    return [_clamp((c[0] * v(3 + 3 * j) + c[1] * v(4 + 3 * j)) + c[2] * v(5 + 3 * j)) for j in range(3)]


def _blend(t00, t01, t10, t11, wx, wy):
    top = t00 + wx * (t01 - t00)
    bot = t10 + wx * (t11 - t10)
    return top + wy * (bot - top)


def _records_on(params, dev):
    """The records as device tensors and accessors of one int / float word as (B, 1, 1)."""
    B = len(params)
    pi = torch.from_numpy(params.ints).to(dev).long()
    pf = torch.from_numpy(params.floats).to(dev)
    return pi, pf, (lambda j: pi[:, j].view(B, 1, 1)), (lambda j: pf[:, j].view(B, 1, 1))


def _gather_images(img1_u8, img2_u8, pi, pf, h, w):
    """Steps 1-3 of the module docstring on (B, Hs, Ws, 3) frames that ARE the samples (no padding):
    (image1, image2), and the taps and weights for a caller that blends more."""
    B, Hs, Ws, _ = img1_u8.shape
    dev = img1_u8.device
    icol = lambda j: pi[:, j].view(B, 1, 1)
    fcol = lambda j: pf[:, j].view(B, 1, 1)

    def axis(n, o, size_r, flip, ratio, size_s, shape):
        u = torch.arange(n, device=dev).view(shape) + o
        u = torch.where(flip != 0, size_r - 1 - u, u)
        s = ((u.float() + 0.5) * ratio - 0.5).clamp(0.0, float(size_s - 1))
        lo = s.floor()
        wgt = s - lo
        lo = lo.long().clamp(0, size_s - 1)
        return lo, (lo + 1).clamp(max=size_s - 1), wgt

    x_lo, x_hi, wx = axis(w, icol(I_X0), icol(I_WR), icol(I_HFLIP), fcol(F_SX), Ws, (1, 1, w))
    y_lo, y_hi, wy = axis(h, icol(I_Y0), icol(I_HR), icol(I_VFLIP), fcol(F_SY), Hs, (1, h, 1))
    bidx = torch.arange(B, device=dev).view(B, 1, 1)
    taps = ((y_lo, x_lo), (y_lo, x_hi), (y_hi, x_lo), (y_hi, x_hi))
    N = Hs * Ws

    images = []
    for k, img in enumerate((img1_u8, img2_u8)):
        mean = ((colour_sums(img) + N // 2) // N).float()                    # (B, 3), integers 0..255
        col = pf[:, (F_COL1, F_COL2)[k]:(F_COL1, F_COL2)[k] + 12]
        m = (col[:, 0] * _luma(mean[:, 0], mean[:, 1], mean[:, 2])).clamp(max=255.0)
        tex = []
        for yi, xi in taps:
            t = img[bidx, yi, xi].float()                                    # (B, h, w, 3)
            if k == 1:
                inside = torch.zeros((B, h, w), dtype=torch.bool, device=dev)
                for j in range(2):
                    r = [icol(I_RECT + 4 * j + q) for q in range(4)]
                    inside |= (icol(I_NRECT) > j) & (xi >= r[0]) & (xi < r[2]) & (yi >= r[1]) & (yi < r[3])
                t = torch.where(inside[..., None], mean.view(B, 1, 1, 3), t)
            tex.append(_texel([t[..., 0], t[..., 1], t[..., 2]], col, m))
        chans = [_blend(tex[0][c], tex[1][c], tex[2][c], tex[3][c], wx, wy) / 255.0 * 2.0 - 1.0 for c in range(3)]
        images.append(torch.stack(chans, dim=-1).contiguous())
    return images[0], images[1], bidx, taps, wx, wy


@torch.no_grad()
def augment_pairs(img1_u8: torch.Tensor, img2_u8: torch.Tensor, flow: torch.Tensor, params: AugmentParams,
                  crop: Tuple[int, int]):
    """The golden op (module docstring): (B, Hs, Ws, 3) uint8 x 2, (B, Hs, Ws, 2) fp32 flow ->
    image1, image2 (B, h, w, 3) fp32 in [-1, 1], flow (B, h, w, 2) fp32, valid (B, h, w) fp32."""
    B, Hs, Ws = check_batch("augment_pairs", img1_u8, img2_u8, flow, None, params)
    h, w = crop
    params.validate((Hs, Ws), (h, w))
    dev = img1_u8.device
    pi, pf, icol, fcol = _records_on(params, dev)
    image1, image2, bidx, taps, wx, wy = _gather_images(img1_u8, img2_u8, pi, pf, h, w)

    ft = [flow[bidx, yi, xi] for yi, xi in taps]
    fx = _blend(*[t[..., 0] for t in ft], wx, wy) * fcol(F_ISX)
    fy = _blend(*[t[..., 1] for t in ft], wx, wy) * fcol(F_ISY)
    fx = torch.where(icol(I_HFLIP) != 0, -fx, fx)
    fy = torch.where(icol(I_VFLIP) != 0, -fy, fy)
    valid = (fx.abs() < MAX_FLOW) & (fy.abs() < MAX_FLOW)
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    out_flow = torch.stack([torch.where(valid, fx, zero), torch.where(valid, fy, zero)], dim=-1).contiguous()
    return image1, image2, out_flow, valid.float()


# ------------------------------------------------------- sparse ground truth
# RAFT's ``SparseFlowAugmentor`` (KITTI, HD1K).  The samples of a batch have sizes of their own
# and sit in the top-left corners of (B, Hb, Wb, ...) buffers.
# record layout (one sample: 20 int32 words + 32 fp32 words; csrc/kernels/augment.hip reads
# the same): words 0..15 of the ints and all floats are the dense record's, then the sample's size
N_INTS_SPARSE = 20
I_HS, I_WS = 16, 17
MAX_RATIO = 4.0        # Ws / Wr, Hs / Hr at most: bounds the kernel's scan
MAX_SCAN = 16          # candidates per axis the kernel scans at most (a valid record needs sx + 5 <= 9)

# RAFT's sparse-augmentor presets: ``kitti`` is the fine-tuning stage of its own, ``sintel`` what
# KITTI / HD1K get inside the Sintel stage (no stretch in either)
SPARSE_STAGES = {
    "kitti": Stage(-0.2, 0.4, (288, 960)),
    "sintel": Stage(-0.3, 0.5, (368, 768)),
}
_SPARSE_HFLIP = {"kitti": 0.0, "sintel": 0.5}


def scan_window(T, ratio, size: int):
    """The source indices ``lo .. hi`` the kernel scans for landers on target ``T`` (an int or an
    array), the formula of ``augment_common.h:scan_window`` in fp32: ``floor((T - 0.5) * ratio)
    - 1 .. ceil((T + 0.5) * ratio) + 1`` clamped to ``[0, size - 1]``.  ``fp32(s) * inv`` is
    monotone in s and ``rint(.) == T`` needs it within 0.5 of T up to rounding, far inside the
    margin of 1."""
    T = np.asarray(T, dtype=np.float32)
    ratio = np.float32(ratio)
    lo = np.maximum(np.floor((T - np.float32(0.5)) * ratio).astype(np.int64) - 1, 0)
    hi = np.minimum(np.ceil((T + np.float32(0.5)) * ratio).astype(np.int64) + 1, size - 1)
    return np.maximum(lo, hi - (MAX_SCAN - 1)), hi


class SparseAugmentParams(AugmentParams):
    """The records of one batch of samples with sizes of their own: ``ints`` (B, 20) int32 -- the
    dense record's 16 words, then (Hs, Ws) -- and ``floats`` (B, 32) fp32 as in the dense record."""

    def __init__(self, ints: np.ndarray, floats: np.ndarray):
        self.ints = np.ascontiguousarray(ints, dtype=np.int32).reshape(-1, N_INTS_SPARSE)
        self.floats = np.ascontiguousarray(floats, dtype=np.float32).reshape(-1, N_FLOATS)
        if len(self.ints) != len(self.floats):
            raise ValueError("SparseAugmentParams: ints and floats of different batch sizes")

    def __eq__(self, other) -> bool:
        return (isinstance(other, SparseAugmentParams) and np.array_equal(self.ints, other.ints)
                and np.array_equal(self.floats.view(np.int32), other.floats.view(np.int32)))

    @property
    def sizes(self):
        return [(int(a), int(b)) for a, b in self.ints[:, [I_HS, I_WS]]]

    @classmethod
    def record(cls, src: Tuple[int, int], *args, **kw) -> "SparseAugmentParams":
        """One record of a sample of size ``src``; the other arguments are ``AugmentParams.record``'s."""
        dense = AugmentParams.record(src, *args, **kw)
        ints = np.zeros((1, N_INTS_SPARSE), dtype=np.int32)
        ints[:, :N_INTS] = dense.ints
        ints[0, [I_HS, I_WS]] = src
        return cls(ints, dense.floats)

    @classmethod
    def identity(cls, sizes: Sequence[Tuple[int, int]], origins=None) -> "SparseAugmentParams":
        origins = origins or [(0, 0)] * len(sizes)
        return cls.cat([cls.record(s, origin=o) for s, o in zip(sizes, origins)])

    @classmethod
    def sample(cls, *a, **kw):
        raise TypeError("SparseAugmentParams: use sample_sparse (the samples have sizes of their own)")

    def validate(self, buffer: Tuple[int, int], crop: Tuple[int, int]) -> None:
        """Every record against its own sample size as the dense check does, plus: the sample fits
        the ``buffer`` (Hb, Wb), and no axis shrinks by more than :data:`MAX_RATIO`."""
        Hb, Wb = buffer
        for n in range(len(self)):
            Hs, Ws = (int(v) for v in self.ints[n, [I_HS, I_WS]])
            if Hs < 1 or Ws < 1 or Hs > Hb or Ws > Wb:
                raise ValueError(f"augment: record {n}: the sample {Hs}x{Ws} does not fit the buffer {Hb}x{Wb}")
            try:
                AugmentParams(self.ints[n:n + 1, :N_INTS], self.floats[n:n + 1]).validate((Hs, Ws), crop)
            except ValueError as e:
                raise ValueError(str(e).replace("record 0", f"record {n}")) from None
            Hr, Wr = (int(v) for v in self.ints[n, [I_HR, I_WR]])
            if Ws > MAX_RATIO * Wr or Hs > MAX_RATIO * Hr:
                raise ValueError(f"augment: record {n}: {Hs}x{Ws} -> {Hr}x{Wr} shrinks an axis by more than {MAX_RATIO:g}")

    # packed(): the base class's, (B, 52) words here


def sample_sparse(batch: int, sizes: Sequence[Tuple[int, int]], stage: str = "kitti",
                  crop: Optional[Tuple[int, int]] = None, seed: int = 0, step: int = 0, rank: int = 0,
                  augment: bool = True, constancy: bool = False) -> SparseAugmentParams:
    """``batch`` records for samples of ``sizes`` from RAFT's sparse-augmentor distributions, a pure
    function of its arguments: spatial augmentation with probability 0.8 -- one scale for both
    axes, never below ``max((h + 1) / Hs, (w + 1) / Ws)`` --, an h-flip where the preset has one,
    a crop origin drawn with margins and clipped (which pulls crops to the borders), symmetric
    colour, the eraser of ``AugmentParams.sample``.  ``augment=False``: identity records with a
    random crop.  ``constancy=True``: the same draws without the eraser rectangles."""
    if stage not in SPARSE_STAGES:
        raise ValueError(f"unknown sparse augmentation stage {stage!r} (one of {sorted(SPARSE_STAGES)})")
    if len(sizes) != batch:
        raise ValueError(f"sample_sparse: {len(sizes)} sizes for a batch of {batch}")
    st = SPARSE_STAGES[stage]
    h, w = crop or st.crop
    out = []
    for n, (Hs, Ws) in enumerate(sizes):
        if Hs < h or Ws < w:
            raise ValueError(f"source {Hs}x{Ws} is smaller than the crop {h}x{w}")
        g = np.random.default_rng([int(seed), int(step), int(rank), n])
        draws = _draw_sparse(g, st, _SPARSE_HFLIP[stage], (Hs, Ws), h, w, augment)
        out.append(SparseAugmentParams.record((Hs, Ws), *(_constancy_safe(draws) if constancy else draws)))
    return SparseAugmentParams.cat(out)


@torch.no_grad()
def augment_pairs_sparse(img1_u8: torch.Tensor, img2_u8: torch.Tensor, flow: torch.Tensor, valid_u8: torch.Tensor,
                         params: SparseAugmentParams, crop: Tuple[int, int], return_landers: bool = False):
    """The golden op for sparse ground truth, this project's definition of RAFT's
    ``SparseFlowAugmentor`` as fp32 operations: (B, Hb, Wb, 3) uint8 x 2, (B, Hb, Wb, 2) fp32 flow,
    (B, Hb, Wb) uint8 valid, sample n in the top-left (Hs, Ws) corner its record names -> the
    outputs of :func:`augment_pairs`.  Nothing outside a sample's own region is read.

    Images: steps 1-3 of the module docstring with the sample's own Hs, Ws and colour sums.

    Flow: a sparse map cannot be interpolated, it is moved point by point.  A forward map from
    every source pixel (ys, xs) with ``valid != 0``:

    1. ``X = rint(fp32(xs) * isx)``, ``Y = rint(fp32(ys) * isy)`` (half to even), isx = Wr / Ws and
       isy = Hr / Hs the record's fp32 words.
    2. The point lands iff ``0 <= X < Wr`` and ``0 <= Y < Hr`` (one that rounds to Wr is dropped).
       RAFT tests ``X > 0`` and so throws away row and column 0; this op does not, so that an
       identity record is a plain crop.
    3. Of several points on one cell the one with the largest ``ys * Ws + xs`` wins (RAFT's
       ``flow_img[yy, xx] = flow1``: the last assignment stays).
    4. The cell's value is ``(fx * isx, fy * isy)`` of the winner; a flip mirrors the cell
       (``Wr - 1 - X``, ``Hr - 1 - Y``) and negates its component; the crop subtracts (y0, x0).
    5. valid = 1 iff a point landed and both scaled components are below 1000 in magnitude
       (false for NaN; there is no fallback to another lander); the flow is 0 where valid = 0.

    Written as that forward scatter (``scatter_reduce(amax)`` of the linear source index, then a
    gather of the winners); the kernel is a gather that inverts the map, so the two are independent.
    ``return_landers``: also the number of landers per output pixel, (B, h, w) int64, and the number
    of valid points dropped at ``X == Wr`` per sample."""
    B, Hb, Wb = check_batch("augment_pairs_sparse", img1_u8, img2_u8, flow, valid_u8, params)
    h, w = crop
    params.validate((Hb, Wb), (h, w))
    dev = img1_u8.device
    outs, landers, dropped = [], [], []
    for n in range(B):
        Hs, Ws = params.sizes[n]
        one = AugmentParams(params.ints[n:n + 1, :N_INTS], params.floats[n:n + 1])
        pi, pf, _, _ = _records_on(one, dev)
        image1, image2 = _gather_images(img1_u8[n:n + 1, :Hs, :Ws], img2_u8[n:n + 1, :Hs, :Ws], pi, pf, h, w)[:2]
        Hr, Wr, y0, x0, hflip, vflip = (int(v) for v in params.ints[n, [I_HR, I_WR, I_Y0, I_X0, I_HFLIP, I_VFLIP]])
        isx, isy = pf[0, F_ISX], pf[0, F_ISY]
        # the forward scatter: the winner of a cell is the largest linear index that lands on it
        X = torch.round(torch.arange(Ws, device=dev).float() * isx).long().view(1, Ws).expand(Hs, Ws)
        Y = torch.round(torch.arange(Hs, device=dev).float() * isy).long().view(Hs, 1).expand(Hs, Ws)
        on = valid_u8[n, :Hs, :Ws] != 0
        lands = on & (X >= 0) & (X < Wr) & (Y >= 0) & (Y < Hr)
        cell = (Y * Wr + X)[lands]
        lin = torch.arange(Hs * Ws, device=dev).view(Hs, Ws)[lands]
        winner = torch.full((Hr * Wr,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, cell, lin, "amax")
        # the gather of the crop: output (y, x) is the cell (y + y0, x + x0), mirrored on a flip
        v = torch.arange(h, device=dev) + y0
        u = torch.arange(w, device=dev) + x0
        v = Hr - 1 - v if vflip else v
        u = Wr - 1 - u if hflip else u
        cells = v.view(h, 1) * Wr + u.view(1, w)
        win = winner[cells]
        landed = win >= 0
        f = flow[n, :Hs, :Ws].reshape(Hs * Ws, 2)[win.clamp(min=0)]
        fx, fy = f[..., 0] * isx, f[..., 1] * isy
        fx = -fx if hflip else fx
        fy = -fy if vflip else fy
        ok = landed & (fx.abs() < MAX_FLOW) & (fy.abs() < MAX_FLOW)
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        out_flow = torch.stack([torch.where(ok, fx, zero), torch.where(ok, fy, zero)], dim=-1)
        outs.append((image1[0], image2[0], out_flow, ok.float()))
        if return_landers:
            count = torch.zeros(Hr * Wr, dtype=torch.int64, device=dev).scatter_add(0, cell, torch.ones_like(cell))
            landers.append(count[cells])
            dropped.append(int((on & (X == Wr)).sum()))
    res = tuple(torch.stack([o[k] for o in outs]).contiguous() for k in range(4))
    return res + (torch.stack(landers), dropped) if return_landers else res


# ------------------------------------------- dense and sparse samples in one batch
# RAFT's Sintel stage draws dense lists (Sintel, FlyingThings) and sparse ones (KITTI, HD1K) into the
# same batches.  The samples sit in PACKED SLOTS: buffers (B, S, ...) with S the largest Hs * Ws, sample
# n in the first Hs * Ws pixels of slot n with row pitch Ws.  The record is the sparse one with one of
# its spare words in use (csrc/kernels/augment.hip reads the same).
I_DENSE = 18           # 1: dense ground truth (the four-tap blend), 0: sparse (the point-by-point move)


class MixedAugmentParams(SparseAugmentParams):
    """The records of a batch of dense and sparse samples: the sparse record's 52 words with
    ``ints[I_DENSE]`` = 1 for a dense sample, 0 for a sparse one."""

    def __eq__(self, other) -> bool:
        return (isinstance(other, MixedAugmentParams) and np.array_equal(self.ints, other.ints)
                and np.array_equal(self.floats.view(np.int32), other.floats.view(np.int32)))

    @property
    def dense_flags(self):
        return [bool(v) for v in self.ints[:, I_DENSE]]

    @classmethod
    def record(cls, src: Tuple[int, int], dense: bool, *args, **kw) -> "MixedAugmentParams":
        """One record of a sample of size ``src``; after ``dense`` the arguments of ``AugmentParams.record``."""
        one = SparseAugmentParams.record(src, *args, **kw)
        one.ints[0, I_DENSE] = bool(dense)
        return cls(one.ints, one.floats)

    @classmethod
    def identity(cls, sizes, dense_flags, origins=None) -> "MixedAugmentParams":
        origins = origins or [(0, 0)] * len(sizes)
        return cls.cat([cls.record(s, d, origin=o) for s, d, o in zip(sizes, dense_flags, origins)])

    def part(self, n: int):
        """Record ``n`` as the existing ops take it: ``AugmentParams`` of a dense sample,
        ``SparseAugmentParams`` of a sparse one."""
        if self.ints[n, I_DENSE]:
            return AugmentParams(self.ints[n:n + 1, :N_INTS], self.floats[n:n + 1])
        ints = self.ints[n:n + 1].copy()
        ints[0, I_DENSE] = 0
        return SparseAugmentParams(ints, self.floats[n:n + 1])

    def validate(self, slot_pixels: int, crop: Tuple[int, int]) -> None:
        """Every record against its own (Hs, Ws) as the dense check does, plus: ``Hs * Ws`` fits the
        slot, the flag is 0 or 1, and a sparse record shrinks no axis by more than :data:`MAX_RATIO`."""
        for n in range(len(self)):
            Hs, Ws, flag = (int(v) for v in self.ints[n, [I_HS, I_WS, I_DENSE]])
            if flag not in (0, 1):
                raise ValueError(f"augment: record {n}: the dense flag must be 0 or 1, got {flag}")
            if Hs < 1 or Ws < 1 or Hs * Ws > slot_pixels:
                raise ValueError(f"augment: record {n}: the sample {Hs}x{Ws} does not fit a slot of {slot_pixels} pixels")
            try:
                one = self.part(n)
                one.validate((Hs, Ws), crop)       # dense: the dense check; sparse: that plus MAX_RATIO
            except ValueError as e:
                raise ValueError(str(e).replace("record 0", f"record {n}")) from None


def sample_mixed(batch: int, sizes: Sequence[Tuple[int, int]], dense_flags: Sequence[bool], stage: str = "sintel",
                 crop: Optional[Tuple[int, int]] = None, seed: int = 0, step: int = 0, rank: int = 0,
                 augment: bool = True, constancy: bool = False) -> MixedAugmentParams:
    """``batch`` records for a mixed batch, a pure function of its arguments.  Sample ``n`` is drawn
    from ``default_rng([seed, step, rank, n])``: a dense one with exactly the draws of
    ``AugmentParams.sample`` (stretch, v-flip, asymmetric colour; ``STAGES[stage]``), a sparse one with
    exactly those of :func:`sample_sparse` (``SPARSE_STAGES[stage]``), so an all-dense or all-sparse
    batch has the existing samplers' records word for word.  ``stage`` must be in both tables.
    ``constancy=True``: the same draws, colour 2 = colour 1 and no eraser rectangles."""
    if stage not in STAGES or stage not in SPARSE_STAGES:
        raise ValueError(f"unknown mixed augmentation stage {stage!r} (one of {sorted(set(STAGES) & set(SPARSE_STAGES))})")
    if len(sizes) != batch or len(dense_flags) != batch:
        raise ValueError(f"sample_mixed: {len(sizes)} sizes and {len(dense_flags)} flags for a batch of {batch}")
    h, w = crop or STAGES[stage].crop
    out = []
    for n, ((Hs, Ws), dense) in enumerate(zip(sizes, dense_flags)):
        if Hs < h or Ws < w:
            raise ValueError(f"source {Hs}x{Ws} is smaller than the crop {h}x{w}")
        g = np.random.default_rng([int(seed), int(step), int(rank), n])
        if dense:
            draws = _draw_dense(g, STAGES[stage], (Hs, Ws), h, w, augment)
        else:
            draws = _draw_sparse(g, SPARSE_STAGES[stage], _SPARSE_HFLIP[stage], (Hs, Ws), h, w, augment)
        if constancy:
            draws = _constancy_safe(draws)
        out.append(MixedAugmentParams.record((Hs, Ws), dense, *draws))
    return MixedAugmentParams.cat(out)


# What the three golden ops and their GPU front-ends (ops/native.py) check first, per layout: the frame
# dims as the messages name them, and the record class (a class with sizes of its own: a valid plane too)
_LAYOUTS = {"augment_pairs": ("Hs, Ws", AugmentParams), "augment_pairs_sparse": ("Hb, Wb", SparseAugmentParams),
            "augment_pairs_mixed": ("S", MixedAugmentParams)}


def check_batch(op: str, img1_u8, img2_u8, flow, valid_u8, params) -> Tuple[int, ...]:
    """``ValueError`` unless this is a batch of op ``op``'s layout: images uint8 of one shape
    ``lead + (3,)``, flow fp32 ``lead + (2,)``, valid uint8 ``lead`` where the layout has one, and
    ``lead[0]`` records of the layout's class -> ``lead``: (B, Hs, Ws), (B, Hb, Wb) or (B, S)."""
    dims, cls = _LAYOUTS[op]
    if (img1_u8.ndim != dims.count(",") + 3 or img1_u8.shape[-1] != 3 or img1_u8.shape != img2_u8.shape
            or img1_u8.dtype != torch.uint8 or img2_u8.dtype != torch.uint8):
        raise ValueError(f"{op}: images must be (B, {dims}, 3) uint8 of one size")
    lead = tuple(img1_u8.shape[:-1])
    if flow.dtype != torch.float32 or tuple(flow.shape) != lead + (2,):
        raise ValueError(f"{op}: flow must be {lead + (2,)} fp32, got {tuple(flow.shape)} {flow.dtype}")
    if cls is not AugmentParams and (valid_u8.dtype != torch.uint8 or tuple(valid_u8.shape) != lead):
        raise ValueError(f"{op}: valid must be {lead} uint8, got {tuple(valid_u8.shape)} {valid_u8.dtype}")
    if not isinstance(params, cls) or len(params) != lead[0]:
        raise ValueError(f"{op}: {cls.__name__} for a batch of {lead[0]} wanted")
    return lead


@torch.no_grad()
def augment_pairs_mixed(img1_u8: torch.Tensor, img2_u8: torch.Tensor, flow: torch.Tensor, valid_u8: torch.Tensor,
                        params: MixedAugmentParams, crop: Tuple[int, int]):
    """The golden op of a mixed batch on packed slots: (B, S, 3) uint8 x 2, (B, S, 2) fp32 flow,
    (B, S) uint8 valid -> the outputs of :func:`augment_pairs`.  A composition, no arithmetic of its
    own: the first ``Hs * Ws`` pixels of slot ``n``, reshaped to ``(1, Hs, Ws, .)``, go through
    :func:`augment_pairs` if the record is dense (valid then follows the dense rule, and the slot's
    valid bytes are not read) or through :func:`augment_pairs_sparse` if it is sparse; the outputs
    are stacked.  Nothing past ``Hs * Ws`` in a slot is read."""
    B, S = check_batch("augment_pairs_mixed", img1_u8, img2_u8, flow, valid_u8, params)
    crop = (int(crop[0]), int(crop[1]))
    params.validate(S, crop)
    outs = []
    for n, (Hs, Ws) in enumerate(params.sizes):
        N = Hs * Ws
        a, b, f = (t[n, :N].reshape(1, Hs, Ws, -1) for t in (img1_u8, img2_u8, flow))
        one = params.part(n)
        if params.ints[n, I_DENSE]:
            outs.append(augment_pairs(a, b, f, one, crop))
        else:
            outs.append(augment_pairs_sparse(a, b, f, valid_u8[n, :N].reshape(1, Hs, Ws), one, crop))
    return tuple(torch.cat([o[k] for o in outs]).contiguous() for k in range(4))
