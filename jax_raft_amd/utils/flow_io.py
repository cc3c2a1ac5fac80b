"""Optical-flow I/O and input padding.

* ``.flo`` (Middlebury) read/write -- reference ``scripts/validate_sintel.py:42-61``
  (``readFlow``; magic 202021.25, little-endian int32 w, h, float32 (u, v)).
* :class:`InputPadder` -- replicate padding to a multiple of 8, 'sintel' mode
  centred, else bottom-only (``validate_sintel.py:23-40``).  Works on NCHW or
  NHWC tensors (``channels_last=True``).
* image loading to NHWC float in [-1, 1] (``examples/demo.py:7-10``,
  ``validate_sintel.py:177-178``).
* ``.pfm`` read/write (:func:`read_pfm`, :func:`write_pfm`): FlyingThings3D's flow.
* PNG of 8 or 16 bits per sample (:func:`read_png`, :func:`write_png`) and KITTI's flow coding
  in it (:func:`read_flow_png`, :func:`write_flow_png`): a 16-bit RGB file, ``R, G = flow * 64 +
  32768``, ``B`` = valid.  The chunk parser and zlib are the standard library's; the row
  un-filter, the one sequential step, is ``csrc/runtime/png.cpp`` in the native library when it is
  built, and a numpy row loop otherwise.
"""
from __future__ import annotations

import ctypes
import os
import struct
import zlib
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

FLO_MAGIC = 202021.25


def read_flo(path: str) -> Optional[np.ndarray]:
    """Read a Middlebury ``.flo`` file -> (H, W, 2) float32, or None on a bad magic."""
    with open(path, "rb") as f:
        magic = np.fromfile(f, np.float32, count=1)
        if magic.size == 0 or magic[0] != np.float32(FLO_MAGIC):
            return None
        w = int(np.fromfile(f, np.int32, count=1)[0])
        h = int(np.fromfile(f, np.int32, count=1)[0])
        data = np.fromfile(f, np.float32, count=2 * w * h)
    return data.reshape(h, w, 2)


def write_flo(path: str, flow: np.ndarray) -> None:
    flow = np.asarray(flow, dtype=np.float32)
    assert flow.ndim == 3 and flow.shape[2] == 2
    h, w = flow.shape[:2]
    with open(path, "wb") as f:
        np.array([FLO_MAGIC], np.float32).tofile(f)
        np.array([w, h], np.int32).tofile(f)
        flow.tofile(f)


# ------------------------------------------------------------------------ PFM
def read_pfm(path: str) -> np.ndarray:
    """A ``.pfm`` file (FlyingThings3D's flow and disparity) -> (H, W, 3) for ``PF`` or (H, W) for
    ``Pf``, float32, top row first.  The header is the magic, ``W H`` and a scale whose sign gives the
    byte order (negative: little endian); the rows are stored bottom to top.  A little-endian file
    comes back as a flipped VIEW of the bytes read, so a caller that copies it (or some of its
    channels) into a buffer of its own makes the only copy.  Truncated data, a bad magic or a bad
    header are a ``ValueError`` naming the file.  The flow of a Things file is ``[..., :2]``."""
    bad = lambda why: ValueError(f"{path}: {why}")
    with open(path, "rb") as f:
        magic = f.readline().strip()
        if magic not in (b"PF", b"Pf"):
            raise bad("not a PFM file (bad magic)")
        C = 3 if magic == b"PF" else 1
        try:
            dims = f.readline().split()
            W, H = int(dims[0]), int(dims[1])
            scale = float(f.readline().strip())
            if len(dims) != 2 or W < 1 or H < 1 or scale == 0.0 or scale != scale:
                raise ValueError
        except (ValueError, IndexError):
            raise bad("bad PFM header") from None
        data = np.fromfile(f, "<f4" if scale < 0 else ">f4", count=H * W * C)
    if data.size != H * W * C:
        raise bad(f"truncated PFM data ({data.size} of {H * W * C} values)")
    data = data.reshape((H, W, C) if C == 3 else (H, W))[::-1]
    return data if data.dtype == np.float32 else data.astype(np.float32)


def write_pfm(path: str, array: np.ndarray, little_endian: bool = True) -> None:
    """The inverse of :func:`read_pfm`: (H, W) or (H, W, 3) float32, in either byte order."""
    array = np.asarray(array, dtype=np.float32)
    if array.ndim not in (2, 3) or (array.ndim == 3 and array.shape[2] != 3) or array.size == 0:
        raise ValueError("write_pfm: (H, W) or (H, W, 3)")
    H, W = array.shape[:2]
    with open(path, "wb") as f:
        f.write(b"PF\n" if array.ndim == 3 else b"Pf\n")
        f.write(f"{W} {H}\n{'-1.0' if little_endian else '1.0'}\n".encode())
        f.write(array[::-1].astype("<f4" if little_endian else ">f4").tobytes())


# ------------------------------------------------------------------------ PNG
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_PNG_CHANNELS = {0: 1, 2: 3, 6: 4}          # colour type -> samples per pixel (gray, RGB, RGBA)
_unfilter_c = None                          # jr_png_unfilter of the loaded library; False: not there


def png_size(path: str) -> Tuple[int, int]:
    """(H, W) of a PNG from its IHDR: the first 24 bytes of the file."""
    with open(path, "rb") as f:
        head = f.read(24)
    if len(head) != 24 or head[:8] != PNG_SIGNATURE or head[12:16] != b"IHDR":
        raise ValueError(f"{path}: not a PNG file")
    w, h = struct.unpack(">II", head[16:24])
    return int(h), int(w)


def _native_unfilter():
    """``jr_png_unfilter`` of the native library through ctypes (the call releases the GIL), or
    None when the library is not built."""
    global _unfilter_c
    if _unfilter_c is None:
        fn = False
        try:
            from ..ops import native as nat

            if nat.available():
                fn = ctypes.CDLL(str(nat.SO_PATH)).jr_png_unfilter
                fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
                fn.restype = ctypes.c_int
        except (OSError, AttributeError):
            fn = False
        _unfilter_c = fn
    return _unfilter_c or None


def _paeth(a, b, c):
    a, b, c = (v.astype(np.int16) for v in (a, b, c))
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def unfilter_numpy(rows: np.ndarray, bpp: int) -> int:
    """The un-filter of ``png.cpp`` in numpy, in place on ``rows`` uint8 (H, 1 + rowbytes): a loop
    over rows, and over pixels in Average and Paeth rows.  Slow; the fallback and the reference."""
    H, rowbytes = rows.shape[0], rows.shape[1] - 1
    zero = np.zeros(rowbytes, np.uint8)
    for y in range(H):
        ft, cur = int(rows[y, 0]), rows[y, 1:]
        up = rows[y - 1, 1:] if y else zero
        if ft == 1:
            n = rowbytes // bpp * bpp          # every lane of a pixel is a running sum modulo 256
            cur[:n] = np.cumsum(cur[:n].reshape(-1, bpp), axis=0, dtype=np.uint8).reshape(-1)
        elif ft == 2:
            cur += up
        elif ft in (3, 4):
            left = upleft = np.zeros(bpp, np.uint8)
            for i in range(0, rowbytes, bpp):
                b = up[i:i + bpp]
                if ft == 3:
                    pred = ((left[:len(b)].astype(np.uint16) + b) >> 1).astype(np.uint8)
                else:
                    pred = _paeth(left[:len(b)], b, upleft[:len(b)])
                cur[i:i + bpp] += pred
                left, upleft = cur[i:i + bpp].copy(), b.copy()
        elif ft != 0:
            return 1 + y
    return 0


def read_png(path: str, native: Optional[bool] = None) -> np.ndarray:
    """A non-interlaced PNG of bit depth 8 or 16, gray, RGB or RGBA -> (H, W[, C]) uint8 / uint16.
    Anything else is a ``ValueError`` naming the file: interlace, a palette, another depth, a bad
    signature or CRC, an inflated size other than ``H * (1 + rowbytes)``, a filter byte above 4.
    ``native``: None takes the C++ un-filter when the library is built, False the numpy one, True
    insists on C++."""
    with open(path, "rb") as f:
        data = f.read()
    bad = lambda why: ValueError(f"{path}: {why}")
    if data[:8] != PNG_SIGNATURE:
        raise bad("not a PNG file (bad signature)")
    at, ihdr, idat, ended = 8, None, [], False
    while at + 12 <= len(data) and not ended:
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        if at + 12 + n > len(data):
            raise bad("truncated chunk")
        if zlib.crc32(kind + body) != struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]:
            raise bad(f"bad CRC in chunk {kind!r}")
        if kind == b"IHDR":
            ihdr = body
        elif kind == b"IDAT":
            idat.append(body)
        ended = kind == b"IEND"
        at += 12 + n
    if ihdr is None or len(ihdr) != 13 or not ended:
        raise bad("no IHDR or no IEND chunk")
    W, H, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", ihdr)
    if interlace != 0:
        raise bad("interlaced PNG is not supported")
    if ctype not in _PNG_CHANNELS or depth not in (8, 16) or comp != 0 or filt != 0 or W < 1 or H < 1:
        raise bad(f"unsupported PNG (colour type {ctype}, bit depth {depth}): 8 / 16 bit gray, RGB or RGBA only")
    C = _PNG_CHANNELS[ctype]
    bpp = C * depth // 8
    rowbytes = W * bpp
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise bad(f"bad image data ({e})") from None
    if len(raw) != H * (1 + rowbytes):
        raise bad(f"image data of {len(raw)} bytes, expected {H * (1 + rowbytes)}")
    rows = np.frombuffer(bytearray(raw), np.uint8).reshape(H, 1 + rowbytes)
    fn = None if native is False else _native_unfilter()
    if native and fn is None:
        raise RuntimeError("read_png: the native library is not built")
    rc = fn(rows.ctypes.data, H, rowbytes, bpp) if fn is not None else unfilter_numpy(rows, bpp)
    if rc != 0:
        raise bad(f"filter type above 4 in row {rc - 1}" if rc > 0 else "un-filter failed")
    px = rows[:, 1:]
    if depth == 16:
        px = np.ascontiguousarray(px).view(">u2").astype(np.uint16)
    else:
        px = np.ascontiguousarray(px)
    return px.reshape((H, W) if C == 1 else (H, W, C))


def write_png(path: str, img: np.ndarray, filters: Union[int, Sequence[int]] = 0, level: int = 6) -> None:
    """(H, W[, C]) uint8 / uint16, C in (1, 3, 4) -> a non-interlaced PNG.  ``filters``: one filter
    type 0..4 for every row, or one per row."""
    img = np.asarray(img)
    if img.dtype not in (np.uint8, np.uint16) or img.ndim not in (2, 3):
        raise ValueError("write_png: (H, W[, C]) uint8 or uint16")
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else img.shape[2]
    ctype = {1: 0, 3: 2, 4: 6}.get(C)
    if ctype is None or H < 1 or W < 1:
        raise ValueError("write_png: 1, 3 or 4 channels, no empty image")
    depth = 8 * img.dtype.itemsize
    bpp = C * depth // 8
    raw = np.ascontiguousarray(img.astype(">u2") if depth == 16 else img).view(np.uint8).reshape(H, W * bpp)
    ft = np.broadcast_to(np.asarray(filters, dtype=np.int64), (H,))
    if ((ft < 0) | (ft > 4)).any():
        raise ValueError("write_png: filter types are 0..4")
    left = np.zeros_like(raw); left[:, bpp:] = raw[:, :-bpp]
    up = np.zeros_like(raw); up[1:] = raw[:-1]
    upleft = np.zeros_like(raw); upleft[1:, bpp:] = raw[:-1, :-bpp]
    pred = [np.zeros_like(raw), left, up, ((left.astype(np.uint16) + up) >> 1).astype(np.uint8), _paeth(left, up, upleft)]
    rows = np.empty((H, 1 + W * bpp), np.uint8)
    rows[:, 0] = ft
    for k in range(5):
        sel = ft == k
        if sel.any():
            rows[sel, 1:] = raw[sel] - pred[k][sel]
    chunk = lambda kind, body: struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))
    with open(path, "wb") as f:
        f.write(PNG_SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + chunk(b"IEND", b""))


def read_flow_png(path: str, native: Optional[bool] = None) -> Tuple[np.ndarray, np.ndarray]:
    """A KITTI flow PNG -> (flow fp32 (H, W, 2), valid uint8 (H, W)): ``flow = (R, G - 32768) / 64``,
    ``valid = B != 0``, the channels in the order of the file (R = u, G = v, B = valid)."""
    px = read_png(path, native)
    if px.dtype != np.uint16 or px.ndim != 3 or px.shape[2] != 3:
        raise ValueError(f"{path}: a KITTI flow file is a 16-bit RGB PNG, got {px.dtype} {px.shape}")
    flow = (px[..., :2].astype(np.float32) - np.float32(32768.0)) / np.float32(64.0)
    return flow, (px[..., 2] != 0).astype(np.uint8)


def write_flow_png(path: str, flow: np.ndarray, valid: Optional[np.ndarray] = None,
                   filters: Union[int, Sequence[int]] = 0) -> None:
    """The inverse of :func:`read_flow_png`: ``round(flow * 64 + 32768)`` (half to even) clipped to
    uint16, B = 1 where ``valid`` (default: everywhere)."""
    flow = np.asarray(flow, dtype=np.float32)
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise ValueError("write_flow_png: flow must be (H, W, 2)")
    px = np.empty(flow.shape[:2] + (3,), np.uint16)
    px[..., :2] = np.clip(np.rint(flow.astype(np.float64) * 64.0 + 32768.0), 0, 65535).astype(np.uint16)
    px[..., 2] = 1 if valid is None else (np.asarray(valid).reshape(flow.shape[:2]) != 0)
    write_png(path, px, filters)


def read_image(path: str) -> np.ndarray:
    """RGB uint8 (H, W, 3); grayscale is replicated (``validate_sintel.py:113-119``)."""
    from PIL import Image

    img = np.array(Image.open(path))
    if img.ndim == 2:
        img = np.tile(img[..., None], (1, 1, 3))
    return img[..., :3].astype(np.uint8)


def normalize_image(img_uint8: np.ndarray) -> torch.Tensor:
    """uint8 (H, W, 3) -> float32 NHWC (1, H, W, 3) in [-1, 1]."""
    return torch.from_numpy(img_uint8.astype(np.float32) / 255.0 * 2.0 - 1.0)[None]


class InputPadder:
    """Pads images so H and W are divisible by 8 (replicate mode)."""

    def __init__(self, dims: Sequence[int], mode: str = "sintel", channels_last: bool = False):
        self.channels_last = channels_last
        if channels_last:
            self.ht, self.wd = dims[-3], dims[-2]
        else:
            self.ht, self.wd = dims[-2], dims[-1]
        pad_ht = (((self.ht // 8) + 1) * 8 - self.ht) % 8
        pad_wd = (((self.wd // 8) + 1) * 8 - self.wd) % 8
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs: torch.Tensor) -> List[torch.Tensor]:
        out = []
        for x in inputs:
            if self.channels_last:
                x = F.pad(x.permute(0, 3, 1, 2), self._pad, mode="replicate").permute(0, 2, 3, 1).contiguous()
            else:
                x = F.pad(x, self._pad, mode="replicate")
            out.append(x)
        return out

    def unpad(self, x: torch.Tensor) -> torch.Tensor:
        if self.channels_last:
            ht, wd = x.shape[-3], x.shape[-2]
            c = [self._pad[2], ht - self._pad[3], self._pad[0], wd - self._pad[1]]
            return x[..., c[0]:c[1], c[2]:c[3], :]
        ht, wd = x.shape[-2:]
        c = [self._pad[2], ht - self._pad[3], self._pad[0], wd - self._pad[1]]
        return x[..., c[0]:c[1], c[2]:c[3]]


def flow_to_color(flow: np.ndarray, max_flow: Optional[float] = None) -> np.ndarray:
    """Middlebury-style colour coding of a (H, W, 2) flow field -> uint8 RGB."""
    u, v = flow[..., 0], flow[..., 1]
    rad = np.sqrt(u * u + v * v)
    maxr = max_flow if max_flow is not None else max(float(rad.max()), 1e-6)
    ang = np.arctan2(-v, -u) / np.pi  # [-1, 1]
    hue = (ang + 1.0) / 2.0
    sat = np.clip(rad / maxr, 0, 1)
    hsv = np.stack([hue, sat, np.ones_like(sat)], -1)
    i = np.floor(hsv[..., 0] * 6).astype(int) % 6
    f = hsv[..., 0] * 6 - np.floor(hsv[..., 0] * 6)
    p, q, t = 1 - sat, 1 - sat * f, 1 - sat * (1 - f)
    rgb = np.select([i[..., None] == k for k in range(6)],
                    [np.stack(c, -1) for c in ((np.ones_like(t), t, p), (q, np.ones_like(t), p), (p, np.ones_like(t), t),
                                               (p, q, np.ones_like(t)), (t, p, np.ones_like(t)), (np.ones_like(t), p, q))])
    return (rgb * 255).astype(np.uint8)
