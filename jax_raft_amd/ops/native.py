"""Loader and thin Python front-end for the gfx950 native library (``_C.so``).

The library is built in-tree by :mod:`jax_raft_amd._build`.  On a GPU machine
the native path is the only GPU implementation: if the library cannot be
loaded, GPU execution fails loudly instead of silently falling back to
PyTorch ops.

Every launch op is one row of the op table in ``csrc/runtime/binding.cpp``; the eager op
``ops().<name>`` and the recording ``new_plan().add_<name>`` are generated from it, and both check
the int list's length against the row (``ops().op_arity(name)``) before anything else.
"""
from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import torch

from .. import knobs
from .._build import SO_PATH as _DEFAULT_SO

# JR_NATIVE_SO: load another build of the library (e.g. the host-sanitizer
# build _C_san.so, jax_raft_amd/_build.py --sanitize); default: the in-tree _C.so
SO_PATH = Path(knobs.get("JR_NATIVE_SO")).resolve() if knobs.get("JR_NATIVE_SO") else _DEFAULT_SO

_lock = threading.Lock()
_loaded = False
_load_error: Optional[BaseException] = None

# activation / epilogue codes (csrc/kernels/common.h, kernels.h)
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_SPLIT_TANH_RELU = 0, 1, 2, 3, 4
EPI_STD, EPI_GRU_A, EPI_GRU_B = 0, 1, 2   # 3, 4: retired epilogues (kernels.h)
EPI_BWD, EPI_TAPS = 5, 6
# tile configs with the EPI_TAPS epilogue (256 channels in one N tile, 16 waves of 64 x 32)
TAPS_CFGS = (34, 22, 35, 38)
# tile configs of conv_igemm.hip: (BCO, BP)
CFG_TILES = {0: (128, 128), 1: (64, 128), 2: (128, 64), 3: (16, 256), 4: (64, 64), 5: (16, 64)}
# configs 6..11: LDS-DMA kernel D2 (csrc/kernels/conv_igemm.hip)
CFG_TILES.update({6: (128, 128), 7: (64, 128), 8: (128, 64), 9: (128, 256), 10: (64, 64), 11: (256, 128)})
# configs 12..15: 32x32x16-MFMA kernel (kernel M32)
CFG_TILES.update({12: (128, 128), 13: (64, 128), 14: (128, 64), 15: (64, 64)})
# configs 16/17: kernel R at 256-wide block tiles (128x64 / 64x128 wave tiles, one block per CU)
CFG_TILES.update({16: (256, 128), 17: (128, 256)})
# configs 18..20: kernel R with 8 waves per block (64x32, 32x64, 64x64 wave tiles)
CFG_TILES.update({18: (128, 128), 19: (128, 128), 20: (256, 128)})
# configs 21/22: 16 waves per block (32x32 / 64x32 wave tiles); 23/24: 8 waves at 128x64 / 64x128
CFG_TILES.update({21: (128, 128), 22: (256, 128), 23: (128, 64), 24: (64, 128)})
# configs 25..28: kernel M32 with 8 waves (64x64 / 64x64 / 64x32 / 64x32 wave tiles)
CFG_TILES.update({25: (256, 128), 26: (128, 256), 27: (128, 128), 28: (64, 256)})
# configs 33/34: kernel P (register double-buffered fragments), 8 / 16 waves
CFG_TILES.update({33: (128, 128), 34: (256, 128)})
# configs 35..41: kernel D2 (LDS-DMA ring) at 8 / 16 waves with the FAST loader
CFG_TILES.update({35: (256, 128), 36: (128, 128), 37: (128, 128), 38: (256, 128), 39: (256, 128), 40: (128, 256),
                  41: (64, 128), 42: (256, 128), 43: (256, 128)})
# Autotune candidates: configs that win at least one RAFT conv on MI355X
# (tools/microbench.py, profiles/r1_microbench_conv_cfgs.txt); the others stay
# compiled and tested but are not timed at plan build.
# Of the D2 configs 35..43 only the 16-wave 64x32 ones (35, 38) come within a few
# percent of kernel P on a loop conv (profiles/r2_conv_d2_microbench.txt).
TUNE_CFGS = (0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 33, 34,
             35, 38)
NUM_CUS = 256
# tile configs served by the grouped two-conv launch (csrc/kernels/conv_fam_grp.hip)
GROUPED_CFGS = frozenset((2, 4, 5, 23, 24, 12, 14, 15))


def gru_fused_tiles(N: int, H: int, W: int, vertical: int) -> int:
    """Workgroups of the fused ConvGRU stage (csrc/kernels/gru_fused.hip; mirrors
    binding.cpp:gru_fused_fits): image rows (1x5, W <= 128) or pairs / singles of
    image columns (5x1, J * H <= 128); 0 when the geometry does not fit a tile."""
    if not vertical:
        return N * H if 1 <= W <= 128 else 0
    J = 2 if 2 * H <= 128 and W % 2 == 0 else 1
    return N * (W // J) if 1 <= H and J * H <= 128 and J * (H + 4) <= 136 and W % J == 0 else 0


def flow_fused_tiles(N: int, H: int, W: int) -> int:
    """Workgroups of the fused flow-feature kernel (csrc/kernels/flowfeat.hip): 8 x 16 pixel tiles."""
    return N * -(-H // 8) * -(-W // 16)


def _m32_chan(r: torch.Tensor) -> torch.Tensor:
    """Channel held by row r of a 32-row MFMA A block whose accumulator register i of lane
    half h is channel 16 h + i (row (i & 3) + 8 (i >> 2) + 4 h of the 32x32x16 tile)."""
    return 16 * ((r >> 2) & 1) + (r & 3) + 4 * (r >> 3)


def pack_gru_halo(kernel: torch.Tensor, cin_pad: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ConvGRU gate kernel (kh, kw, cin, cout) HWIO -> the weight stream of gru_halo.hip:
    bf16 [cout/32][kh*kw*cin_pad/16][64][8], fragment (blk, s), lane l, element j holding
    W[k = 16 s + 8 (l >> 5) + j][co = 32 blk + _m32_chan(l & 31)] with k = tap * cin_pad + ci
    (tap row-major, input channels zero-padded to cin_pad): one contiguous 1 KB load per
    MFMA A fragment."""
    kh, kw, cin, cout = kernel.shape
    assert cout % 32 == 0 and cin <= cin_pad and cin_pad % 16 == 0, (kernel.shape, cin_pad)
    dev = kernel.device
    k = torch.zeros(kh * kw, cin_pad, cout, dtype=torch.float32, device=dev)
    k[:, :cin] = kernel.detach().float().reshape(kh * kw, cin, cout)
    k = k.reshape(kh * kw * cin_pad, cout)
    ks = kh * kw * cin_pad // 16
    blk = torch.arange(cout // 32, device=dev).view(-1, 1, 1, 1)
    s = torch.arange(ks, device=dev).view(1, -1, 1, 1)
    l = torch.arange(64, device=dev).view(1, 1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 1, 8)
    kk = (16 * s + 8 * (l >> 5) + j).expand(cout // 32, ks, 64, 8)
    co = (32 * blk + _m32_chan(l & 31)).expand(cout // 32, ks, 64, 8)
    w = k[kk, co].to(torch.bfloat16).contiguous()
    if out is not None:
        assert out.shape == w.shape and out.dtype == torch.bfloat16
        out.copy_(w)
        return out
    return w


# (hd, mode) -> the (nb1, nb2) block counts gru_halo.hip instantiates (JR_HALO_CASES)
GRU_HALO_BLOCKS = {(128, 0): ((1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (5, 4)), (96, 1): ((2, 1), (2, 2), (3, 2))}


def gru_halo_lds(hd: int, mode: int, TR: int, TC: int, nb1: int, nb2: int) -> int:
    """LDS bytes of one gru_halo workgroup (mirrors gru_halo.hip:lds_bytes)."""
    f_rows = TC + 8 if mode == 0 else (TR + 4) * (TC + 4)
    f_elems = max(f_rows * 256, (hd // 32) * nb2 * 4 * 256 * 2)
    return (round_up(f_elems, 8) + 32 * nb1 * 128) * 2


def gru_halo_geom_ok(hd: int, mode: int, TR: int, TC: int, nb1: int, nb2: int) -> bool:
    """Host-side mirror of binding.cpp:gru_halo_geom_ok (no library needed)."""
    if (nb1, nb2) not in GRU_HALO_BLOCKS.get((hd, mode), ()) or TR < 1 or TC < 1:
        return False
    if mode == 0 and TR != 1:
        return False
    nreg = TC + 4 if mode == 0 else (TR + 2) * (TC + 2)
    return nreg <= 32 * nb1 and TR * TC <= 32 * nb2 and gru_halo_lds(hd, mode, TR, TC, nb1, nb2) <= 160 * 1024


def gru_halo_tiles(mode: int, axis: int, N: int, H: int, W: int, TR: int, TC: int) -> int:
    """Workgroups of a gru_halo stage (binding.cpp:make_gru_halo)."""
    if mode == 0:
        length, lines = (H, W) if axis else (W, H)
        return N * lines * -(-length // TC)
    return N * -(-H // TR) * -(-W // TC)


def gru_halo_candidates(hd: int, mode: int, axis: int, N: int, H: int, W: int) -> List[Tuple[int, int, int, int]]:
    """(TR, TC, nb1, nb2) tilings of one gru_halo stage worth timing: per instantiated block
    count, the largest tile that fits it, balanced so the last tile along the run / the
    block grid is not a sliver (mode 0: runs of L = ceil(len / segments) pixels)."""
    out = []
    if mode == 0:
        length = H if axis else W
        for nb1, nb2 in ((1, 1), (2, 1), (2, 2), (3, 2), (3, 3), (5, 4)):
            lmax = min(32 * nb1 - 4, 32 * nb2)
            segs = -(-length // lmax)
            L = -(-length // segs)
            if (L + 4 > 32 * (nb1 - 1) or nb1 == 1) and (L > 32 * (nb2 - 1) or nb2 == 1):
                out.append((1, L, nb1, nb2))
    else:
        for nb1, nb2, tr, tc in ((2, 1, 5, 6), (2, 1, 4, 8), (2, 2, 6, 6), (3, 2, 7, 8)):
            out.append((min(tr, H), min(tc, W), nb1, nb2))
    seen, res = set(), []
    for c in out:
        if c not in seen and gru_halo_geom_ok(hd, mode, *c):
            seen.add(c)
            res.append(c)
    return res


def load(build_if_missing: bool = True) -> None:
    """Load ``_C.so`` (building it with hipcc first if it is missing)."""
    global _loaded, _load_error
    if _loaded:
        return
    with _lock:
        if _loaded:
            return
        try:
            if not SO_PATH.exists() and build_if_missing:
                from .._build import build

                build()
            torch.ops.load_library(str(SO_PATH))
            _loaded = True
        except BaseException as e:  # pragma: no cover - reported by require()
            _load_error = e
            raise


def available() -> bool:
    try:
        load(build_if_missing=False)
        return True
    except BaseException:
        return False


def require() -> None:
    """Raise if the native library is not usable (GPU path must not fall back)."""
    try:
        load()
    except BaseException as e:
        raise RuntimeError(f"jax_raft_amd native library unavailable ({SO_PATH}): {e}") from e


def ops():
    require()
    return torch.ops.jax_raft_amd


def new_plan():
    require()
    return torch.classes.jax_raft_amd.Plan()


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


# ------------------------------------------------------------------ conv specs


@dataclass
class ConvSpec:
    """A packed convolution ready for the implicit-GEMM kernel.

    ``w``: bf16 [cout_pad, kpad], K ordered (kh, kw, cin8) with the input
    channels zero-padded to ``cin8``; ``b``: fp32 [cout]; ``wh``: for a 3x3 /
    stride-1 / pad-1 conv with cin8 % 16 == 0, the weights of the halo kernel
    (conv_halo.hip; :func:`pack_halo_conv`), else None."""

    w: torch.Tensor
    b: torch.Tensor
    kh: int
    kw: int
    sh: int
    sw: int
    ph: int
    pw: int
    cin: int
    cin8: int
    cout: int
    wh: Optional[torch.Tensor] = None

    def out_hw(self, H: int, W: int) -> Tuple[int, int]:
        return (H + 2 * self.ph - self.kh) // self.sh + 1, (W + 2 * self.pw - self.kw) // self.sw + 1

    @property
    def halo_shape(self) -> bool:
        return self.halo_ks != 0

    @property
    def halo_ks(self) -> int:
        """3: a 3x3 / stride-1 / pad-1 conv the halo kernel runs; 4: the space-to-depth stem
        (4x4 / pad 2, output cropped to the input size, 16 input channels); else 0."""
        g = (self.kh, self.kw, self.sh, self.sw, self.ph, self.pw)
        if g == (3, 3, 1, 1, 1, 1) and self.cin8 % 16 == 0:
            return 3
        if g == (4, 4, 1, 1, 2, 2) and self.cin8 == 16:
            return 4
        return 0


# halo 3x3 conv tile configs (csrc/kernels/conv_halo.hip kCfgs; conv op cfg id = HALO_CFG0 + index):
# (cin, waves along cout, waves along pixels, 32-pixel blocks per wave, tile rows, tile cols)
HALO_CFG0 = 100
HALO_CFGS = ((64, 2, 2, 4, 16, 16), (64, 2, 2, 2, 8, 16), (96, 3, 2, 2, 8, 16), (96, 3, 1, 2, 4, 16),
             (128, 4, 2, 2, 8, 16), (128, 4, 1, 2, 4, 16), (128, 2, 2, 2, 8, 16), (128, 2, 1, 1, 4, 8),
             (256, 2, 2, 2, 8, 16), (256, 2, 1, 1, 4, 8), (128, 4, 1, 1, 4, 8), (256, 4, 1, 1, 4, 8),
             (256, 2, 1, 2, 4, 16), (256, 6, 1, 4, 8, 16), (256, 4, 1, 4, 8, 16), (128, 8, 1, 4, 8, 16),
             (128, 2, 1, 4, 8, 16), (256, 6, 1, 2, 4, 16), (256, 4, 1, 2, 4, 16), (256, 1, 2, 2, 8, 16),
             (256, 1, 4, 1, 8, 16), (128, 1, 2, 2, 8, 16), (128, 1, 4, 1, 8, 16))
# the 4x4 space-to-depth stem (kCfgs entries with ks = 4): conv op cfg id -> the same fields
HALO_STEM_CFGS = {HALO_CFG0 + len(HALO_CFGS): (16, 2, 2, 2, 8, 16), HALO_CFG0 + len(HALO_CFGS) + 1: (16, 2, 2, 4, 16, 16)}
# round-6 3x3 configs, after the stem entries of kCfgs (ids of the older configs unchanged)
HALO_CFGS_R6 = ((256, 6, 2, 2, 8, 16), (256, 4, 2, 2, 8, 16), (128, 8, 2, 2, 8, 16), (128, 4, 2, 4, 16, 16),
                (128, 2, 4, 2, 16, 16))
# every 3x3 config: cfg id -> (cin, waves along cout, waves along pixels, blocks per wave, tile rows, tile cols)
HALO_3X3 = {**{HALO_CFG0 + i: c for i, c in enumerate(HALO_CFGS)},
            **{HALO_CFG0 + len(HALO_CFGS) + len(HALO_STEM_CFGS) + i: c for i, c in enumerate(HALO_CFGS_R6)}}


def halo_cfg(cfg: int) -> Tuple[int, int, int, int, int, int]:
    """(cin, waves along cout, waves along pixels, blocks per wave, tile rows, tile cols) of a halo cfg id."""
    return HALO_STEM_CFGS[cfg] if cfg in HALO_STEM_CFGS else HALO_3X3[cfg]


def halo_max_blocks(cin8: int, H: int, W: int) -> int:
    """The most statistics-partial blocks per image any 3x3 config of ``cin8`` input channels
    writes for an H x W output (tiles x pixel waves): the size of a ``stats_part`` buffer."""
    return max(-(-H // c[4]) * -(-W // c[5]) * c[2] for c in HALO_3X3.values() if c[0] == cin8)


def pack_halo_conv(kernel: torch.Tensor, cin8: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(3, 3, cin, cout) HWIO -> the halo conv's weight stream: :func:`pack_gru_halo` with the
    input channels padded to cin8 and the output channels to a multiple of 32."""
    kh, kw, cin, cout = kernel.shape
    k = kernel.detach().float()
    if cout % 32:
        k = torch.cat([k, torch.zeros(kh, kw, cin, round_up(cout, 32) - cout, device=k.device)], dim=3)
    return pack_gru_halo(k, cin8, out=out)


def halo_cfgs_for(spec: "ConvSpec", kw: dict) -> Tuple[int, ...]:
    """Halo conv configs that can run this conv (shape, epilogue, channel count).
    """
    if spec.wh is None or not spec.halo_shape:
        return ()
    if kw.get("epi", EPI_STD) != EPI_STD or kw.get("act", ACT_NONE) not in (ACT_NONE, ACT_RELU):
        return ()
    if kw.get("alpha", 1.0) != 1.0 or kw.get("bmap") is not None or kw.get("h32") is not None:
        return ()
    if kw.get("y") is not None and kw["y"].dtype != torch.bfloat16:
        return ()
    if spec.halo_ks == 4:   # the stem: its output is the input's size (out_hw given by the caller)
        if kw.get("out_hw") is None or spec.cout > 512:
            return ()
        return tuple(HALO_STEM_CFGS)
    if kw.get("out_hw") is not None:
        return ()
    return tuple(i for i, c in HALO_3X3.items() if c[0] == spec.cin8 and spec.cout <= 512)


def _row_perm(cout_pad: int) -> torch.Tensor:
    """Storage row s -> output channel.  Within each 64-row group the rows are
    ordered so that D row (4*q + r) of the 16-row MFMA tile t is channel
    q*16 + t*4 + r: every lane of the conv epilogue then owns contiguous
    channels and both GEMM operands are read from LDS in natural row order."""
    s = torch.arange(cout_pad)
    g, i = s // 64, s % 64
    t, q, r = i // 16, (i % 16) // 4, i % 4
    return g * 64 + q * 16 + t * 4 + r


def pack_weight(kernel: torch.Tensor, cin8: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """HWIO fp32 kernel -> bf16 [cout_pad, kpad] (GEMM A operand), K ordered
    (kh, kw, cin8), rows permuted per :func:`_row_perm`, cout padded to 64."""
    kh, kw, cin, cout = kernel.shape
    cin8 = cin8 or round_up(cin, 8)
    kraw = kh * kw * cin8
    kpad = round_up(kraw, 64)
    cout_pad = round_up(cout, 64)
    k = torch.zeros(kh, kw, cin8, cout, dtype=torch.float32, device=kernel.device)
    k[:, :, :cin, :] = kernel.detach().float()
    w = torch.zeros(cout_pad, kpad, dtype=torch.float32, device=kernel.device)
    w[:cout, :kraw] = k.permute(3, 0, 1, 2).reshape(cout, kraw)
    w = w[_row_perm(cout_pad).to(w.device)].to(torch.bfloat16).contiguous()
    if out is not None:
        assert out.shape == w.shape and out.dtype == torch.bfloat16
        out.copy_(w)
        return out
    return w


def pack_direct_weight(kernel: torch.Tensor) -> torch.Tensor:
    """HWIO kernel (kh, kw, 2, cout) -> bf16 MFMA A fragments [cout/16][NKC][64][8]
    for the 2-channel conv (conv_direct.hip).  K is ordered (kh, kw padded to
    KWP = 4 | 8, c): fragment (t, kc), lane l, element e holds
    W[co = 16t + l % 16][k = 32 kc + 8 (l // 16) + e]."""
    kh, kw, cin, cout = kernel.shape
    assert cin == 2 and cout % 32 == 0, "2-channel conv with cout % 32 == 0"
    kwp = 4 if kw <= 4 else 8
    nkc = (kh * kwp * 2 + 31) // 32
    k = torch.zeros(kh, kwp, 2, cout, dtype=torch.float32, device=kernel.device)
    k[:, :kw] = kernel.detach().float()
    wk = torch.zeros(cout, nkc * 32, dtype=torch.float32, device=kernel.device)
    wk[:, : kh * kwp * 2] = k.reshape(kh * kwp * 2, cout).t()
    wk = wk.reshape(cout // 16, 16, nkc, 4, 8).permute(0, 2, 3, 1, 4)  # [t][kc][kg][i][e]
    return wk.reshape(cout // 16, nkc, 64, 8).to(torch.bfloat16).contiguous()


def direct_conv_ok(kernel: torch.Tensor, stride=(1, 1)) -> bool:
    """Shapes the direct VALU conv kernel supports (the flow branch's 7x7 / 3x3 on 2 channels)."""
    kh, kw, cin, cout = kernel.shape
    return cin == 2 and (kh, kw) in ((7, 7), (3, 3)) and tuple(stride) == (1, 1) and cout % 32 == 0


def make_spec(kernel: torch.Tensor, bias: torch.Tensor, stride=(1, 1), padding=(0, 0), cin8: Optional[int] = None,
              device=None) -> ConvSpec:
    kh, kw, cin, cout = kernel.shape
    cin8 = cin8 or round_up(cin, 8)
    k = kernel.to(device) if device is not None else kernel
    w = pack_weight(k, cin8)
    b = bias.detach().float().to(w.device).contiguous()
    spec = ConvSpec(w, b, kh, kw, stride[0], stride[1], padding[0], padding[1], cin, cin8, cout)
    if spec.halo_ks == 4 or (spec.halo_shape and any(c[0] == cin8 for c in HALO_CFGS)):
        spec.wh = pack_halo_conv(k, cin8)
    return spec


def s2d_stem_kernel(kernel: torch.Tensor) -> torch.Tensor:
    """A 7x7 / stride-2 / pad-3 conv over 3 channels (the encoders' stem, model.py:238-240)
    as the equivalent 4x4 / stride-1 conv (top / left pad 2, output H/2 x W/2) over the 2x2
    space-to-depth input (channel (sy * 2 + sx) * 3 + c, 16 with zero padding):
    W'[ty][tx][(sy, sx, c)] = W[2 ty + sy - 1][2 tx + sx - 1][c] where that tap exists."""
    kh, kw, cin, cout = kernel.shape
    assert (kh, kw, cin) == (7, 7, 3), kernel.shape
    k = kernel.detach().float()
    out = torch.zeros(4, 4, 16, cout, dtype=k.dtype, device=k.device)
    for ty in range(4):
        for tx in range(4):
            for sy in range(2):
                for sx in range(2):
                    a, b = 2 * ty + sy - 1, 2 * tx + sx - 1
                    if 0 <= a < 7 and 0 <= b < 7:
                        c0 = (sy * 2 + sx) * 3
                        out[ty, tx, c0:c0 + 3] = k[a, b]
    return out


def pick_cfg(M: int, cout: int) -> int:
    """Tile-config heuristic: minimise (waves of blocks) x (tile cost), where a
    tile's per-FLOP cost rises as it shrinks; keeps >= one wave of blocks over
    256 CUs whenever the problem allows."""
    if cout <= 16:
        return 5
    best, best_cost = 0, None
    # (cfg, relative per-FLOP efficiency of the tile); time ~ blocks per CU x tile area / eff
    for cfg, eff in ((0, 1.0), (2, 0.85), (1, 0.85), (4, 0.65)):
        bco, bp = CFG_TILES[cfg]
        nb = math.ceil(M / bp) * math.ceil(cout / bco)
        cost = math.ceil(nb / NUM_CUS) * (bco * bp) / eff
        if best_cost is None or cost < best_cost - 1e-9:
            best, best_cost = cfg, cost
    return best


def conv_args(spec: ConvSpec, x: torch.Tensor, N: int, H: int, W: int, y: torch.Tensor, *, x_coff: int = 0,
              y_coff: int = 0, act: int = ACT_NONE, split: int = 0, alpha: float = 1.0, y2=None, y2_coff: int = 0,
              res=None, res_coff: int = 0, res_post: int = 0, h32=None, zbuf=None, hidden: int = 0, coords=None,
              flow32=None, y3=None, y3_coff: int = 0, epi: int = EPI_STD, cfg: Optional[int] = None,
              bmap=None, bmap_coff: int = 0, tapw=None, out_hw: Optional[Tuple[int, int]] = None,
              stats_part=None, in_stats=None, in_relu: int = 0, in_hw: int = 0, in_res=None, in_res_stats=None,
              xn=None):
    """Build the (tensors, ints, alpha) argument triple of the ``conv`` op.
    ``bmap``: optional fp32 per-pixel bias map [M, C], channels from ``bmap_coff``.
    Halo tile configs only (cfg >= HALO_CFG0): ``stats_part`` receives per-tile channel
    (sum, sumsq) partials of the output; ``in_stats`` ([N][cin][2] sums over ``in_hw``
    pixels) normalises the input (instance norm; ``in_relu`` bit 0: relu, bit 1: relu before the
    residual add) as it is loaded;
    ``in_res`` (+ ``in_res_stats``: normalised too) is added before the relu (a residual
    block's output built on the fly) and ``xn`` receives the built input."""
    OH, OW = out_hw if out_hw is not None else spec.out_hw(H, W)
    if cfg is None:
        cfg = pick_cfg(N * OH * OW, spec.cout)
    t = [x, spec.w, spec.b, y, y2, res, h32, zbuf, coords, flow32, y3, bmap]
    if tapw is not None:
        t.append(tapw)
    elif cfg >= HALO_CFG0:   # the halo 3x3 kernel (conv_halo.hip): its own weight stream
        assert spec.wh is not None, "halo tile config for a conv without halo weights"
        t.append(spec.wh)
        if in_res is not None or in_res_stats is not None or xn is not None:
            t += [stats_part, in_stats, in_res, in_res_stats, xn]
        elif stats_part is not None or in_stats is not None:
            t += [stats_part, in_stats]
    assert (stats_part is None and in_stats is None and in_res is None and xn is None) or cfg >= HALO_CFG0, \
        "stats / input norm need a halo config"
    i = [N, H, W, x_coff, spec.cin8, spec.kh, spec.kw, spec.sh, spec.sw, spec.ph, spec.pw, spec.cout, act, split,
         y_coff, y2_coff, res_coff, hidden, y3_coff, epi, cfg, res_post]
    if bmap is not None or out_hw is not None or in_stats is not None:
        i += [OH if out_hw is not None else 0, OW if out_hw is not None else 0, 0, 0, bmap_coff]
    if in_stats is not None:
        i += [int(in_relu), int(in_hw)]
    return t, i, float(alpha)


def pack_convex_head(kernel: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """MaskPredictor 1x1 conv (1, 1, 256, 576) -> the A-fragment order of
    csrc/kernels/convex_head.hip: [kstep 8][tap 9][wave 4][lane 64][8] bf16 with
    lane = 16 q + r holding W[ci = 32 kstep + 8 q + j][co = 64 tap + 16 wave + r]
    (co in the reference order k*64 + s, ``model.py:86``); bias stays fp32 [576]."""
    kh, kw, cin, c = kernel.shape
    assert (kh, kw, cin, c) == (1, 1, 256, 576), kernel.shape
    wc = kernel.detach().float().reshape(8, 4, 8, 9, 4, 16)      # (ks, q, j, k, w, r)
    wp = wc.permute(0, 3, 4, 1, 5, 2).contiguous().to(torch.bfloat16)
    return wp.reshape(-1), bias.detach().float().contiguous()


def pack_taps_epi(kernel: torch.Tensor) -> torch.Tensor:
    """FlowHead conv2 (3, 3, 256, 2) -> the A fragments of the EPI_TAPS conv
    epilogue (csrc/kernels/conv_igemm.h:taps_epilogue): [group 4][kstep 2][tile 2][lane 64][8]
    bf16 with lane = 16 q + r holding Wt[o = 16 tile + r][c = 64 group + 16 q + 8 kstep + j],
    Wt[o = 2 tap + comp][c] = W[tap // 3, tap % 3, c, comp] (rows 18..31 zero) -- the k
    order of the 16 contiguous channels each conv1 epilogue lane owns."""
    kh, kw, cin, co = kernel.shape
    assert (kh, kw, cin, co) == (3, 3, 256, 2), kernel.shape
    dev = kernel.device
    wt = torch.zeros(32, 256, dtype=torch.float32, device=dev)
    wt[:18] = kernel.detach().float().reshape(9, cin, 2).permute(0, 2, 1).reshape(18, cin)
    g = torch.arange(4, device=dev).view(4, 1, 1, 1, 1)
    s = torch.arange(2, device=dev).view(1, 2, 1, 1, 1)
    t = torch.arange(2, device=dev).view(1, 1, 2, 1, 1)
    lane = torch.arange(64, device=dev).view(1, 1, 1, 64, 1)
    j = torch.arange(8, device=dev).view(1, 1, 1, 1, 8)
    o = 16 * t + lane % 16
    c = 64 * g + 16 * (lane // 16) + 8 * s + j
    return wt[o.expand(4, 2, 2, 64, 8), c.expand(4, 2, 2, 64, 8)].to(torch.bfloat16).contiguous()


CONV1X1_KPADS = (128, 256, 352, 384)


def pack_conv1x1(kernel: torch.Tensor, kpad: int) -> torch.Tensor:
    """1x1 conv (1, 1, K, N) -> the A fragments of conv1x1.hip: per output group
    g of 64 channels [g][k-step kpad/32][row tile 4][lane 64][8] bf16, lane =
    16 q + r holding W[k = 32 ks + 8 q + j][co = 64 g + 16 (r >> 2) + 4 t + (r & 3)]
    (zero for k >= K), so that a lane's accumulators are 16 contiguous channels."""
    _, _, K, N = kernel.shape
    assert N % 64 == 0 and K <= kpad and kpad % 32 == 0, (kernel.shape, kpad)
    w = torch.zeros(kpad, N, dtype=torch.float32, device=kernel.device)
    w[:K] = kernel.detach().float().reshape(K, N)
    dev = kernel.device
    g, ks, t, l, j = torch.meshgrid(torch.arange(N // 64, device=dev), torch.arange(kpad // 32, device=dev),
                                    torch.arange(4, device=dev), torch.arange(64, device=dev),
                                    torch.arange(8, device=dev), indexing="ij")
    r = l & 15
    k = 32 * ks + 8 * (l >> 4) + j
    co = 64 * g + 16 * (r >> 2) + 4 * t + (r & 3)
    return w[k, co].to(torch.bfloat16).reshape(-1).contiguous()


def conv1x1(x: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, kvalid: int, kpad: int, cout: int,
            act: int = ACT_NONE) -> torch.Tensor:
    """Eager pointwise conv with LDS-resident weights: x bf16 [M][cs] -> bf16 [M][cout]."""
    M = x.shape[0]
    y = torch.empty(M, cout, device=x.device, dtype=torch.bfloat16)
    ops().conv1x1([x, wpk, bias, y], [M, kvalid, kpad, cout, act, 0])
    return y


def flow_features_fused(flow: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, spec2: ConvSpec, N: int, H: int,
                        W: int, y: torch.Tensor, y_coff: int = 0) -> torch.Tensor:
    """Eager fused flow branch (csrc/kernels/flowfeat.hip): flow bf16 [N*H*W][2] through the 7x7
    conv 2 -> 128 + relu (``w1``: :func:`pack_direct_weight`, ``b1``) and the 3x3 / pad-1 conv
    128 -> 64 + relu ``spec2`` into channels ``y_coff .. + 64`` of y bf16 [N*H*W][cs]: what
    ``conv_direct`` followed by the halo conv writes, bitwise.  The kernel assumes exactly these
    shapes, the compact flow rows and the halo weight stream; checked here (and in the op)."""
    assert flow.dtype == torch.bfloat16 and flow.shape[-1] == 2 and flow.numel() == N * H * W * 2 and flow.is_contiguous()
    assert w1.numel() == 128 * 4 * 32 and b1.numel() == 128, "7x7 conv 2 -> 128 (pack_direct_weight)"
    assert spec2.halo_ks == 3 and spec2.cin8 == 128 and spec2.cout == 64 and spec2.wh is not None, "3x3 conv 128 -> 64"
    assert y.dtype == torch.bfloat16 and y.shape[-1] % 8 == 0 and y_coff % 8 == 0 and y_coff + 64 <= y.shape[-1]
    ops().flow_features_fused([flow, w1, b1, spec2.wh, spec2.b, y], [N, H, W, y_coff])
    return y


def pack_taps(kernel: torch.Tensor) -> torch.Tensor:
    """Flow head output conv (3, 3, K, 2) -> the A fragments of
    flowhead.hip:taps_gemm_kernel: rows o = tap * 2 + c (18 real of 32), packed
    [k-step K/32][row tile 2][lane 64][8] bf16 with lane = 16 q + r holding
    W[k = 32 ks + 8 q + j][o = 16 t + r]."""
    kh, kw, K, co = kernel.shape
    assert (kh, kw, co) == (3, 3, 2) and K % 32 == 0, kernel.shape
    w = kernel.detach().float().reshape(9, K, 2).permute(1, 0, 2).reshape(K, 18)     # [k][tap * 2 + c]
    a = torch.zeros(K, 32, dtype=torch.float32, device=kernel.device)
    a[:, :18] = w
    a = a.reshape(K // 32, 4, 8, 2, 16)            # (ks, q, j, t, r)
    return a.permute(0, 3, 1, 4, 2).contiguous().to(torch.bfloat16).reshape(-1)


def taps_gemm(fm: torch.Tensor, wpk: torch.Tensor, K: int, coff: int = 0) -> torch.Tensor:
    """Eager flow-head taps: fm bf16 [M][cs] -> fp32 [M][24]."""
    M = fm.shape[0]
    out = torch.empty(M, 24, device=fm.device, dtype=torch.float32)
    ops().taps_gemm([fm, wpk, out], [M, K, coff])
    return out


def convex_head(feat: torch.Tensor, wpk: torch.Tensor, bias: torch.Tensor, flow: torch.Tensor, B: int, h: int,
                w: int, alpha: float, coff: int = 0, out: Optional[torch.Tensor] = None, tiles: int = 0) -> torch.Tensor:
    """Eager fused mask head: feat bf16 [M][cs] (channels coff..coff+256), flow fp32
    [M][2] -> upsampled flow (B, 8h, 8w, 2) (csrc/kernels/convex_head.hip)."""
    if out is None:
        out = torch.empty(B, 8 * h, 8 * w, 2, device=feat.device, dtype=torch.float32)
    ops().convex_head([feat, wpk, bias, flow, out], [B, h, w, coff, 0, tiles], float(alpha))
    return out


def project_keys(B: int, h: int, w: int, device) -> torch.Tensor:
    """The key buffer of :func:`forward_project` for (B, h, w) maps: two planes of 64-bit
    splat keys + two control words, all ones (csrc/kernels/warm.hip).  Every call leaves it
    clean for the next, so one buffer serves any number of calls on one stream."""
    return torch.full((2 * B * h * w + 2,), -1, dtype=torch.int64, device=device)


def forward_project(flow: torch.Tensor, fill_radius: int = 4, keys: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Project a (B, h, w, 2) fp32 flow field forward in time (the warm-start flow of the
    next pair): ``models/reference.py:forward_project`` -- that golden op itself on a CPU
    tensor, the HIP kernels (bitwise equal, two launches, no host synchronisation) on a GPU
    tensor.  ``keys``: a :func:`project_keys` buffer to reuse across calls."""
    if not flow.is_cuda:
        from ..models.reference import forward_project as golden

        return golden(flow, fill_radius)
    if flow.ndim != 4 or flow.shape[-1] != 2 or flow.dtype != torch.float32:
        raise ValueError(f"forward_project: flow must be (B, h, w, 2) fp32, got {tuple(flow.shape)} {flow.dtype}")
    B, h, w, _ = flow.shape
    flow = flow.contiguous()
    if keys is None:
        keys = project_keys(B, h, w, flow.device)
    if out is None:
        out = torch.empty_like(flow)
    ops().forward_project([flow, keys, out], [B, h, w, int(fill_radius)])
    return out


def fb_check(flow_fw: torch.Tensor, flow_bw: torch.Tensor, alpha: float = 0.01, beta: float = 0.5,
             window: Optional[Tuple[int, int, int, int]] = None, return_err: bool = False,
             thr: Optional[torch.Tensor] = None):
    """Forward-backward occlusion masks ``(occ_fw, occ_bw)`` of a (B, H, W, 2) fp32 flow pair
    (+ the fp32 error maps with ``return_err``): ``models/reference.py:fb_consistency`` -- that
    golden op itself on CPU tensors, the HIP kernel (bitwise equal, one launch for both
    directions) on GPU tensors.  ``window = (H0, W0, top, left)``: the frame's rectangle inside
    the map (default: the whole map).

    This stand-alone front-end uploads ``[alpha, beta]`` from the host on every call; pass
    ``thr``, a 2-element fp32 device tensor that already holds them (``alpha`` / ``beta`` are then
    ignored), to avoid that copy.  A width that is no multiple of 4 costs a padded copy of both
    flows.  (In a bidirectional plan the thresholds are written only when they change.)"""
    if not flow_fw.is_cuda:
        from ..models.reference import fb_consistency

        return fb_consistency(flow_fw, flow_bw, alpha, beta, window, return_err)
    for f in (flow_fw, flow_bw):
        if f.ndim != 4 or f.shape[-1] != 2 or f.dtype != torch.float32:
            raise ValueError(f"fb_check: flows must be (B, H, W, 2) fp32, got {tuple(f.shape)} {f.dtype}")
    if flow_fw.shape != flow_bw.shape:
        raise ValueError("fb_check: flow_fw and flow_bw must have the same shape")
    B, H, W, _ = flow_fw.shape
    win = [H, W, 0, 0] if window is None else [int(v) for v in window]
    Wp = round_up(W, 4)
    if Wp != W:   # the kernel takes 4 pixels per thread: zero columns outside the frame window
        flow_fw = torch.nn.functional.pad(flow_fw, (0, 0, 0, Wp - W))
        flow_bw = torch.nn.functional.pad(flow_bw, (0, 0, 0, Wp - W))
    dev = flow_fw.device
    occ = torch.empty((2, B, H, Wp), dtype=torch.uint8, device=dev)
    err = torch.empty((2, B, H, Wp), dtype=torch.float32, device=dev) if return_err else None
    if thr is None:
        thr = torch.tensor([alpha, beta], dtype=torch.float32, device=dev)

    def vec(f):   # the kernel's 16-byte loads: a view at an odd pixel offset is copied
        f = f.contiguous()
        return f.clone() if f.data_ptr() % 16 else f

    ops().fb_check([vec(flow_fw), vec(flow_bw), occ, err, thr], [B, H, Wp] + win)
    occ = occ[..., :W].bool()
    if return_err:
        return occ[0], occ[1], err[0, ..., :W], err[1, ..., :W]
    return occ[0], occ[1]


def warp_frames(src: torch.Tensor, flow: torch.Tensor, occ: Optional[torch.Tensor] = None,
                own: Optional[torch.Tensor] = None, window: Optional[Tuple[int, int, int, int]] = None):
    """Motion-compensated frame and masked photometric error of one direction, ``(warped,
    photo)``: ``models/reference.py:warp_frames`` -- that golden op itself on CPU tensors, the HIP
    kernel (csrc/kernels/framewarp.hip, bitwise equal, one launch after the clear of the two
    sums) on GPU tensors.  src / own: (B, H0, W0, 3) uint8, flow: (B, H, W, 2) fp32, occ:
    (B, H, W) bool, ``window = (H0, W0, top, left)`` (default: the whole map).  Returns fresh
    tensors; ``photo`` is None without ``own``.  Wrong shapes or dtypes raise ``ValueError``
    before anything is launched."""
    if flow.ndim != 4 or flow.shape[-1] != 2 or flow.dtype != torch.float32:
        raise ValueError(f"warp_frames: flow must be (B, H, W, 2) fp32, got {tuple(flow.shape)} {flow.dtype}")
    B, H, W, _ = flow.shape
    win = [H, W, 0, 0] if window is None else [int(v) for v in window]
    H0, W0, top, left = win
    if len(win) != 4 or H0 < 1 or W0 < 1 or top < 0 or left < 0 or top + H0 > H or left + W0 > W:
        raise ValueError(f"warp_frames: window (H0, W0, top, left) = {tuple(win)} must lie inside the {H} x {W} map")
    for name, t in (("src", src), ("own", own)):
        if t is None and name == "own":
            continue
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (B, H0, W0, 3) or t.dtype != torch.uint8:
            raise ValueError(f"warp_frames: {name} must be {(B, H0, W0, 3)} uint8, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else t} {getattr(t, 'dtype', '')}")
        if t.device != flow.device:
            raise ValueError(f"warp_frames: {name} is on {t.device}, flow on {flow.device}")
    if occ is not None:
        if tuple(occ.shape) != (B, H, W) or occ.dtype != torch.bool:
            raise ValueError(f"warp_frames: occ must be {(B, H, W)} bool, got {tuple(occ.shape)} {occ.dtype}")
        if occ.device != flow.device:
            raise ValueError(f"warp_frames: occ is on {occ.device}, flow on {flow.device}")
    if not flow.is_cuda:
        from ..models.reference import warp_frames as golden

        return golden(src, flow, occ, own, win)
    dev = flow.device
    flow = flow.contiguous()
    if flow.data_ptr() % 8:   # the kernel's 8-byte loads
        flow = flow.clone()
    warped = torch.empty((1, B, H0, W0, 3), dtype=torch.uint8, device=dev)
    photo = None if own is None else torch.zeros((1, B, 2), dtype=torch.int64, device=dev)
    mask = None if occ is None else occ.contiguous().view(torch.uint8).view(1, B, H, W)
    ops().warp_frames([src.contiguous(), None, None if own is None else own.contiguous(), None, flow, None, mask,
                       warped, photo], [B, H, W] + win + [1])
    return warped[0], (None if photo is None else photo[0])


def _augment_sums(kernel: str, img1_u8, img2_u8, rec, out):
    """Launch 1 of layout ``kernel`` (``augment``, ``augment_sparse`` or ``augment_mixed``); ``rec``: the
    packed records on the device where the layout's sums read them."""
    B, *geom = img1_u8.shape[:-1]
    if out is None:
        out = torch.empty((2, B, 3), dtype=torch.int32, device=img1_u8.device)
    getattr(ops(), kernel + "_sums")([img1_u8, img2_u8] + ([] if rec is None else [rec]) + [out], [B, *geom])
    return out


def _augment_pairs(op: str, img1_u8, img2_u8, flow, valid_u8, params, crop):
    """The GPU path of front-end ``op`` (``augment_pairs``, ``_sparse`` or ``_mixed``): the batch check it
    shares with its golden op, the records validated on the host, uploaded pinned and ``non_blocking``,
    the sums launch, four fresh outputs, the gather launch.  No host synchronisation.  ``valid_u8`` is
    None for the dense layout, which has no valid plane and whose sums launch reads no records."""
    from ..train import augment as A

    B, *geom = A.check_batch(op, img1_u8, img2_u8, flow, valid_u8, params)
    h, w = int(crop[0]), int(crop[1])
    params.validate(tuple(geom) if len(geom) == 2 else geom[0], (h, w))
    dev = img1_u8.device
    kernel = op.replace("_pairs", "")
    rec = params.packed(pin=True).to(dev, non_blocking=True)
    sums = _augment_sums(kernel, img1_u8, img2_u8, None if valid_u8 is None else rec, None)
    out1 = torch.empty((B, h, w, 3), dtype=torch.float32, device=dev)
    out2 = torch.empty_like(out1)
    oflow = torch.empty((B, h, w, 2), dtype=torch.float32, device=dev)
    valid = torch.empty((B, h, w), dtype=torch.float32, device=dev)
    planes = [img1_u8, img2_u8, flow] + ([] if valid_u8 is None else [valid_u8])
    getattr(ops(), kernel)(planes + [rec, sums, out1, out2, oflow, valid], [B, *geom, h, w])
    return out1, out2, oflow, valid


def interpolate_frames(frame1: torch.Tensor, frame2: torch.Tensor, flow_fw: torch.Tensor, flow_bw: torch.Tensor, t,
                       occ_fw: Optional[torch.Tensor] = None, occ_bw: Optional[torch.Tensor] = None,
                       window: Optional[Tuple[int, int, int, int]] = None, min_cover: float = 1.0 / 64):
    """The frame at time ``t`` between two frames by forward splatting, ``(frame_t, holes)``:
    ``models/reference.py:interpolate_frames`` -- that golden op itself on CPU tensors, the HIP
    kernels (csrc/kernels/interp.hip, bitwise equal: the clear of the accumulator, the splat of both
    directions and the resolve, per time, one accumulator reused) on GPU tensors.  frame1 / frame2:
    (B, H0, W0, 3) uint8, flow_fw / flow_bw: (B, H, W, 2) fp32, occ_fw / occ_bw: (B, H, W) bool or
    None, ``window = (H0, W0, top, left)`` (default: the whole map).  ``t``: a float, or a sequence
    of K floats, which returns (K, B, H0, W0, 3) uint8 and (K, B, H0, W0) bool.  Returns fresh
    tensors.  Wrong arguments raise ``ValueError`` before anything is launched."""
    from ..models.reference import INTERP_MAX_MAPS, INTERP_MAX_PIXELS, interp_times

    rows, many = interp_times(t, min_cover)
    for name, f in (("flow_fw", flow_fw), ("flow_bw", flow_bw)):
        if not isinstance(f, torch.Tensor) or f.ndim != 4 or f.shape[-1] != 2 or f.dtype != torch.float32:
            raise ValueError(f"interpolate_frames: {name} must be (B, H, W, 2) fp32, got "
                             f"{tuple(f.shape) if isinstance(f, torch.Tensor) else f} {getattr(f, 'dtype', '')}")
    if flow_fw.shape != flow_bw.shape or flow_fw.device != flow_bw.device:
        raise ValueError("interpolate_frames: flow_fw and flow_bw must have the same shape and device")
    B, H, W, _ = flow_fw.shape
    win = [H, W, 0, 0] if window is None else [int(v) for v in window]
    if len(win) != 4 or win[0] < 1 or win[1] < 1 or win[2] < 0 or win[3] < 0 or win[2] + win[0] > H or win[3] + win[1] > W:
        raise ValueError(f"interpolate_frames: window (H0, W0, top, left) = {tuple(win)} must lie inside the {H} x {W} map")
    H0, W0, top, left = win
    if B < 1 or H0 * W0 > INTERP_MAX_PIXELS or 2 * B > INTERP_MAX_MAPS:
        raise ValueError(f"interpolate_frames: sizes (1 <= 2 * B <= {INTERP_MAX_MAPS}, H0 * W0 <= {INTERP_MAX_PIXELS}), "
                         f"got B = {B}, {H0} x {W0}")
    dev = flow_fw.device
    for name, fr in (("frame1", frame1), ("frame2", frame2)):
        if not isinstance(fr, torch.Tensor) or tuple(fr.shape) != (B, H0, W0, 3) or fr.dtype != torch.uint8:
            raise ValueError(f"interpolate_frames: {name} must be {(B, H0, W0, 3)} uint8, got "
                             f"{tuple(fr.shape) if isinstance(fr, torch.Tensor) else fr} {getattr(fr, 'dtype', '')}")
        if fr.device != dev:
            raise ValueError(f"interpolate_frames: {name} is on {fr.device}, the flows on {dev}")
    for name, o in (("occ_fw", occ_fw), ("occ_bw", occ_bw)):
        if o is None:
            continue
        if not isinstance(o, torch.Tensor) or tuple(o.shape) != (B, H, W) or o.dtype != torch.bool:
            raise ValueError(f"interpolate_frames: {name} must be {(B, H, W)} bool, got "
                             f"{tuple(o.shape) if isinstance(o, torch.Tensor) else o} {getattr(o, 'dtype', '')}")
        if o.device != dev:
            raise ValueError(f"interpolate_frames: {name} is on {o.device}, the flows on {dev}")
    if not flow_fw.is_cuda:
        from ..models.reference import interpolate_frames as golden

        res = [golden(frame1, frame2, flow_fw, flow_bw, v, occ_fw, occ_bw, win, min_cover) for v in (t if many else [t])]
        return (torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])) if many else res[0]
    flows = []
    for f in (flow_fw, flow_bw):
        f = f.contiguous()
        flows.append(f.clone() if f.data_ptr() % 8 else f)   # the kernel's 8-byte loads
    mask = None
    if occ_fw is not None or occ_bw is not None:   # one mask only: the other direction is all consistent
        zeros = torch.zeros((B, H, W), dtype=torch.bool, device=dev)
        mask = torch.stack([zeros if occ_fw is None else occ_fw, zeros if occ_bw is None else occ_bw]).view(torch.uint8)
    K = len(rows)
    frame1, frame2 = frame1.contiguous(), frame2.contiguous()
    par = torch.tensor(rows, dtype=torch.int32).to(dev)
    acc = torch.empty((2, B, H0, W0, 4), dtype=torch.int64, device=dev)
    out = torch.empty((K, B, H0, W0, 3), dtype=torch.uint8, device=dev)
    holes = torch.empty((K, B, H0, W0), dtype=torch.uint8, device=dev)
    for k in range(K):
        acc.zero_()
        ops().interp_splat([frame1, frame2, flows[0], flows[1], mask, acc, par], [B, H, W] + win + [k])
        ops().interp_resolve([frame1, frame2, acc, par, out[k], holes[k]], [B, H0, W0, k])
    holes = holes.bool()
    return (out, holes) if many else (out[0], holes[0])


def augment_sums(img1_u8: torch.Tensor, img2_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact per-channel integer sums of two batches of (B, Hs, Ws, 3) uint8 GPU frames ->
    int32 (2, B, 3) (launch 1 of :func:`augment_pairs`; the kernel clears ``out`` itself)."""
    return _augment_sums("augment", img1_u8, img2_u8, None, out)


def augment_pairs(img1_u8: torch.Tensor, img2_u8: torch.Tensor, flow: torch.Tensor, params,
                  crop: Tuple[int, int]):
    """RAFT's dense augmentation of a batch of frame pairs as they were uploaded ->
    ``(image1, image2, flow, valid)`` at the crop size, the format the training step takes:
    ``train/augment.py:augment_pairs`` -- that golden op itself on CPU tensors, the HIP kernels
    (bitwise equal; two launches and the upload of the records, no host synchronisation) on
    GPU tensors.  ``params``: the batch's :class:`~jax_raft_amd.train.augment.AugmentParams`,
    validated here on the host before anything is uploaded or launched."""
    if not img1_u8.is_cuda:
        from ..train import augment as A

        return A.augment_pairs(img1_u8, img2_u8, flow, params, crop)
    return _augment_pairs("augment_pairs", img1_u8, img2_u8, flow, None, params, crop)


def augment_sums_sparse(img1_u8: torch.Tensor, img2_u8: torch.Tensor, rec: torch.Tensor,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact per-channel integer sums of each sample's own region of two batches of (B, Hb, Wb, 3)
    uint8 GPU buffers -> int32 (2, B, 3); ``rec``: the packed sparse records on the device."""
    return _augment_sums("augment_sparse", img1_u8, img2_u8, rec, out)


def augment_pairs_sparse(img1_u8: torch.Tensor, img2_u8: torch.Tensor, flow: torch.Tensor, valid_u8: torch.Tensor,
                         params, crop: Tuple[int, int]):
    """RAFT's sparse augmentation (KITTI / HD1K) of a batch of samples of several sizes, each in
    the top-left corner of its (Hb, Wb) buffer -> ``(image1, image2, flow, valid)`` at the crop
    size: ``train/augment.py:augment_pairs_sparse`` itself on CPU tensors, the sparse layout of the
    HIP kernels of ``augment.hip`` (bitwise equal; two launches and the upload of the records, no host
    synchronisation) on GPU tensors.  ``params``: the batch's
    :class:`~jax_raft_amd.train.augment.SparseAugmentParams`, validated here on the host before
    anything is uploaded or launched."""
    if not img1_u8.is_cuda:
        from ..train import augment as A

        return A.augment_pairs_sparse(img1_u8, img2_u8, flow, valid_u8, params, crop)
    return _augment_pairs("augment_pairs_sparse", img1_u8, img2_u8, flow, valid_u8, params, crop)


def augment_sums_mixed(img1_u8: torch.Tensor, img2_u8: torch.Tensor, rec: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact per-channel integer sums of each sample's packed pixels in two batches of (B, S, 3) uint8
    GPU slots -> int32 (2, B, 3); ``rec``: the packed mixed records on the device."""
    return _augment_sums("augment_mixed", img1_u8, img2_u8, rec, out)


def augment_pairs_mixed(img1_u8: torch.Tensor, img2_u8: torch.Tensor, flow: torch.Tensor, valid_u8: torch.Tensor,
                        params, crop: Tuple[int, int]):
    """The augmentation of a batch of dense and sparse samples (RAFT's Sintel stage) in packed slots --
    (B, S, 3) uint8 x 2, (B, S, 2) fp32, (B, S) uint8, sample n in the first Hs * Ws pixels of slot n --
    -> ``(image1, image2, flow, valid)`` at the crop size: ``train/augment.py:augment_pairs_mixed``
    itself on CPU tensors, the mixed layout of the HIP kernels of ``augment.hip`` (bitwise equal; two
    launches and the upload of the records, no host synchronisation) on GPU tensors.  ``params``: the
    batch's :class:`~jax_raft_amd.train.augment.MixedAugmentParams`, validated here on the host before
    anything is uploaded or launched."""
    if not img1_u8.is_cuda:
        from ..train import augment as A

        return A.augment_pairs_mixed(img1_u8, img2_u8, flow, valid_u8, params, crop)
    return _augment_pairs("augment_pairs_mixed", img1_u8, img2_u8, flow, valid_u8, params, crop)


METRICS_RUN, METRICS_BLOCK = 4, 256      # pixels per thread and threads per block of metrics.hip


def flow_metrics_blocks(Hs: int, Ws: int) -> int:
    """Blocks of the partials kernel that a sample of Hs x Ws occupies."""
    return (Hs * ((Ws + METRICS_RUN - 1) // METRICS_RUN) + METRICS_BLOCK - 1) // METRICS_BLOCK


def flow_metrics(pred: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor] = None, sizes=None,
                 acc: Optional[torch.Tensor] = None):
    """Validation metrics of a batch, accumulated: ``eval/metrics.py:flow_metrics`` -- that golden op
    itself on CPU tensors, the HIP kernels of ``metrics.hip`` on GPU tensors (every count bitwise equal,
    the fp64 sums equal up to the order of their additions and bitwise repeatable; two launches and
    the upload of the sizes, no host synchronisation; ``rows`` and ``acc`` stay on the device).
    The arguments, ``sizes`` above all, are checked here on the host before anything is launched."""
    from ..eval import metrics as M

    if not pred.is_cuda:
        return M.flow_metrics(pred, gt, valid, sizes, acc)
    sizes = M.check_args(pred, gt, valid, sizes, acc)
    dev = pred.device
    B, Hp, Wp, _ = pred.shape
    Hg, Wg = int(gt.shape[1]), int(gt.shape[2])
    nb = max(flow_metrics_blocks(h, w) for h, w in sizes)
    host = torch.empty((B, 2), dtype=torch.int32, pin_memory=True)
    host.copy_(torch.tensor(sizes, dtype=torch.int32))
    dsizes = host.to(dev, non_blocking=True)
    part = torch.empty(B * nb * 2, dtype=torch.float64, device=dev)
    rows = torch.empty((B, M.ROW), dtype=torch.float64, device=dev)
    if acc is None:
        acc = torch.zeros(M.ACC, dtype=torch.float64, device=dev)
    elif not acc.is_contiguous():
        raise ValueError("flow_metrics: acc must be contiguous")
    ops().flow_metrics([pred.contiguous(), gt.contiguous(), None if valid is None else valid.contiguous(), dsizes, part,
                        rows, acc], [B, Hp, Wp, Hg, Wg, nb])
    return rows, acc


# The label-free losses (csrc/kernels/loss_common.h: the constants and the reduction their kernels share).
UNSUP_BLOCK, UNSUP_GRID_X = 256, 1024    # threads per block and the loss kernel's blocks per round (unsup.hip)
_floats = {}


def _cached_floats(values, device) -> torch.Tensor:
    """A few floats as an fp32 device tensor, uploaded once per device and set of values, so that a training
    step does not copy from the host: the one cache of the kernels' small parameter tensors."""
    key = (str(device),) + tuple(float(v) for v in values)
    if key not in _floats:
        if len(_floats) >= 64:
            _floats.clear()
        _floats[key] = torch.tensor(key[1:], dtype=torch.float32, device=device)
    return _floats[key]


def _gpu_operands(op, named, aligned, N, pixels, copy=False):
    """The GPU-only checks the loss front ends share -> the tensors of ``named`` ((name, tensor or None) pairs) as
    the kernels take them: fp32, contiguous and, where named in ``aligned``, 8-byte aligned (the kernels' 8-byte
    loads) -- refused otherwise, or with ``copy`` made so; at most 32 predictions of fewer than 2^31 pixels."""
    out = []
    for name, t in named:
        if t is not None:
            if t.dtype != torch.float32:
                raise ValueError(f"{op}: {name} must be fp32 on the GPU, got {t.dtype}")
            if copy:
                t = t.contiguous()
                if name in aligned and t.data_ptr() % 8:
                    t = t.clone()
            elif not t.is_contiguous():
                raise ValueError(f"{op}: {name} must be contiguous on the GPU")
            elif name in aligned and t.data_ptr() % 8:
                raise ValueError(f"{op}: {name} must be 8-byte aligned")
        out.append(t)
    if N > 32 or pixels >= 2 ** 31:
        raise ValueError(f"{op}: 1..32 predictions of fewer than 2^31 pixels, got N = {N} of {pixels} pixels")
    return out


def _cpu_grad(sums, preds: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The CPU path of a ``*_loss_grad``: the gradient of ``(sums(f) * scale).sum()`` in f = preds, by autograd
    through the golden op's differentiable sums."""
    with torch.enable_grad():
        f = preds.detach().requires_grad_(True)
        s = sums(f)
        return torch.autograd.grad((s * scale.to(s.dtype)).sum(), f)[0]


def unsup_loss_blocks(P: int) -> int:
    """Rows of block partials that ``unsup_loss`` writes for P pixels."""
    return min(UNSUP_GRID_X, (P + UNSUP_BLOCK - 1) // UNSUP_BLOCK)


def unsup_params(eps: float, eps_s: float, edge_kappa: float, out_penalty: float, device) -> torch.Tensor:
    """``(eps, eps_s, edge_kappa, out_penalty)`` as the fp32 device tensor the kernels read (cached)."""
    return _cached_floats((eps, eps_s, edge_kappa, out_penalty), device)


def _unsup_args(op, preds, image1, image2, mask, eps, eps_s, edge_kappa, out_penalty, prm):
    from ..train import unsup as U

    N, B, H, W = U._check(preds, image1, image2, mask)
    if not preds.is_cuda:
        return None
    named = (("flow_preds", preds), ("image1", image1), ("image2", image2), ("mask", mask))
    t = _gpu_operands(op, named, ("flow_preds",), N, B * H * W, copy=True)    # a front end for any layout: it copies
    return t + [unsup_params(eps, eps_s, edge_kappa, out_penalty, preds.device) if prm is None else prm], [B, H, W, N]


def unsup_loss_partials(flow_preds: torch.Tensor, image1: torch.Tensor, image2: torch.Tensor,
                        mask: Optional[torch.Tensor] = None, eps: float = 0.01, eps_s: float = 0.001,
                        edge_kappa: float = 10.0, out_penalty: float = 0.5, prm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The partial sums of the label-free loss, fp32 (blocks, N, 4): per iteration ``sum(mask pix)``,
    the smoothness sum, the count of masked pixels that land outside and, for the last iteration,
    the sum of pix over the inside masked pixels -- ``train/unsup.py:unsup_sums`` itself on CPU
    tensors (one row of partials), the HIP kernel on GPU tensors (``csrc/kernels/unsup.hip``; one
    launch, bitwise repeatable).  ``prm``: :func:`unsup_params`, in place of the four floats."""
    args = _unsup_args("unsup_loss", flow_preds, image1, image2, mask, eps, eps_s, edge_kappa, out_penalty, prm)
    if args is None:
        from ..train.unsup import unsup_sums

        with torch.no_grad():
            return unsup_sums(flow_preds, image1, image2, mask, eps, eps_s, edge_kappa, out_penalty)[None]
    t, i = args
    B, H, W, N = i
    part = torch.empty((unsup_loss_blocks(B * H * W), N, 4), dtype=torch.float32, device=flow_preds.device)
    ops().unsup_loss(t + [part], i)
    return part


def unsup_loss_grad(flow_preds: torch.Tensor, image1: torch.Tensor, image2: torch.Tensor, mask: Optional[torch.Tensor],
                    scale: torch.Tensor, eps: float = 0.01, eps_s: float = 0.001, edge_kappa: float = 10.0,
                    out_penalty: float = 0.5, prm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of ``sum_i scale[i, 0] sum(mask pix_i) + scale[i, 1] (smoothness sum)_i`` in the
    predictions, (N, B, H, W, 2): autograd through ``train/unsup.py:unsup_sums`` on CPU tensors, the
    gather kernel on GPU tensors (one launch, no atomics).  scale: (N, 2)."""
    args = _unsup_args("unsup_loss_bwd", flow_preds, image1, image2, mask, eps, eps_s, edge_kappa, out_penalty, prm)
    N = flow_preds.shape[0]
    if tuple(scale.shape) != (N, 2) or scale.device != flow_preds.device:
        raise ValueError(f"unsup_loss_bwd: scale must be {(N, 2)} on {flow_preds.device}, got {tuple(scale.shape)} on {scale.device}")
    if args is None:
        from ..train.unsup import unsup_sums

        return _cpu_grad(lambda f: unsup_sums(f, image1, image2, mask, eps, eps_s, edge_kappa, out_penalty)[:, :2],
                         flow_preds, scale)
    t, i = args
    if scale.dtype != torch.float32:
        raise ValueError(f"unsup_loss_bwd: scale must be fp32 on the GPU, got {scale.dtype}")
    grad = torch.empty(flow_preds.shape, dtype=torch.float32, device=flow_preds.device)
    ops().unsup_loss_bwd(t + [scale.contiguous(), grad], i)
    return grad


CENSUS_TILE, CENSUS_ITERS = (32, 8), 4   # the pixel tile (x, y) and the iterations of a block (census.hip)


def census_tiles(B: int, H: int, W: int) -> int:
    """Rows of tile partials that ``census_loss`` writes."""
    tx, ty = CENSUS_TILE
    return B * ((H + ty - 1) // ty) * ((W + tx - 1) // tx)


def _census_args(op, preds, gray, mask):
    """Host checks shared by the census front ends; (N, B, H, W).  Nothing is launched before they pass."""
    if preds.ndim != 5 or preds.shape[-1] != 2 or not preds.is_floating_point() or 0 in preds.shape:
        raise ValueError(f"{op}: flow_preds must be a non-empty (N, B, H, W, 2) floating point tensor, got "
                         f"{tuple(preds.shape)} {preds.dtype}")
    N, B, H, W, _ = preds.shape
    named = ([] if gray is None else [("gray", gray, (2, B, H, W))]) + ([] if mask is None else [("mask", mask, (B, H, W))])
    for name, t, shape in named:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.device != preds.device:
            raise ValueError(f"{op}: {name} must be {shape} on {preds.device}, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else t} on {getattr(t, 'device', None)}")
    if preds.is_cuda:
        _gpu_operands(op, (("flow_preds", preds), ("gray", gray), ("mask", mask)), ("flow_preds",), N, B * H * W)
    return N, B, H, W


def census_gray_planes(image1: torch.Tensor, image2: torch.Tensor) -> torch.Tensor:
    """The grey planes of both images in 8-bit levels, (2, B, H, W): ``train/unsup.py:census_gray``
    on CPU tensors, one launch of ``csrc/kernels/census.hip`` on GPU tensors."""
    ok = lambda t: isinstance(t, torch.Tensor) and t.ndim == 4 and t.shape[-1] == 3 and t.is_floating_point() and t.numel() > 0
    if not (ok(image1) and ok(image2) and image1.shape == image2.shape and image1.device == image2.device):
        raise ValueError("census_gray: image1 and image2 must be non-empty (B, H, W, 3) floating point tensors of one "
                         "shape on one device")
    if not image1.is_cuda:
        from ..train.unsup import census_gray

        return torch.stack([census_gray(image1), census_gray(image2)])
    B, H, W, _ = image1.shape
    _gpu_operands("census_gray", (("image1", image1), ("image2", image2)), (), 1, B * H * W)
    gray = torch.empty((2, B, H, W), dtype=torch.float32, device=image1.device)
    ops().census_gray([image1, image2, gray], [B, H, W])
    return gray


def _census_images(op, preds, image1, image2, mask, gray):
    from ..train import unsup as U

    N, B, H, W = U._check(preds, image1, image2, mask)
    if preds.is_cuda:
        _census_args(op, preds, gray, mask)
        if gray is None:
            gray = census_gray_planes(image1, image2)
    return N, B, H, W, gray


def census_loss_partials(flow_preds: torch.Tensor, image1: torch.Tensor, image2: torch.Tensor,
                         mask: Optional[torch.Tensor] = None, out_penalty: float = 0.5, prm: Optional[torch.Tensor] = None,
                         gray: Optional[torch.Tensor] = None):
    """The census term's partial sums, fp32 (tiles, N, 4) -- per pixel tile and iteration
    ``sum(mask term)``, the masked pixels that are not inside, the masked pixels inside but in the
    border band and, for the last iteration, the sum of cen over the valid masked pixels -- and the
    backward's coefficient plane ``mask valid 0.4 (h + 0.01)^-0.6``, fp32 (N, B, H, W):
    ``(train/unsup.py:census_sums[None], None)`` on CPU tensors, the HIP kernel on GPU tensors
    (``csrc/kernels/census.hip``; one launch, bitwise repeatable).  ``prm``: :func:`unsup_params`, in
    place of ``out_penalty``; ``gray``: :func:`census_gray_planes` of the images, if at hand."""
    N, B, H, W, gray = _census_images("census_loss", flow_preds, image1, image2, mask, gray)
    if not flow_preds.is_cuda:
        from ..train.unsup import census_sums

        with torch.no_grad():
            return census_sums(flow_preds, image1, image2, mask, out_penalty)[None], None
    if prm is None:
        prm = unsup_params(0.01, 0.001, 10.0, out_penalty, flow_preds.device)
    part = torch.empty((census_tiles(B, H, W), N, 4), dtype=torch.float32, device=flow_preds.device)
    coef = torch.empty((N, B, H, W), dtype=torch.float32, device=flow_preds.device)
    ops().census_loss([flow_preds, gray, mask, prm, part, coef], [B, H, W, N])
    return part, coef


def census_loss_grad(flow_preds: torch.Tensor, image1: torch.Tensor, image2: torch.Tensor, mask: Optional[torch.Tensor],
                     scale: torch.Tensor, out_penalty: float = 0.5, prm: Optional[torch.Tensor] = None,
                     gray: Optional[torch.Tensor] = None, coef: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of ``sum_i scale[i] sum(mask term_i)`` in the predictions, (N, B, H, W, 2):
    autograd through ``train/unsup.py:census_sums`` on CPU tensors, the gather kernel of
    ``csrc/kernels/census.hip`` on GPU tensors (one launch, no atomics).  scale: (N,); ``gray`` and
    ``coef``: what :func:`census_gray_planes` and :func:`census_loss_partials` returned for the same
    operands (computed here when missing); ``out``: a gradient tensor to add into, in place of a new one."""
    N, B, H, W, gray = _census_images("census_loss_bwd", flow_preds, image1, image2, mask, gray)
    dev = flow_preds.device
    named = (("scale", scale, (N,)),) + (() if out is None else (("out", out, tuple(flow_preds.shape)),)) + (
        () if coef is None else (("coef", coef, (N, B, H, W)),))
    for name, t, shape in named:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"census_loss_bwd: {name} must be {shape} on {dev}")
    if not flow_preds.is_cuda:
        from ..train.unsup import census_sums

        g = _cpu_grad(lambda f: census_sums(f, image1, image2, mask, out_penalty)[:, 0], flow_preds, scale)
        return g if out is None else out.add_(g)
    _gpu_operands("census_loss_bwd", [v[:2] for v in named], ("scale", "out", "coef"), N, B * H * W)
    if coef is None:
        coef = census_loss_partials(flow_preds, image1, image2, mask, out_penalty, prm, gray)[1]
    grad = torch.empty(flow_preds.shape, dtype=torch.float32, device=dev) if out is None else out
    ops().census_loss_bwd([flow_preds, gray, coef, scale, grad], [B, H, W, N, 0 if out is None else 1])
    return grad


def smooth2_loss_blocks(P: int) -> int:
    """Rows of block partials that ``smooth2_loss`` writes for P pixels."""
    return min(UNSUP_GRID_X, (P + UNSUP_BLOCK - 1) // UNSUP_BLOCK)


def _smooth2_args(op, preds, image1, extra, eps_s, edge_kappa, prm):
    """Host checks shared by the second-order smoothness front ends; ``extra``: (name, tensor, shape) of the operands
    beside the predictions and the image.  Nothing is launched before they pass -> (N, B, H, W, prm)."""
    if preds.ndim != 5 or preds.shape[-1] != 2 or not preds.is_floating_point() or 0 in preds.shape:
        raise ValueError(f"{op}: flow_preds must be a non-empty (N, B, H, W, 2) floating point tensor, got "
                         f"{tuple(preds.shape)} {preds.dtype}")
    N, B, H, W, _ = preds.shape
    named = [("image1", image1, (B, H, W, 3))] + list(extra)
    for name, t, shape in named:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.device != preds.device or not t.is_floating_point():
            raise ValueError(f"{op}: {name} must be floating point {shape} on {preds.device}, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else t} on {getattr(t, 'device', None)}")
    if preds.is_cuda:
        _gpu_operands(op, [("flow_preds", preds)] + [v[:2] for v in named], ("flow_preds", "out"), N, B * H * W)
        if prm is None:
            prm = unsup_params(0.01, eps_s, edge_kappa, 0.5, preds.device)
        elif not (isinstance(prm, torch.Tensor) and prm.is_cuda and prm.dtype == torch.float32 and prm.numel() == 4):
            raise ValueError(f"{op}: prm must be the fp32 device tensor of unsup_params")
    return N, B, H, W, prm


def smooth2_loss_partials(flow_preds: torch.Tensor, image1: torch.Tensor, eps_s: float = 0.001, edge_kappa: float = 10.0,
                          prm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The partial sums of the second-order smoothness term, fp32 (blocks, N, 4): per iteration the sum over the
    triples along x, the sum over the triples along y, 0, 0 -- ``train/unsup.py:smooth2_sums`` itself on CPU tensors
    (one row of partials), the HIP kernel on GPU tensors (``csrc/kernels/smooth2.hip``; one launch, bitwise
    repeatable).  ``prm``: :func:`unsup_params`, in place of the two floats."""
    N, B, H, W, prm = _smooth2_args("smooth2_loss", flow_preds, image1, (), eps_s, edge_kappa, prm)
    if not flow_preds.is_cuda:
        from ..train.unsup import smooth2_sums

        with torch.no_grad():
            s = smooth2_sums(flow_preds, image1, eps_s, edge_kappa)
            return torch.cat([s, torch.zeros_like(s)], dim=-1)[None]
    part = torch.empty((smooth2_loss_blocks(B * H * W), N, 4), dtype=torch.float32, device=flow_preds.device)
    ops().smooth2_loss([flow_preds, image1, prm, part], [B, H, W, N])
    return part


def smooth2_loss_grad(flow_preds: torch.Tensor, image1: torch.Tensor, scale: torch.Tensor, eps_s: float = 0.001,
                      edge_kappa: float = 10.0, prm: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of ``sum_i scale[i] (x-axis sum + y-axis sum)_i`` in the predictions, (N, B, H, W, 2): fp32
    autograd through ``train/unsup.py:smooth2_sums`` on CPU tensors, the gather kernel of ``csrc/kernels/smooth2.hip``
    on GPU tensors (one launch, no atomics).  scale: (N,); ``out``: a gradient tensor to add into, in place of a new
    one (it is returned)."""
    N = flow_preds.shape[0] if flow_preds.ndim == 5 else 0
    extra = (("scale", scale, (N,)),) + (() if out is None else (("out", out, tuple(flow_preds.shape)),))
    N, B, H, W, prm = _smooth2_args("smooth2_loss_bwd", flow_preds, image1, extra, eps_s, edge_kappa, prm)
    if not flow_preds.is_cuda:
        from ..train.unsup import smooth2_sums

        g = _cpu_grad(lambda f: smooth2_sums(f.float(), image1.float(), eps_s, edge_kappa).sum(-1), flow_preds, scale)
        return g if out is None else out.add_(g)
    grad = torch.empty(flow_preds.shape, dtype=torch.float32, device=flow_preds.device) if out is None else out
    ops().smooth2_loss_bwd([flow_preds, image1, prm, scale, grad], [B, H, W, N, 0 if out is None else 1])
    return grad


def _range_flows(op: str, flow_fw, flow_bw):
    """Host checks of a flow pair (flow_bw may be None), before any launch -> (B, H, W)."""
    from ..train import occlusion as O

    B, H, W = O._check_flow(op, flow_fw)
    if flow_bw is not None:
        O._check_flow(op, flow_bw)
        if flow_bw.shape != flow_fw.shape or flow_bw.device != flow_fw.device:
            raise ValueError(f"{op}: flow_fw and flow_bw must have the same shape and device")
    if flow_fw.is_cuda:
        for name, f in (("flow_fw", flow_fw), ("flow_bw", flow_bw)):
            if f is not None and (not f.is_contiguous() or f.data_ptr() % 8):
                raise ValueError(f"{op}: {name} must be contiguous and 8-byte aligned on the GPU")
        if 2 * B > 65535:
            raise ValueError(f"{op}: at most 32767 samples, got {B}")
    return B, H, W


def range_map(flow_fw: torch.Tensor, flow_bw: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The range map of a (B, H, W, 2) fp32 flow, int32 (B, H, W) in 1/256 of a source pixel -- with
    ``flow_bw`` both directions' maps, (2, B, H, W), from one launch: ``train/occlusion.py:range_map``
    on CPU tensors, the clear + the integer-atomic splat of ``csrc/kernels/occlusion.hip`` on GPU tensors
    (bitwise equal, any width, no host synchronisation)."""
    from ..train import occlusion as O

    B, H, W = _range_flows("range_map", flow_fw, flow_bw)
    O.check_pixels("range_map", H, W)
    if not flow_fw.is_cuda:
        return O.range_map(flow_fw) if flow_bw is None else torch.stack([O.range_map(flow_fw), O.range_map(flow_bw)])
    fw, bw = flow_fw.detach(), None if flow_bw is None else flow_bw.detach()
    acc = torch.empty((B, H, W) if bw is None else (2, B, H, W), dtype=torch.int32, device=fw.device)
    acc.zero_()
    ops().range_splat([fw, bw, acc], [B, H, W])
    return acc


def fb_thresholds(alpha: float, beta: float, device) -> torch.Tensor:
    """``(alpha, beta)`` of the forward-backward check as the fp32 device tensor ``fb_check`` reads (cached)."""
    return _cached_floats((alpha, beta), device)


def visibility_masks(flow_fw: torch.Tensor, flow_bw: torch.Tensor, kind: str, thr: float = 0.5, alpha: float = 0.01,
                     beta: float = 0.5) -> torch.Tensor:
    """The visibility masks of a (B, H, W, 2) fp32 flow pair, fp32 (2, B, H, W) (0: fw, 1: bw; 1.0 = use
    the pixel), so that ``masks.view(2 * B, H, W)`` is the mask of the stacked batch:
    ``train/occlusion.py:visibility_masks`` on CPU tensors; on GPU tensors ``kind="range"`` runs the
    clear, the splat and the mask launch of ``csrc/kernels/occlusion.hip``, ``kind="fb"`` :func:`fb_check`
    plus elementwise ops on its output (both bitwise equal, no gradient)."""
    from ..train import occlusion as O

    if kind not in O.KINDS:
        raise ValueError(f"visibility_masks: unknown kind {kind!r} (range or fb)")
    if flow_bw is None:
        raise ValueError("visibility_masks: both flows are needed")
    B, H, W = _range_flows("visibility_masks", flow_fw, flow_bw)
    if kind == "range":
        O.check_pixels("visibility_masks", H, W)
    if not flow_fw.is_cuda:
        return torch.stack(O.visibility_masks(flow_fw, flow_bw, kind, thr, alpha, beta))
    fw, bw = flow_fw.detach(), flow_bw.detach()
    if kind == "range":
        acc = range_map(fw, bw)
        vis = torch.empty((2, B, H, W), dtype=torch.float32, device=fw.device)
        ops().range_visible([fw, bw, acc, vis], [B, H, W, O.range_threshold(thr)])
        return vis
    occ_fw, occ_bw = fb_check(fw, bw, thr=fb_thresholds(alpha, beta, fw.device))
    return torch.stack([~O.lands_inside(fw) | ~occ_fw, ~O.lands_inside(bw) | ~occ_bw]).float()


SELFSUP_BLOCK, SELFSUP_GRID_X = 256, 1024    # threads per block (2 pixels each) and blocks per round (selfsup.hip)


def crop_resize(x: torch.Tensor, c: int, scale=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The centre crop ``[c, H-c) x [c, W-c)`` of x (B, H, W, C) resampled bilinearly back to H x W, channel k
    times ``scale[k]``: ``train/selfsup.py:crop_resize`` itself on CPU tensors (C <= 4, any float dtype), the HIP
    kernel on GPU tensors (``csrc/kernels/selfsup.hip``; fp32, C <= 3, contiguous; bitwise equal, one launch,
    no host synchronisation).  ``out``: a contiguous fp32 tensor like x to write into.  Wrong shapes, dtypes,
    devices or crops raise ``ValueError`` before anything is launched."""
    from ..train import selfsup as S

    B, H, W, C = S.check_crop(x, c, scale)
    if out is not None and (not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype
                            or out.device != x.device or not out.is_contiguous()):
        raise ValueError(f"crop_resize: out must be a contiguous {tuple(x.shape)} {x.dtype} tensor on {x.device}")
    if not x.is_cuda:
        v = S.crop_resize(x, c, scale)
        return v if out is None else out.copy_(v)
    if x.dtype != torch.float32 or C > 3:
        raise ValueError(f"crop_resize: fp32 with at most 3 channels on the GPU, got {x.dtype} with C = {C}")
    if not x.is_contiguous():
        raise ValueError("crop_resize: x must be contiguous on the GPU")
    if B > 65535 or H > 65535 or B * H * W * C >= 2 ** 31:
        raise ValueError(f"crop_resize: B and H at most 65535 and fewer than 2^31 elements, got {tuple(x.shape)}")
    if out is None:
        out = torch.empty_like(x)
    elif out.data_ptr() < x.data_ptr() + x.numel() * 4 and x.data_ptr() < out.data_ptr() + x.numel() * 4:
        raise ValueError("crop_resize: out must not overlap x")
    sc = [1.0] * 4 if scale is None else [float(s) for s in scale] + [1.0] * (4 - C)
    prm = _cached_floats(S.crop_ratios(H, W, c) + tuple(sc), x.device)
    ops().crop_resize([x.detach(), prm, out], [B, H, W, C, int(c)])
    return out


def selfsup_loss_blocks(P: int) -> int:
    """Rows of block partials that ``selfsup_loss`` writes for P pixels."""
    return min(SELFSUP_GRID_X, ((P + 1) // 2 + SELFSUP_BLOCK - 1) // SELFSUP_BLOCK)


def selfsup_params(eps: float, device) -> torch.Tensor:
    """``(eps,)`` as the fp32 device tensor the loss kernels read, uploaded once per device and value."""
    return _cached_floats((eps,), device)


def _selfsup_args(op, preds, target, weight, eps, prm, batch0):
    """Host checks of the loss ops -> None on CPU tensors, else (tensors, ints) of the launch.  ``preds`` is the
    whole (N, Btot, H, W, 2) stack, of which the batches [batch0, batch0 + B) are used, B = target.shape[0]."""
    from ..train import selfsup as S

    if not isinstance(preds, torch.Tensor) or preds.ndim != 5 or not isinstance(target, torch.Tensor) or target.ndim != 4:
        raise ValueError(f"{op}: flow_preds must be (N, Btot, H, W, 2) and target (B, H, W, 2)")
    Btot, B = preds.shape[1], target.shape[0]
    if isinstance(batch0, bool) or not isinstance(batch0, int) or batch0 < 0 or B < 1 or batch0 + B > Btot:
        raise ValueError(f"{op}: the batch window [{batch0}, {batch0} + {B}) must lie inside the stack's {Btot} batches")
    win = preds[:, batch0:batch0 + B]
    N, B, H, W = S._check(win, target, weight)
    if not preds.is_cuda:
        return None
    named = (("flow_preds", preds), ("target", target), ("weight", weight))
    _gpu_operands(op, named, ("flow_preds", "target"), N, Btot * H * W)     # the stack is read in place: no copies
    if prm is None:
        prm = selfsup_params(eps, preds.device)
    return [preds.detach(), target, weight, prm], [N, B, H, W, Btot, batch0]


def selfsup_loss_partials(flow_preds: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None,
                          eps: float = 0.001, prm: Optional[torch.Tensor] = None, batch0: int = 0) -> torch.Tensor:
    """The partial sums of the self-supervision loss, fp32 (blocks, N, 4): per iteration the sum of the terms and,
    for the last iteration, that sum again, the sum of the weights and the count of weights above 0 --
    ``train/selfsup.py:selfsup_sums`` itself on CPU tensors (one row of partials), the HIP kernel on GPU tensors
    (``csrc/kernels/selfsup.hip``; one launch, bitwise repeatable).  ``flow_preds`` is a whole contiguous stack
    (N, Btot, H, W, 2), read in place at the batches ``[batch0, batch0 + B)``, B = ``target.shape[0]``."""
    args = _selfsup_args("selfsup_loss", flow_preds, target, weight, eps, prm, batch0)
    if args is None:
        from ..train.selfsup import selfsup_sums

        with torch.no_grad():
            return selfsup_sums(flow_preds[:, batch0:batch0 + target.shape[0]], target, weight, eps)[None]
    t, i = args
    N, B, H, W = i[:4]
    part = torch.empty((selfsup_loss_blocks(B * H * W), N, 4), dtype=torch.float32, device=flow_preds.device)
    ops().selfsup_loss(t + [part], i)
    return part


def selfsup_loss_grad(flow_preds: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor], scale: torch.Tensor,
                      eps: float = 0.001, prm: Optional[torch.Tensor] = None, batch0: int = 0) -> torch.Tensor:
    """The gradient of ``sum_i scale[i] (sum of terms)_i`` in the window's predictions, (N, B, H, W, 2) contiguous:
    autograd through ``train/selfsup.py:selfsup_sums`` on CPU tensors, the one-pass kernel on GPU tensors.
    scale: (N,)."""
    args = _selfsup_args("selfsup_loss_bwd", flow_preds, target, weight, eps, prm, batch0)
    N = flow_preds.shape[0]
    if not isinstance(scale, torch.Tensor) or tuple(scale.shape) != (N,) or scale.device != flow_preds.device:
        raise ValueError(f"selfsup_loss_bwd: scale must be {(N,)} on {flow_preds.device}, got "
                         f"{tuple(scale.shape) if isinstance(scale, torch.Tensor) else scale}")
    if args is None:
        from ..train.selfsup import selfsup_sums

        return _cpu_grad(lambda f: selfsup_sums(f, target, weight, eps)[:, 0], flow_preds[:, batch0:batch0 + target.shape[0]],
                         scale)
    t, i = args
    if scale.dtype != torch.float32:
        raise ValueError(f"selfsup_loss_bwd: scale must be fp32 on the GPU, got {scale.dtype}")
    N, B, H, W = i[:4]
    grad = torch.empty((N, B, H, W, 2), dtype=torch.float32, device=flow_preds.device)
    ops().selfsup_loss_bwd(t + [scale.contiguous(), grad], i)
    return grad


def conv2d(spec: ConvSpec, x: torch.Tensor, act: int = ACT_NONE, out_dtype=torch.bfloat16, alpha: float = 1.0,
           res: Optional[torch.Tensor] = None, res_post: int = 0, cfg: Optional[int] = None) -> torch.Tensor:
    """Eager NHWC conv of a contiguous bf16 tensor [N, H, W, C] (C == cin8)."""
    N, H, W, C = x.shape
    assert C == spec.cin8, f"input channels {C} != packed cin8 {spec.cin8}"
    OH, OW = spec.out_hw(H, W)
    y = torch.empty(N, OH, OW, round_up(spec.cout, 8), device=x.device, dtype=out_dtype)
    t, i, a = conv_args(spec, x, N, H, W, y, act=act, alpha=alpha, res=res, res_post=res_post, cfg=cfg)
    ops().conv(t, i, a)
    return y[..., : spec.cout] if y.shape[-1] != spec.cout else y


# ------------------------------------------------------ fp32 parity mode convs


@dataclass
class ConvSpecF32:
    """A conv for the fp32 implicit-GEMM kernel (csrc/kernels/conv_f32.hip):
    ``w`` fp32 [cout, K], K ordered (kh, kw, cin4) with the input channels
    zero-padded to ``cin4`` (a multiple of 4), rows in natural channel order;
    ``b`` fp32 [cout]."""

    w: torch.Tensor
    b: torch.Tensor
    kh: int
    kw: int
    sh: int
    sw: int
    ph: int
    pw: int
    cin: int
    cin4: int
    cout: int

    def out_hw(self, H: int, W: int) -> Tuple[int, int]:
        return (H + 2 * self.ph - self.kh) // self.sh + 1, (W + 2 * self.pw - self.kw) // self.sw + 1


def pack_weight_f32(kernel: torch.Tensor, cin4: Optional[int] = None) -> torch.Tensor:
    """HWIO kernel -> fp32 [cout, kh*kw*cin4] (input channels zero-padded)."""
    kh, kw, cin, cout = kernel.shape
    cin4 = cin4 or round_up(cin, 4)
    assert cin4 >= cin and cin4 % 4 == 0
    k = torch.zeros(kh, kw, cin4, cout, dtype=torch.float32, device=kernel.device)
    k[:, :, :cin, :] = kernel.detach().float()
    return k.permute(3, 0, 1, 2).reshape(cout, kh * kw * cin4).contiguous()


def make_spec_f32(kernel: torch.Tensor, bias: torch.Tensor, stride=(1, 1), padding=(0, 0),
                  cin4: Optional[int] = None, device=None) -> ConvSpecF32:
    kh, kw, cin, cout = kernel.shape
    cin4 = cin4 or round_up(cin, 4)
    w = pack_weight_f32(kernel.to(device) if device is not None else kernel, cin4)
    b = bias.detach().float().to(w.device).contiguous()
    return ConvSpecF32(w, b, kh, kw, stride[0], stride[1], padding[0], padding[1], cin, cin4, cout)


def conv_f32_args(spec: ConvSpecF32, x: torch.Tensor, N: int, H: int, W: int, y: torch.Tensor, *, x_coff: int = 0,
                  y_coff: int = 0, act: int = ACT_NONE, split: int = 0, alpha: float = 1.0, y2=None, y2_coff: int = 0,
                  res=None, res_coff: int = 0, res_post: int = 0, h32=None, zbuf=None, hidden: int = 0, bmap=None,
                  bmap_coff: int = 0, epi: int = EPI_STD, ksplit: int = 0):
    """(tensors, ints, alpha) of the ``conv_f32`` op / ``Plan.add_conv_f32``; ``ksplit`` > 0 forces
    an n-way split-K (0: the kernel's own choice)."""
    t = [x, spec.w, spec.b, y, y2, res, h32, zbuf, bmap]
    i = [N, H, W, x_coff, spec.cin4, spec.kh, spec.kw, spec.sh, spec.sw, spec.ph, spec.pw, spec.cout, act, split,
         y_coff, y2_coff, res_coff, res_post, hidden, bmap_coff, epi, ksplit]
    return t, i, float(alpha)


def conv2d_f32(spec: ConvSpecF32, x: torch.Tensor, act: int = ACT_NONE, alpha: float = 1.0, res=None,
               res_post: int = 0) -> torch.Tensor:
    """Eager fp32 NHWC conv (x: (N, H, W, C >= cin4) fp32) -> (N, OH, OW, cout)."""
    N, H, W, _ = x.shape
    OH, OW = spec.out_hw(H, W)
    y = torch.empty((N, OH, OW, spec.cout), dtype=torch.float32, device=x.device)
    ops().conv_f32(*conv_f32_args(spec, x, N, H, W, y, act=act, alpha=alpha, res=res, res_post=res_post))
    return y
