"""fp64 references, an fp32 emulation and the derived tolerances of the on-demand correlation
kernels (csrc/kernels/corr_od.hip: ``feat_pool``, ``lookup_od``).

The references take the same bf16-valued inputs the kernels see and compute in float64.  The
emulation repeats the kernels' operation order in fp32 torch ops.  The GPU tests
(tests/test_ondemand_gpu.py) check the kernels, the CPU tests (tests/test_ondemand.py) check
the emulation against the same tolerance, which shows the tolerance is attainable by correct
fp32 code, i.e. neither vacuous nor too tight.

Notation.  ``u = 2^-24`` is the fp32 unit roundoff, ``ub = 2^-8`` the bf16 one (8 significant
bits: half an ulp is at most 2^-8 relative), ``gamma(n) = n u / (1 - n u)`` bounds the relative
error of a result every term of which passes through at most ``n`` fp32 roundings.

One output element is ``sum_t w_t V_l(q; cell_t)`` over the four bilinear taps of its sample,
``w_t >= 0``, ``sum w_t <= 1`` (taps outside the map contribute 0), with
``V_l(q; y, x) = sum_c f1[q, c] * pool_l(f2)[y, x, c] / sqrt(C)``.  Behind it stand the products
``w_t f1[q, c] f2[y', x', c] / (4^l sqrt(C))``; ``A`` is the sum of their absolute values
(:func:`lookup_ref` returns it), ``Vabs = sum_t w_t |V_l(q; cell_t)|``.

Tolerances (derived, no fitted constants):

* ``feat_pool`` (fp32 storage): a level-l cell is l nested 2x2 means, each 3 fp32 additions and an
  exact multiplication by 0.25: ``|err| <= gamma(3 l) * pool_l(|f2|)``.  Storing fp32 adds no
  further term (a bf16 store would add ``ub * pool_l(|f2|)``, and ``ub * A`` to every lookup).
* ``lookup_od``: ``tol = ub (|ref| + g A) + g A``, ``g = gamma(C + 3 l + 8)``:
  the dot product's terms pass through at most C roundings (C / 16 FMAs per lane and 4 tree
  additions: fewer), the pooled features carry 3 l, the scale is a rounded constant times a
  rounded product (2), the blend is ``1 - fy``, two products and a sum, twice (at most 6: fused
  multiply-adds skip some); the window coordinates and the fractions ``fx, fy`` are exact in
  both (``c * 2^-l`` and ``x - floor(x)`` round nothing).  The fp32 result is then rounded to bf16
  once: ``ub`` of its magnitude ``<= |ref| + g A``.
* the volume path (``corr`` + ``lookup`` with bf16 levels) against the same reference:
  ``tol_vol = ub (|ref| + e) + e``, ``e = ub Vabs + g A``: its fp32 accumulation, pooling,
  scale and blend are bounded by the same ``g A``, every level value is rounded to bf16 before
  the blend (``ub Vabs``), and the output once more.
"""
from __future__ import annotations

import functools
import math

import torch

U32 = 2.0 ** -24
U_BF16 = 2.0 ** -8


def gamma(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


def bf(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep fp32 storage."""
    return x.to(torch.bfloat16).float()


def pool(f: torch.Tensor, num_levels: int):
    """[f, 2x2 VALID mean of f, ...] in f's dtype; a level is 0.25 * ((a + b) + (c + d)) of the
    level below (top row pair, then bottom row pair), the kernel's order."""
    out = [f]
    for _ in range(num_levels - 1):
        B, h, w, C = f.shape
        hh, ww = h // 2, w // 2
        t = f[:, : 2 * hh, : 2 * ww].reshape(B, hh, 2, ww, 2, C)
        f = 0.25 * ((t[:, :, 0, :, 0] + t[:, :, 0, :, 1]) + (t[:, :, 1, :, 0] + t[:, :, 1, :, 1]))
        out.append(f)
    return out


# ------------------------------------------------------------------------------- feat_pool
def feat_pool_ref(f2: torch.Tensor, num_levels: int):
    """fp64 pooled levels 1 .. L-1 of the (bf16-valued) features and their tolerances."""
    lv = pool(f2.double(), num_levels)
    mag = pool(f2.double().abs(), num_levels)
    return [(lv[l], gamma(3 * l) * mag[l]) for l in range(1, num_levels)]


def feat_pool_emul(f2: torch.Tensor, num_levels: int):
    return pool(f2.float(), num_levels)[1:]


# -------------------------------------------------------------------------------- lookup_od
def _windows(c: torch.Tensor, radius: int, hl: int, wl: int):
    """c: (B, Q, 2) level coordinates.  Returns the linear cell index (B, Q, W1*W1) [row][column],
    its validity and the fractions (wx, wy), each (B, Q, 1, 1)."""
    B, Q, _ = c.shape
    W1 = 2 * radius + 2
    x0 = torch.floor(c[..., 0])
    y0 = torch.floor(c[..., 1])
    wx = (c[..., 0] - x0).view(B, Q, 1, 1)
    wy = (c[..., 1] - y0).view(B, Q, 1, 1)
    win = torch.arange(W1)
    xs = (x0.clamp(-2.0 ** 20, 2.0 ** 20).long() - radius).view(B, Q, 1, 1) + win.view(1, 1, 1, W1)
    ys = (y0.clamp(-2.0 ** 20, 2.0 ** 20).long() - radius).view(B, Q, 1, 1) + win.view(1, 1, W1, 1)
    valid = (xs >= 0) & (xs < wl) & (ys >= 0) & (ys < hl)
    lin = (ys.clamp(0, hl - 1) * wl + xs.clamp(0, wl - 1)).reshape(B, Q, W1 * W1)
    return lin, valid.reshape(B, Q, W1 * W1), wx, wy


def _blend(cells: torch.Tensor, wx: torch.Tensor, wy: torch.Tensor) -> torch.Tensor:
    """cells (B, Q, W1, W1) [row][column] -> (B, Q, S*S) in the order [i (x)][j (y)]: vertical,
    then horizontal, as the kernels blend."""
    v = (1.0 - wy) * cells[:, :, :-1, :] + wy * cells[:, :, 1:, :]
    s = (1.0 - wx) * v[..., :-1] + wx * v[..., 1:]
    return s.transpose(2, 3).reshape(cells.shape[0], cells.shape[1], -1)


def lookup_ref(f1: torch.Tensor, f2: torch.Tensor, coords: torch.Tensor, radius: int, num_levels: int):
    """fp64 on-demand lookup of the given (already rounded) feature maps.  f1, f2: (B, h, w, C),
    coords: (B, h, w, 2) fp32.  Returns ``(ref, A, Vabs, level)``, each (B*h*w, L*S*S): the value,
    the sum of absolute products behind it, the blend of the absolute cell values and the
    element's level index (module docstring)."""
    B, h, w, C = f1.shape
    Q = h * w
    W1 = 2 * radius + 2
    S = W1 - 1
    q = f1.double().reshape(B, Q, C)
    lv = pool(f2.double(), num_levels)
    mag = pool(f2.double().abs(), num_levels)
    c = coords.double().reshape(B, Q, 2)
    ref, A, Vabs, level = [], [], [], []
    for l in range(num_levels):
        hl, wl = lv[l].shape[1:3]
        # pooling is linear: the level-l volume of the definition, all pairs in fp64 (small here)
        V = torch.matmul(q, lv[l].reshape(B, hl * wl, C).transpose(1, 2)) / math.sqrt(C)
        P = torch.matmul(q.abs(), mag[l].reshape(B, hl * wl, C).transpose(1, 2)) / math.sqrt(C)
        lin, valid, wx, wy = _windows(c / 2.0 ** l, radius, hl, wl)
        vf = valid.double()
        cells = (torch.gather(V, 2, lin) * vf).view(B, Q, W1, W1)
        prods = (torch.gather(P, 2, lin) * vf).view(B, Q, W1, W1)
        ref.append(_blend(cells, wx, wy))
        A.append(_blend(prods, wx, wy))
        Vabs.append(_blend(cells.abs(), wx, wy))
        level.append(torch.full((B, Q, S * S), l, dtype=torch.long))
    cat = lambda xs: torch.cat(xs, dim=-1).reshape(B * Q, -1)   # noqa: E731
    return cat(ref), cat(A), cat(Vabs), cat(level)


def _g(level: torch.Tensor, C: int) -> torch.Tensor:
    n = (C + 8 + 3 * level).double()
    return n * U32 / (1.0 - n * U32)


def lookup_tol(ref, A, level, C: int) -> torch.Tensor:
    """Per-element tolerance of ``lookup_od``'s bf16 output (module docstring)."""
    gA = _g(level, C) * A
    return U_BF16 * (ref.abs() + gA) + gA


def volume_tol(ref, A, Vabs, level, C: int) -> torch.Tensor:
    """Per-element tolerance of the volume path (bf16 levels, bf16 output) against the same
    reference (module docstring)."""
    e = U_BF16 * Vabs + _g(level, C) * A
    return U_BF16 * (ref.abs() + e) + e


def ratio(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """Largest |got - ref| / tol (0 / 0 = 0; a NaN or an error where tol = 0 is inf)."""
    err = (got.double() - ref.double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol.double())
    r = torch.nan_to_num(r, nan=float("inf"), posinf=float("inf"))
    return float(r.max())


def lookup_emul(f1: torch.Tensor, f2: torch.Tensor, coords: torch.Tensor, radius: int, num_levels: int) -> torch.Tensor:
    """``lookup_od_kernel``'s arithmetic in fp32 torch ops -> bf16-valued (B*h*w, L*S*S).

    The pooled levels in fp32 in the kernel's order; per cell the 16 lane partials (lane ``sub``
    sums the 8-channel chunks sub, sub + 16, .. in channel order), the xor tree 8, 4, 2, 1, the
    fp32 scale, the vertical-then-horizontal blend and one bf16 rounding.  A product and its
    addition are two fp32 operations here and one fused multiply-add in the kernel: one more
    rounding per term, inside the tolerance's count of C."""
    B, h, w, C = f1.shape
    Q = h * w
    W1 = 2 * radius + 2
    nch = max(1, -(-C // 128))
    pad = nch * 128 - C
    scale = torch.tensor(1.0 / math.sqrt(C), dtype=torch.float32)
    lv = pool(f2.float(), num_levels)
    out = []
    c = coords.float().reshape(B, Q, 2)
    for l in range(num_levels):
        hl, wl = lv[l].shape[1:3]
        lin, valid, wx, wy = _windows(c, radius, hl, wl)
        rows = []
        for b in range(B):
            feats = lv[l][b].reshape(hl * wl, C)[lin[b]]                        # (Q, W1*W1, C)
            prod = feats * f1[b].float().reshape(Q, 1, C)
            prod = torch.nn.functional.pad(prod, (0, pad))                       # idle lanes add 0
            # channel = 8 * (sub + 16 n) + e  ->  [n][sub][e]  ->  lane sub sums over (n, e) in order
            lanes = prod.view(Q, W1 * W1, nch, 16, 8).permute(0, 1, 3, 2, 4).reshape(Q, W1 * W1, 16, nch * 8)
            acc = torch.zeros(Q, W1 * W1, 16)
            for k in range(nch * 8):
                acc = acc + lanes[..., k]
            for half in (8, 4, 2, 1):                                            # xor tree
                acc = acc.view(Q, W1 * W1, 2, half)
                acc = acc[:, :, 0] + acc[:, :, 1]
            rows.append(acc.reshape(Q, W1 * W1) * scale)
        cells = (torch.stack(rows) * valid.float()).view(B, Q, W1, W1)
        out.append(_blend(cells, wx.float(), wy.float()))
        c = c / 2
    return bf(torch.cat(out, dim=-1).reshape(B * Q, -1))


# ------------------------------------------------------------------------------------ cases
def features(B: int, h: int, w: int, C: int, seed: int):
    """bf16-valued fp32 feature maps (f1, f2) of a case."""
    g = torch.Generator().manual_seed(seed)
    return bf(torch.randn(B, h, w, C, generator=g)), bf(torch.randn(B, h, w, C, generator=g))


def grid(B: int, h: int, w: int) -> torch.Tensor:
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    return torch.stack([xs, ys], dim=-1).unsqueeze(0).repeat(B, 1, 1, 1)


def special_queries(coords: torch.Tensor) -> torch.Tensor:
    """Overwrite a few queries of ``coords`` (B, h, w, 2) with the special cases: an integer-exact
    coordinate, coordinates far outside (+-1000) and one on each border of the map."""
    B, h, w, _ = coords.shape
    c = coords.clone()
    c[0, 1, 1] = torch.tensor([3.0, 5.0])                    # integer-exact
    c[0, 2, 3] = torch.tensor([1000.25, 2.5])                # far outside, each side and both
    c[0, 3, 2] = torch.tensor([4.5, -1000.75])
    c[B - 1, 4, 4] = torch.tensor([-1000.0, 1000.0])
    c[0, 5, 1] = torch.tensor([0.0, 6.25])                   # left border
    c[0, 5, 2] = torch.tensor([float(w - 1), 6.25])          # right border
    c[B - 1, 6, 1] = torch.tensor([7.5, 0.0])                # top border
    c[B - 1, 6, 2] = torch.tensor([7.5, float(h - 1)])       # bottom border
    return c


def coord_field(kind: str, B: int, h: int, w: int, seed: int) -> torch.Tensor:
    """The coordinate fields of the GPU tests: ``smooth`` (the grid plus a constant subpixel shift:
    neighbouring queries' windows overlap), ``scattered`` (an independent jump of +-h per query and
    axis: windows of neighbouring queries are disjoint, many partly or wholly off the map) and
    ``special`` (smooth with :func:`special_queries`)."""
    base = grid(B, h, w) + torch.tensor([0.375, -0.6875])
    if kind == "smooth":
        return base
    if kind == "special":
        return special_queries(base)
    assert kind == "scattered", kind
    g = torch.Generator().manual_seed(seed)
    jump = (torch.randint(0, 2, (B, h, w, 2), generator=g).float() * 2 - 1) * h
    return base + jump + torch.rand(B, h, w, 2, generator=g)


@functools.lru_cache(maxsize=None)
def lookup_case(h: int, w: int, C: int, r: int, L: int, kind: str, B: int = 2):
    """(f1, f2, coords, ref, tol) of one lookup case, computed once per process and shared."""
    seed = 1000 * h + 10 * w + C + r + L
    f1, f2 = features(B, h, w, C, seed)
    coords = coord_field(kind, B, h, w, seed + 1)
    ref, A, _, level = lookup_ref(f1, f2, coords, r, L)
    return f1, f2, coords, ref, lookup_tol(ref, A, level, C)
