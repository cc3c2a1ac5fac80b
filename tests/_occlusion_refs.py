"""Shared inputs and independent references for the occlusion tests (test_occlusion.py on the CPU,
test_occlusion_gpu.py on the GPU): flow fields, a per-pixel Python reading of the range map, an fp64
bilinear splat and the two-layer scene with known occlusion."""
import math

import numpy as np
import torch

NAN, INF = float("nan"), float("inf")


def range_map_loops(flow: torch.Tensor) -> torch.Tensor:
    """``range_map`` read off its four steps, one source pixel at a time (numpy fp32 for the add, exact
    Python arithmetic after it; ``round`` is ties-to-even)."""
    B, H, W, _ = flow.shape
    f = flow.numpy()
    acc = np.zeros((B, H, W), dtype=np.int64)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                px = float(np.float32(x) + f[b, y, x, 0])
                py = float(np.float32(y) + f[b, y, x, 1])
                if not (-1 < px < W and -1 < py < H):
                    continue
                x0, y0 = math.floor(px), math.floor(py)
                qx, qy = round((px - x0) * 16), round((py - y0) * 16)
                for dy in (0, 1):
                    for dx in (0, 1):
                        tx, ty = x0 + dx, y0 + dy
                        if 0 <= tx < W and 0 <= ty < H:
                            acc[b, ty, tx] += (qx if dx else 16 - qx) * (qy if dy else 16 - qy)
    return torch.from_numpy(acc).to(torch.int32)


def splat_fp64(flow: torch.Tensor):
    """An fp64 bilinear splat of the fp32 landing points (step 1 is part of the definition; nothing
    after it is quantised): ``(ref (B, H, W) fp64 in source pixels, n (B, H, W) taps received)``."""
    B, H, W, _ = flow.shape
    px = (torch.arange(W, dtype=torch.float32).view(1, 1, W) + flow[..., 0]).double()
    py = (torch.arange(H, dtype=torch.float32).view(1, H, 1) + flow[..., 1]).double()
    ok = (px > -1) & (px < W) & (py > -1) & (py < H)
    ref = torch.zeros(B, H, W, dtype=torch.float64)
    n = torch.zeros(B, H, W, dtype=torch.int64)
    bidx = torch.arange(B).view(B, 1, 1).expand(B, H, W)
    for dy in (0, 1):
        for dx in (0, 1):
            x0, y0 = torch.floor(px), torch.floor(py)
            wx = (px - x0) if dx else (1.0 - (px - x0))
            wy = (py - y0) if dy else (1.0 - (py - y0))
            tx, ty = x0.long() + dx, y0.long() + dy
            sel = ok & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            ref.index_put_((bidx[sel], ty[sel], tx[sel]), (wx * wy)[sel], accumulate=True)
            n.index_put_((bidx[sel], ty[sel], tx[sel]), torch.ones_like(tx[sel]), accumulate=True)
    return ref, n


def smooth_field(B, H, W, seed=0, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    ph = torch.rand(B, 4, generator=g) * 6.283
    y = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    p = lambda k: ph[:, k].view(B, 1, 1)
    fx = amp * torch.sin(0.21 * x + 0.13 * y + p(0)) + 0.7 * amp * torch.cos(0.08 * y + p(1)) + 0.37
    fy = amp * torch.cos(0.17 * y - 0.11 * x + p(2)) + 0.7 * amp * torch.sin(0.09 * x + p(3)) - 0.21
    return torch.stack([fx.expand(B, H, W), fy.expand(B, H, W)], -1).contiguous()


def random_field(B, H, W, seed=0):
    """Uniform in +-2 max(H, W): many sources land outside."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, H, W, 2, generator=g) * 2.0 - 1.0) * (2.0 * max(H, W))


def one_cell_field(B, H, W, ty, tx):
    """Every source lands exactly on cell (ty, tx): the contention case, acc there = 256 H W."""
    y = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    return torch.stack([tx - x, ty - y], -1).contiguous()


def special_field(B, H, W):
    """Zero flow with, where the map has room, the special sources of the CPU tests: NaN, +-inf, +-1e30,
    landings in (-1, 0) and (W-1, W) / (H-1, H), the 1/32 and 3/32 ties."""
    f = torch.zeros(B, H, W, 2)
    vals = [(NAN, 0.0), (0.0, NAN), (INF, 0.0), (0.0, -INF), (1e30, 0.0), (0.0, -1e30), (1 / 32, 0.0), (3 / 32, 1 / 32),
            (0.0, 3 / 32)]
    k = 0
    for y in range(1, H - 1):
        for x in range(1, W - 1):
            if k < len(vals) and (x + y) % 2 == 0:
                f[:, y, x] = torch.tensor(vals[k])
                k += 1
    f[:, 0, 0] = torch.tensor([-0.5, -0.25])
    f[:, H - 1, W - 1] = torch.tensor([0.5, 0.75])
    f[:, 0, W - 1] = torch.tensor([0.96875, -0.96875])
    f[:, H - 1, 0] = torch.tensor([-1.0, 1.0])                # px = -1, py = H: contributes nothing
    return f


# ---------------------------------------------------------------- the two-layer scene
SCENE_HW = (32, 40)
SQ, SQ_Y, SQ_X, SHIFT = 12, 9, 10, 6
RIM = 1          # pixels on either side of a layer boundary that the scene tests leave out


def two_layer_scene(B=1):
    """A background with zero flow and a 12x12 foreground square moving by (+6, 0): exact forward and
    backward flows and the visibility masks that follow from the geometry.  In frame 1 the square covers
    x in [10, 22), in frame 2 [16, 28): the background strip [22, 28) of frame 1 is covered in frame 2,
    the strip [10, 16) of frame 2 is covered in frame 1."""
    H, W = SCENE_HW
    fw, bw = torch.zeros(B, H, W, 2), torch.zeros(B, H, W, 2)
    rows = slice(SQ_Y, SQ_Y + SQ)
    fw[:, rows, SQ_X:SQ_X + SQ, 0] = float(SHIFT)
    bw[:, rows, SQ_X + SHIFT:SQ_X + SHIFT + SQ, 0] = -float(SHIFT)
    vis_fw, vis_bw = torch.ones(B, H, W), torch.ones(B, H, W)
    vis_fw[:, rows, SQ_X + SQ:SQ_X + SQ + SHIFT] = 0.0
    vis_bw[:, rows, SQ_X:SQ_X + SHIFT] = 0.0
    # off the rim: not within RIM pixels of the boundary of the square in either frame
    off = torch.ones(H, W, dtype=torch.bool)
    for x_lo in (SQ_X, SQ_X + SHIFT):
        box = torch.zeros(H, W, dtype=torch.bool)
        box[SQ_Y - RIM:SQ_Y + SQ + RIM, x_lo - RIM:x_lo + SQ + RIM] = True
        box[SQ_Y + RIM:SQ_Y + SQ - RIM, x_lo + RIM:x_lo + SQ - RIM] = False
        off &= ~box
    return fw, bw, vis_fw, vis_bw, off.expand(B, H, W)
