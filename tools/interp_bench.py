#!/usr/bin/env python3
"""What frame interpolation by forward splatting costs: batch 1, 436 x 1024 uint8 frames (flows at
the padded 440 x 1024), on an MI355X.

1. The clear of the accumulator and the two launches (csrc/kernels/interp.hip), each and together,
   from device events over 500 repetitions, with the number of atomics issued and the bytes that
   must move -- for a scattered flow field (every pixel's flow drawn on its own) and for a smooth
   one (what a video has), since where the atomics land decides what the splat costs.
2. Clear + splat + resolve against the same result composed from PyTorch ops on the same GPU
   tensors -- int64 ``index_add_`` per tap plus integer ops, which is what a user writes without
   the kernels (checked bitwise against them first).  The arms are alternated in one process and
   each arm is run twice; the native path counts as faster only if it wins by more than the larger
   spread between the two runs of one arm.
3. ``forward(bidirectional=True, interpolate=(0.5,))`` against ``forward(bidirectional=True)``,
   raft_large at 32 iterations and raft_small at 12, in the ``b1_sync`` protocol of bench.py (per
   step: H2D from pageable host memory + forward with all iterations upsampled + synchronise),
   each on two engines (two captures of the same plans): the difference next to the
   capture-to-capture spread.  No end-to-end gain is claimed.

  python tools/interp_bench.py [--out profiles/interp_overhead.txt] [--block-s 0.5] [--rounds 2] [--kernels-only]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_raft_amd import raft_large, raft_small  # noqa: E402
from jax_raft_amd.models.reference import CONSISTENT, interp_params  # noqa: E402
from jax_raft_amd.ops import native as nat  # noqa: E402
from jax_raft_amd.runtime.engine import RaftEngine, sintel_pad  # noqa: E402

H0, W0 = 436, 1024
T = 0.5


def compose(f1, f2, fw, bw, occ, tq, dmin, win, count=False):
    """interpolate_frames from PyTorch ops without a host synchronisation: a tap outside the frame
    adds weight 0 to cell 0.  Returns (frame_t, holes, acc, taps of weight != 0 inside the frame if ``count``)."""
    H0, W0, top, left = win
    dev = fw.device
    B = fw.shape[0]
    P = H0 * W0
    acc = torch.zeros((2, B * P, 4), dtype=torch.int64, device=dev)
    xs = torch.arange(W0, device=dev, dtype=torch.float32).view(1, 1, W0)
    ys = torch.arange(H0, device=dev, dtype=torch.float32).view(1, H0, 1)
    base = (torch.arange(B, device=dev, dtype=torch.int64) * P).view(B, 1, 1)
    taps = torch.zeros((), dtype=torch.int64, device=dev)
    for d, (frame, flow, step) in enumerate(((f1, fw, tq), (f2, bw, 256 - tq))):
        s = torch.tensor(float(step), dtype=torch.float32, device=dev) / 256.0
        f = flow[:, top:top + H0, left:left + W0]
        px, py = xs + s * f[..., 0], ys + s * f[..., 1]
        ok = (px > -1) & (px < W0) & (py > -1) & (py < H0)
        pxs, pys = torch.where(ok, px, 0.0), torch.where(ok, py, 0.0)
        x0f, y0f = torch.floor(pxs), torch.floor(pys)
        qx, qy = torch.round((pxs - x0f) * 16.0).long(), torch.round((pys - y0f) * 16.0).long()
        x0, y0 = x0f.long(), y0f.long()
        k = torch.where(occ[d, :, top:top + H0, left:left + W0] != 0, 1, CONSISTENT)
        rgb1 = torch.cat([torch.ones((B, H0, W0, 1), dtype=torch.int64, device=dev), frame.long()], -1)
        for dy in (0, 1):
            for dx in (0, 1):
                tx, ty = x0 + dx, y0 + dy
                sel = ok & (tx >= 0) & (tx < W0) & (ty >= 0) & (ty < H0)
                w = torch.where(sel, (qx if dx else 16 - qx) * (qy if dy else 16 - qy) * k, 0)
                idx = torch.where(sel, base + ty * W0 + tx, 0)
                acc[d].index_add_(0, idx.reshape(-1), (w.unsqueeze(-1) * rgb1).reshape(-1, 4))
                if count:
                    taps += (w != 0).sum()
    acc = acc.view(2, B, H0, W0, 4)
    tot = (256 - tq) * acc[0] + tq * acc[1]
    D = tot[..., :1]
    holes = D[..., 0] < dmin
    Ds = torch.where(holes.unsqueeze(-1), 1, D)
    v = torch.div(2 * tot[..., 1:] + Ds, 2 * Ds, rounding_mode="floor").clamp_(0, 255).to(torch.uint8)
    return torch.where(holes.unsqueeze(-1), f1 if tq <= 128 else f2, v), holes, acc, taps


def timed(fn, reps):
    """us per call of ``fn`` from device events over ``reps`` calls (after 20 warm-up calls)."""
    for _ in range(20):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return 1000 * s.elapsed_time(e) / reps


FLOWS = {"scattered": "every pixel's flow drawn on its own, sigma 4 px: neighbouring sources land on unrelated cells, the "
                      "worst case for the locality of the atomics",
         "smooth": "a translation of (5.3, -2.7) px plus a smooth field of a few pixels (a 6 x 12 random grid, bicubic): "
                   "neighbouring sources land on neighbouring cells, as in a video"}


def make_flow(kind, H, W, g):
    if kind == "scattered":
        return torch.randn(1, H, W, 2, generator=g) * 4
    coarse = torch.randn(1, 2, 6, 12, generator=g) * 3
    f = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=True).permute(0, 2, 3, 1)
    return (f + torch.tensor([5.3, -2.7])).contiguous()


def kernels_alone(dev, lines, kind, reps=500):
    pt, pb, pl, pr = sintel_pad(H0, W0)
    H, W = H0 + pt + pb, W0 + pl + pr
    win = [H0, W0, pt, pl]
    g = torch.Generator().manual_seed(5)
    f1, f2 = (torch.randint(0, 256, (1, H0, W0, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(2))
    fw, bw = (make_flow(kind, H, W, g).to(dev) for _ in range(2))
    occ = (torch.rand(2, 1, H, W, generator=g) < 0.2).to(torch.uint8).to(dev)
    tq, dmin = interp_params(T)
    par = torch.tensor([[tq, dmin]], dtype=torch.int32, device=dev)
    acc = torch.zeros((2, 1, H0, W0, 4), dtype=torch.int64, device=dev)
    out = torch.empty((1, H0, W0, 3), dtype=torch.uint8, device=dev)
    holes = torch.empty((1, H0, W0), dtype=torch.uint8, device=dev)
    st, si = [f1, f2, fw, bw, occ, acc, par], [1, H, W] + win + [0]
    rt, ri = [f1, f2, acc, par, out, holes], [1, H0, W0, 0]
    ops = nat.ops()
    clear = lambda: ops.memset([acc])
    splat = lambda: ops.interp_splat(st, si)
    resolve = lambda: ops.interp_resolve(rt, ri)

    def native():
        clear()
        splat()
        resolve()

    native()
    want = compose(f1, f2, fw, bw, occ, tq, dmin, win, count=True)
    torch.cuda.synchronize(dev)
    same = torch.equal(out, want[0]) and torch.equal(holes.bool(), want[1]) and torch.equal(acc, want[2])
    assert same, "the composition from PyTorch ops and the kernels disagree"
    taps, n_holes = int(want[3]), int(want[1].sum())
    # 1. each launch and the three together (the splat alone keeps adding to acc: the same work every time)
    us = {name: timed(fn, reps) for name, fn in (("clear", clear), ("splat", splat), ("resolve", resolve), ("all", native))}
    native()
    P = H0 * W0
    b_clear, b_splat, b_res = 2 * P * 32, 2 * P * (8 + 1 + 3) + taps * 32, 2 * P * 32 + P * 4 + 3 * n_holes
    lines += [f"{kind} flows ({FLOWS[kind]})",
              f"1. the launches alone, t = {T} (tq = {tq}, Dmin = {dmin}), 20 % occluded, {reps} repetitions each, device events:",
              f"   clear of acc     {us['clear']:7.2f} us   {b_clear / 1e6:6.2f} MB written = {b_clear / us['clear'] / 1e3:5.0f} GB/s",
              f"   interp_splat     {us['splat']:7.2f} us   {taps} taps of weight != 0 inside the frame = {4 * taps} 64-bit integer "
              f"atomics ({4 * taps / us['splat'] / 1e3:.2f} G atomics/s); {b_splat / 1e6:.2f} MB must move (flow, mask, colour "
              f"per source, 32 B per tap)",
              f"   interp_resolve   {us['resolve']:7.2f} us   {b_res / 1e6:6.2f} MB must move (64 B of acc per pixel, 4 B out, the "
              f"fallback texel of {n_holes} holes) = {b_res / us['resolve'] / 1e3:5.0f} GB/s",
              f"   the three in a row {us['all']:6.2f} us (sum of the parts {us['clear'] + us['splat'] + us['resolve']:.2f} us)", ""]
    # 2. against the composition, alternated, each arm twice
    runs = {"native": [], "torch": []}
    fn = {"native": native, "torch": lambda: compose(f1, f2, fw, bw, occ, tq, dmin, win)}
    for _ in range(2):
        for arm in ("native", "torch"):
            runs[arm].append(timed(fn[arm], reps if arm == "native" else 50))
    spread = max(abs(v[0] - v[1]) for v in runs.values())
    gain = min(runs["torch"]) - max(runs["native"])
    lines += ["2. clear + splat + resolve against the same result (checked bitwise) composed from PyTorch ops on the same GPU "
              "tensors (int64 index_add_ per tap + integer ops, no host synchronisation), arms alternated, each run twice:",
              f"   native {runs['native'][0]:8.2f} / {runs['native'][1]:8.2f} us   torch {runs['torch'][0]:8.2f} / "
              f"{runs['torch'][1]:8.2f} us   larger spread between two runs of one arm {spread:.2f} us",
              f"   native faster by more than that spread: " + (f"yes (slowest native run {gain:.2f} us below the fastest torch run, "
              f"{min(runs['torch']) / max(runs['native']):.1f}x)" if gain > spread else f"NO (difference {gain:.2f} us)"), ""]
    for ln in lines[-13:]:
        print(ln, flush=True)


def step(eng, a, b, dev, iters, arm):
    f1, f2 = a.to(dev), b.to(dev)
    res = eng.forward(f1, f2, iters, bidirectional=True, **(dict(interpolate=(T,)) if arm == "interp" else {}))
    torch.cuda.synchronize(dev)
    return res


def block(eng, pairs, dev, iters, arm, seconds):
    """Steady steps of one arm for ~``seconds``: the latencies in ms."""
    lat, i, t_end = [], 0, time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(lat) < 8:
        a, b = pairs[i % len(pairs)]
        t0 = time.perf_counter()
        res = step(eng, a, b, dev, iters, arm)
        lat.append(1000 * (time.perf_counter() - t0))
        i += 1
    assert res.flows_fw.shape[1:] == (1, H0, W0, 2) and (arm != "interp" or res.frames.shape == (1, 1, H0, W0, 3))
    return lat


def end_to_end(dev, lines, block_s, rounds):
    g = torch.Generator().manual_seed(99)
    pairs = [tuple(torch.randint(0, 256, (1, H0, W0, 3), dtype=torch.uint8, generator=g) for _ in range(2)) for _ in range(4)]
    lines += [f"3. forward(bidirectional=True, interpolate=({T},)) against forward(bidirectional=True): b1_sync protocol (H2D "
              f"pageable + forward, all iterations upsampled + sync), arms alternated on two engines x {rounds} in one process, "
              f"~{block_s} s per block;",
              "   arm' = the same arm on a second engine (another capture of the same plans).  ms per step: mean over the arm's "
              "blocks (per-block means in brackets)"]
    for name, factory, iters in (("raft_large", raft_large, 32), ("raft_small", raft_small, 12)):
        model = factory(seed=0)[0].to(dev).eval()
        eng, twin = RaftEngine(model, dev), RaftEngine(model, dev)
        order = [(arm + suffix, e, arm) for suffix, e in (("", eng), ("'", twin)) for arm in ("bidir", "interp")]
        for _ in range(2):   # every plan built, graphs captured, steady clocks
            for _, e, arm in order:
                block(e, pairs, dev, iters, arm, 0.1)
        arms = {k: [] for k, _, _ in order}
        for _ in range(rounds):
            for k, e, arm in order:
                arms[k].append(block(e, pairs, dev, iters, arm, block_s))
        mean = {k: sum(map(sum, v)) / sum(map(len, v)) for k, v in arms.items()}
        per = {k: ", ".join(f"{sum(b) / len(b):.3f}" for b in v) for k, v in arms.items()}
        bidir, interp = ((mean[k] + mean[k + "'"]) / 2 for k in ("bidir", "interp"))
        spread = max(abs(mean[k + "'"] - mean[k]) for k in ("bidir", "interp"))
        lines.append(f"   {name:10s} {iters:2d} it  " + "  ".join(f"{k} {mean[k]:6.3f} ms [{per[k]}]" for k in arms))
        lines.append(f"   {'':10s}        mean of both captures: bidir {bidir:6.3f}  interp {interp:6.3f} ms   interp - bidir "
                     f"{interp - bidir:+6.3f} ms   capture spread {spread:5.3f} ms   the difference "
                     + ("exceeds" if abs(interp - bidir) > spread else "lies within") + " the capture spread")
        print(lines[-2], flush=True)
        print(lines[-1], flush=True)
        eng.release()
        twin.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/interp_overhead.txt")
    ap.add_argument("--block-s", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2, help="rounds over all arms per configuration")
    ap.add_argument("--kernels-only", action="store_true", help="parts 1 and 2 only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "interp_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    lines = [f"frame interpolation by forward splatting (csrc/kernels/interp.hip), {torch.cuda.get_device_name(dev)}",
             f"batch 1, {H0}x{W0} uint8 frames, flows at the padded size; what these numbers do not show: any quality of the "
             "interpolated frames (random weights, random flows), other batch sizes or resolutions.", ""]
    for kind in FLOWS:
        kernels_alone(dev, lines, kind)
    if not args.kernels_only:
        end_to_end(dev, lines, args.block_s, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
