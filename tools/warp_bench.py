#!/usr/bin/env python3
"""What the motion-compensated frames and the photometric error cost inside the bidirectional
plan, against composing them from PyTorch ops after the call: batch 1, 436 x 1024 uint8 frames
(run at the padded 440 x 1024), raft_large at 32 iterations and raft_small at 12.

Protocol: ``b1_sync`` of bench.py (per step: H2D from pageable host memory + forward with all
iterations upsampled + synchronise; no cross-step overlap).  Arms, alternated in one process,
~0.5 s of steady steps per block after a warm-up of every plan:

* ``bidir``: ``forward(bidirectional=True)``.
* ``warp``:  ``forward(bidirectional=True, warp=True)``: the same plan + the clear of the sums +
  one ``warp_frames`` launch (csrc/kernels/framewarp.hip) + the copies of its two outputs.
* ``torch``: ``bidir`` followed by the same result composed from PyTorch ops, which is what a
  user writes today: ``grid_sample`` in pixel coordinates (``align_corners=True``), rounding,
  the inside / occlusion masks, ``where`` and the abs-diff reductions, for both directions.
* ``bidir'``, ``warp'``, ``torch'``: the same arms on a second engine (its own plans, its own
  captured graphs).  Two captures of one plan do not replay equally fast, so |arm' - arm| is
  the spread below which a difference between arms says nothing.

The figure is the mean latency of each arm; the verdict is whether ``warp - bidir`` lies below
``torch - bidir`` by more than the capture spread of this run.  The ``warp_frames`` launch alone
(both directions, the sums cleared before each) is also timed from device events over 500
repetitions, with the bytes it moves.

  python tools/warp_bench.py [--out profiles/warp_overhead.txt] [--block-s 0.5] [--rounds 2]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_raft_amd import raft_large, raft_small  # noqa: E402
from jax_raft_amd.ops import native as nat  # noqa: E402
from jax_raft_amd.runtime.engine import RaftEngine, sintel_pad  # noqa: E402

H0, W0 = 436, 1024
_GRID = {}


def compose(f1, f2, res):
    """The warp and the photometric sums of both directions from PyTorch ops (within one level of
    the kernel: grid_sample weighs the four texels in another order)."""
    dev = f1.device
    if dev not in _GRID:
        _GRID[dev] = torch.meshgrid(torch.arange(H0, dtype=torch.float32, device=dev),
                                    torch.arange(W0, dtype=torch.float32, device=dev), indexing="ij")
    ys, xs = _GRID[dev]
    out = []
    for src, own, flow, occ in ((f2, f1, res.flows_fw[-1], res.occ_fw), (f1, f2, res.flows_bw[-1], res.occ_bw)):
        px, py = xs + flow[..., 0], ys + flow[..., 1]
        inside = (px >= 0) & (px <= W0 - 1) & (py >= 0) & (py <= H0 - 1)
        grid = torch.stack([px / (W0 - 1) * 2 - 1, py / (H0 - 1) * 2 - 1], -1)
        w = torch.nn.functional.grid_sample(src.permute(0, 3, 1, 2).float(), grid, mode="bilinear", padding_mode="border",
                                            align_corners=True).permute(0, 2, 3, 1).round().to(torch.uint8)
        keep = inside & ~occ
        warped = torch.where(keep.unsqueeze(-1), w, own)
        d = (w.to(torch.int32) - own.to(torch.int32)).abs().sum(-1)
        out.append((warped, torch.stack([(d * keep).sum((1, 2)), keep.sum((1, 2))], -1)))
    return out[0][0], out[1][0], torch.stack([out[0][1], out[1][1]])


def step(eng, a, b, dev, iters, arm):
    f1, f2 = a.to(dev), b.to(dev)
    if arm == "warp":
        res = eng.forward(f1, f2, iters, bidirectional=True, warp=True)
        out = res.warped_fw, res.warped_bw, res.photo
    else:
        res = eng.forward(f1, f2, iters, bidirectional=True)
        out = compose(f1, f2, res) if arm == "torch" else None
    torch.cuda.synchronize(dev)
    return res, out


def block(eng, pairs, dev, iters, arm, seconds):
    """Steady steps of one arm for ~``seconds``: the latencies in ms."""
    lat, i, t_end = [], 0, time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(lat) < 8:
        a, b = pairs[i % len(pairs)]
        t0 = time.perf_counter()
        res, out = step(eng, a, b, dev, iters, arm)
        lat.append(1000 * (time.perf_counter() - t0))
        i += 1
    assert res.flows_fw.shape[1:] == (1, H0, W0, 2) and (out is None or out[0].shape == (1, H0, W0, 3))
    return lat


def launch_alone(dev, reps=500):
    """The warp_frames launch for both directions on buffers of the plan's shapes: us per launch
    (the clear of the sums included) and the bytes it moves."""
    pt, pb, pl, pr = sintel_pad(H0, W0)
    H, W = H0 + pt + pb, W0 + pl + pr
    g = torch.Generator().manual_seed(5)
    f1, f2 = (torch.randint(0, 256, (1, H0, W0, 3), dtype=torch.uint8, generator=g).to(dev) for _ in range(2))
    fw, bw = ((torch.randn(1, H, W, 2, generator=g) * 4).to(dev) for _ in range(2))
    occ = (torch.rand(2, 1, H, W, generator=g) < 0.2).to(torch.uint8).to(dev)
    warped = torch.empty((2, 1, H0, W0, 3), dtype=torch.uint8, device=dev)
    photo = torch.zeros((2, 1, 2), dtype=torch.int64, device=dev)
    t, i = [f2, f1, f1, f2, fw, bw, occ, warped, photo], [1, H, W, H0, W0, pt, pl, 2]

    def run():
        nat.ops().memset([photo])
        nat.ops().warp_frames(t, i)

    for _ in range(20):
        run()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    e.synchronize()
    us = 1000 * s.elapsed_time(e) / reps
    px = 2 * H0 * W0
    moved = px * (8 + 1 + 3 + 3 + 3)   # flow, mask, sampled frame (each texel once), own, warped
    return us, moved, int(photo[0, 0, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/warp_overhead.txt")
    ap.add_argument("--block-s", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2, help="rounds over all arms per configuration")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "warp_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(99)
    pairs = [tuple(torch.randint(0, 256, (1, H0, W0, 3), dtype=torch.uint8, generator=g) for _ in range(2)) for _ in range(4)]
    lines = [f"motion-compensated frames + photometric error: in the bidirectional plan vs composed from PyTorch ops, "
             f"{torch.cuda.get_device_name(dev)}",
             f"batch 1, {H0}x{W0} uint8 frames, b1_sync protocol (H2D pageable + forward, all iterations upsampled + sync),",
             f"arms alternated bidir/warp/torch on two engines x {args.rounds} in one process, ~{args.block_s} s per block;",
             "bidir = forward(bidirectional=True); warp = forward(bidirectional=True, warp=True);",
             "torch = bidir + grid_sample / masks / abs-diff reductions of both directions from PyTorch ops;",
             "arm' = the same arm on a second engine (another capture of the same plans): the spread of this protocol.",
             "ms per step: mean over the arm's blocks (per-block means in brackets)", ""]
    for name, factory, iters in (("raft_large", raft_large, 32), ("raft_small", raft_small, 12)):
        model = factory(seed=0)[0].to(dev).eval()
        eng, twin = RaftEngine(model, dev), RaftEngine(model, dev)
        order = [(arm + suffix, e, arm) for suffix, e in (("", eng), ("'", twin)) for arm in ("bidir", "warp", "torch")]
        for _ in range(2):   # every plan built, graphs captured, steady clocks
            for _, e, arm in order:
                block(e, pairs, dev, iters, arm, 0.1)
        arms = {k: [] for k, _, _ in order}
        for _ in range(args.rounds):
            for k, e, arm in order:
                arms[k].append(block(e, pairs, dev, iters, arm, args.block_s))
        mean = {k: sum(map(sum, v)) / sum(map(len, v)) for k, v in arms.items()}
        per = {k: ", ".join(f"{sum(b) / len(b):.3f}" for b in v) for k, v in arms.items()}
        bidir, warp, tor = ((mean[k] + mean[k + "'"]) / 2 for k in ("bidir", "warp", "torch"))
        spread = max(abs(mean[k + "'"] - mean[k]) for k in ("bidir", "warp", "torch"))
        saved = (tor - bidir) - (warp - bidir)
        lines.append(f"{name:10s} {iters:2d} it  " + "  ".join(f"{k} {mean[k]:6.3f} ms [{per[k]}]" for k in arms))
        lines.append(f"{'':10s}        mean of both captures: bidir {bidir:6.3f}  warp {warp:6.3f}  torch {tor:6.3f} ms"
                     f"   warp - bidir {warp - bidir:+6.3f} ms   torch - bidir {tor - bidir:+6.3f} ms"
                     f"   capture spread {spread:5.3f} ms"
                     f"   in-plan warp cheaper than the composition by more than the spread: "
                     + ("yes" if saved > spread else "NO (within the capture spread)" if saved > -spread else "NO (dearer)")
                     + f" ({saved:+6.3f} ms)")
        print(lines[-2], flush=True)
        print(lines[-1], flush=True)
        eng.release()
        twin.release()
    us, moved, kept = launch_alone(dev)
    lines += ["", f"warp_frames alone (memset of the sums + one launch, both directions, 500 repetitions, device events): "
                  f"{us:.2f} us per repetition, {moved / 1e6:.2f} MB moved (flows, masks, each sampled texel once, own, "
                  f"warped) = {moved / us / 1e3:.0f} GB/s; {kept} of {H0 * W0} pixels kept in direction 0"]
    print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
