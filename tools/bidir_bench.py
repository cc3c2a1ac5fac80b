#!/usr/bin/env python3
"""One bidirectional call against the two unidirectional calls it replaces:
``forward(i1, i2, bidirectional=True)`` (one plan: one feature-encoder pass, a loop of
batch 2, the forward-backward check in the epilogue) vs ``forward(i1, i2)`` then
``forward(i2, i1)`` on the unchanged cold plan (no masks), raft_large and raft_small,
batch 1, 440 x 1024, 12 and 32 iterations.

Protocol: ``b1_sync`` of bench.py (per step: H2D from pageable host memory + forward with
all iterations upsampled + synchronise; no cross-step overlap).  Arms, alternated in one
process, ~0.5 s of steady steps per block after a warm-up of every plan:

* ``bidir``: H2D of the pair, one bidirectional forward, synchronise.
* ``two``:   two full b1_sync steps, (i1, i2) then (i2, i1): what calling the engine
  twice costs today (each step uploads its frames and synchronises).
* ``two1``:  an extra arm outside the b1_sync protocol, reported next to the comparison and
  not part of its verdict: the most favourable form of the two calls (one H2D of the pair,
  both forwards enqueued back to back, one synchronise).
* ``bidir'``, ``two'``, ``two1'``: the same arms on a second engine (its own plans, its
  own captured graphs).  Two captures of one plan do not replay equally fast (the
  replayed branches are placed per capture), so |arm' - arm| is the spread below which a
  difference between arms says nothing.

The figure is the mean latency of each arm; "gain" is ``two - bidir`` (positive: the
bidirectional call is faster), to be read against the capture spread printed next to it;
the slowest bidirectional capture is also set against the fastest capture of the two calls.

  python tools/bidir_bench.py [--out profiles/bidir_overhead.txt] [--block-s 0.5] [--rounds 2]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_raft_amd import raft_large, raft_small  # noqa: E402
from jax_raft_amd.runtime.engine import RaftEngine  # noqa: E402

H, W = 440, 1024


def step(eng, a, b, dev, iters, arm):
    if arm == "bidir":
        res = eng.forward(a.to(dev), b.to(dev), iters, bidirectional=True)
        torch.cuda.synchronize(dev)
        return res.flows_fw[-1], res.flows_bw[-1]
    if arm == "two":
        fw = eng.forward(a.to(dev), b.to(dev), iters)[-1]
        torch.cuda.synchronize(dev)
        bw = eng.forward(b.to(dev), a.to(dev), iters)[-1]
        torch.cuda.synchronize(dev)
        return fw, bw
    da, db = a.to(dev), b.to(dev)
    fw = eng.forward(da, db, iters)[-1]
    bw = eng.forward(db, da, iters)[-1]
    torch.cuda.synchronize(dev)
    return fw, bw


def block(eng, pairs, dev, iters, arm, seconds):
    """Steady steps of one arm for ~``seconds``: the latencies in ms."""
    lat, i, t_end = [], 0, time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(lat) < 8:
        a, b = pairs[i % len(pairs)]
        t0 = time.perf_counter()
        fw, bw = step(eng, a, b, dev, iters, arm)
        lat.append(1000 * (time.perf_counter() - t0))
        i += 1
    assert fw.shape == bw.shape == (1, H, W, 2)
    return lat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/bidir_overhead.txt")
    ap.add_argument("--block-s", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2, help="rounds over all arms per configuration")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bidir_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(99)
    pairs = [(torch.rand(1, H, W, 3, generator=g) * 2 - 1, torch.rand(1, H, W, 3, generator=g) * 2 - 1)
             for _ in range(4)]
    lines = [f"one bidirectional call vs the two unidirectional calls it replaces, {torch.cuda.get_device_name(dev)}",
             f"batch 1, {H}x{W}, b1_sync protocol (H2D pageable + forward, all iterations upsampled + sync),",
             f"arms alternated bidir/two/two1 on two engines x {args.rounds} in one process, ~{args.block_s} s per block;",
             "bidir = forward(bidirectional=True): both flows + both occlusion masks from one plan (loop batch 2);",
             "two = b1_sync step (i1, i2) then b1_sync step (i2, i1) on the cold plan: the comparison;",
             "two1 = extra arm outside the protocol (one H2D, both forwards, one sync), not part of the verdict;",
             "arm' = the same arm on a second engine (another capture of the same plans): the spread of this protocol.",
             "ms per step: mean over the arm's blocks (per-block means in brackets)", ""]
    for name, factory in (("raft_large", raft_large), ("raft_small", raft_small)):
        model = factory(seed=0)[0].to(dev).eval()
        eng, twin = RaftEngine(model, dev), RaftEngine(model, dev)
        order = [(arm + suffix, e, arm) for suffix, e in (("", eng), ("'", twin)) for arm in ("bidir", "two", "two1")]
        for iters in (12, 32):
            for _ in range(2):   # every plan built, graphs captured, steady clocks
                for _, e, arm in order:
                    block(e, pairs, dev, iters, arm, 0.1)
            arms = {k: [] for k, _, _ in order}
            for _ in range(args.rounds):
                for k, e, arm in order:
                    arms[k].append(block(e, pairs, dev, iters, arm, args.block_s))
            mean = {k: sum(map(sum, v)) / sum(map(len, v)) for k, v in arms.items()}
            per = {k: ", ".join(f"{sum(b) / len(b):.3f}" for b in v) for k, v in arms.items()}
            bidir = (mean["bidir"] + mean["bidir'"]) / 2
            two, two1 = (mean["two"] + mean["two'"]) / 2, (mean["two1"] + mean["two1'"]) / 2
            worst, best = max(mean["bidir"], mean["bidir'"]), min(mean["two"], mean["two'"])
            best1 = min(mean["two1"], mean["two1'"])
            spread = max(abs(mean[k + "'"] - mean[k]) for k in ("bidir", "two"))
            lines.append(f"{name:10s} {iters:2d} it  " + "  ".join(f"{k} {mean[k]:6.3f} ms [{per[k]}]" for k in arms))
            lines.append(f"{'':10s}        mean of both captures: bidir {bidir:6.3f}  two {two:6.3f}  two1 {two1:6.3f} ms"
                         f"   gain two - bidir {two - bidir:+6.3f} ms ({100 * (two - bidir) / two:+5.1f} %)"
                         f"   capture spread {spread:5.3f} ms"
                         f"   slowest bidir capture {worst:6.3f} vs fastest two capture {best:6.3f} ms"
                         f"   bidir not slower than two: "
                         + ("yes, every capture" if worst <= best else "within the capture spread"
                            if bidir <= two + spread else "NO")
                         + f"   (extra: two1 - bidir {two1 - bidir:+6.3f} ms, fastest two1 capture "
                           f"{best1:6.3f} ms)")
            print(lines[-2], flush=True)
            print(lines[-1], flush=True)
        eng.release()
        twin.release()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
