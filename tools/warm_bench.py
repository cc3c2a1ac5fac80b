#!/usr/bin/env python3
"""Overhead of a warm start at EQUAL iteration counts: cold ``forward`` vs
``forward(flow_init="previous")`` (seed kernel in place of ``init_coords`` + the
two forward-projection launches before the replay), raft_large and raft_small,
batch 1, 440 x 1024, 12 and 32 iterations.

Protocol: ``b1_sync`` of bench.py (per pair: H2D from pageable host memory +
forward with all iterations upsampled + synchronise; no cross-pair overlap).
The arms alternate in one process, A/B/A/B, ~0.5 s of steady steps per block
after a warm-up of every plan; the figure is the mean latency of each arm and
their difference.  The arms "twin" and "warm2" are the SAME cold and warm forwards
on a second engine (its own plans, its own captured graphs): two captures of one
plan do not replay equally fast (the replayed branches are placed per capture), so
twin - cold and warm2 - warm are the floor below which warm - cold says nothing
about the seed.
What a warm start is FOR -- fewer iterations at equal accuracy
-- cannot be measured here (random-init weights, no data), so this measures only
what the seeding and the projection cost.

  python tools/warm_bench.py [--out profiles/warm_start_overhead.txt] [--block-s 0.5] [--rounds 2]
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


def block(eng, pairs, dev, iters, warm, seconds):
    """Steady steps of one arm for ~``seconds``: the latencies in ms."""
    lat, i, t_end = [], 0, time.perf_counter() + seconds
    kw = dict(flow_init="previous") if warm else {}
    while time.perf_counter() < t_end or len(lat) < 8:
        a, b = pairs[i % len(pairs)]
        t0 = time.perf_counter()
        flow = eng.forward(a.to(dev), b.to(dev), iters, **kw)[-1]
        torch.cuda.synchronize(dev)
        lat.append(1000 * (time.perf_counter() - t0))
        i += 1
    assert flow.shape == (1, H, W, 2)
    return lat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/warm_start_overhead.txt")
    ap.add_argument("--block-s", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=2, help="A/B rounds per configuration")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "warm_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(99)
    pairs = [(torch.rand(1, H, W, 3, generator=g) * 2 - 1, torch.rand(1, H, W, 3, generator=g) * 2 - 1)
             for _ in range(4)]
    lines = [f"warm-start overhead at equal iterations, {torch.cuda.get_device_name(dev)}",
             f"batch 1, {H}x{W}, b1_sync protocol (H2D pageable + forward, all iterations upsampled + sync),",
             f"arms alternated cold/warm/twin/warm2 x {args.rounds} in one process, ~{args.block_s} s per block;",
             "warm = forward(flow_init='previous'): seed kernel + 2 projection launches per call;",
             "twin / warm2 = the cold / warm forward on a second engine (another capture of the same plan): the noise floor.",
             "ms per call: mean over the arm's blocks (per-block means in brackets)", ""]
    for name, factory in (("raft_large", raft_large), ("raft_small", raft_small)):
        model = factory(seed=0)[0].to(dev).eval()
        eng, twin = RaftEngine(model, dev), RaftEngine(model, dev)
        order = (("cold", eng, False), ("warm", eng, True), ("twin", twin, False), ("warm2", twin, True))
        for iters in (12, 32):
            for _ in range(2):   # every plan built, graphs captured, steady clocks
                for _, e, warm in order:
                    block(e, pairs, dev, iters, warm, 0.1)
            arms = {k: [] for k, _, _ in order}
            for _ in range(args.rounds):
                for k, e, warm in order:
                    arms[k].append(block(e, pairs, dev, iters, warm, args.block_s))
            mean = {k: sum(map(sum, v)) / sum(map(len, v)) for k, v in arms.items()}
            per = {k: ", ".join(f"{sum(b) / len(b):.3f}" for b in v) for k, v in arms.items()}
            lines.append(f"{name:10s} {iters:2d} it  " + "  ".join(f"{k} {mean[k]:6.3f} ms [{per[k]}]" for k in arms)
                         + f"   warm - cold {1000 * (mean['warm'] - mean['cold']):+7.1f} us"
                         + f"   twin - cold {1000 * (mean['twin'] - mean['cold']):+7.1f} us"
                         + f"   warm2 - warm {1000 * (mean['warm2'] - mean['warm']):+7.1f} us")
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
