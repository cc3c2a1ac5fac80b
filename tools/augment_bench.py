#!/usr/bin/env python3
"""What training on real data costs next to training on ``SyntheticFlow``, at the ``chairs``
sizes (source 384 x 512, crop 368 x 496, batch 6), in one fresh process on one GPU:

(a) the GPU time of the two augmentation launches (colour sums incl. its memset, the gather)
    per batch, from device events over ``--reps`` repetitions each, on sampled ``chairs``
    records (buffers preallocated, records already on the device);
(b) the step rate of the training loop (``Trainer.batch_for`` + ``train_step``, raft_large,
    12 iterations) on a throw-away PPM / ``.flo`` dataset of random frames that the tool writes
    into a temporary directory, against the same loop on ``SyntheticFlow`` at the crop size.
    Two trainers in one process, blocks of ``--block`` steps alternated real / synth for
    ``--rounds`` rounds after a warm-up of both; every block ends in a device synchronise.
    Next to it: the host time one batch takes to decode when nothing overlaps it, and the
    host time ``batch_for`` holds the loop per step (decode not hidden by the prefetch,
    upload, record sampling, launches).

PNG decoding (Sintel) is not covered: the generated dataset is PPM.

  python tools/augment_bench.py [--out profiles/augment_overhead.txt]
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jax_raft_amd.ops import native as nat  # noqa: E402
from jax_raft_amd.train import AugmentParams, FlowPairs, PairLoader  # noqa: E402
from jax_raft_amd.train.trainer import TrainConfig, Trainer  # noqa: E402
from jax_raft_amd.utils.flow_io import write_flo  # noqa: E402

SRC, CROP, BATCH = (384, 512), (368, 496), 6


def write_dataset(root, n, seed=0):
    from PIL import Image

    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:SRC[0], 0:SRC[1]].astype(np.float32)
    for k in range(n):
        base = rng.integers(0, 256, (SRC[0] // 8 + 1, SRC[1] // 8 + 1, 3), dtype=np.uint8)
        img = np.kron(base, np.ones((8, 8, 1), np.uint8))[:SRC[0], :SRC[1]]        # blocky texture
        a, b = rng.uniform(-4, 4, 2)
        flow = np.stack([a + 0.01 * (xs - SRC[1] / 2), b + 0.01 * (ys - SRC[0] / 2)], -1).astype(np.float32)
        stem = os.path.join(root, f"{k + 1:05d}")
        Image.fromarray(img).save(stem + "_img1.ppm")
        Image.fromarray(np.roll(img, (int(round(b)), int(round(a))), (0, 1))).save(stem + "_img2.ppm")
        write_flo(stem + "_flow.flo", flow)


def kernel_times(dev, reps):
    g = torch.Generator().manual_seed(0)
    i1 = torch.randint(0, 256, (BATCH, *SRC, 3), generator=g, dtype=torch.uint8).to(dev)
    i2 = torch.randint(0, 256, (BATCH, *SRC, 3), generator=g, dtype=torch.uint8).to(dev)
    flow = torch.randn(BATCH, *SRC, 2, generator=g).to(dev)
    recs = [AugmentParams.sample(BATCH, SRC, "chairs", step=s).packed().to(dev) for s in range(8)]
    sums = torch.empty(2, BATCH, 3, dtype=torch.int32, device=dev)
    o1, o2 = (torch.empty(BATCH, *CROP, 3, device=dev) for _ in range(2))
    of, ov = torch.empty(BATCH, *CROP, 2, device=dev), torch.empty(BATCH, *CROP, device=dev)
    run_sums = lambda k: nat.ops().augment_sums([i1, i2, sums], [BATCH, *SRC])
    run_gather = lambda k: nat.ops().augment([i1, i2, flow, recs[k % 8], sums, o1, o2, of, ov], [BATCH, *SRC, *CROP])
    out = {}
    for name, fns in (("sums", (run_sums,)), ("gather", (run_gather,)), ("both", (run_sums, run_gather))):
        for k in range(10):
            for f in fns:
                f(k)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(reps):
            for f in fns:
                f(k)
        e1.record()
        torch.cuda.synchronize(dev)
        out[name] = 1000 * e0.elapsed_time(e1) / reps          # us per batch
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/augment_overhead.txt")
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--pairs", type=int, default=48, help="pairs in the generated dataset")
    ap.add_argument("--block", type=int, default=20, help="steps per block")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--arch", default="raft_large")
    ap.add_argument("--iters", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    lines = [f"training on real data vs SyntheticFlow, {torch.cuda.get_device_name(dev)}",
             f"chairs sizes: source {SRC[0]}x{SRC[1]}, crop {CROP[0]}x{CROP[1]}, batch {BATCH}", ""]
    kt = kernel_times(dev, args.reps)
    lines += [f"(a) GPU time per batch, device events over {args.reps} repetitions (sampled chairs records):",
              f"    colour sums (memset + kernel) {kt['sums']:8.1f} us",
              f"    gather                        {kt['gather']:8.1f} us",
              f"    both, back to back            {kt['both']:8.1f} us", ""]
    print("\n".join(lines), flush=True)

    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_dataset(root, args.pairs)
        t_write = time.perf_counter() - t0
        total = args.warmup + args.block * args.rounds
        kw = dict(arch=args.arch, steps=total, batch=BATCH, iters=args.iters, size=CROP, log_every=10 ** 9)
        arms = {"real": Trainer(TrainConfig(data=root, **kw)), "synth": Trainer(TrainConfig(**kw))}
        ld = PairLoader(FlowPairs.chairs(root), BATCH)          # a CPU loader: decode alone, nothing overlapping
        dec = []
        for s in range(5):
            t0 = time.perf_counter()
            ld.host_batch(s)
            dec.append(1000 * (time.perf_counter() - t0))
        ld.close()
        for name, tr in arms.items():
            t0 = time.perf_counter()
            for _ in range(args.warmup):
                tr.train_step(tr.batch_for(tr.step))
            tr.flush()
            torch.cuda.synchronize(dev)
            print(f"warm-up of {name}: {time.perf_counter() - t0:.1f} s", flush=True)
        torch.cuda.synchronize(dev)
        rate = {k: [] for k in arms}
        held = {k: [] for k in arms}
        for _ in range(args.rounds):
            for name, tr in arms.items():
                h = 0.0
                t0 = time.perf_counter()
                for _ in range(args.block):
                    h0 = time.perf_counter()
                    batch = tr.batch_for(tr.step)
                    h += time.perf_counter() - h0
                    m = tr.train_step(batch)
                tr.flush()
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                rate[name].append(BATCH * args.block / dt)
                held[name].append(1000 * h / args.block)
                assert torch.isfinite(m["loss"]).item(), name
        arms["real"].loader.close()
    mean = lambda v: sum(v) / len(v)
    r, s = mean(rate["real"]), mean(rate["synth"])
    ms = lambda x: 1000 * BATCH / x
    spread = max(max(v) - min(v) for v in rate.values())
    lines += [f"(b) training loop, {args.arch}, {args.iters} iterations, {args.block} steps per block, blocks alternated "
              f"real / synth x {args.rounds} in one process after {args.warmup} warm-up steps each",
              f"    ({args.pairs} generated PPM / .flo pairs, written in {t_write:.1f} s; decode threads: "
              f"{__import__('jax_raft_amd.train.datasets', fromlist=['x']).decode_threads()})"]
    for k in arms:
        lines.append(f"    {k:5s} {mean(rate[k]):7.1f} pairs/s  {ms(mean(rate[k])):6.2f} ms/step  [per block: "
                     + ", ".join(f"{v:.1f}" for v in rate[k]) + f"]   batch_for holds the loop {mean(held[k]):5.2f} ms/step")
    lines += [f"    real - synth: {ms(r) - ms(s):+.2f} ms/step ({100 * (r - s) / s:+.1f} % pairs/s); "
              f"largest spread between blocks of one arm {spread:.1f} pairs/s",
              f"    one batch decoded alone (PPM + .flo read into staging buffers, no overlap): "
              f"{min(dec):.2f} ms best, {mean(dec[1:]):.2f} ms mean of {len(dec) - 1}",
              f"    the two launches of (a) are {kt['both'] / 1000:.3f} ms of a real step",
              "    PNG decoding (Sintel) is not covered: the generated dataset is PPM.", ""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
