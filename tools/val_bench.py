#!/usr/bin/env python3
"""What validating during training costs, in one fresh process on one GPU, on generated trees:
24 Sintel-sized pairs (436 x 1024 PNG frames + ``.flo``) and a KITTI tree with two frame sizes
(375 x 1242 and 370 x 1226, PNG frames + KITTI flow PNG).

(a) wall time of one pass over the Sintel tree: the stand-alone ``validate_sintel(batch_size=b)``
    against the streaming ``evaluate(batch=b)``, b = 1 and 4; and of ``validate_kitti`` against
    ``evaluate("kitti")``.  Both arms run once untimed (plan builds, tuning), then alternate for
    ``--rounds`` rounds; every pass ends in a device synchronise (both read their result back).
(b) GPU time of the ``flow_metrics`` kernels alone (both launches), from device events over
    ``--reps`` repetitions on preallocated buffers: (4, 436, 1024) dense and (1, 375, 1242) with
    a valid plane.
(c) the pause one validation of the Sintel tree causes in a raft_large training loop
    (``Trainer.validate`` between two blocks of steps on ``SyntheticFlow``; the first
    validation, which builds the inference plans, apart from the later ones).

  python tools/val_bench.py [--out profiles/val_overhead.txt]
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jax_raft_amd import raft_large, raft_small  # noqa: E402
from jax_raft_amd.eval.kitti import validate_kitti  # noqa: E402
from jax_raft_amd.eval.sintel import validate_sintel  # noqa: E402
from jax_raft_amd.eval.validate import evaluate  # noqa: E402
from jax_raft_amd.ops import native as nat  # noqa: E402
from jax_raft_amd.train.datasets import decode_threads  # noqa: E402
from jax_raft_amd.train.trainer import TrainConfig, Trainer  # noqa: E402
from jax_raft_amd.utils.flow_io import write_flo, write_flow_png  # noqa: E402

SINTEL, KITTI_SIZES = (436, 1024), [(375, 1242), (370, 1226)]


def _scene(rng, Hs, Ws):
    """A blocky frame, its shifted successor and the (affine) flow between them."""
    ys, xs = np.mgrid[0:Hs, 0:Ws].astype(np.float32)
    base = rng.integers(0, 256, (Hs // 8 + 1, Ws // 8 + 1, 3), dtype=np.uint8)
    img = np.kron(base, np.ones((8, 8, 1), np.uint8))[:Hs, :Ws]
    a, b = rng.uniform(-4, 4, 2)
    flow = np.stack([a + 0.01 * (xs - Ws / 2), b + 0.01 * (ys - Hs / 2)], -1).astype(np.float32)
    return img, np.roll(img, (int(round(b)), int(round(a))), (0, 1)), flow


def write_trees(root, pairs, kitti_pairs, seed=0):
    from PIL import Image

    rng = np.random.default_rng(seed)
    sintel, kitti = os.path.join(root, "Sintel"), os.path.join(root, "KITTI")
    for d in ("clean", "flow"):
        os.makedirs(os.path.join(sintel, "training", d, "alley_1"))
    for k in range(pairs + 1):                       # one scene: pairs + 1 frames
        img, _, flow = _scene(rng, *SINTEL)
        Image.fromarray(img).save(os.path.join(sintel, "training", "clean", "alley_1", f"frame_{k + 1:04d}.png"))
        if k < pairs:
            write_flo(os.path.join(sintel, "training", "flow", "alley_1", f"frame_{k + 1:04d}.flo"), flow)
    for d in ("image_2", "flow_occ"):
        os.makedirs(os.path.join(kitti, "training", d))
    for k in range(kitti_pairs):
        Hs, Ws = KITTI_SIZES[k % 2]
        img, nxt, flow = _scene(rng, Hs, Ws)
        Image.fromarray(img).save(os.path.join(kitti, "training", "image_2", f"{k:06d}_10.png"))
        Image.fromarray(nxt).save(os.path.join(kitti, "training", "image_2", f"{k:06d}_11.png"))
        write_flow_png(os.path.join(kitti, "training", "flow_occ", f"{k:06d}_10.png"), flow, rng.random((Hs, Ws)) < 0.5,
                       np.arange(Hs) % 5)
    return sintel, kitti


def alternate(arms, rounds, dev):
    """``arms``: name -> callable of one pass.  One untimed pass each, then ``rounds`` alternated
    rounds -> seconds per pass of each arm."""
    for f in arms.values():
        f()
    torch.cuda.synchronize(dev)
    out = {k: [] for k in arms}
    for _ in range(rounds):
        for name, f in arms.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            out[name].append(time.perf_counter() - t0)
    return out


def kernel_time(dev, B, H, W, with_valid, reps):
    g = torch.Generator().manual_seed(0)
    pred, gt = torch.randn(B, H, W, 2, generator=g).to(dev) * 3, torch.randn(B, H, W, 2, generator=g).to(dev) * 3
    valid = (torch.rand(B, H, W, generator=g) < 0.5).to(torch.uint8).to(dev) if with_valid else None
    nb = nat.flow_metrics_blocks(H, W)
    sizes = torch.tensor([(H, W)] * B, dtype=torch.int32, device=dev)
    part = torch.empty(B * nb * 2, dtype=torch.float64, device=dev)
    rows, acc = torch.empty(B, 6, dtype=torch.float64, device=dev), torch.zeros(8, dtype=torch.float64, device=dev)
    run = lambda: nat.ops().flow_metrics([pred, gt, valid, sizes, part, rows, acc], [B, H, W, H, W, nb])
    for _ in range(20):
        run()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize(dev)
    us = 1000 * e0.elapsed_time(e1) / reps
    nbytes = B * H * W * (16 + (1 if with_valid else 0))
    return us, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/val_overhead.txt")
    ap.add_argument("--pairs", type=int, default=24)
    ap.add_argument("--kitti-pairs", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--arch", default="raft_large")
    ap.add_argument("--train-block", type=int, default=10, help="training steps before and after each validation")
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "val_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    mean = lambda v: sum(v) / len(v)
    fmt = lambda v: f"{mean(v):7.3f} s mean, {min(v):7.3f} best  [" + ", ".join(f"{x:.3f}" for x in v) + "]"
    lines = [f"validation during training: what it costs, {torch.cuda.get_device_name(dev)}",
             f"generated trees: {args.pairs} Sintel pairs {SINTEL[0]}x{SINTEL[1]} (PNG + .flo), {args.kitti_pairs} KITTI pairs "
             f"{' / '.join(f'{h}x{w}' for h, w in KITTI_SIZES)} (PNG + flow PNG); decode threads: {decode_threads()}", ""]
    factory = raft_large if args.arch == "raft_large" else raft_small
    model = factory(seed=0)[0].to(dev).eval()
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        sintel, kitti = write_trees(root, args.pairs, args.kitti_pairs)
        lines.append(f"(trees written in {time.perf_counter() - t0:.1f} s)")
        lines += ["", f"(a) one pass, {args.arch}, the protocol's iterations (Sintel 32, KITTI 24); one untimed pass of every arm, "
                  f"then {args.rounds} alternated rounds; wall time with a device synchronise at both ends"]
        for b in (1, 4):
            arms = {f"validate_sintel(batch_size={b})": lambda b=b: validate_sintel(model, sintel, dstypes=("clean",), verbose=False, batch_size=b),
                    f"evaluate(batch={b})": lambda b=b: evaluate(model, "sintel-clean", sintel, batch=b)}
            res = alternate(arms, args.rounds, dev)
            for name, v in res.items():
                lines.append(f"    {name:32s} {fmt(v)}   {args.pairs / mean(v):6.1f} pairs/s")
            a, e = (mean(v) for v in res.values())
            lines.append(f"    evaluate / validate_sintel at batch {b}: {e / a:.2f} x the time")
            print("\n".join(lines[-3:]), flush=True)
        arms = {"validate_kitti": lambda: validate_kitti(model, kitti, verbose=False),
                "evaluate('kitti')": lambda: evaluate(model, "kitti", kitti)}
        res = alternate(arms, args.rounds, dev)
        for name, v in res.items():
            lines.append(f"    {name:32s} {fmt(v)}   {args.kitti_pairs / mean(v):6.1f} pairs/s")
        a, e = (mean(v) for v in res.values())
        lines.append(f"    evaluate / validate_kitti: {e / a:.2f} x the time")
        del model
        torch.cuda.empty_cache()

        lines += ["", f"(b) flow_metrics kernels alone (partials + finish), device events over {args.reps} repetitions:"]
        for B, H, W, v in ((4, *SINTEL, False), (1, *KITTI_SIZES[0], True)):
            us, nbytes = kernel_time(dev, B, H, W, v, args.reps)
            lines.append(f"    ({B}, {H}, {W}) {'with a valid plane' if v else 'dense':18s} {us:7.1f} us   "
                         f"({nbytes / 1e6:.1f} MB read: {nbytes / us / 1e3:.0f} GB/s)")

        if not args.skip_train:
            blk = args.train_block
            cfg = TrainConfig(arch=args.arch, steps=10 ** 6, batch=6, iters=12, log_every=10 ** 9,
                              val=(f"sintel-clean={sintel}",))
            tr = Trainer(cfg)

            def block():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(blk):
                    tr.train_step(tr.batch_for(tr.step))
                tr.flush()
                torch.cuda.synchronize(dev)
                return (time.perf_counter() - t0) / blk

            block()                                      # warm-up: plans, tuning
            steps, pauses = [block()], []
            for _ in range(3):
                pauses.append(tr.validate(log=lambda line: None))
                steps.append(block())
            lines += ["", f"(c) the pause of one validation ({args.pairs} Sintel pairs, batch {cfg.val_batch}, 32 iterations) in a "
                      f"{args.arch} training loop (SyntheticFlow 384x512, batch 6, 12 iterations), blocks of {blk} steps between:",
                      f"    step time per block: " + ", ".join(f"{1000 * s:.1f}" for s in steps) + " ms",
                      f"    first validation (builds the trainer's inference engine and plans; tile configs already decided in (a)): "
                      f"{pauses[0]:.3f} s",
                      f"    later validations: " + ", ".join(f"{p:.3f}" for p in pauses[1:]) + f" s  = "
                      f"{mean(pauses[1:]) / mean(steps[1:]):.1f} training steps each",
                      f"    EPE of the (untrained) model, last validation: {tr.val_history[-1]['sintel-clean']['epe']:.3f}"]
    lines += ["", "Not measured: accuracy.  The frames are generated and the weights random, so the EPE above says nothing about a",
              "trained model; on real data the trainer prints that figure by itself.", ""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
