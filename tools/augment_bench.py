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

``--sparse``: the same for sparse ground truth at the KITTI sizes (sources 375 x 1242 and
370 x 1226 mixed in one batch, crop 288 x 960, batch 6): the two launches of
``augment.hip``'s sparse layout on sampled ``kitti`` records, the training loop on a generated KITTI tree
(PNG frames, flow written by ``write_flow_png`` with the five filter types cycling over the rows)
against ``SyntheticFlow`` at the crop size, and the host time of one flow-PNG decode with the
C++ un-filter and with the numpy fallback.

``--mixed``: RAFT's Sintel-stage mixture on a generated tree with all five parts at their real frame
sizes (Sintel 436 x 1024, FlyingThings3D 540 x 960, KITTI, HD1K 1080 x 2560; crop 368 x 768, batch 6):
the two launches of ``augment.hip``'s mixed layout on sampled ``sintel`` records, the bytes and stream time of the
prefix uploads and the decode time of a batch with and without an HD1K sample, and the training loop
with RAFT's weights (``mix``) and with HD1K weighted up so that most batches hold one (``mix+``) against
``SyntheticFlow`` at the crop size.

  python tools/augment_bench.py [--out profiles/augment_overhead.txt]
  python tools/augment_bench.py --sparse [--out profiles/sparse_augment_overhead.txt]
  python tools/augment_bench.py --mixed [--out profiles/mixed_augment_overhead.txt]
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
from jax_raft_amd.train import AugmentParams, FlowPairs, PairLoader, sample_sparse  # noqa: E402
from jax_raft_amd.train.trainer import TrainConfig, Trainer  # noqa: E402
from jax_raft_amd.utils.flow_io import read_flow_png, write_flo, write_flow_png  # noqa: E402

SRC, CROP, BATCH = (384, 512), (368, 496), 6
KITTI_SIZES, KITTI_CROP = [(375, 1242), (370, 1226)], (288, 960)


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


def timed(fns_by_name, dev, reps):
    """us per batch of each named sequence of launches, from device events over ``reps`` repetitions."""
    out = {}
    for name, fns in fns_by_name:
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
        out[name] = 1000 * e0.elapsed_time(e1) / reps
    return out


def alternate(arms, args, dev):
    """Warm both trainers up, then blocks of ``args.block`` steps alternated between them for
    ``args.rounds`` rounds: pairs/s per block and the ms per step ``batch_for`` holds the loop."""
    for name, tr in arms.items():
        t0 = time.perf_counter()
        for _ in range(args.warmup):
            tr.train_step(tr.batch_for(tr.step))
        tr.flush()
        torch.cuda.synchronize(dev)
        print(f"warm-up of {name}: {time.perf_counter() - t0:.1f} s", flush=True)
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
    return rate, held


def write_kitti_dataset(root, n, seed=0):
    """A KITTI-2015 training tree of n pairs, the two sizes alternating; half of the flow is valid."""
    from PIL import Image

    rng = np.random.default_rng(seed)
    for d in ("image_2", "flow_occ"):
        os.makedirs(os.path.join(root, "training", d))
    for k in range(n):
        Hs, Ws = KITTI_SIZES[k % 2]
        ys, xs = np.mgrid[0:Hs, 0:Ws].astype(np.float32)
        base = rng.integers(0, 256, (Hs // 8 + 1, Ws // 8 + 1, 3), dtype=np.uint8)
        img = np.kron(base, np.ones((8, 8, 1), np.uint8))[:Hs, :Ws]                # blocky texture
        a, b = rng.uniform(-4, 4, 2)
        flow = np.stack([a + 0.01 * (xs - Ws / 2), b + 0.01 * (ys - Hs / 2)], -1).astype(np.float32)
        valid = rng.random((Hs, Ws)) < 0.5
        Image.fromarray(img).save(os.path.join(root, "training", "image_2", f"{k:06d}_10.png"))
        Image.fromarray(np.roll(img, (int(round(b)), int(round(a))), (0, 1))).save(
            os.path.join(root, "training", "image_2", f"{k:06d}_11.png"))
        write_flow_png(os.path.join(root, "training", "flow_occ", f"{k:06d}_10.png"), flow, valid, np.arange(Hs) % 5)


def sparse_kernel_times(dev, reps):
    g = torch.Generator().manual_seed(0)
    sizes = [KITTI_SIZES[n % 2] for n in range(BATCH)]
    Hb, Wb = KITTI_SIZES[0]
    i1 = torch.randint(0, 256, (BATCH, Hb, Wb, 3), generator=g, dtype=torch.uint8).to(dev)
    i2 = torch.randint(0, 256, (BATCH, Hb, Wb, 3), generator=g, dtype=torch.uint8).to(dev)
    flow = torch.randn(BATCH, Hb, Wb, 2, generator=g).to(dev)
    valid = (torch.rand(BATCH, Hb, Wb, generator=g) < 0.5).to(torch.uint8).to(dev)
    recs = [sample_sparse(BATCH, sizes, "kitti", step=s).packed().to(dev) for s in range(8)]
    sums = torch.empty(2, BATCH, 3, dtype=torch.int32, device=dev)
    o1, o2 = (torch.empty(BATCH, *KITTI_CROP, 3, device=dev) for _ in range(2))
    of, ov = torch.empty(BATCH, *KITTI_CROP, 2, device=dev), torch.empty(BATCH, *KITTI_CROP, device=dev)
    run_sums = lambda k: nat.ops().augment_sparse_sums([i1, i2, recs[k % 8], sums], [BATCH, Hb, Wb])
    run_gather = lambda k: nat.ops().augment_sparse([i1, i2, flow, valid, recs[k % 8], sums, o1, o2, of, ov],
                                                    [BATCH, Hb, Wb, *KITTI_CROP])
    out = timed((("sums", (run_sums,)), ("gather", (run_gather,)), ("both", (run_sums, run_gather))), dev, reps)
    # the upload of one batch as PairLoader.fetch does it: pinned staging buffers -> fresh device tensors, in-stream
    pinned = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (i1, i2, flow, valid)]
    upload = lambda k: [torch.empty(b.shape, dtype=b.dtype, device=dev).copy_(b, non_blocking=True) for b in pinned]
    out["upload"] = timed((("upload", (upload,)),), dev, 50)["upload"]
    out["upload_mb"] = sum(b.numel() * b.element_size() for b in pinned) / 1e6
    return out


def sparse_main(args, dev):
    lines = [f"training on sparse ground truth vs SyntheticFlow, {torch.cuda.get_device_name(dev)}",
             f"KITTI sizes: sources {' and '.join(f'{h}x{w}' for h, w in KITTI_SIZES)} mixed, crop "
             f"{KITTI_CROP[0]}x{KITTI_CROP[1]}, batch {BATCH}", ""]
    kt = sparse_kernel_times(dev, args.reps)
    lines += [f"(a) GPU time per batch, device events over {args.reps} repetitions (sampled kitti records):",
              f"    sized colour sums (memset + kernel) {kt['sums']:8.1f} us",
              f"    gather (images + flow scan)         {kt['gather']:8.1f} us",
              f"    both, back to back                  {kt['both']:8.1f} us",
              f"    upload of one batch, {kt['upload_mb']:.1f} MB pinned -> device in the stream (images, fp32 flow, valid): "
              f"{kt['upload']:8.1f} us", ""]
    print("\n".join(lines), flush=True)
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_kitti_dataset(root, args.pairs)
        t_write = time.perf_counter() - t0
        one = os.path.join(root, "training", "flow_occ", "000000_10.png")
        dec_c = []
        for _ in range(5):
            t0 = time.perf_counter()
            read_flow_png(one, native=True)
            dec_c.append(1000 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        read_flow_png(one, native=False)
        dec_np = 1000 * (time.perf_counter() - t0)
        total = args.warmup + args.block * args.rounds
        kw = dict(arch=args.arch, steps=total, batch=BATCH, iters=args.iters, size=KITTI_CROP, log_every=10 ** 9)
        arms = {"real": Trainer(TrainConfig(data=root, dataset="kitti", stage="kitti", **kw)), "synth": Trainer(TrainConfig(**kw))}
        ld = PairLoader(FlowPairs.kitti(root), BATCH)           # a CPU loader: decode alone, nothing overlapping
        dec = []
        for s in range(4):
            t0 = time.perf_counter()
            ld.host_batch(s)
            dec.append(1000 * (time.perf_counter() - t0))
        ld.close()
        rate, held = alternate(arms, args, dev)
        arms["real"].loader.close()
    mean = lambda v: sum(v) / len(v)
    r, s = mean(rate["real"]), mean(rate["synth"])
    ms = lambda x: 1000 * BATCH / x
    spread = max(max(v) - min(v) for v in rate.values())
    threads = __import__("jax_raft_amd.train.datasets", fromlist=["x"]).decode_threads()
    lines += [f"(b) training loop, {args.arch}, {args.iters} iterations, {args.block} steps per block, blocks alternated "
              f"real / synth x {args.rounds} in one process after {args.warmup} warm-up steps each",
              f"    ({args.pairs} generated pairs, PNG frames + KITTI flow PNG, written in {t_write:.1f} s; decode threads: {threads})"]
    for k in arms:
        lines.append(f"    {k:5s} {mean(rate[k]):7.1f} pairs/s  {ms(mean(rate[k])):6.2f} ms/step  [per block: "
                     + ", ".join(f"{v:.1f}" for v in rate[k]) + f"]   batch_for holds the loop {mean(held[k]):5.2f} ms/step")
    lines += [f"    real - synth: {ms(r) - ms(s):+.2f} ms/step ({100 * (r - s) / s:+.1f} % pairs/s); "
              f"largest spread between blocks of one arm {spread:.1f} pairs/s",
              f"    one batch decoded alone (2 PNG frames + 1 flow PNG per sample into staging buffers, no overlap): "
              f"{min(dec):.2f} ms best, {mean(dec[1:]):.2f} ms mean of {len(dec) - 1}",
              f"    the two launches of (a) are {kt['both'] / 1000:.3f} ms and the upload {kt['upload'] / 1000:.3f} ms of a real step", "",
              f"(c) host time of one flow-PNG decode ({KITTI_SIZES[0][0]}x{KITTI_SIZES[0][1]}, 16-bit RGB, filter types 0..4 "
              "cycling over the rows), read + inflate + un-filter + decode:",
              f"    C++ un-filter (csrc/runtime/png.cpp) {min(dec_c):8.2f} ms best of {len(dec_c)}, {mean(dec_c[1:]):.2f} ms mean",
              f"    numpy fallback                       {dec_np:8.2f} ms (one run)", ""]
    return "\n".join(lines) + "\n"


# ------------------------------------------------ dense and sparse samples in one batch (--mixed)
MIX_CROP = (368, 768)
MIX_SIZES = dict(sintel=(436, 1024), things=(540, 960), kitti=KITTI_SIZES, hd1k=(1080, 2560))


def _scene(rng, Hs, Ws):
    """A blocky frame, its shifted successor and the (affine) flow between them."""
    ys, xs = np.mgrid[0:Hs, 0:Ws].astype(np.float32)
    base = rng.integers(0, 256, (Hs // 8 + 1, Ws // 8 + 1, 3), dtype=np.uint8)
    img = np.kron(base, np.ones((8, 8, 1), np.uint8))[:Hs, :Ws]
    a, b = rng.uniform(-4, 4, 2)
    flow = np.stack([a + 0.01 * (xs - Ws / 2), b + 0.01 * (ys - Hs / 2)], -1).astype(np.float32)
    return img, np.roll(img, (int(round(b)), int(round(a))), (0, 1)), flow


def write_mixed_dataset(root, n, seed=0):
    """The five parts of RAFT's Sintel stage at their real frame sizes under ``root`` (Sintel, KITTI, HD1K,
    FlyingThings3D), ``n`` frames per sequence; a KITTI tree of ``n`` pairs."""
    from PIL import Image

    from jax_raft_amd.utils.flow_io import write_pfm

    rng = np.random.default_rng(seed)

    def save(img, *path):
        os.makedirs(os.path.join(root, *path[:-1]), exist_ok=True)
        Image.fromarray(img).save(os.path.join(root, *path))

    Hs, Ws = MIX_SIZES["sintel"]
    os.makedirs(os.path.join(root, "Sintel", "training", "flow", "alley_1"))
    for k in range(n):
        img, _, flow = _scene(rng, Hs, Ws)
        for p in ("clean", "final"):
            save(img, "Sintel", "training", p, "alley_1", f"frame_{k + 1:04d}.png")
        if k + 1 < n:
            write_flo(os.path.join(root, "Sintel", "training", "flow", "alley_1", f"frame_{k + 1:04d}.flo"), flow)
    write_kitti_dataset(os.path.join(root, "KITTI"), n, seed)
    Hs, Ws = MIX_SIZES["hd1k"]
    os.makedirs(os.path.join(root, "HD1K", "hd1k_flow_gt", "flow_occ"))
    for k in range(n):
        img, _, flow = _scene(rng, Hs, Ws)
        save(img, "HD1K", "hd1k_input", "image_2", f"000000_{k + 10:04d}.png")
        write_flow_png(os.path.join(root, "HD1K", "hd1k_flow_gt", "flow_occ", f"000000_{k + 10:04d}.png"), flow,
                       rng.random((Hs, Ws)) < 0.5, np.arange(Hs) % 5)
    Hs, Ws = MIX_SIZES["things"]
    for k in range(n):
        img, _, flow = _scene(rng, Hs, Ws)
        save(img, "FlyingThings3D", "frames_cleanpass", "TRAIN", "A", "0000", "left", f"{k + 6:04d}.png")
        for direction, tag in (("into_future", "IntoFuture"), ("into_past", "IntoPast")):
            d = os.path.join(root, "FlyingThings3D", "optical_flow", "TRAIN", "A", "0000", direction, "left")
            os.makedirs(d, exist_ok=True)
            write_pfm(os.path.join(d, f"OpticalFlow{tag}_{k + 6:04d}_L.pfm"), np.concatenate([flow, flow[..., :1] * 0], -1))


def mixed_kernel_times(dev, reps):
    """The two launches on a batch of every kind (Sintel, Things, KITTI x 2, HD1K, Sintel), and the prefix
    uploads of that batch and of the same batch with a KITTI sample in the HD1K sample's place."""
    from jax_raft_amd.train import sample_mixed

    g = torch.Generator().manual_seed(0)
    sizes = [MIX_SIZES["sintel"], MIX_SIZES["things"], *KITTI_SIZES, MIX_SIZES["hd1k"], MIX_SIZES["sintel"]]
    dense = [True, True, False, False, False, True]
    S = max(h * w for h, w in sizes)
    i1 = torch.randint(0, 256, (BATCH, S, 3), generator=g, dtype=torch.uint8).to(dev)
    i2 = torch.randint(0, 256, (BATCH, S, 3), generator=g, dtype=torch.uint8).to(dev)
    flow = torch.randn(BATCH, S, 2, generator=g).to(dev)
    valid = (torch.rand(BATCH, S, generator=g) < 0.5).to(torch.uint8).to(dev)
    recs = [sample_mixed(BATCH, sizes, dense, "sintel", step=s).packed().to(dev) for s in range(8)]
    sums = torch.empty(2, BATCH, 3, dtype=torch.int32, device=dev)
    o1, o2 = (torch.empty(BATCH, *MIX_CROP, 3, device=dev) for _ in range(2))
    of, ov = torch.empty(BATCH, *MIX_CROP, 2, device=dev), torch.empty(BATCH, *MIX_CROP, device=dev)
    run_sums = lambda k: nat.ops().augment_mixed_sums([i1, i2, recs[k % 8], sums], [BATCH, S])
    run_gather = lambda k: nat.ops().augment_mixed([i1, i2, flow, valid, recs[k % 8], sums, o1, o2, of, ov], [BATCH, S, *MIX_CROP])
    out = timed((("sums", (run_sums,)), ("gather", (run_gather,)), ("both", (run_sums, run_gather))), dev, reps)
    pinned = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in (i1, i2, flow, valid)]

    def uploader(sz):
        def upload(k):                              # as PairLoader.fetch does it: fresh device tensors, one copy per prefix
            dst = [torch.empty(b.shape, dtype=b.dtype, device=dev) for b in pinned]
            for n, ((h, w), d) in enumerate(zip(sz, dense)):
                for a, b in zip(dst[:3 if d else 4], pinned):
                    a[n, :h * w].copy_(b[n, :h * w], non_blocking=True)
        return upload

    nbytes = lambda sz: sum(h * w * (14 + (not d)) for (h, w), d in zip(sz, dense))
    no_hd1k = sizes[:4] + [KITTI_SIZES[0]] + sizes[5:]
    for name, sz in (("with", sizes), ("without", no_hd1k)):
        out["upload_" + name] = timed(((name, (uploader(sz),)),), dev, 50)[name]
        out["mb_" + name] = nbytes(sz) / 1e6
    out["mb_padded"] = BATCH * S * 15 / 1e6
    return out


def mixed_main(args, dev):
    from jax_raft_amd.train.datasets import decode_threads

    lines = [f"training on RAFT's Sintel-stage mixture vs SyntheticFlow, {torch.cuda.get_device_name(dev)}",
             "frame sizes: Sintel 436x1024, FlyingThings3D 540x960, KITTI 375x1242 and 370x1226, HD1K 1080x2560; packed slots of "
             f"1080*2560 pixels, crop {MIX_CROP[0]}x{MIX_CROP[1]}, batch {BATCH}", ""]
    kt = mixed_kernel_times(dev, args.reps)
    lines += [f"(a) GPU time per batch, device events over {args.reps} repetitions (sampled sintel records; the batch: Sintel, "
              "Things, KITTI x 2, HD1K, Sintel):",
              f"    packed colour sums (memset + kernel) {kt['sums']:8.1f} us",
              f"    gather (images + blend or scan)      {kt['gather']:8.1f} us",
              f"    both, back to back                   {kt['both']:8.1f} us",
              f"    prefix uploads of that batch, {kt['mb_with']:.1f} MB pinned -> device in the stream: {kt['upload_with']:8.1f} us",
              f"    the same with a KITTI sample in the HD1K sample's place, {kt['mb_without']:.1f} MB: {kt['upload_without']:8.1f} us",
              f"    (whole slots would be {kt['mb_padded']:.1f} MB per batch)", ""]
    print("\n".join(lines), flush=True)
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_mixed_dataset(root, args.pairs)
        t_write = time.perf_counter() - t0
        hd = os.path.join(root, "HD1K", "hd1k_flow_gt", "flow_occ", "000000_0010.png")
        ki = os.path.join(root, "KITTI", "training", "flow_occ", "000000_10.png")
        png = {}
        for name, path in (("hd1k", hd), ("kitti", ki)):
            t = []
            for _ in range(4):
                t0 = time.perf_counter()
                read_flow_png(path, native=True)
                t.append(1000 * (time.perf_counter() - t0))
            png[name] = min(t)
        # decode of one batch alone on a CPU loader, batches with and without an HD1K sample
        mix = FlowPairs.open(root, "mix")
        ld = PairLoader(mix, BATCH)
        dec = {True: [], False: []}
        for s in range(ld.steps_per_epoch):
            has = MIX_SIZES["hd1k"] in ld.sizes_for(s)
            if len(dec[has]) < 4:
                t0 = time.perf_counter()
                ld.host_batch(s)
                dec[has].append(1000 * (time.perf_counter() - t0))
        ld.close()
        total = args.warmup + args.block * args.rounds
        kw = dict(arch=args.arch, steps=total, batch=BATCH, iters=args.iters, size=MIX_CROP, log_every=10 ** 9)
        heavy = (100, 100, 200, 300, 1)             # HD1K drawn about as often as the other parts: most batches hold one
        arms = {"mix": Trainer(TrainConfig(data=root, dataset="mix", stage="sintel", **kw)),
                "mix+": Trainer(TrainConfig(data=root, dataset="mix", stage="sintel", mix_weights=heavy, **kw)),
                "synth": Trainer(TrainConfig(**kw))}
        share = {k: sum(MIX_SIZES["hd1k"] in arms[k].loader.sizes_for(s) for s in range(total)) / total for k in ("mix", "mix+")}
        rate, held = alternate(arms, args, dev)
        for k in ("mix", "mix+"):
            arms[k].loader.close()
    mean = lambda v: sum(v) / len(v) if v else float("nan")
    ms = lambda x: 1000 * BATCH / x
    s = mean(rate["synth"])
    lines += [f"(b) training loop, {args.arch}, {args.iters} iterations, {args.block} steps per block, blocks alternated mix / mix+ / "
              f"synth x {args.rounds} in one process after {args.warmup} warm-up steps each",
              f"    ({args.pairs} generated frames per sequence, written in {t_write:.1f} s; decode threads: {decode_threads()}; "
              f"mix: RAFT's weights 100, 100, 200, 5, 1, {100 * share['mix']:.0f} % of its batches hold an HD1K sample; "
              f"mix+: HD1K weighted 300, {100 * share['mix+']:.0f} % of its batches)"]
    for k in arms:
        lines.append(f"    {k:5s} {mean(rate[k]):7.1f} pairs/s  {ms(mean(rate[k])):6.2f} ms/step  [per block: "
                     + ", ".join(f"{v:.1f}" for v in rate[k]) + f"]   batch_for holds the loop {mean(held[k]):5.2f} ms/step")
    for k in ("mix", "mix+"):
        r = mean(rate[k])
        lines.append(f"    {k} - synth: {ms(r) - ms(s):+.2f} ms/step ({100 * (r - s) / s:+.1f} % pairs/s)")
    verdict = lambda d: "fits inside a step: the prefetch hides it" if d < ms(s) else "is longer than a step: NOT GPU-bound"
    lines += [f"    one batch decoded alone (no overlap): without an HD1K sample {mean(dec[False]):.1f} ms mean of {len(dec[False])}, "
              f"with at least one {mean(dec[True]):.1f} ms mean of {len(dec[True])}; a synth step is {ms(s):.1f} ms",
              f"    -> a batch without an HD1K sample {verdict(mean(dec[False]))}; a batch with one {verdict(mean(dec[True]))}",
              f"    one flow PNG decoded alone (C++ un-filter, best of 4): HD1K 1080x2560 {png['hd1k']:.1f} ms, KITTI 375x1242 "
              f"{png['kitti']:.1f} ms ({png['hd1k'] / png['kitti']:.1f} x)",
              f"    the two launches of (a) are {kt['both'] / 1000:.3f} ms and the uploads {kt['upload_with'] / 1000:.3f} ms of a step",
              "    (the mix+ arm shows the loop when nearly every batch holds HD1K samples; the share of such batches in the mix",
              "    arm is stated above and depends on the lists' real lengths, which a generated tree does not have)", "",
              "Not measured: accuracy.  There is no checkpoint and no real dataset here, the frames are generated, so no EPE of a",
              "model trained on this mixture can be given.", ""]
    return "\n".join(lines) + "\n"


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
    return timed((("sums", (run_sums,)), ("gather", (run_gather,)), ("both", (run_sums, run_gather))), dev, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sparse", action="store_true", help="sparse ground truth at the KITTI sizes")
    ap.add_argument("--mixed", action="store_true", help="RAFT's Sintel-stage mixture at the real frame sizes")
    ap.add_argument("--out", default=None, help="default: profiles/augment_overhead.txt, profiles/sparse_augment_overhead.txt "
                    "or profiles/mixed_augment_overhead.txt")
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--pairs", type=int, default=None, help="pairs in the generated dataset (default 48, sparse: 24; "
                    "mixed: frames per sequence, default 5)")
    ap.add_argument("--block", type=int, default=20, help="steps per block")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--arch", default="raft_large")
    ap.add_argument("--iters", type=int, default=12)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    if args.mixed:
        args.pairs = args.pairs or 5
        return finish(mixed_main(args, dev), args.out or "profiles/mixed_augment_overhead.txt")
    args.out = args.out or ("profiles/sparse_augment_overhead.txt" if args.sparse else "profiles/augment_overhead.txt")
    args.pairs = args.pairs or (24 if args.sparse else 48)
    if args.sparse:
        return finish(sparse_main(args, dev), args.out)
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
        rate, held = alternate(arms, args, dev)
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
    finish("\n".join(lines) + "\n", args.out)


def finish(text, out):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
