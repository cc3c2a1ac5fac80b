#!/usr/bin/env python3
"""What the label-free loss (train/unsup.py, csrc/kernels/unsup.hip) costs, in one fresh process
on one GPU, at the ``chairs`` shape (N, B, H, W) = (12, 6, 368, 496):

(a) the GPU time of the two launches (``unsup_loss``, ``unsup_loss_bwd``) from device events over
    ``--reps`` repetitions each, buffers preallocated, next to the bytes each must move at least
    (every operand read once, every result written once);
(b) the native forward + backward (``unsup_loss(...)[0].backward()``) against the golden op
    ``unsup_loss_reference`` run on the same GPU tensors under autograd, i.e. the PyTorch
    composition: the arms alternate in one process, each runs twice, ``--pair-reps`` repetitions
    per run.  The condition: native is faster by more than the larger difference between the two
    runs of either arm;
(c) the raft_large training step (384 x 512, batch 6, 12 iterations, ``SyntheticFlow``) with
    ``loss="unsup"`` against ``loss="sequence"``: two trainers in one process, blocks of
    ``--block`` steps alternated for ``--rounds`` rounds after a warm-up of both.  No target: the
    difference and the spread between blocks of one arm are reported.

``--photo census`` measures the census photometric term (csrc/kernels/census.hip) the same way: (a)
its three launches, (b) ``unsup_loss(..., photo="census")`` against the golden op with
``photo="census"``, (c) the training step with ``unsup_photo="census"`` against
``unsup_photo="charbonnier"``; the default output is then ``profiles/census_loss_overhead.txt``.

``--occlusion fb | range`` measures the occlusion masks of the training step instead (train/occlusion.py,
csrc/kernels/occlusion.hip; default output ``profiles/occlusion_overhead.txt``): (a) the two launches
``range_splat`` and ``range_visible`` (+ the clear) at 12 maps of 368 x 496 per direction, with the bytes
they move and the atomics they issue; (c) the training step in three arms, blocks alternated in one
process: ``unsup_occlusion="none"`` at batch 6 (the step as it was), ``"none"`` at batch 12 (what the second
direction costs: as many images through the model) and the chosen kind at batch 6 (12 images + the masks).

``--selfsup`` measures self-supervision instead (train/selfsup.py, csrc/kernels/selfsup.hip; default output
``profiles/selfsup_overhead.txt``), at the chairs shape of a batch-6 step, (N, 2B, H, W) = (12, 12, 368, 496): (a) the
three ``crop_resize`` launches of a step (the image stack, the flow, the teacher's plane) and the two loss launches
on the student half of a 4B stack, read in place, with the bytes they must move; (b) ``selfsup_loss`` forward +
backward against the golden op on the same GPU tensors, arms alternated, each run twice; (c) the training step in
three arms alternated in one process: ``"range"`` at batch 6 without self-supervision, ``"range"`` at batch 12 (what
4B pairs through the model cost) and self-supervision on at batch 6.

``--smooth-order 2`` measures the second-order smoothness term (csrc/kernels/smooth2.hip; default output
``profiles/smooth2_overhead.txt``): (a) its two launches with the bytes they must move, and each kernel's registers and
occupancy from the compiler's resource-usage remarks; (b) ``unsup_loss(..., smooth_order=2)`` against the golden op with
``smooth_order=2``; (c) the training step with ``unsup_smooth_order=2`` against ``unsup_smooth_order=1``, the step as it
was.  ``--photo census`` combines with it in (b) and (c).

  python tools/unsup_bench.py [--photo census | --smooth-order 2 | --occlusion range | --selfsup] [--out profiles/unsup_loss_overhead.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_raft_amd.ops import native as nat  # noqa: E402
from jax_raft_amd.train import unsup_loss, unsup_loss_reference  # noqa: E402
from jax_raft_amd.train.data import SyntheticFlow  # noqa: E402
from jax_raft_amd.train.trainer import TrainConfig, Trainer  # noqa: E402

N, B, H, W = 12, 6, 368, 496
BATCH = 6


def inputs(dev):
    """Frames of SyntheticFlow and predictions around its ground truth (most pixels land inside)."""
    i1, i2, flow, _ = SyntheticFlow((H, W), seed=0, device=dev).batch(list(range(B)))
    g = torch.Generator(device=dev).manual_seed(0)
    preds = flow[None] + torch.randn(N, B, H, W, 2, generator=g, device=dev) * torch.linspace(3.0, 0.3, N, device=dev).view(N, 1, 1, 1, 1)
    return preds.contiguous(), i1.contiguous(), i2.contiguous()


def events(fn, dev, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return 1000 * e0.elapsed_time(e1) / reps            # us


def launches(dev, reps):
    preds, i1, i2 = inputs(dev)
    P = B * H * W
    prm = nat.unsup_params(0.01, 0.001, 10.0, 0.5, dev)
    part = torch.empty(nat.unsup_loss_blocks(P), N, 4, device=dev)
    grad = torch.empty_like(preds)
    scale = torch.full((N, 2), 1.0 / P, device=dev)
    fwd = lambda: nat.ops().unsup_loss([preds, i1, i2, None, prm, part], [B, H, W, N])
    bwd = lambda: nat.ops().unsup_loss_bwd([preds, i1, i2, None, prm, scale, grad], [B, H, W, N])
    mb = lambda *ts: sum(t.numel() * t.element_size() for t in ts) / 1e6
    return {"fwd": events(fwd, dev, reps), "bwd": events(bwd, dev, reps),
            "fwd_mb": mb(preds, i1, i2, part), "bwd_mb": mb(preds, i1, i2, grad)}


def census_launches(dev, reps):
    preds, i1, i2 = inputs(dev)
    P = B * H * W
    prm = nat.unsup_params(0.01, 0.001, 10.0, 0.5, dev)
    gray = torch.empty(2, B, H, W, device=dev)
    part, coef = torch.empty(nat.census_tiles(B, H, W), N, 4, device=dev), torch.empty(N, B, H, W, device=dev)
    grad = torch.zeros_like(preds)
    scale = torch.full((N,), 1.0 / P, device=dev)
    ops = {"census_gray": (lambda: nat.ops().census_gray([i1, i2, gray], [B, H, W]), (i1, i2, gray), "both images, grey planes"),
           "census_loss": (lambda: nat.ops().census_loss([preds, gray, None, prm, part, coef], [B, H, W, N]),
                           (preds, gray, part, coef), "predictions, grey planes, partials, coefficients"),
           "census_loss_bwd": (lambda: nat.ops().census_loss_bwd([preds, gray, coef, scale, grad], [B, H, W, N, 0]),
                               (preds, gray, coef, grad), "predictions, grey planes, coefficients, gradient")}
    mb = lambda ts: sum(t.numel() * t.element_size() for t in ts) / 1e6
    out = []
    for name, (fn, ts, what) in ops.items():                # in this order: each needs the one before
        out.append((name, events(fn, dev, reps), mb(ts), what))
    return out


def smooth2_launches(dev, reps):
    preds, i1, _ = inputs(dev)
    P = B * H * W
    prm = nat.unsup_params(0.01, 0.001, 10.0, 0.5, dev)
    part = torch.empty(nat.smooth2_loss_blocks(P), N, 4, device=dev)
    grad = torch.zeros_like(preds)
    scale = torch.full((N,), 1.0 / P, device=dev)
    mb = lambda ts: sum(t.numel() * t.element_size() for t in ts) / 1e6
    rows = [("smooth2_loss", lambda: nat.ops().smooth2_loss([preds, i1, prm, part], [B, H, W, N]), (preds, i1, part),
             "predictions, image 1, partials"),
            ("smooth2_loss_bwd", lambda: nat.ops().smooth2_loss_bwd([preds, i1, prm, scale, grad], [B, H, W, N, 0]),
             (preds, i1, grad), "predictions, image 1, gradient written"),
            ("smooth2_loss_bwd add", lambda: nat.ops().smooth2_loss_bwd([preds, i1, prm, scale, grad], [B, H, W, N, 1]),
             (preds, i1, grad, grad), "predictions, image 1, gradient read and written")]
    return [(name, events(fn, dev, reps), mb(ts), what) for name, fn, ts, what in rows]


def resource_usage(src):
    """(kernel, VGPRs, occupancy in waves per SIMD) of every kernel of a .hip file, from the compiler's
    resource-usage remarks: a compile, no GPU needed.  None where there is no compiler."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return None
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(root, src), "-o",
                            os.path.join(d, "o.o"), "-Rpass-analysis=kernel-resource-usage"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        return None
    out, name = [], None
    for line in r.stdout.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], stdout=subprocess.PIPE, text=True).stdout.strip() or m.group(2)
            out.append([re.search(r"(\w+(<\w+>)?)\(", name.replace("(anonymous namespace)::", "")).group(1)])
        elif out:
            out[-1].append(m.group(2))
    return out


def pair(dev, reps, photo="charbonnier", order=1):
    preds, i1, i2 = inputs(dev)
    f = preds.clone().requires_grad_(True)
    kw = {**({} if photo == "charbonnier" else {"photo": photo}), **({} if order == 1 else {"smooth_order": order})}

    def run(loss_fn):
        def step():
            f.grad = None
            loss_fn(f, i1, i2, **kw)[0].backward()
        return step

    arms = {"native": run(unsup_loss), "torch": run(unsup_loss_reference)}
    times = {k: [] for k in arms}
    peak = {}
    for _ in range(2):
        for name, step in arms.items():
            f.grad = None                                # the other arm's gradient is not this arm's baseline
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            times[name].append(events(step, dev, reps, warm=2) / 1000)     # ms
            peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
    return times, peak


def training(args, dev):
    total = args.warmup + args.block * args.rounds
    kw = dict(arch=args.arch, steps=total, batch=BATCH, iters=args.iters, size=(384, 512), log_every=10 ** 9)
    if args.smooth_order == 2:
        photo = {} if args.photo == "charbonnier" else {"unsup_photo": args.photo}
        arms = {"order 2": Trainer(TrainConfig(loss="unsup", unsup_smooth_order=2, **photo, **kw)),
                "order 1": Trainer(TrainConfig(loss="unsup", **photo, **kw))}
    elif args.photo == "census":
        arms = {"census": Trainer(TrainConfig(loss="unsup", unsup_photo="census", **kw)),
                "charbonnier": Trainer(TrainConfig(loss="unsup", **kw))}
    else:
        arms = {"unsup": Trainer(TrainConfig(loss="unsup", **kw)), "sequence": Trainer(TrainConfig(**kw))}
    for name, tr in arms.items():
        t0 = time.perf_counter()
        for _ in range(args.warmup):
            tr.train_step(tr.batch_for(tr.step))
        tr.flush()
        torch.cuda.synchronize(dev)
        print(f"warm-up of {name}: {time.perf_counter() - t0:.1f} s", flush=True)
    rate = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, tr in arms.items():
            t0 = time.perf_counter()
            for _ in range(args.block):
                m = tr.train_step(tr.batch_for(tr.step))
            tr.flush()
            torch.cuda.synchronize(dev)
            rate[name].append(BATCH * args.block / (time.perf_counter() - t0))
            assert torch.isfinite(m["loss"]).item(), name
    return rate, {k: tr.skipped for k, tr in arms.items()}


def occlusion_launches(dev, reps, Bm=12):
    """The range-map launches at (Bm, H, W) per direction, flows around SyntheticFlow's ground truth."""
    _, _, flow, _ = SyntheticFlow((H, W), seed=0, device=dev).batch(list(range(Bm)))
    g = torch.Generator(device=dev).manual_seed(0)
    fw = (flow + 0.3 * torch.randn(Bm, H, W, 2, generator=g, device=dev)).contiguous()
    bw = (-flow + 0.3 * torch.randn(Bm, H, W, 2, generator=g, device=dev)).contiguous()
    acc = torch.zeros(2, Bm, H, W, dtype=torch.int32, device=dev)
    vis = torch.empty(2, Bm, H, W, device=dev)
    mb = lambda *ts: sum(t.numel() * t.element_size() for t in ts) / 1e6
    # the atomics the splat issues: the taps inside the map with a weight that is not zero
    taps = 0
    for f in (fw, bw):
        px = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W) + f[..., 0]
        py = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1) + f[..., 1]
        ok = (px > -1) & (px < W) & (py > -1) & (py < H)
        x0, y0 = torch.floor(px), torch.floor(py)
        qx, qy = torch.round((px - x0) * 16), torch.round((py - y0) * 16)
        for dy in (0, 1):
            for dx in (0, 1):
                w = (qx if dx else 16 - qx) * (qy if dy else 16 - qy)
                taps += int((ok & (w != 0) & (x0 + dx >= 0) & (x0 + dx < W) & (y0 + dy >= 0) & (y0 + dy < H)).sum())

    def splat():
        acc.zero_()
        nat.ops().range_splat([fw, bw, acc], [Bm, H, W])

    out = [("clear + range_splat", events(splat, dev, reps), mb(fw, bw, acc, acc),
            f"both flows read, acc cleared and added to; {taps} integer atomics, {taps / (2 * Bm * H * W):.2f} per source"),
           ("clear", events(acc.zero_, dev, reps), mb(acc), "acc written"),
           ("range_visible", events(lambda: nat.ops().range_visible([fw, bw, acc, vis], [Bm, H, W, 128]), dev, reps),
            mb(fw, bw, acc, vis), "both flows and acc read, masks written")]
    return Bm, out


def occlusion_training(args, dev):
    total = args.warmup + args.block * args.rounds
    kw = dict(arch=args.arch, steps=total, iters=args.iters, size=(384, 512), log_every=10 ** 9, loss="unsup")
    arms = {"none b6": Trainer(TrainConfig(batch=BATCH, **kw)),
            "none b12": Trainer(TrainConfig(batch=2 * BATCH, **kw)),
            f"{args.occlusion} b6": Trainer(TrainConfig(batch=BATCH, unsup_occlusion=args.occlusion, **kw))}
    for name, tr in arms.items():
        t0 = time.perf_counter()
        for _ in range(args.warmup):
            tr.train_step(tr.batch_for(tr.step))
        tr.flush()
        torch.cuda.synchronize(dev)
        print(f"warm-up of {name}: {time.perf_counter() - t0:.1f} s", flush=True)
    step_ms = {k: [] for k in arms}
    visible = []
    for _ in range(args.rounds):
        for name, tr in arms.items():
            t0 = time.perf_counter()
            for _ in range(args.block):
                m = tr.train_step(tr.batch_for(tr.step))
            tr.flush()
            torch.cuda.synchronize(dev)
            step_ms[name].append(1000 * (time.perf_counter() - t0) / args.block)
            assert torch.isfinite(m["loss"]).item(), name
            if "visible" in m:
                visible.append(float(m["visible"]))
    return step_ms, {k: tr.skipped for k, tr in arms.items()}, visible


def occlusion_main(args, dev):
    mean = lambda v: sum(v) / len(v)
    lines = [f"occlusion masks of the label-free training step (kind {args.occlusion!r}), {torch.cuda.get_device_name(dev)}", ""]
    Bm, rows = occlusion_launches(dev, args.reps)
    lines += [f"(a) GPU time per launch, device events over {args.reps} repetitions, {Bm} maps of {H} x {W} per direction "
              f"(flows (B, H, W) = ({Bm}, {H}, {W}) x 2 directions):"]
    for name, us, mbytes, what in rows:
        lines.append(f"    {name:20s} {us:8.1f} us   {mbytes:6.1f} MB at least ({what})  -> {mbytes / us * 1e3:6.0f} GB/s of them")
    lines += ["    (the splat uses global integer atomics; the block-local LDS image of the target tile was not built, so there is no A/B of it)",
              "    (kind 'fb' runs the existing fb_check kernel and elementwise torch ops instead of these two launches)", ""]
    print("\n".join(lines), flush=True)
    if not args.skip_training:
        step_ms, skipped, visible = occlusion_training(args, dev)
        a, b, c = list(step_ms)
        lines += [f"(c) training step, {args.arch}, 384x512, {args.iters} iterations, SyntheticFlow, loss='unsup'; {args.block} steps per block, "
                  f"blocks alternated {a} / {b} / {c} x {args.rounds} in one process after {args.warmup} warm-up steps each"]
        for k, v in step_ms.items():
            lines.append(f"    {k:9s} {mean(v):7.2f} ms/step  [per block: " + ", ".join(f"{x:.2f}" for x in v)
                         + f"]  spread {max(v) - min(v):.2f} ms   skipped steps: {skipped[k]}")
        lines += [f"    {a} is the step as it was (the parent commit's step: unsup_occlusion='none' changes nothing in it)",
                  f"    second direction ({b} - {a}): {mean(step_ms[b]) - mean(step_ms[a]):+.2f} ms/step "
                  f"({mean(step_ms[b]) / mean(step_ms[a]):.2f} x)",
                  f"    masks ({c} - {b}): {mean(step_ms[c]) - mean(step_ms[b]):+.2f} ms/step; largest spread between blocks of one arm "
                  f"{max(max(v) - min(v) for v in step_ms.values()):.2f} ms",
                  f"    share of visible pixels in the masked arm, last step of each block: " + ", ".join(f"{v:.3f}" for v in visible),
                  "    (all arms also run the sequence loss's forward kernel for the EPE metrics of the labelled synthetic set)", ""]
    lines += ["No accuracy figure follows from this: the weights are random and there is no dataset here, so whether the masks "
              "help is not measured.", ""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def selfsup_inputs(dev, B2=2 * BATCH, c=64):
    """A 4B stack of predictions whose student half lies around the teacher's flow in the student's frame, the
    target, and a weight with the share of selected pixels a step has (a band near the border)."""
    from jax_raft_amd.train.selfsup import flow_scale

    _, _, flow, _ = SyntheticFlow((H, W), seed=0, device=dev).batch(list(range(B2)))
    g = torch.Generator(device=dev).manual_seed(0)
    target = nat.crop_resize(flow.contiguous(), c, flow_scale(H, W, c))
    stack = torch.empty(N, 2 * B2, H, W, 2, device=dev)
    stack[:, :B2] = flow[None]
    stack[:, B2:] = target[None] + torch.randn(N, B2, H, W, 2, generator=g, device=dev) * torch.linspace(3.0, 0.3, N, device=dev).view(N, 1, 1, 1, 1)
    T = nat.crop_resize(torch.ones(B2, H, W, 1, device=dev), c).view(B2, H, W)
    S = torch.ones(B2, H, W, device=dev)
    S[:, :24], S[:, -24:], S[:, :, :32], S[:, :, -32:] = 0.0, 0.0, 0.0, 0.0
    return stack, target, (T * (1.0 - S)).contiguous(), flow.contiguous(), c


def selfsup_launches(dev, reps):
    from jax_raft_amd.train.selfsup import crop_ratios, flow_scale

    stack, target, weight, flow, c = selfsup_inputs(dev)
    B2 = target.shape[0]
    P = B2 * H * W
    mb = lambda *ts: sum(t.numel() * t.element_size() for t in ts) / 1e6
    crop_mb = lambda x: 2 * x.numel() * 4 * ((H - 2 * c) * (W - 2 * c) / (H * W) + 1.0) / 2 / 1e6   # the crop read, the frame written
    imgs = torch.rand(B2, H, W, 3, device=dev)
    plane = torch.ones(B2, H, W, 1, device=dev)
    rx, ry = crop_ratios(H, W, c)
    prm1 = torch.tensor([rx, ry, 1, 1, 1, 1], dtype=torch.float32, device=dev)
    prm2 = torch.tensor([rx, ry, *flow_scale(H, W, c), 1, 1], dtype=torch.float32, device=dev)
    out3, out2, out1 = torch.empty_like(imgs), torch.empty_like(flow), torch.empty_like(plane)
    eps = nat.selfsup_params(0.001, dev)
    part = torch.empty(nat.selfsup_loss_blocks(P), N, 4, device=dev)
    grad = torch.empty(N, B2, H, W, 2, device=dev)
    scale = torch.full((N,), 1.0 / P, device=dev)
    ints = [N, B2, H, W, 2 * B2, B2]
    half = stack[:, B2:]
    rows = [("crop_resize C=3", lambda: nat.ops().crop_resize([imgs, prm1, out3], [B2, H, W, 3, c]), crop_mb(imgs),
             "the crop of the image stack read, the frames written"),
            ("crop_resize C=2", lambda: nat.ops().crop_resize([flow, prm2, out2], [B2, H, W, 2, c]), crop_mb(flow),
             "the crop of the teacher's flow read, the target written"),
            ("crop_resize C=1", lambda: nat.ops().crop_resize([plane, prm1, out1], [B2, H, W, 1, c]), crop_mb(plane),
             "the crop of the teacher's plane read, the weight's factor written"),
            ("selfsup_loss", lambda: nat.ops().selfsup_loss([stack, target, weight, eps, part], ints), mb(half, target, weight, part),
             "the student half of the predictions, target, weight, partials"),
            ("selfsup_loss_bwd", lambda: nat.ops().selfsup_loss_bwd([stack, target, weight, eps, scale, grad], ints),
             mb(half, target, weight, grad), "the student half, target, weight, gradient")]
    return [(name, events(fn, dev, reps), mbytes, what) for name, fn, mbytes, what in rows], float((weight > 0).float().mean())


def selfsup_pair(dev, reps):
    from jax_raft_amd.train import selfsup_loss, selfsup_loss_reference

    stack, target, weight, _, _ = selfsup_inputs(dev)
    B2 = target.shape[0]
    f = stack.requires_grad_(True)

    def run(loss_fn):
        def step():
            f.grad = None
            loss_fn(f[:, B2:], target, weight, 0.8, 0.001)[0].backward()
        return step

    arms = {"native": run(selfsup_loss), "torch": run(selfsup_loss_reference)}
    times = {k: [] for k in arms}
    peak = {}
    for _ in range(2):
        for name, step in arms.items():
            f.grad = None
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            times[name].append(events(step, dev, reps, warm=2) / 1000)     # ms
            peak[name] = (torch.cuda.max_memory_allocated(dev) - base) / 1e6
    return times, peak


def selfsup_training(args, dev):
    total = args.warmup + args.block * args.rounds
    kw = dict(arch=args.arch, steps=total, iters=args.iters, size=(384, 512), log_every=10 ** 9, loss="unsup", unsup_occlusion="range")
    arms = {"range b6": Trainer(TrainConfig(batch=BATCH, **kw)),
            "range b12": Trainer(TrainConfig(batch=2 * BATCH, **kw)),
            "selfsup b6": Trainer(TrainConfig(batch=BATCH, unsup_selfsup_weight=0.3, unsup_selfsup_crop=64, **kw))}
    for name, tr in arms.items():
        t0 = time.perf_counter()
        for _ in range(args.warmup):
            tr.train_step(tr.batch_for(tr.step))
        tr.flush()
        torch.cuda.synchronize(dev)
        print(f"warm-up of {name}: {time.perf_counter() - t0:.1f} s", flush=True)
    step_ms = {k: [] for k in arms}
    share = []
    for _ in range(args.rounds):
        for name, tr in arms.items():
            t0 = time.perf_counter()
            for _ in range(args.block):
                m = tr.train_step(tr.batch_for(tr.step))
            tr.flush()
            torch.cuda.synchronize(dev)
            step_ms[name].append(1000 * (time.perf_counter() - t0) / args.block)
            assert torch.isfinite(m["loss"]).item(), name
            if "selfsup_w" in m:
                share.append(float(m["selfsup_w"]))
    return step_ms, {k: tr.skipped for k, tr in arms.items()}, share


def selfsup_main(args, dev):
    mean = lambda v: sum(v) / len(v)
    B2 = 2 * BATCH
    lines = [f"self-supervision of the label-free training step, {torch.cuda.get_device_name(dev)}",
             f"student predictions (N, 2B, H, W) = ({N}, {B2}, {H}, {W}), fp32, the second half of a (N, 4B, H, W, 2) stack; crop margin 64", ""]
    rows, on = selfsup_launches(dev, args.reps)
    lines += [f"(a) GPU time per launch, device events over {args.reps} repetitions (weight > 0 on {100 * on:.1f} % of the pixels):"]
    for name, us, mbytes, what in rows:
        lines.append(f"    {name:17s} {us:8.1f} us   {mbytes:6.1f} MB at least ({what})  -> {mbytes / us * 1e3:6.0f} GB/s of them")
    launch_ms = sum(us for _, us, _, _ in rows) / 1000
    lines += [f"    the five launches of a step: {launch_ms:.3f} ms (the swapped image stack is the swapped crop: one launch for both)",
              "    (the taps of crop_resize are re-reads that the caches serve; they are not in the byte counts)", ""]
    print("\n".join(lines), flush=True)
    times, peak = selfsup_pair(dev, args.pair_reps)
    spread = max(abs(v[0] - v[1]) for v in times.values())
    gain = mean(times["torch"]) - mean(times["native"])
    lines += [f"(b) selfsup_loss forward + backward through the slice of the 4B stack, {args.pair_reps} repetitions per run, arms alternated "
              "native / torch x 2:"]
    for k, v in times.items():
        lines.append(f"    {k:7s} {mean(v):8.3f} ms   [runs: {v[0]:.3f}, {v[1]:.3f}]   peak extra memory {peak[k]:8.0f} MB")
    lines += [f"    torch - native: {gain:+.3f} ms ({mean(times['torch']) / mean(times['native']):.1f} x); larger difference "
              f"between the two runs of one arm: {spread:.3f} ms",
              "    -> " + ("native is faster by more than that spread" if gain > spread else
                           "NOT faster by more than that spread: the condition does not hold"),
              "    (both arms include autograd's padding of the window's gradient into the 4B stack)", ""]
    print("\n".join(lines[-len(times) - 5:]), flush=True)
    if not args.skip_training:
        step_ms, skipped, share = selfsup_training(args, dev)
        a, b, c = list(step_ms)
        lines += [f"(c) training step, {args.arch}, 384x512, {args.iters} iterations, SyntheticFlow, loss='unsup', unsup_occlusion='range'; "
                  f"{args.block} steps per block, blocks alternated {a} / {b} / {c} x {args.rounds} in one process after {args.warmup} "
                  "warm-up steps each"]
        for k, v in step_ms.items():
            lines.append(f"    {k:10s} {mean(v):7.2f} ms/step  [per block: " + ", ".join(f"{x:.2f}" for x in v)
                         + f"]  spread {max(v) - min(v):.2f} ms   skipped steps: {skipped[k]}")
        worst = max(max(v) - min(v) for v in step_ms.values())
        extra = mean(step_ms[c]) - mean(step_ms[b])
        lines += [f"    {a} is the step as it was; {b} runs as many pairs through the model as {c} (24), without self-supervision",
                  f"    4B pairs ({b} - {a}): {mean(step_ms[b]) - mean(step_ms[a]):+.2f} ms/step ({mean(step_ms[b]) / mean(step_ms[a]):.2f} x)",
                  f"    self-supervision on top ({c} - {b}): {extra:+.2f} ms/step; the measured launches: {launch_ms:.2f} ms; largest spread "
                  f"between blocks of one arm {worst:.2f} ms",
                  "    -> " + ("the self-supervised step costs no more than the batch-12 arm plus the launches, within that spread"
                               if extra <= launch_ms + worst else
                               "the self-supervised step costs MORE than the batch-12 arm plus the launches and the spread: the condition "
                               "does not hold"),
                  "    share of pixels with weight > 0, last step of each block: " + ", ".join(f"{v:.3f}" for v in share),
                  "    (beside the five launches the step runs a second visibility_masks call, two lands_inside compositions, the slice "
                  "copy of the full-frame half for unsup_loss and the padding of both halves' gradients)", ""]
    lines += ["No accuracy figure follows from this: the weights are random and there is no dataset here, so whether self-supervision "
              "helps is not measured.", ""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--selfsup", action="store_true", help="measure self-supervision instead of the loss")
    ap.add_argument("--occlusion", default=None, choices=("fb", "range"), help="measure the occlusion masks instead of the loss")
    ap.add_argument("--photo", default="charbonnier", choices=("charbonnier", "census"))
    ap.add_argument("--smooth-order", type=int, default=1, choices=(1, 2), help="2: measure the second-order smoothness term")
    ap.add_argument("--out", default=None, help="default: profiles/unsup_loss_overhead.txt, census_loss_overhead.txt with --photo census, "
                    "smooth2_overhead.txt with --smooth-order 2")
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--pair-reps", type=int, default=20)
    ap.add_argument("--block", type=int, default=20, help="steps per block")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--arch", default="raft_large")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--skip-training", action="store_true", help="(a) and (b) only")
    args = ap.parse_args()
    census = args.photo == "census"
    if args.selfsup:
        assert torch.cuda.is_available(), "unsup_bench measures on the GPU"
        args.out = args.out or "profiles/selfsup_overhead.txt"
        return selfsup_main(args, torch.device("cuda", 0))
    if args.occlusion:
        assert torch.cuda.is_available(), "unsup_bench measures on the GPU"
        args.out = args.out or "profiles/occlusion_overhead.txt"
        return occlusion_main(args, torch.device("cuda", 0))
    order2 = args.smooth_order == 2
    args.out = args.out or ("profiles/smooth2_overhead.txt" if order2 else
                            "profiles/census_loss_overhead.txt" if census else "profiles/unsup_loss_overhead.txt")
    assert torch.cuda.is_available(), "unsup_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    mean = lambda v: sum(v) / len(v)
    lines = [f"label-free loss ({'census' if census else 'photometric'} + edge-aware {'second-order ' if order2 else ''}smoothness), "
             f"{torch.cuda.get_device_name(dev)}",
             f"predictions (N, B, H, W) = ({N}, {B}, {H}, {W}), fp32; no mask", ""]
    if order2:
        lines += [f"(a) GPU time per launch, device events over {args.reps} repetitions:"]
        for name, us, mbytes, what in smooth2_launches(dev, args.reps):
            lines.append(f"    {name:20s} {us:8.1f} us   {mbytes:6.1f} MB at least ({what})  -> {mbytes / us * 1e3:6.0f} GB/s of them")
        lines += ["    (neighbouring flows and image texels are re-reads that the caches serve; they are not in the byte counts;",
                  "     the training step uses the adding form of the backward: unsup.hip's or census.hip's launch writes the gradient first)"]
        usage = resource_usage("csrc/kernels/smooth2.hip")
        if usage is None:
            lines += ["    compiler resource usage: no compiler here, not recorded"]
        for row in usage or []:
            lines.append("    compiler resource usage (gfx950): {:32s} VGPRs {}, scratch {} bytes/lane, occupancy {} waves/SIMD".format(*row))
        lines += [""]
    elif census:
        lines += [f"(a) GPU time per launch, device events over {args.reps} repetitions:"]
        for name, us, mbytes, what in census_launches(dev, args.reps):
            lines.append(f"    {name:16s} {us:8.1f} us   {mbytes:6.1f} MB at least ({what})  -> {mbytes / us * 1e3:6.0f} GB/s of them")
        lines += ["    (the halo's samples and the texel gathers are re-reads that the caches serve; they are not in the byte counts;",
                  "     the census loss also runs unsup_loss and unsup_loss_bwd for the smoothness term: profiles/unsup_loss_overhead.txt)", ""]
    kt = None if census or order2 else launches(dev, args.reps)
    if kt:
        lines += [f"(a) GPU time per launch, device events over {args.reps} repetitions:",
                  f"    unsup_loss     {kt['fwd']:8.1f} us   {kt['fwd_mb']:6.1f} MB at least (predictions, both images, partials)"
                  f"  -> {kt['fwd_mb'] / kt['fwd'] * 1e3:6.0f} GB/s of them",
                  f"    unsup_loss_bwd {kt['bwd']:8.1f} us   {kt['bwd_mb']:6.1f} MB at least (predictions, both images, gradient)"
                  f"  -> {kt['bwd_mb'] / kt['bwd'] * 1e3:6.0f} GB/s of them",
                  "    (neighbouring flows and the texel gathers are re-reads that the caches serve; they are not in the byte counts)", ""]
    print("\n".join(lines), flush=True)
    times, peak = pair(dev, args.pair_reps, args.photo, args.smooth_order)
    spread = max(abs(v[0] - v[1]) for v in times.values())
    gain = mean(times["torch"]) - mean(times["native"])
    lines += [f"(b) loss forward + backward, {args.pair_reps} repetitions per run, arms alternated native / torch x 2:"]
    for k, v in times.items():
        lines.append(f"    {k:7s} {mean(v):8.3f} ms   [runs: {v[0]:.3f}, {v[1]:.3f}]   peak extra memory {peak[k]:8.0f} MB")
    lines += [f"    torch - native: {gain:+.3f} ms ({mean(times['torch']) / mean(times['native']):.1f} x); larger difference "
              f"between the two runs of one arm: {spread:.3f} ms",
              "    -> " + ("native is faster by more than that spread" if gain > spread else
                           "NOT faster by more than that spread: the condition does not hold"), ""]
    print("\n".join(lines[-len(times) - 4:]), flush=True)
    if not args.skip_training:
        rate, skipped = training(args, dev)
        ms = lambda x: 1000 * BATCH / x
        first, second = list(rate)
        u, s = mean(rate[first]), mean(rate[second])
        lines += [f"(c) training step, {args.arch}, 384x512, batch {BATCH}, {args.iters} iterations, SyntheticFlow; {args.block} steps per "
                  f"block, blocks alternated {first} / {second} x {args.rounds} in one process after {args.warmup} warm-up steps each"]
        for k in rate:
            lines.append(f"    {k:8s} {mean(rate[k]):7.1f} pairs/s  {ms(mean(rate[k])):6.2f} ms/step  [per block: "
                         + ", ".join(f"{v:.1f}" for v in rate[k]) + f"]   skipped steps: {skipped[k]}")
        lines += [f"    {first} - {second}: {ms(u) - ms(s):+.2f} ms/step ({100 * (u - s) / s:+.1f} % pairs/s); largest spread between "
                  f"blocks of one arm {max(max(v) - min(v) for v in rate.values()):.1f} pairs/s",
                  f"    ({second} is the step as it was: unsup_smooth_order=1 changes nothing in it; both arms also run the sequence loss's "
                  "forward kernel for the EPE metrics)" if order2 else
                  "    (both arms also run the sequence loss's forward kernel for the EPE metrics of the labelled synthetic set)" if census
                  else "    (the unsup step also runs the sequence loss's forward kernel for the EPE metrics of the labelled synthetic set)", ""]
    lines += ["Not measured: accuracy.  There is no checkpoint and no real data here, and the loss's default weights are placeholders.", ""]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
