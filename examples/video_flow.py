#!/usr/bin/env python3
"""Optical flow over a frame sequence with graph-pipelined engine steps
(``RaftEngine.pipelined``): each call replays one hipGraph that holds the
previous pair's refinement loop and this pair's encoders + correlation
pyramid, and returns the previous pair's flow; ``flush()`` drains the last.

  python examples/video_flow.py frame_0000.png frame_0001.png ... [--arch raft_small] [--iters 12] [--warm-start | --bidirectional [--warp | --interpolate K] [--out DIR]]

``--warm-start`` runs the synchronous path instead (``RaftEngine.forward``) and
starts every pair after the first from the previous pair's flow, projected
forward in time on the GPU (``flow_init="previous"``); ``--iters`` applies as
given.  (A pipelined step cannot warm-start: it runs the next pair's prologue
next to the previous pair's loop.)

``--bidirectional`` also runs the synchronous path: every pair yields the flows in both
directions and the two forward-backward occlusion masks from one engine call
(``forward(bidirectional=True)``); the backward flows and the masks are kept next to the
forward flows.  This path feeds the raw uint8 frames: the engine pads them on the GPU, crops
the flows and the masks back, and its check treats the frame -- not the padded map -- as the
image, so a landing point in the padding counts as outside.

``--bidirectional --warp`` adds the motion-compensated frames and the masked photometric error
from the same call (``forward(bidirectional=True, warp=True)``): frame 2 sampled with the flow
1 -> 2 (and frame 1 with the flow 2 -> 1), occluded pixels taken from the frame itself.  It prints
the mean absolute error in 8-bit levels over the kept pixels and the share of pixels kept, per
direction over the sequence -- a label-free check of the flow, not an accuracy figure (with
random weights it says nothing about accuracy at all); ``--out DIR`` writes ``warped_fw_NNNN.png``
(the PNG encoder runs on the host between the calls, so the printed pairs/s then measures it too).

``--bidirectional --interpolate K`` adds K frames between the two of every pair, at the times
``t = j / (K + 1)``, from the same call (``forward(bidirectional=True, interpolate=t)``): every
pixel of both frames is splatted forward along a fraction of its flow and the contributions are
normalised, on the GPU, bit for bit repeatable.  It prints the share of hole pixels (cells
nothing reached, filled from the nearer frame) per ``t`` over the sequence; ``--out DIR`` writes
``interp_NNNN_j.png``.  With random weights the frames say nothing about interpolation quality.

Without frames a synthetic drifting sequence is used.  Needs an MI355X (the
native engine); prints the pairs/s of the steady state.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from jax_raft_amd import photometric_error, raft_large, raft_small  # noqa: E402
from jax_raft_amd.utils.flow_io import InputPadder, normalize_image, read_image, write_png  # noqa: E402


def frames(paths, n_synth=16, raw=False):
    """Float NHWC frames in [-1, 1]; ``raw``: the uint8 frames themselves, (1, H, W, 3)."""
    prep = (lambda a: torch.from_numpy(np.ascontiguousarray(a))[None]) if raw else normalize_image
    if paths:
        for p in paths:
            yield prep(read_image(p))
        return
    rng = np.random.default_rng(0)
    base = rng.integers(0, 255, (440 + 8 * n_synth, 1024 + 8 * n_synth, 3), dtype=np.uint8)
    for k in range(n_synth):
        yield prep(base[3 * k:3 * k + 436, 2 * k:2 * k + 1024])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("frames", nargs="*")
    ap.add_argument("--arch", default="raft_large", choices=["raft_large", "raft_small"])
    ap.add_argument("--weights", default=None, help="Flax msgpack checkpoint (else random init)")
    ap.add_argument("--iters", type=int, default=32)
    ap.add_argument("--warm-start", action="store_true",
                    help="synchronous forwards, each pair after the first started from the previous pair's flow")
    ap.add_argument("--bidirectional", action="store_true",
                    help="synchronous forwards that return both directions' flows and the occlusion masks")
    ap.add_argument("--warp", action="store_true",
                    help="with --bidirectional: also the motion-compensated frames and the masked photometric error")
    ap.add_argument("--interpolate", type=int, default=0, metavar="K",
                    help="with --bidirectional: also K frames between the two of every pair, at t = j / (K + 1) (1 to 8)")
    ap.add_argument("--out", default=None, help="with --warp: a directory for warped_fw_NNNN.png; with --interpolate: "
                                                "for interp_NNNN_j.png")
    args = ap.parse_args()
    assert not (args.warm_start and args.bidirectional), "--warm-start and --bidirectional exclude each other"
    assert args.bidirectional or not args.warp, "--warp needs --bidirectional"
    assert args.bidirectional or not args.interpolate, "--interpolate needs --bidirectional"
    assert not (args.warp and args.interpolate), "--warp and --interpolate exclude each other (one consumer per plan)"
    assert 0 <= args.interpolate <= 8, "--interpolate takes 1 to 8 frames per pair"
    assert args.warp or args.interpolate or args.out is None, "--out needs --warp or --interpolate"
    times = [j / (args.interpolate + 1) for j in range(1, args.interpolate + 1)]
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    assert torch.cuda.is_available(), "the pipelined engine runs on the GPU"
    factory = raft_large if args.arch == "raft_large" else raft_small
    model, _ = factory(weights=args.weights) if args.weights else factory()
    dev = torch.device("cuda", 0)
    model = model.to(dev).eval()
    eng = model.engine(dev)

    flows, prev, padder = [], None, None
    flows_bw, occ_fw, occ_bw = [], [], []
    photo, frame = None, None   # --warp: the running (2, 2) int64 sums over the sequence, on the device
    n_holes = None              # --interpolate: the running hole counts (K,) over the sequence, on the device
    t0, n_pairs = None, 0
    for img in frames(args.frames, raw=args.bidirectional):
        if args.bidirectional:   # raw frames: padded, cropped and windowed by the engine
            cur = img.to(dev)
            if prev is not None:
                res = eng.forward(prev, cur, args.iters, return_all_iters=False, bidirectional=True, warp=args.warp,
                                  interpolate=times or None)
                if times:
                    holes = res.holes.sum((1, 2, 3))
                    n_holes = holes if n_holes is None else n_holes + holes
                    frame = tuple(cur.shape[1:3])
                    if args.out:
                        for j in range(len(times)):
                            write_png(os.path.join(args.out, f"interp_{len(flows):04d}_{j + 1}.png"),
                                      res.frames[j, 0].cpu().numpy())
                if args.warp:
                    photo = res.photo.sum(1) if photo is None else photo + res.photo.sum(1)
                    frame = tuple(cur.shape[1:3])
                    if args.out:
                        write_png(os.path.join(args.out, f"warped_fw_{len(flows):04d}.png"), res.warped_fw[0].cpu().numpy())
                flows.append(res.flows_fw[-1])
                flows_bw.append(res.flows_bw[-1])
                occ_fw.append(res.occ_fw)
                occ_bw.append(res.occ_bw)
                if t0 is None:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                else:
                    n_pairs += 1
            prev = cur
            continue
        if padder is None:
            padder = InputPadder(img.shape, channels_last=True)
        (cur,) = padder.pad(img)
        cur = cur.to(dev)
        if prev is not None and args.warm_start:
            out = eng.forward(prev, cur, args.iters, return_all_iters=False, flow_init="previous" if flows else None)
            flows.append(padder.unpad(out[-1]))
            if t0 is None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            else:
                n_pairs += 1
        elif prev is not None:
            out = eng.pipelined(prev, cur, args.iters, return_all_iters=False)   # the previous pair's flow
            if out is not None:
                flows.append(padder.unpad(out[-1]))
                if t0 is None:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                else:
                    n_pairs += 1
        prev = cur
    last = eng.flush()
    if last is not None:
        flows.append(padder.unpad(last[-1]))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0 if t0 is not None else 0.0
    if occ_fw:
        frac = [float(torch.stack(m).float().mean()) for m in (occ_fw, occ_bw)]
        print(f"{len(flows_bw)} backward flow fields, {len(occ_fw)} mask pairs {tuple(occ_fw[0].shape)}; "
              f"occluded 1->2 {100 * frac[0]:.1f} %, 2->1 {100 * frac[1]:.1f} %")
    if photo is not None:
        mae, cov = photometric_error(photo.cpu(), frame)
        cov = cov / len(flows)   # the sums run over every pair of the sequence
        print("masked photometric error (8-bit levels) / pixels kept: "
              f"1->2 {float(mae[0]):.2f} / {100 * float(cov[0]):.1f} %, 2->1 {float(mae[1]):.2f} / {100 * float(cov[1]):.1f} %")
    if n_holes is not None:
        share = n_holes.cpu().double() / (len(flows) * cur.shape[0] * frame[0] * frame[1])
        print("interpolated frames, hole pixels: " + ", ".join(f"t = {t:.3f}: {100 * float(v):.2f} %" for t, v in zip(times, share)))
    print(f"{len(flows)} flow fields {tuple(flows[0].shape) if flows else ()}; "
          f"steady state {n_pairs / dt if dt > 0 and n_pairs else float('nan'):.1f} pairs/s")


if __name__ == "__main__":
    main()
