#!/usr/bin/env python3
"""Solo device time of the mask lane's flow features at the loop's shapes: the two launches
(``conv_direct`` 7x7, 2 -> 128, then the halo 3x3 conv 128 -> 64 in the config <128, 2, 2, 2, 8, 16>)
against the one launch ``flow_features_fused`` (flowfeat.hip), each as a captured graph of --reps
launches (tools/conv_bench.py:graph_time), rounds interleaved.

  python tools/masklane_bench.py            # batch 4 and 1 at 55 x 128
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from conv_bench import graph_time   # noqa: E402


def main():
    from jax_raft_amd.ops import native as nat

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    nat.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    k1 = torch.randn(7, 7, 2, 128, generator=g) / math.sqrt(98) / 8
    k2 = torch.randn(3, 3, 128, 64, generator=g) / math.sqrt(9 * 128)
    w1, b1 = nat.pack_direct_weight(k1).to(dev), torch.zeros(128, device=dev)
    sp2 = nat.make_spec(k2, torch.zeros(64), (1, 1), (1, 1), cin8=128, device=dev)
    cfg = nat.HALO_CFG0 + nat.HALO_CFGS.index((128, 2, 2, 2, 8, 16))
    for N, H, W in ((4, 55, 128), (1, 55, 128)):
        M = N * H * W
        flow8 = (torch.randn(M, 2, generator=g) * 15).to(dev, torch.bfloat16)
        f1 = torch.empty(M, 128, device=dev, dtype=torch.bfloat16)
        cf = torch.empty(M, 256, device=dev, dtype=torch.bfloat16)
        first = lambda: nat.ops().conv_direct([flow8, w1, b1, f1], [N, H, W, 2, 7, 7, 3, 3, 128, 1, 0])
        second = lambda: nat.ops().conv(*nat.conv_args(sp2, f1, N, H, W, cf, y_coff=192, act=nat.ACT_RELU, cfg=cfg))
        variants = {"conv_direct": first, "convflow2 (halo)": second, "pair": lambda: (first(), second()),
                    "flow_features_fused": lambda: nat.flow_features_fused(flow8, w1, b1, sp2, N, H, W, cf, 192)}
        best = {}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                t = graph_time(fn, a.reps)
                best[name] = min(best.get(name, t), t)
        print(f"batch {N}, {H} x {W} ({nat.flow_fused_tiles(N, H, W)} tiles): "
              + ", ".join(f"{k} {v:.1f} us" for k, v in best.items()))


if __name__ == "__main__":
    main()
