#!/usr/bin/env python3
"""Cost and memory of on-demand correlation: ``RaftEngine(corr="volume")`` against
``RaftEngine(corr="on_demand")``, raft_large and raft_small, at 440 x 1024 (batch 1 and 4),
1088 x 1920 and 2160 x 3840 (batch 1), plus one on-demand-only row at 4320 x 7680 (batch 1, few
iterations), where the volume would need 714 GB.

Protocol: ``b1_sync`` of bench.py (per call: H2D from pageable host memory + forward with all
iterations upsampled + synchronise; no cross-call overlap), the arms alternated in one process,
vol / od / vol2 / od2, ~``--block-s`` of steady calls per block after a warm-up of every plan.
``vol2`` / ``od2`` are the same forwards on a second engine (another capture of the same plan):
two captures of one plan do not replay equally fast, so ``vol2 - vol`` and ``od2 - od`` are the
spread below which ``od - vol`` resolves nothing.  The second engines are left out from
2160 x 3840 on (a second 45 GB pyramid), and from that size on the engines are built with
``autotune=False`` (no timing of tile candidates at plan build), both arms alike.

Per configuration it also records the ``lookup`` / ``lookup_od`` launch alone (device events
around repeated eager launches on the plan's own buffers, at the coordinates the forward left)
and the bytes of the plan's buffers (all of them, and the correlation share: ``corr.l*`` levels
or the pooled feature levels ``fpool.l*``).

  python tools/ondemand_bench.py [--out profiles/ondemand_overhead.txt] [--block-s 0.4] [--rounds 2]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_raft_amd import raft_large, raft_small  # noqa: E402
from jax_raft_amd.ops import native as nat  # noqa: E402
from jax_raft_amd.runtime.engine import RaftEngine  # noqa: E402

CONFIGS = [   # H, W, B, iterations, second engines, autotune
    (440, 1024, 1, 12, True, True),
    (440, 1024, 4, 12, True, True),
    (1088, 1920, 1, 12, True, True),
    (2160, 3840, 1, 12, False, False),
]
BIG = (4320, 7680, 1, 2)   # on demand only


def block(eng, pairs, dev, iters, seconds, min_calls=4):
    """Steady calls of one arm for ~``seconds``: the latencies in ms."""
    lat, i, t_end = [], 0, time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(lat) < min_calls:
        a, b = pairs[i % len(pairs)]
        t0 = time.perf_counter()
        flow = eng.forward(a.to(dev), b.to(dev), iters)[-1]
        torch.cuda.synchronize(dev)
        lat.append(1000 * (time.perf_counter() - t0))
        i += 1
    assert flow.shape == pairs[0][0].shape[:3] + (2,)
    return lat


def plan_state(eng, B, H, W, iters):
    return eng._states[(B, H, W, iters, True)]


def plan_bytes(st):
    """(all plan buffers incl. inputs and output, the correlation share) in bytes."""
    size = lambda t: t.numel() * t.element_size()   # noqa: E731
    total = sum(size(t) for t in st.bufs.values()) + size(st.inp1) + size(st.inp2) + size(st.out)
    corr = sum(size(t) for k, t in st.bufs.items() if ".corr.l" in k or ".fpool.l" in k)
    return total, corr


def lookup_alone(eng, st, B, H, W, dev, reps=20):
    """us per ``lookup`` / ``lookup_od`` launch on the plan's own buffers (no fused update)."""
    h, w, L = H // 8, W // 8, eng.num_levels
    bufs = st.bufs
    coords, corr = bufs["p0.coords"], bufs["p0.corr"]
    if eng.corr_mode == "on_demand":
        fmap = bufs["p0.fmap"]
        pooled = [bufs[f"p0.fpool.l{l}"] for l in range(1, L)]
        t = [coords, corr, fmap[:B], fmap[B:]] + pooled + [None] * (4 - L)
        i = [L, B, h, w, eng.radius, eng.fmap_ch]
        op = nat.ops().lookup_od
    else:
        t = [coords, corr] + [bufs[f"p0.corr.l{l}"] for l in range(L)] + [None] * (4 - L)
        i = [L, B, h, w, eng.radius, h * w, int(eng.corr_blocked)]
        op = nat.ops().lookup
    for _ in range(3):
        op(t, i)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        op(t, i)
    e1.record()
    torch.cuda.synchronize(dev)
    return 1000 * e0.elapsed_time(e1) / reps


def gib(n):
    return f"{n / 2 ** 30:8.3f} GiB"


def pairs_for(B, H, W, n=2):
    g = torch.Generator().manual_seed(99)
    return [(torch.rand(B, H, W, 3, generator=g) * 2 - 1, torch.rand(B, H, W, 3, generator=g) * 2 - 1)
            for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ondemand_overhead.txt")
    ap.add_argument("--block-s", type=float, default=0.4)
    ap.add_argument("--rounds", type=int, default=2, help="rounds of the alternated arms per configuration")
    ap.add_argument("--skip-big", action="store_true", help="leave the 4320 x 7680 row out")
    ap.add_argument("--quick", action="store_true", help="the first configuration only (a probe)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ondemand_bench measures on the GPU"
    dev = torch.device("cuda", 0)
    lines = [f"on-demand correlation against the all-pairs volume, {torch.cuda.get_device_name(dev)}",
             "b1_sync protocol (H2D pageable + forward, all iterations upsampled + sync), arms alternated",
             f"vol / od / vol2 / od2 x {args.rounds} in one process, ~{args.block_s} s per block;",
             "vol2 / od2 = the same forward on a second engine (another capture of the same plan): the spread.",
             "ms per call: mean over the arm's blocks (per-block means in brackets); lookup: us per launch alone;",
             "bytes: all plan buffers (correlation share: pyramid levels, or pooled feature levels)", ""]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    def write():
        text = "\n".join(lines) + "\n"
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return text

    def failed(tag, ex):
        """Record the exact error.  Out of memory leaves the device usable and the run goes on;
        after anything else nothing more is launched."""
        msg = str(ex).splitlines()[0] if str(ex) else ""
        emit(f"{tag}  FAILED: {type(ex).__name__}: {msg}")
        if not (isinstance(ex, torch.cuda.OutOfMemoryError) or "out of memory" in str(ex).lower()):
            emit("stopped: not an out-of-memory error")
            write()
            sys.exit(1)

    models = {name: f(seed=0)[0].to(dev).eval() for name, f in (("raft_large", raft_large), ("raft_small", raft_small))}
    configs = CONFIGS[:1] if args.quick else CONFIGS
    for H, W, B, iters, second, tune in configs:
        pairs = pairs_for(B, H, W)
        for name, model in models.items():
            tag = f"{name:10s} {H}x{W} b{B} {iters} it"
            order = []
            for arm, mode in (("vol", "volume"), ("od", "on_demand")) + ((("vol2", "volume"), ("od2", "on_demand")) if second else ()):
                e = None
                try:   # the plan built, its graph captured, steady clocks; an arm that fails is left out
                    e = RaftEngine(model, dev, corr=mode, autotune=tune)
                    block(e, pairs, dev, iters, 0.2, min_calls=2)
                    order.append((arm, e))
                except Exception as ex:
                    if e is not None:
                        e.release()
                    del e
                    torch.cuda.empty_cache()
                    failed(f"{tag}  {arm}", ex)
            arms = {k: [] for k, _ in order}
            try:
                for _ in range(args.rounds):
                    for k, e in order:
                        arms[k].append(block(e, pairs, dev, iters, args.block_s))
                mean = {k: sum(map(sum, v)) / sum(map(len, v)) for k, v in arms.items()}
                per = {k: ", ".join(f"{sum(b) / len(b):.3f}" for b in v) for k, v in arms.items()}
                s = tag + "  " + "  ".join(f"{k} {mean[k]:8.3f} ms [{per[k]}]" for k in arms)
                if "od" in mean and "vol" in mean:
                    s += f"   od / vol {mean['od'] / mean['vol']:.3f}"
                if "vol2" in mean and "vol" in mean:
                    s += f"   vol2 - vol {mean['vol2'] - mean['vol']:+.3f} ms"
                if "od2" in mean and "od" in mean:
                    s += f"   od2 - od {mean['od2'] - mean['od']:+.3f} ms"
                emit(s)
                info = []
                for k, e in order:
                    if k not in ("vol", "od"):
                        continue
                    st = plan_state(e, B, H, W, iters)
                    total, corr = plan_bytes(st)
                    info.append(f"{k}: {'lookup_od' if k == 'od' else 'lookup'} {lookup_alone(e, st, B, H, W, dev):9.1f} us, "
                                f"plan {gib(total)} (correlation {gib(corr)})")
                emit(" " * len(tag) + "  " + "   ".join(info))
            except Exception as ex:   # the row records the exact error
                failed(tag, ex)
            for _, e in order:
                e.release()
            del order
            torch.cuda.empty_cache()
    if not (args.skip_big or args.quick):
        H, W, B, iters = BIG
        pairs = pairs_for(B, H, W, n=1)
        for name, model in models.items():
            tag = f"{name:10s} {H}x{W} b{B} {iters} it (on demand only; the volume: 714 GB bf16)"
            eng = None
            try:
                eng = RaftEngine(model, dev, corr="on_demand", autotune=False)
                block(eng, pairs, dev, iters, 0.0, min_calls=1)
                lat = block(eng, pairs, dev, iters, args.block_s, min_calls=3)
                st = plan_state(eng, B, H, W, iters)
                total, corr = plan_bytes(st)
                emit(f"{tag}  od {sum(lat) / len(lat):9.3f} ms ({len(lat)} calls)   lookup_od "
                     f"{lookup_alone(eng, st, B, H, W, dev, reps=5):9.1f} us, plan {gib(total)} (correlation {gib(corr)})")
            except Exception as ex:
                failed(tag, ex)
            if eng is not None:
                eng.release()
            del eng
            torch.cuda.empty_cache()
    print(write())


if __name__ == "__main__":
    main()
