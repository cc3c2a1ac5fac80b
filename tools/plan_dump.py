#!/usr/bin/env python3
"""Fingerprints of the plans the inference engine records, on the CPU: one SHA-256 per case over
the canonical form of the plan state the engine builds against a recording stand-in for the
native Plan.  Two trees that print the same JSON record the same plans -- every op, in the same
segment / lane / defer position, over the same buffers -- so a refactor of the lowering runs this
file on both sides, and a schedule change shows exactly which plans it touched.

Canonical form of one plan state: for every batch part the full op list ``(segment, lane, defer,
op, args)``, every tensor argument replaced by ``(storage index in order of first appearance,
storage offset, shape, strides, dtype)``, other values as they are; the sorted ``(name, shape,
dtype)`` of ``st.bufs``; ``st.slot_ok``; ``st.flow_out``; ``inp1``, ``inp2``, ``out``,
``out_slot``, ``flow_init``, ``occ``, ``thr``, ``warped`` and ``photo``; and ``eng.gru_path`` /
``eng.corr_blocked`` after the build.  A case that raises counts with its exception text.

The cases (128 x 256, 3 iterations, weights seeded with ``torch.manual_seed(0)``,
``autotune=False``) use only the engine's stable entry points: ``RaftEngine(model, "cpu", ...)``,
``_build_key``, ``_slot_state`` and the lowering choices' class attributes.

  python tools/plan_dump.py [--out plan_dump.json] [--only SUBSTRING]
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_raft_amd import raft_large, raft_small  # noqa: E402
from jax_raft_amd.ops import native as nat  # noqa: E402
from jax_raft_amd.runtime import engine as E  # noqa: E402
from jax_raft_amd.runtime import tunedb  # noqa: E402

H, W, ITERS = 128, 256, 3
U8 = ("u8", 125, 250, 1, 3)   # 125 x 250 frames inside the padded 128 x 256 plan
FACTORIES = {"raft_large": raft_large, "raft_small": raft_small}
STATE_TENSORS = ("inp1", "inp2", "out", "out_slot", "flow_init", "occ", "thr", "warped", "photo")


class FakePlan:
    """Records (segment, lane, defer, op, args) for every add_* call."""

    def __init__(self):
        self.ops = []
        self.seg, self.ln, self.defer = 0, 0, 0

    def set_segment(self, s):
        self.seg = s

    def set_lane(self, l):
        self.ln = l

    def set_defer(self, d):
        self.defer = d

    def __getattr__(self, name):
        if not name.startswith("add_"):
            raise AttributeError(name)

        def rec(*args):
            self.ops.append((self.seg, self.ln, self.defer, name[4:], args))
        return rec


@contextlib.contextmanager
def fake_native():
    """No native library, the recording plan, a fixed architecture name (restored on exit)."""
    saved = nat.require, nat.new_plan, tunedb.gpu_arch
    nat.require, nat.new_plan, tunedb.gpu_arch = (lambda: None), FakePlan, (lambda device=None: "cpu")
    try:
        yield
    finally:
        nat.require, nat.new_plan, tunedb.gpu_arch = saved


@contextlib.contextmanager
def class_attrs(attrs):
    saved = {k: getattr(E.RaftEngine, k) for k in attrs}
    for k, v in attrs.items():
        setattr(E.RaftEngine, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(E.RaftEngine, k, v)


def cases():
    """[(name, model, engine keywords, class attributes, plan key, pipelined slot or None)]."""
    out = []

    def add(name, model, B, all_iters, suffix=(), kw=None, attrs=None, slot=None):
        out.append((name, model, dict(kw or {}), dict(attrs or {}), (B, H, W, ITERS, all_iters) + tuple(suffix), slot))

    od = dict(corr="on_demand")
    variants = [("cold", (), None, None), ("warm", ("warm",), None, None), ("bidir", ("bidir",), None, None),
                ("u8", U8, None, None), ("u8_bidir_warp", U8 + ("bidir", "warp"), None, None),
                ("ondemand", (), od, None), ("ondemand_warm", ("warm",), od, None), ("pslot", (), None, 0),
                ("u8_bidir_interp2", U8 + ("bidir", "interp", 2), None, None)]
    for model in FACTORIES:
        for B in (1, 2, 4):
            for all_iters in (True, False):
                for vname, suffix, kw, slot in variants:
                    add(f"{model}.b{B}.{'all' if all_iters else 'final'}.{vname}", model, B, all_iters, suffix, kw,
                        slot=slot)
    for gru in ("unfused", "halo", "fused"):
        for parity in (False, True):
            add(f"raft_large.b4.gru_{gru}.parity_{int(parity)}", "raft_large", 4, True,
                attrs=dict(GRU=gru, MASK_PARITY=parity))
    for model in FACTORIES:
        for attr, val in (("MERGED_UP", False), ("CONV_GROUP", False), ("PRO_LANES", "on"), ("PRO_LANES", "off"),
                          ("HALO_NORM", False)):
            add(f"{model}.b1.{attr}_{val}", model, 1, True, attrs={attr: val})
    add("raft_large.b4.split2.cold", "raft_large", 4, True, kw=dict(split=2))
    add("raft_large.b4.split2.warm", "raft_large", 4, True, ("warm",), kw=dict(split=2))
    add("raft_large.b2.all.cp", "raft_large", 2, True, kw=dict(cp_group=True))
    add("raft_small.b2.final.cp", "raft_small", 2, False, kw=dict(cp_group=True))
    add("raft_large.b4.streams_off", "raft_large", 4, True, kw=dict(streams=False))
    add("raft_large.b1.streams_on", "raft_large", 1, True, kw=dict(streams=True))
    # without autotuning no conv has a tile config a grouped launch serves: pin one, so that the
    # one-lane loop records the last correlation conv + convflow2 as one conv_group
    add("raft_large.b1.grouped", "raft_large", 1, True, kw=dict(cfg_override={"me.convcorr2": 2}))
    add("raft_small.b1.grouped", "raft_small", 1, True, kw=dict(cfg_override={"me.convcorr1": 2}))
    add("raft_large.b1.final.grouped", "raft_large", 1, False, kw=dict(cfg_override={"me.convcorr2": 2}))
    return out


class _Canon:
    """Canonical (JSON-able) form of op arguments; storages numbered by first appearance."""

    def __init__(self):
        self.storages = {}

    def __call__(self, v):
        if isinstance(v, torch.Tensor):
            sid = self.storages.setdefault(v.untyped_storage()._cdata, len(self.storages))
            return ["T", sid, v.storage_offset(), list(v.shape), list(v.stride()), str(v.dtype)]
        if isinstance(v, (list, tuple)):
            return [self(x) for x in v]
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        raise TypeError(f"plan_dump: cannot canonicalise {type(v).__name__}")


def canonical(eng, st):
    c = _Canon()
    parts = [[[seg, ln, d, op, c(args)] for seg, ln, d, op, args in plan.ops] for plan in st.plans]
    return dict(parts=parts,
                bufs=sorted((k, list(t.shape), str(t.dtype)) for k, t in st.bufs.items()),
                slot_ok=st.slot_ok,
                flow_out=c(st.flow_out),
                state={k: c(getattr(st, k)) for k in STATE_TENSORS},
                gru_path=eng.gru_path,
                corr_blocked=eng.corr_blocked)


_MODELS = {}


def _model(name):
    if name not in _MODELS:
        torch.manual_seed(0)
        _MODELS[name] = FACTORIES[name]()[0].eval()
    return _MODELS[name]


def run_case(case):
    """SHA-256 of the case's canonical plan state, or ``"raised: ..."``."""
    name, model, kw, attrs, key, slot = case
    try:
        with fake_native(), class_attrs(attrs):
            eng = E.RaftEngine(_model(model), "cpu", autotune=False, **kw)
            st = eng._build_key(key) if slot is None else eng._slot_state(key, slot)
            text = json.dumps(canonical(eng, st), sort_keys=True)
        return hashlib.sha256(text.encode()).hexdigest()
    except Exception as e:   # the text is the case's value: both trees must fail alike
        return f"raised: {type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default="plan_dump.json")
    ap.add_argument("--only", default="", help="run the cases whose name contains this")
    a = ap.parse_args()
    res = {c[0]: run_case(c) for c in cases() if a.only in c[0]}
    raised = sum(v.startswith("raised: ") for v in res.values())
    with open(a.out, "w") as f:
        json.dump(dict(cases=res, raised=raised), f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(res)} cases, {raised} raised -> {a.out}")
    return 1 if raised else 0


if __name__ == "__main__":
    sys.exit(main())
