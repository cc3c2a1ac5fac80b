"""The native binding surface (csrc/runtime/binding.cpp): every launch op is one row of the
op table, from which its eager op, its ``Plan.add_<op>`` method and its int-list arity check
are generated.  Needs the built library, but no GPU: only schemas and host checks are used.

``golden/binding_surface.json`` is the surface of the last build with hand-written
registrations (50 op schemas, 70 ``Plan`` methods): sorted ``str(schema)`` of every
``jax_raft_amd::*`` entry of ``torch._C._jit_get_all_schemas()``, and
``{n: str(p._get_method(n).schema) for n in p._method_names()}`` of a ``Plan``."""
import json
import os
import re

import pytest
import torch

from jax_raft_amd import raft_large, raft_small
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import tunedb
from test_engine_lowering import FakePlan

pytestmark = pytest.mark.skipif(not nat.available(), reason="native library not built")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_surface.json")
SIG_T, SIG_TI, SIG_TIA = 0, 1, 2
# Plan methods that record a conv through build_conv's own int-list check: op -> positions of int lists
CONV_FORMS = {"conv_alt": (1,), "conv_train": (1,), "conv_group": (1, 4)}


def _arity(name):
    return list(torch.ops.jax_raft_amd.op_arity(name))


def _op_schemas():
    return {s.name.split("::")[1]: str(s) for s in torch._C._jit_get_all_schemas() if s.name.startswith("jax_raft_amd::")}


def _table_ops():
    return sorted(n for n in _op_schemas() if _arity(n))


def test_surface_is_preserved():
    want = json.load(open(GOLDEN))
    assert len(want["ops"]) == 50 and len(want["plan_methods"]) == 70
    have = _op_schemas()
    for schema in want["ops"]:
        assert schema in have.values(), schema
    p = torch.classes.jax_raft_amd.Plan()
    methods = {n: str(p._get_method(n).schema) for n in p._method_names()}
    for n, schema in want["plan_methods"].items():
        assert methods.get(n) == schema, n
    # what is new: op_arity, and the form a table op had only one of
    for n in set(have) - {s.split("::")[1].split("(")[0] for s in want["ops"]}:
        assert n == "op_arity" or _arity(n), n
    for n in set(methods) - set(want["plan_methods"]):
        assert n.startswith("add_") and _arity(n[4:]), n
    # both forms of every table op, with the table's signature class
    assert _arity("no_such_op") == [] and len(_table_ops()) >= 40
    for n in _table_ops():
        sig = _arity(n)[0]
        args = have[n].split("(", 1)[1]
        assert args.count(",") == sig and args.startswith("Tensor?[] t") and ("int[] i" in args) == (sig >= SIG_TI), have[n]
        assert methods["add_" + n].count(",") == sig + 1, n


def test_arity_is_checked_first():
    """One int too few / too many fails in the generated check, before any tensor check
    (the tensor list is [None]): host code only, nothing is launched."""
    ops = [n for n in _table_ops() if _arity(n)[0] != SIG_T]
    assert len(ops) >= 40
    for n in ops:
        sig, lo, hi = _arity(n)
        assert 1 <= lo <= hi, n
        expected = str(lo) if lo == hi else f"{lo}..{hi}"
        for k in (lo - 1, hi + 1):
            args = ([None], [0] * k) + ((1.0,) if sig == SIG_TIA else ())
            with pytest.raises(RuntimeError, match=rf"{n}: expected {re.escape(expected)} ints, got {k}\b"):
                getattr(torch.ops.jax_raft_amd, n)(*args)
            with pytest.raises(RuntimeError, match=rf"{n}: expected {re.escape(expected)} ints, got {k}\b"):
                getattr(torch.classes.jax_raft_amd.Plan(), "add_" + n)(*args)


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(nat, "require", lambda: None)
    monkeypatch.setattr(nat, "new_plan", FakePlan)
    monkeypatch.setattr(tunedb, "gpu_arch", lambda device=None: "cpu")


LOWERINGS = {
    "large_b4_lanes": (raft_large, 4, {}, {}),
    "large_b1": (raft_large, 1, {}, {}),
    "small_b1": (raft_small, 1, {}, {}),
    "final_only": (raft_large, 4, {}, dict(all_iters=False)),
    "warm": (raft_large, 1, {}, dict(warm=True)),
    "fp32": (raft_small, 1, dict(precision="fp32"), {}),
}


@pytest.mark.parametrize("case", sorted(LOWERINGS))
def test_lowerings_stay_inside_the_table(fake, case):
    """Every int list the engines record has a length the table accepts (this is what checks
    the table's max_ints against the real call sites without a GPU)."""
    factory, B, eng_kw, build_kw = LOWERINGS[case]
    eng = E.RaftEngine(factory()[0].eval(), "cpu", autotune=False, **eng_kw)
    plan = eng._build(B, 128, 256, 3, build_kw.pop("all_iters", True), **build_kw).plan
    if case == "large_b4_lanes":
        assert eng.uses_lanes(4)
    seen = set()
    for _, _, _, op, args in plan.ops:
        if op in ("record", "wait"):
            continue
        seen.add(op)
        sig, lo, hi = _arity("conv" if op in CONV_FORMS else op)   # an op without a row: ValueError
        for pos in CONV_FORMS.get(op, (1,) if sig >= SIG_TI else ()):
            assert lo <= len(args[pos]) <= hi, (op, len(args[pos]), lo, hi)
    assert len(seen) >= 8, seen
    if case == "warm":
        assert "init_flow" in seen
    if case == "fp32":
        assert "conv_f32" in seen and "lookup_f32" in seen
