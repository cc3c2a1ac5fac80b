"""CPU checks of the plan recording's layers (runtime/lowering.py): the choices as a pure function,
the choices kept per plan, builds that leave the engine alone, and tools/plan_dump.py."""
import dataclasses
import importlib.util
import pathlib

import pytest
import torch

from jax_raft_amd import raft_large, raft_small
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import lowering as L

_spec = importlib.util.spec_from_file_location(
    "plan_dump", pathlib.Path(__file__).resolve().parent.parent / "tools" / "plan_dump.py")
plan_dump = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(plan_dump)

h, w = 16, 32   # the feature maps of 128 x 256 frames


@pytest.fixture
def fake():
    with plan_dump.fake_native():
        yield


@pytest.fixture(scope="module")
def models():
    return {f: f()[0].eval() for f in (raft_large, raft_small)}


def _engine(models, factory=raft_large, **kw):
    return E.RaftEngine(models[factory], "cpu", autotune=False, **kw)


def _choose(eng, B, all_iters=True, Bi=None, **kw):
    lanes = (0, 1, 2) if eng.uses_lanes(B, all_iters, parts=1) else (0, 0, 0)
    return L.choose(eng, Bi or B, B, h, w, all_iters, lanes, **kw)


def test_choose_is_pure(fake, models, monkeypatch):
    """No plan, no allocation, nothing written to the engine."""
    eng = _engine(models)

    def boom(*a, **k):
        raise AssertionError("choose() must not allocate or touch a plan")

    before = dict(eng.__dict__)
    with monkeypatch.context() as m:
        for name in ("zeros", "empty", "tensor"):
            m.setattr(torch, name, boom)
        m.setattr(L.nat, "new_plan", boom)
        m.setattr(E.RaftEngine, "__setattr__", boom)
        cs = [_choose(eng, B, a, slot=s) for B in (1, 4) for a in (True, False) for s in (False, True)]
    assert {k: id(v) for k, v in eng.__dict__.items()} == {k: id(v) for k, v in before.items()}
    assert all(isinstance(c, L.PartChoices) for c in cs)
    with pytest.raises(dataclasses.FrozenInstanceError):
        cs[0].schedule = "final"


def test_schedules(fake, models):
    eng = _engine(models)
    assert _choose(eng, 4).schedule == "lanes"
    c = _choose(eng, 1)
    assert c.schedule == "one_lane" and c.merged_up and c.c1_merged
    assert _choose(eng, 1, all_iters=False).schedule == "final_merged"
    assert _choose(eng, 4, all_iters=False).schedule == "final"
    assert _choose(_engine(models, cp_group=True), 2).schedule == "cp"
    # a pipelined slot's plan differs in the pyramid kernel alone
    assert dataclasses.replace(_choose(eng, 1, slot=True), bl=2) == c and _choose(eng, 1, slot=True).bl == 1


def test_flags(fake, models, monkeypatch):
    eng, small = _engine(models), _engine(models, raft_small)
    monkeypatch.setattr(E.RaftEngine, "GRU", "fused")
    c = _choose(eng, 4)
    assert c.gru_path == "fused" and not c.parity and c.hm and c.mask_wait == 1
    monkeypatch.setattr(E.RaftEngine, "MASK_PARITY", True)
    c = _choose(eng, 4)
    assert c.parity and c.mask_wait is None
    monkeypatch.setattr(E.RaftEngine, "GRU", "halo")
    c = _choose(eng, 4)
    assert c.gru_path == "halo" and not c.parity and c.mask_wait == 1 and not c.halo_pp and not c.qx_x
    monkeypatch.setattr(E.RaftEngine, "GRU", "unfused")
    c = _choose(eng, 4)
    assert c.gru_path == "unfused" and not c.parity and c.mask_wait == 0 and c.qx_x and not c.hm
    monkeypatch.setattr(E.RaftEngine, "GRU", "auto")
    c = _choose(small, 1)
    assert c.gru_path == "halo" and c.halo_pp and c.qx_x and c.mask_wait is None


def test_bidirectional_takes_the_loop_batch(fake, models):
    """A bidirectional plan of 2 image pairs chooses as the batch-4 plan does, and records it."""
    eng = _engine(models)
    cb, c4 = _choose(eng, 4, Bi=2, bidir=True), _choose(eng, 4)
    assert dataclasses.replace(cb, bidir=False) == c4 and cb.schedule == "lanes"
    st = eng._build_bidir(2, 128, 256, 3, True, None)
    assert st.choices == [cb]


def test_choices_belong_to_the_plan(fake, models):
    eng = _engine(models)
    st4 = eng._build(4, 128, 256, 3)
    g4 = eng.gru_path
    st1 = eng._build(1, 128, 256, 3)
    assert [c.schedule for c in st4.choices] == ["lanes"] and [c.schedule for c in st1.choices] == ["one_lane"]
    assert st4.choices[0].gru_path == g4 and eng.gru_path == st1.choices[0].gru_path   # the engine's: the last build's
    assert eng.corr_blocked == bool(st1.choices[0].blocked)
    st = _engine(models, split=2)._build(4, 128, 256, 3)
    assert len(st.plans) == 2 and [c.schedule for c in st.choices] == ["one_lane"] * 2   # one entry per batch part


@pytest.mark.parametrize("suffix", [(), ("bidir",)])
def test_builds_write_nothing_but_the_last_plan_facts(fake, models, monkeypatch, suffix):
    """A pipelined slot's plan and a bidirectional plan are one part on an engine with split=2,
    and ``eng.split`` is not written at any moment of the build."""
    eng = _engine(models, split=2)
    key = (4, 128, 256, 3, True) + suffix
    written = []

    def spy(self, name, value):
        assert name != "split", "a build must not write eng.split"
        written.append(name)
        object.__setattr__(self, name, value)

    monkeypatch.setattr(E.RaftEngine, "__setattr__", spy)
    st = eng._slot_state(key, 0) if not suffix else eng._build_key(key)
    assert len(st.plans) == 1 and eng.split == 2
    assert set(written) <= {"gru_path", "corr_blocked"}
    if not suffix:   # ... recorded as a slot's plan: not the persistent pyramid kernel
        (corr,) = [a for *_, op, a in st.plan.ops if op == "corr"]
        assert corr[1][-1] == 1 and st.choices[0].bl == 1 and not hasattr(eng, "_slot_build")


@pytest.mark.parametrize("slot", [False, True])
def test_a_build_that_raises_leaves_the_engine_as_it_was(fake, models, monkeypatch, slot):
    class Failing(plan_dump.FakePlan):
        def add_corr(self, *a):
            raise RuntimeError("corr")

    eng = _engine(models, split=2)
    eng._build(1, 128, 256, 3)
    before = {k: id(v) for k, v in eng.__dict__.items()}
    states = dict(eng._states)
    monkeypatch.setattr(L.nat, "new_plan", Failing)
    key = (4, 128, 256, 3, True)
    with pytest.raises(RuntimeError, match="corr"):
        eng._slot_state(key, 0) if slot else eng._build_key(key)
    assert {k: id(v) for k, v in eng.__dict__.items()} == before and dict(eng._states) == states
    assert eng.split == 2 and not hasattr(eng, "_slot_build")


def test_recording_leaves_no_reference_cycle(fake, models):
    """An engine and its plans die by reference count (tests/test_lifecycle_gpu.py on the GPU):
    the recorder, which holds the engine, must not survive the build in a cycle of its own."""
    import gc
    import weakref

    gc.collect()
    gc.disable()
    try:
        eng = _engine(models)
        for B, all_iters in ((4, True), (1, True), (1, False)):
            eng._plan_state((B, 128, 256, 3, all_iters), lambda: eng._build(B, 128, 256, 3, all_iters))
        eng._build_bidir(1, 128, 256, 3, True, None)
        ref = weakref.ref(eng)
        del eng
        assert ref() is None, "the engine is held by a reference cycle"
    finally:
        gc.enable()


def test_plan_dump_smoke():
    names = ("raft_large.b4.all.cold", "raft_small.b1.final.pslot", "raft_large.b2.all.bidir")
    cases = [c for c in plan_dump.cases() if c[0] in names]
    assert len(cases) == 3
    first = [plan_dump.run_case(c) for c in cases]
    assert first == [plan_dump.run_case(c) for c in cases]
    assert len(set(first)) == 3 and all(len(v) == 64 for v in first)   # SHA-256 each: none raised
