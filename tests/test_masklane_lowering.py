"""Lowering of the fused flow features (``RaftEngine.FLOW_FUSED``, op ``flow_features_fused``): plan
recording on CPU tensors, as tests/test_warm_start.py does it.  The fusion changes the mask lane's
flow-feature launches and the ``f1`` buffer, nothing else of a plan, and "auto" takes it only on
lane-schedule plans whose tiles fill the GPU."""
import pytest

from jax_raft_amd import raft_large, raft_small
from jax_raft_amd.models.layers import MaskPredictor
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import tunedb
from jax_raft_amd.runtime.lowering import E_FH, E_FLOW, E_MASK

# the plan of raft_large, batch 4, 128 x 256, 3 iterations (autotune off) as it was before the fusion existed:
# (segment, lane, ops in order; "op*n" = n times in a row)
OFF_PLAN = [
    (0, 0, 'memset*4 prep record'),
    (0, 1, 'wait conv*16 copy_channels conv*2 init_coords record'),
    (0, 2, 'wait conv stats conv stats_final conv stats_final conv stats_final conv stats_final norm_act conv stats '
           'conv stats_final conv stats conv stats_final conv stats_final norm_act conv stats conv stats_final conv '
           'stats conv stats_final conv stats_final norm_act conv record'),
    (0, 0, 'conv stats conv stats_final conv stats_final conv stats_final conv stats_final norm_act conv stats conv '
           'stats_final conv stats conv stats_final conv stats_final norm_act conv stats conv stats_final conv stats '
           'conv stats_final conv stats_final norm_act conv wait corr wait conv_direct conv'),
    (1, 0, 'lookup record'),
    (1, 2, 'wait conv_direct conv record conv convex_head record'),
    (1, 0, 'conv1x1 conv wait conv gru_halo wait gru_halo conv'),
    (2, 0, 'flow_taps conv convex_head'),
]
OFF_NAMES = [(s, ln, op) for s, ln, run in OFF_PLAN for item in run.split()
             for op in [item.split("*")[0]] * int((item.split("*") + ["1"])[1])]


class RecPlan:
    """Records (segment, lane, op, args) of every add_* call of a plan build."""

    def __init__(self):
        self.ops, self.seg, self.ln = [], 0, 0

    def set_segment(self, s):
        self.seg = s

    def set_lane(self, l):
        self.ln = l

    def set_defer(self, d):
        pass

    def __getattr__(self, name):
        if not name.startswith("add_"):
            raise AttributeError(name)
        return lambda *args: self.ops.append((self.seg, self.ln, name[4:], args))

    def names(self, seg=None):
        return [op for s, _, op, _ in self.ops if seg is None or s == seg]


@pytest.fixture
def rec(monkeypatch):
    monkeypatch.setattr(nat, "require", lambda: None)
    monkeypatch.setattr(nat, "new_plan", RecPlan)
    monkeypatch.setattr(tunedb, "gpu_arch", lambda device=None: "cpu")


def _build(monkeypatch, knob, factory=raft_large, B=4, H=128, W=256, all_iters=True, model=None, **kw):
    monkeypatch.setattr(E.RaftEngine, "FLOW_FUSED", knob)
    eng = E.RaftEngine(model if model is not None else factory()[0].eval(), "cpu", autotune=False, **kw)
    return eng, eng._build(B, H, W, 3, all_iters)


def _lane(plan, lane, seg=1):
    """(op, args) of one lane's loop segment; records / waits as ("record", (event,))."""
    return [(op, a) for s, ln, op, a in plan.ops if s == seg and ln == lane]


def _shape(ops):
    return [(op, a) if op in ("record", "wait") else op for op, a in ops]


def test_on_fuses_the_mask_lanes_flow_features_and_nothing_else(rec, monkeypatch):
    eng_on, on = _build(monkeypatch, "on")
    eng_off, off = _build(monkeypatch, "off")
    assert on.choices[0].schedule == "lanes" and on.choices[0].flow_fused and not off.choices[0].flow_fused
    main, _, side = on.choices[0].lanes
    # the mask lane: one launch between the E_FH wait and the E_FLOW record, then the mask head as before
    assert _shape(_lane(on.plan, side)) == [("wait", (E_FH,)), "flow_features_fused", ("record", (E_FLOW,)), "conv",
                                            "convex_head", ("record", (E_MASK,))]
    assert _shape(_lane(off.plan, side)) == [("wait", (E_FH,)), "conv_direct", "conv", ("record", (E_FLOW,)), "conv",
                                             "convex_head", ("record", (E_MASK,))]
    # the main lane: the same ops, the three waits / records where they were
    assert _shape(_lane(on.plan, main)) == _shape(_lane(off.plan, main))
    assert [x for x in _shape(_lane(on.plan, main)) if isinstance(x, tuple)] == [
        ("record", (E_FH,)), ("wait", (E_FLOW,)), ("wait", (E_MASK,))]
    # the prologue's iteration-0 flow features come from the same emitter; the epilogue is unchanged
    pro_on, pro_off = on.plan.names(0), off.plan.names(0)
    assert pro_on.count("flow_features_fused") == 1 and "conv_direct" not in pro_on
    k = pro_off.index("conv_direct")
    assert pro_off[k + 1] == "conv" and pro_on == pro_off[:k] + ["flow_features_fused"] + pro_off[k + 2:]
    assert on.plan.names(2) == off.plan.names(2)
    # operands: flow8, the 7x7 conv's packed weights, convflow2's halo stream, the cf slice
    (t, i), = [a for s, _, op, a in on.plan.ops if op == "flow_features_fused" and s == 1]
    sp2 = eng_on._specs["me.convflow2"]
    assert t[0].shape == (4 * 16 * 32, 2) and t[1] is eng_on._cf1_w and t[3] is sp2.wh and t[4] is sp2.b
    assert t[5] is on.bufs["p0.cf"] and i == [4, 16, 32, eng_on.model.update_block.motion_encoder.corr_layers[-1]]
    # no f1 buffer
    assert "p0.f1" in off.bufs and "p0.f1" not in on.bufs
    assert set(off.bufs) - set(on.bufs) == {"p0.f1"}


def test_off_is_the_plan_from_before(rec, monkeypatch):
    _, off = _build(monkeypatch, "off")
    assert [(s, ln, op) for s, ln, op, _ in off.plan.ops] == OFF_NAMES


def test_auto_needs_the_lane_schedule_the_shapes_and_enough_tiles(rec, monkeypatch):
    fused = lambda st: [c.flow_fused for c in st.choices]
    # 128 x 256 at batch 4: 16 tiles of 8 x 16 -- lanes, but far from filling the GPU
    assert fused(_build(monkeypatch, "auto")[1]) == [False]
    # the benchmark's shape: 4 x 7 x 8 = 224 tiles >= 192
    eng, st = _build(monkeypatch, "auto", H=440, W=1024)
    assert st.choices[0].schedule == "lanes" and fused(st) == [True] and nat.flow_fused_tiles(4, 55, 128) == 224
    assert "flow_features_fused" in st.plan.names(1) and "p0.f1" not in st.bufs
    # ... and never: raft_small, batch 1, final-only plans, context parallelism, an injected mask predictor's
    # one-lane plan -- under "auto" and under "on" alike where there is no lane schedule
    for knob in ("auto", "on"):
        assert fused(_build(monkeypatch, knob, factory=raft_small, H=440, W=1024)[1]) == [False]
        assert fused(_build(monkeypatch, knob, B=1, H=440, W=1024)[1]) == [False]
        assert fused(_build(monkeypatch, knob, H=440, W=1024, all_iters=False)[1]) == [False]
        assert fused(_build(monkeypatch, knob, B=2, cp_group=True)[1]) == [False]
    model = raft_large()[0].eval()
    model.mask_predictor = MaskPredictor(in_channels=128, hidden_size=64)
    eng, st = _build(monkeypatch, "auto", model=model, H=440, W=1024)
    assert eng._convex_w is None
    # (the flow features do not depend on the mask head: an injected predictor keeps the lane schedule's
    # choice; the plan's mask head is the generic one)
    assert "convex_head" not in st.plan.names(1)
    assert fused(st) == [st.choices[0].schedule == "lanes"]
