"""Warm start on the CPU: the golden forward projection (models/reference.py:
forward_project), the golden model's ``flow_init`` / ``return_flow_low``, and the
lowering of warm plans (a recording stand-in for the native Plan).  The HIP
kernels and the engines are covered on the GPU by tests/test_warm_start_gpu.py."""
import math

import numpy as np
import pytest
import torch

from jax_raft_amd import raft_large, raft_small
from jax_raft_amd.models import reference as R
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime import engine as E
from jax_raft_amd.runtime import tunedb

OFF = 100.0   # a flow that leaves any small map


# --------------------------------------------------------------- forward_project
def _scalar_project(flow: np.ndarray, radius: int) -> np.ndarray:
    """The definition cell by cell in numpy fp32 / Python ints (independent of the vectorised golden)."""
    f32 = np.float32
    B, h, w, _ = flow.shape
    out = np.zeros_like(flow)
    offs = sorted(((dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)),
                  key=lambda o: (o[0] ** 2 + o[1] ** 2, o[0], o[1]))
    for b in range(B):
        best = {}
        for y in range(h):
            for x in range(w):
                fx, fy = flow[b, y, x]
                x1, y1 = f32(x) + fx, f32(y) + fy
                tx, ty = np.floor(x1 + f32(0.5)), np.floor(y1 + f32(0.5))
                if not (0 <= tx <= w - 1 and 0 <= ty <= h - 1):
                    continue
                ix = int(np.rint((x1 - tx) * f32(256)))
                iy = int(np.rint((y1 - ty) * f32(256)))
                key = ((ix * ix + iy * iy) << 32) | (y * w + x)
                c = (int(ty), int(tx))
                if c not in best or key < best[c]:
                    best[c] = key
        for y in range(h):
            for x in range(w):
                for dy, dx in offs:
                    k = best.get((y + dy, x + dx))
                    if k is not None:
                        s = k & 0xFFFFFFFF
                        out[b, y, x] = flow[b, s // w, s % w]
                        break
    return out


def test_project_zero_flow_is_zero():
    z = torch.zeros(2, 16, 32, 2)
    assert torch.equal(R.forward_project(z), z)


def test_project_constant_integer_flow_reproduces_itself():
    f = torch.zeros(1, 16, 32, 2)
    f[..., 0], f[..., 1] = 3.0, -2.0
    out = R.forward_project(f, fill_radius=0)
    # defined where a source lands: x in [3, 32), y in [0, 14)
    assert torch.equal(out[:, :14, 3:], f[:, :14, 3:])
    assert torch.equal(out[:, 14:], torch.zeros_like(out[:, 14:])) and torch.equal(out[:, :, :3], torch.zeros_like(out[:, :, :3]))
    assert torch.equal(R.forward_project(f, fill_radius=4), f)   # the border holes filled from the hit cells


def _hand_case():
    """4 x 5 map, every source off-frame except two pairs that collide."""
    f = torch.full((1, 4, 5, 2), OFF)
    f[0, 0, 0] = torch.tensor([2.2, 1.0])      # lands (2.2, 1.0) -> cell (y 1, x 2), 51/256 away
    f[0, 3, 4] = torch.tensor([-1.9, -2.0])    # lands (2.1, 1.0) -> the same cell, 26/256 away: nearer, higher index
    f[0, 0, 1] = torch.tensor([2.25, 2.0])     # lands (3.25, 2.0) -> cell (y 2, x 3), 64/256 away
    f[0, 3, 3] = torch.tensor([-0.25, -1.0])   # lands (2.75, 2.0) -> the same cell, 64/256 away: exact tie
    f[0, 2, 2] = torch.tensor([float("nan"), 0.0])
    f[0, 1, 1] = torch.tensor([0.0, float("inf")])
    return f


def test_project_collisions_nearest_then_lower_index():
    f = _hand_case()
    out = R.forward_project(f, fill_radius=0)
    want = torch.zeros_like(f)
    want[0, 1, 2] = f[0, 3, 4]    # the nearer landing wins although its source index is higher
    want[0, 2, 3] = f[0, 0, 1]    # exact tie: the lower source index
    # ... and the off-frame, NaN and inf sources leave no trace anywhere
    assert torch.equal(out, want)


def test_project_hole_filling_order_and_radius():
    f = _hand_case()
    out = R.forward_project(f, fill_radius=1)
    a, b = f[0, 3, 4], f[0, 0, 1]            # the values of the hit cells (1, 2) and (2, 3)
    assert torch.equal(out[0, 0, 0], torch.zeros(2)) and torch.equal(out[0, 3, 0], torch.zeros(2))   # outside the radius
    assert torch.equal(out[0, 3, 4], b)      # only (2, 3) in reach
    # equidistant from both hit cells: (dy, dx) = (0, -1) comes before (1, 0) ...
    assert torch.equal(out[0, 1, 3], a)
    # ... and (-1, 0) before (0, 1)
    assert torch.equal(out[0, 2, 2], a)
    assert torch.isfinite(out).all()
    # holes are filled from hit cells only: with radius 1 the corner (0, 0) stays empty although
    # its neighbour (1, 1) was filled; radius 2 reaches the hit cell (1, 2) itself
    assert torch.equal(out[0, 1, 1], a)
    assert torch.equal(R.forward_project(f, fill_radius=2)[0, 0, 0], a)


@pytest.mark.parametrize("radius", [0, 2, 4])
def test_project_matches_cell_by_cell_definition(radius):
    g = torch.Generator().manual_seed(7)
    f = (torch.rand(2, 9, 11, 2, generator=g) - 0.5) * 8
    f[0, 2:5, 3:6] = torch.tensor([3.0, 2.5])     # an occluding patch
    f[1, 0:3, 0:3] = torch.tensor([-6.0, -6.0])   # a patch leaving the frame
    f[1, 4, 4, 0] = float("nan")
    out = R.forward_project(f, fill_radius=radius)
    assert np.array_equal(out.numpy(), _scalar_project(f.numpy(), radius))


def test_fill_offsets_order():
    o = R.fill_offsets(4)
    assert len(o) == 81 and o[0] == (0, 0) and o[1:5] == [(-1, 0), (0, -1), (0, 1), (1, 0)]
    assert [dy * dy + dx * dx for dy, dx in o] == sorted(dy * dy + dx * dx for dy, dx in o)


def test_front_end_runs_the_golden_op_on_cpu_tensors():
    f = _hand_case()
    assert torch.equal(nat.forward_project(f, 1), R.forward_project(f, 1))


# ------------------------------------------------------------------ golden model
def _images(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(B, H + 8, W + 8, 3, generator=g) * 2 - 1
    return base[:, 4:4 + H, 4:4 + W].contiguous(), base[:, 2:2 + H, 6:6 + W].contiguous()


@pytest.fixture(scope="module", params=[raft_small, raft_large], ids=["raft_small", "raft_large"])
def golden(request):
    model, _ = request.param()
    i1, i2 = _images(1, 128, 160)
    with torch.no_grad():
        cold = model(i1, i2, num_flow_updates=2)
    return model, i1, i2, cold


def test_golden_zero_init_equals_cold(golden):
    model, i1, i2, cold = golden
    with torch.no_grad():
        warm, low = model(i1, i2, num_flow_updates=2, flow_init=torch.zeros(1, 16, 20, 2), return_flow_low=True)
    assert torch.equal(warm, cold)
    assert low.shape == (1, 16, 20, 2)
    if model.mask_predictor is None:   # bilinear x8: the last flow is the low-resolution flow upsampled
        assert torch.equal(warm[-1], R.upsample_flow(low, None))


def test_golden_nonzero_init_changes_the_output(golden):
    model, i1, i2, cold = golden
    init = torch.zeros(1, 16, 20, 2)
    init[..., 0] = 1.5
    with torch.no_grad():
        warm = model(i1, i2, num_flow_updates=2, flow_init=init)
        via_apply = model.apply(model.variables(), i1, i2, num_flow_updates=2, flow_init=init)
    assert warm.shape == cold.shape and torch.isfinite(warm).all()
    assert (warm - cold).abs().max().item() > 1.0
    assert torch.equal(via_apply, warm)


def test_golden_guards(golden):
    model, i1, i2, _ = golden
    with pytest.raises(ValueError, match=r"\(1, 16, 20, 2\)"):
        model(i1, i2, num_flow_updates=2, flow_init=torch.zeros(1, 20, 16, 2))
    with pytest.raises(NotImplementedError):
        model(i1, i2, train=True, num_flow_updates=2, flow_init=torch.zeros(1, 16, 20, 2))
    with pytest.raises(ValueError):
        model(i1, i2, num_flow_updates=2, flow_init="previous")   # a mode of the native engine


def test_golden_u8_frames_use_the_padded_size():
    """uint8 frames of any size: flow_init / flow_low are at the padded size / 8."""
    model, _ = raft_small()
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, 256, (1, 122, 130, 3), generator=g, dtype=torch.uint8)
    b = torch.randint(0, 256, (1, 122, 130, 3), generator=g, dtype=torch.uint8)
    with torch.no_grad():
        cold = model(a, b, num_flow_updates=1)
        warm, low = model(a, b, num_flow_updates=1, flow_init=torch.zeros(1, 16, 17, 2), return_flow_low=True)
        with pytest.raises(ValueError, match=r"\(1, 16, 17, 2\)"):
            model(a, b, num_flow_updates=1, flow_init=torch.zeros(1, 15, 16, 2))
    assert low.shape == (1, math.ceil(122 / 8), math.ceil(130 / 8), 2)
    assert warm.shape == (1, 1, 122, 130, 2) and torch.equal(warm, cold)


# ---------------------------------------------------------------------- lowering
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


def _build(factory, B, warm, **kw):
    eng = E.RaftEngine(factory()[0].eval(), "cpu", autotune=False, **kw)
    return eng, eng._build(B, 128, 256, 3, True, warm=warm)


@pytest.mark.parametrize("factory,B", [(raft_large, 4), (raft_small, 1), (raft_large, 1)])
def test_warm_plan_seeds_instead_of_init_coords(rec, factory, B):
    eng, cold = _build(factory, B, warm=False)
    _, warm = _build(factory, B, warm=True)
    assert eng.uses_lanes(B) == (factory is raft_large and B == 4)
    c, w_ = cold.plan.names(), warm.plan.names()
    # a cold plan is what it was: init_coords, no seed, no flow_init buffer
    assert c.count("init_coords") == 1 and "init_flow" not in c and cold.flow_init is None
    # a warm plan differs in exactly that one op, in the prologue
    assert w_.count("init_flow") == 1 and "init_coords" not in w_
    assert [("init_coords" if op == "init_flow" else op) for op in w_] == c
    assert "init_flow" in warm.plan.names(0)
    seed = [a for _, _, op, a in warm.plan.ops if op == "init_flow"][0]
    t, i = seed
    assert t[0].data_ptr() == warm.flow_init.data_ptr() and tuple(warm.flow_init.shape) == (B, 16, 32, 2)
    assert i == [B, 16, 32, eng.flow_off, eng.flow_off]
    # both plans expose their final-flow buffers (return_flow_low / "previous")
    assert len(cold.flow_out) == len(warm.flow_out) == 1 and warm.flow_out[0][:2] == (0, B)


def test_lane_schedule_seed_precedes_iteration0_flow_features(rec):
    """The seed runs on the context lane before E_CTX is recorded; the main lane waits for E_CTX
    before the prologue's flow features of iteration 0 (conv_direct over flow8) -- and the seed
    comes after the memsets of the buffers it writes (E_PREP, recorded after them)."""
    eng, st = _build(raft_large, 4, warm=True)
    pro = [(ln, op, a) for s, ln, op, a in st.plan.ops if s == 0]
    idx = {op: [k for k, (_, o, _) in enumerate(pro) if o == op] for op in ("init_flow", "conv_direct", "memset")}
    (k_seed,), (k_cd,) = idx["init_flow"], idx["conv_direct"]
    ln_seed, ln_main = pro[k_seed][0], pro[k_cd][0]
    assert ln_seed != ln_main and ln_main == 0
    E_PREP, E_CTX = 0, 1
    rec_ctx = [k for k, (ln, op, a) in enumerate(pro) if op == "record" and a == (E_CTX,) and ln == ln_seed]
    wait_ctx = [k for k, (ln, op, a) in enumerate(pro) if op == "wait" and a == (E_CTX,) and ln == ln_main]
    assert len(rec_ctx) == 1 and len(wait_ctx) == 1
    assert k_seed < rec_ctx[0] and wait_ctx[0] < k_cd
    rec_prep = [k for k, (ln, op, a) in enumerate(pro) if op == "record" and a == (E_PREP,)][0]
    wait_prep = [k for k, (ln, op, a) in enumerate(pro) if op == "wait" and a == (E_PREP,) and ln == ln_seed][0]
    assert max(idx["memset"]) < rec_prep and all(pro[k][0] == ln_main for k in idx["memset"])
    assert wait_prep < k_seed


def test_split_parts_seed_their_own_batch_slice(rec):
    eng, st = _build(raft_large, 4, warm=True, split=2)
    assert len(st.plans) == 2 and [f[:2] for f in st.flow_out] == [(0, 2), (2, 2)]
    for part, plan in enumerate(st.plans):
        (t, i), = [a for _, _, op, a in plan.ops if op == "init_flow"]
        assert i[0] == 2 and t[0].data_ptr() == st.flow_init[2 * part:].data_ptr()


def test_flow_low_takes_the_buffer_of_the_last_iteration():
    """Parity-buffered flow (MASK_PARITY): the last update runs at launch index n_iters and writes
    the odd-iteration buffer when that is odd; parts are assembled in batch order."""
    even, odd = torch.zeros(2 * 6, 2), torch.ones(2 * 6, 2)
    parts = [(0, 2, even, odd), (2, 2, even + 2, None)]
    lo = E.RaftEngine._flow_low(parts, 3, 2, 3)
    assert lo.shape == (4, 2, 3, 2) and torch.equal(lo[:2], odd.view(2, 2, 3, 2)) and (lo[2:] == 2).all()
    assert torch.equal(E.RaftEngine._flow_low(parts, 4, 2, 3)[:2], even.view(2, 2, 3, 2))
    one = E.RaftEngine._flow_low(parts[:1], 4, 2, 3)
    assert torch.equal(one, even.view(2, 2, 3, 2)) and one.data_ptr() != even.data_ptr()   # a copy


def test_plan_keys_group_and_build(rec):
    """The "warm" key element: a group of its own for the LRU, stripped before the build."""
    eng = E.RaftEngine(raft_small()[0].eval(), "cpu", autotune=False)
    i = torch.zeros(1, 128, 256, 3)
    key = eng._key(i, i, 3, True)
    wkey = key + ("warm",)
    assert eng._group(wkey) == wkey != eng._group(key)
    assert eng._build_key(wkey).flow_init is not None and eng._build_key(key).flow_init is None
    u8 = torch.zeros(1, 122, 250, 3, dtype=torch.uint8)
    ukey = eng._key(u8, u8, 3, True) + ("warm",)
    st = eng._build_key(ukey)
    assert st.src == (122, 250, 3, 3) and tuple(st.flow_init.shape) == (1, 16, 32, 2)
    eng.max_plans = 1
    eng._plan_state(key, lambda: eng._build_key(key))
    eng._plan_state(wkey, lambda: eng._build_key(wkey))
    assert list(eng._states) == [wkey]
