"""Bidirectional flow + forward-backward occlusion masks on the GPU: the fb_check kernel
(csrc/kernels/fbcheck.hip) bitwise against the golden op, its maker's argument checks, and the
engine's bidirectional plan against the golden model, its own masks, replays and cold plans."""
import functools

import pytest
import torch

from jax_raft_amd import BidirectionalFlow, fb_consistency, raft_large, raft_small
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime.engine import RaftEngine
from test_engine_gpu import REL_EPE, _epe, _inputs

pytestmark = pytest.mark.gpu

FACTORIES = {"raft_small": raft_small, "raft_large": raft_large}


# --------------------------------------------------------------------- kernel
def _smooth_pair(B, H, W, window=None, seed=0):
    """Seeded smooth flows of up to ~6 px (a coarse random field upsampled), roughly opposite, with
    planted pixels: integer landings, landings exactly on the last row / column of the frame,
    just outside it, and NaNs."""
    g = torch.Generator().manual_seed(seed)
    H0, W0, top, left = window or (H, W, 0, 0)

    def field(scale):
        c = (torch.rand(B, 2, 3, 4, generator=g) * 2 - 1) * scale
        return torch.nn.functional.interpolate(c, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)

    fw = field(6.0).contiguous()
    bw = (-fw + field(1.5)).contiguous()
    y, x = top + min(3, H0 - 1), left + min(2, W0 - 1)      # a frame pixel, map coordinates
    fy, fx = y - top, x - left                               # ... frame coordinates
    fw[0, y, x] = torch.tensor([2.0, 1.0])                                   # lands on an integer,
    bw[0, y + 1, x + 2] = torch.tensor([-2.0, -1.0])                         # ... consistently: err == 0
    fw[0, y, x + 1] = torch.tensor([float(W0 - 1 - (fx + 1)), 0.0])          # exactly the last column
    fw[0, y + 1, x] = torch.tensor([0.0, float(H0 - 1 - (fy + 1))])          # exactly the last row
    fw[0, y + 1, x + 1] = torch.tensor([float(W0 - 1 - (fx + 1)) + 2.0 ** -10, 0.0])   # just outside
    bw[0, y, x] = torch.tensor([-float(fx) - 2.0 ** -10, 0.0])               # just outside, to the left
    fw[-1, y + 2, x] = float("nan")                                          # a NaN landing point
    bw[-1, y + 2, x + 1, 1] = float("nan")
    fw[-1, y + 2, x + 1] = 0.0                                               # ... and a gathered NaN
    return fw, bw


KERNEL_CASES = {
    "b1_8x8": (1, 8, 8, None),
    "b2_24x40": (2, 24, 40, None),
    "b2_24x40_window": (2, 24, 40, (21, 37, 1, 2)),
    "b1_16x264": (1, 16, 264, None),     # a row spans several wavefronts
}


@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
def test_kernel_equals_golden_bitwise(case):
    B, H, W, window = KERNEL_CASES[case]
    fw, bw = _smooth_pair(B, H, W, window)
    want = fb_consistency(fw, bw, 0.01, 0.5, window, return_err=True)
    # the planted pixels exercise what they are meant to
    assert want[0].any() and not want[0].all() and torch.isinf(want[2]).any() and torch.isnan(want[2]).any()
    dfw, dbw = fw.cuda(), bw.cuda()
    got = nat.fb_check(dfw, dbw, 0.01, 0.5, window, return_err=True)
    again = nat.fb_check(dfw, dbw, 0.01, 0.5, window, return_err=True)
    masks_only = nat.fb_check(dfw, dbw, 0.01, 0.5, window)
    torch.cuda.synchronize()
    for g_, a_, w_ in zip(got, again, want):
        assert g_.dtype == w_.dtype and g_.shape == w_.shape
        assert torch.equal(g_.cpu().nan_to_num(nan=-1.0), w_.nan_to_num(nan=-1.0))
        assert torch.equal(g_.nan_to_num(nan=-1.0), a_.nan_to_num(nan=-1.0))
    assert torch.equal(masks_only[0], got[0]) and torch.equal(masks_only[1], got[1])


def test_kernel_same_buffers_twice_and_other_thresholds():
    B, H, W = 2, 24, 40
    fw, bw = _smooth_pair(B, H, W, seed=4)
    dfw, dbw = fw.cuda(), bw.cuda()
    occ = torch.zeros(2, B, H, W, dtype=torch.uint8, device="cuda")
    err = torch.zeros(2, B, H, W, dtype=torch.float32, device="cuda")
    thr = torch.tensor([0.05, 0.125], dtype=torch.float32, device="cuda")
    args = ([dfw, dbw, occ, err, thr], [B, H, W, H, W, 0, 0])
    nat.ops().fb_check(*args)
    o1, e1 = occ.clone(), err.clone()
    nat.ops().fb_check(*args)
    torch.cuda.synchronize()
    assert torch.equal(o1, occ) and torch.equal(e1.nan_to_num(nan=-1.0), err.nan_to_num(nan=-1.0))
    want = fb_consistency(fw, bw, 0.05, 0.125, return_err=True)
    assert torch.equal(occ.cpu().bool(), torch.stack(want[:2]))
    assert torch.equal(err.cpu().nan_to_num(nan=-1.0), torch.stack(want[2:]).nan_to_num(nan=-1.0))
    assert int(occ.max()) == 1


def test_maker_checks():
    B, H, W = 1, 8, 16
    dev = "cuda"
    fw = torch.zeros(B, H, W, 2, device=dev)
    bw = torch.zeros(B, H, W, 2, device=dev)
    occ = torch.zeros(2, B, H, W, dtype=torch.uint8, device=dev)
    thr = torch.tensor([0.01, 0.5], device=dev)
    ints = [B, H, W, H, W, 0, 0]
    op = nat.ops().fb_check

    def rejected(t, i=ints):
        with pytest.raises(RuntimeError, match="fb_check"):
            op(t, i)

    rejected([fw.half(), bw, occ, None, thr])                                   # dtype of a flow
    rejected([fw, bw, occ.float(), None, thr])                                  # dtype of occ
    rejected([fw, bw, occ, None, thr.double()])                                 # dtype of thr
    big = torch.zeros(B * H * W * 2 + 2, device=dev)
    rejected([big[2:].view(B, H, W, 2), bw, occ, None, thr])                    # 8-byte aligned only
    wide = torch.zeros(B, H, 2 * W, 2, device=dev)
    rejected([wide[:, :, :W], bw, occ, None, thr])                              # not contiguous
    alias = fw.view(torch.uint8).view(-1)[: 2 * B * H * W].view(2, B, H, W)
    rejected([fw, bw, alias, None, thr])                                        # occ aliases a flow
    rejected([fw, bw, occ, bw.view(-1)[: 2 * B * H * W].view(2, B, H, W), thr])  # err aliases a flow
    rejected([fw, bw, occ, None, thr], [B, H, W, H, W, 1, 0])                   # window below the map
    rejected([fw, bw, occ, None, thr], [B, H, W, H, W + 1, 0, 0])               # window wider than the map
    rejected([fw, bw, occ, None, thr], [B, H, W, 0, W, 0, 0])                   # empty window
    torch.cuda.synchronize()
    op([fw, bw, occ, None, thr], ints)                                          # the valid call runs
    torch.cuda.synchronize()
    assert not occ.any()


# --------------------------------------------------------------------- engine
@functools.lru_cache(maxsize=None)
def _golden(name, B, W, iters=4):
    """(model, i1, i2, golden flows 1 -> 2, golden flows 2 -> 1), computed once per configuration
    on the CPU and left unchanged."""
    torch.manual_seed(0)
    model, variables = FACTORIES[name]()
    i1, i2 = _inputs(B, 128, W)
    fw = model.apply(variables, i1, i2, train=False, num_flow_updates=iters)
    bw = model.apply(variables, i2, i1, train=False, num_flow_updates=iters)
    return model, i1, i2, fw, bw


def _gpu_model(name):
    """A fresh model on the GPU (the factories seed their own generator: the golden model's weights)."""
    return FACTORIES[name]()[0].cuda()


@pytest.mark.parametrize("name", ["raft_small", "raft_large"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B,W", [(1, 160), (1, 256), (2, 256)])
def test_engine_matches_golden_both_ways(name, use_graph, B, W):
    """Loop batch 2 (one lane) and 4 (raft_large: the lane schedule), row-major and blocked pyramids."""
    iters = 4
    _, i1, i2, ref_fw, ref_bw = _golden(name, B, W)
    model = _gpu_model(name)
    res = model(i1.cuda(), i2.cuda(), num_flow_updates=iters, use_graph=use_graph, bidirectional=True)
    torch.cuda.synchronize()
    assert isinstance(res, BidirectionalFlow)
    assert res.occ_fw.shape == res.occ_bw.shape == (B, 128, W) and res.occ_fw.dtype == torch.bool
    for got, ref, tag in ((res.flows_fw, ref_fw, "fw"), (res.flows_bw, ref_bw, "bw")):
        assert got.shape == ref.shape == (iters, B, 128, W, 2)
        assert torch.isfinite(got).all()
        got = got.cpu()
        mag = ref.norm(dim=-1).mean().item()
        for it in range(iters):
            e = _epe(got[it], ref[it])
            print(f"{name} graph={use_graph} B={B} W={W} {tag} it={it} epe={e:.6f} mag={mag:.6f} rel={e / mag:.4f}")
            assert e < REL_EPE[name] * mag, (tag, it, e, mag)


@pytest.mark.parametrize("name", ["raft_small", "raft_large"])
@pytest.mark.parametrize("copy_output", [True, False])
def test_masks_belong_to_the_returned_flows(name, copy_output):
    """The epilogue's check read the final flows where this replay wrote them (the output slot:
    a fresh tensor per call with copy_output, the plan's buffer without)."""
    model = _gpu_model(name)
    eng = RaftEngine(model, torch.device("cuda"), use_graph=True, copy_output=copy_output)
    for seed, final_only in ((1, False), (2, False), (3, True)):
        i1, i2 = (t.cuda() for t in _inputs(1, 128, 256, seed=seed))
        res = eng.forward(i1, i2, 3, return_all_iters=not final_only, bidirectional=True)
        assert res.flows_fw.shape == (1 if final_only else 3, 1, 128, 256, 2)
        occ_fw, occ_bw, err_fw, _ = nat.fb_check(res.flows_fw[-1], res.flows_bw[-1], 0.01, 0.5, return_err=True)
        torch.cuda.synchronize()
        assert torch.equal(res.occ_fw, occ_fw) and torch.equal(res.occ_bw, occ_bw)
        want = fb_consistency(res.flows_fw[-1].cpu(), res.flows_bw[-1].cpu())
        assert torch.equal(occ_fw.cpu(), want[0]) and torch.equal(occ_bw.cpu(), want[1])
        # random weights give flows that are nowhere consistent at UnFlow's thresholds: a second
        # call (the same plan) at the median error of this pair splits the pixels into both classes
        beta = float(err_fw[torch.isfinite(err_fw)].median())
        res = eng.forward(i1, i2, 3, return_all_iters=not final_only, bidirectional=True, fb_alpha=0.0, fb_beta=beta)
        occ_fw, occ_bw = nat.fb_check(res.flows_fw[-1], res.flows_bw[-1], 0.0, beta)
        torch.cuda.synchronize()
        assert torch.equal(res.occ_fw, occ_fw) and torch.equal(res.occ_bw, occ_bw)
        assert 0.2 < res.occ_fw.float().mean().item() < 0.8
    assert eng.num_plans() == 2


def test_replay_is_bitwise_and_thresholds_do_not_rebuild():
    model = _gpu_model("raft_large")
    eng = RaftEngine(model, torch.device("cuda"), use_graph=True)
    i1, i2 = (t.cuda() for t in _inputs(2, 128, 256, seed=7))     # loop batch 4: the lane schedule
    a = eng.forward(i1, i2, 3, bidirectional=True)
    b = eng.forward(i1, i2, 3, bidirectional=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert a.flows_fw.data_ptr() != b.flows_fw.data_ptr() and a.occ_fw.data_ptr() != b.occ_fw.data_ptr()
    plans = eng.num_plans()
    # alpha = beta = 0: everything that is not exactly consistent is occluded; a huge beta: only
    # the pixels that land outside the frame
    sums = []
    for beta in (0.0, 1e12):
        c = eng.forward(i1, i2, 3, bidirectional=True, fb_alpha=0.0, fb_beta=beta)
        torch.cuda.synchronize()
        assert eng.num_plans() == plans == 1
        assert torch.equal(c.flows_fw, a.flows_fw) and torch.equal(c.flows_bw, a.flows_bw)
        want = nat.fb_check(c.flows_fw[-1], c.flows_bw[-1], 0.0, beta)
        assert torch.equal(c.occ_fw, want[0]) and torch.equal(c.occ_bw, want[1])
        sums.append(int(c.occ_fw.sum()))
    assert sums[0] > sums[1]
    d = eng.forward(i1, i2, 3, bidirectional=True)
    torch.cuda.synchronize()
    assert eng.num_plans() == plans and all(torch.equal(x, y) for x, y in zip(a, d))


def test_uint8_frames():
    """Frames of 122 x 150 run at the padded 128 x 152 (the smallest map the pyramid takes is
    128 pixels a side); everything is returned at the frame size, and the masks are the golden
    op's with the frame window on the uncropped flows."""
    model = _gpu_model("raft_small")
    g = torch.Generator().manual_seed(11)
    base = torch.randint(0, 256, (1, 130, 158, 3), generator=g, dtype=torch.uint8)
    f1, f2 = base[:, 4:126, 4:154].contiguous(), base[:, 2:124, 6:156].contiguous()
    eng = RaftEngine(model, torch.device("cuda"), use_graph=True, copy_output=False)
    res = eng.forward(f1, f2, 3, bidirectional=True)
    torch.cuda.synchronize()
    assert res.flows_fw.shape == res.flows_bw.shape == (3, 1, 122, 150, 2)
    assert res.occ_fw.shape == res.occ_bw.shape == (1, 122, 150)
    (st,) = eng._states.values()
    assert st.src == (122, 150, 3, 1) and tuple(st.out.shape) == (3, 2, 128, 152, 2)
    full = st.out[-1].cpu()
    want = fb_consistency(full[:1].contiguous(), full[1:].contiguous(), window=st.src)
    assert torch.equal(res.occ_fw.cpu(), want[0][:, 3:125, 1:151]) and torch.equal(res.occ_bw.cpu(), want[1][:, 3:125, 1:151])
    assert not want[0][:, :3].any() and not want[0][:, :, :1].any()
    assert torch.equal(res.flows_fw.cpu(), st.out[:, :1, 3:125, 1:151].cpu())
    # the same through the model's front door
    res2 = model(f1, f2, num_flow_updates=3, bidirectional=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(res, res2))


def test_cold_call_after_a_bidirectional_one():
    model = _gpu_model("raft_small")
    eng = RaftEngine(model, torch.device("cuda"), use_graph=True)
    i1, i2 = (t.cuda() for t in _inputs(1, 128, 256, seed=9))
    cold = eng.forward(i1, i2, 3)
    res = eng.forward(i1, i2, 3, bidirectional=True)
    with pytest.raises(ValueError, match="previous"):
        eng.forward(i1, i2, 3, flow_init="previous")
    again = eng.forward(i1, i2, 3)
    warm = eng.forward(i1, i2, 3, flow_init="previous")   # seeds from the cold call
    torch.cuda.synchronize()
    assert torch.equal(cold, again) and torch.isfinite(warm).all()
    assert res.flows_fw.shape == cold.shape
