"""Motion-compensated frames + masked photometric error on the GPU: the warp_frames kernel
(csrc/kernels/framewarp.hip) bitwise against the golden op (models/reference.py:warp_frames), its
maker's argument checks, and the engine's "warp" plan against the plain bidirectional plan, the
kernel and the golden op applied to the flows and masks it returns."""
import functools

import pytest
import torch

from jax_raft_amd import BidirectionalFlow, BidirectionalWarp, raft_large, raft_small, warp_frames
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime.engine import RaftEngine

pytestmark = pytest.mark.gpu

FACTORIES = {"raft_small": raft_small, "raft_large": raft_large}

# (B, H, W, window): an odd left, a tail of 2 pixels and a row pitch that is no multiple of 4; the
# 32-bit store path ((W0 * 3) % 4 == 0) over the whole map; fewer pixels than a block, a tail-only row
KERNEL_CASES = {
    "window_122x150": (2, 128, 152, (122, 150, 3, 1)),
    "rows4_120x152": (2, 120, 152, None),
    "tiny_9x5": (2, 9, 5, None),
}


def _flow(B, H, W, window, seed):
    """Seeded flows over the map: random sub-pixel values of a few pixels, rows of exact half-pixel
    offsets (ties on odd texel differences), far-outside landings, and planted pixels: landings
    exactly on the last column / row of the frame, just outside it, NaNs."""
    g = torch.Generator().manual_seed(seed)
    H0, W0, top, left = window or (H, W, 0, 0)
    f = torch.randn(B, H, W, 2, generator=g) * 2.5
    f[:, top::3, :, 0], f[:, top::3, :, 1] = 0.5, 0.0              # x + 0.5 (the last column lands outside)
    f[:, top + 1::6, :, 0], f[:, top + 1::6, :, 1] = -1.0, 0.5     # y + 0.5
    far = torch.rand(B, H, W, generator=g) < 0.05
    f[far] = f[far] * 1e4
    y, x = top + min(2, H0 - 1), left + min(1, W0 - 1)              # a frame pixel, map coordinates
    fy, fx = y - top, x - left
    f[0, y, x] = torch.tensor([float(W0 - 1 - fx), 0.0])                       # exactly the last column
    f[0, y, x + 1] = torch.tensor([0.0, float(H0 - 1 - fy)])                   # exactly the last row
    f[0, y + 1, x] = torch.tensor([float(W0 - 1 - fx) + 2.0 ** -10, 0.0])      # just outside
    f[0, y + 1, x + 1] = torch.tensor([-float(fx + 1) - 2.0 ** -10, 0.0])      # just outside, to the left
    f[0, y + 2, x] = torch.tensor([-float(fx), -float(fy + 2)])                # exactly the first column and row
    f[-1, y + 2, x + 1] = float("nan")
    f[-1, y + 3, x, 1] = float("nan")
    f[-1, y + 3, x + 1] = torch.tensor([float("inf"), 0.0])
    return f


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs of both directions and the golden results of every variant, computed once on the CPU
    and left unchanged: {(with_occ, with_own): [(warped, photo) per direction]}."""
    B, H, W, window = KERNEL_CASES[name]
    H0, W0, top, left = window or (H, W, 0, 0)
    g = torch.Generator().manual_seed(len(name))
    frames = [torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, generator=g) for _ in range(2)]
    flows = [_flow(B, H, W, window, seed) for seed in (1, 2)]
    occ = torch.rand(2, B, H, W, generator=g) < 0.3
    src, own = [frames[1], frames[0]], [frames[0], frames[1]]
    want = {}
    for with_occ in (False, True):
        for with_own in (False, True):
            want[with_occ, with_own] = [warp_frames(src[d], flows[d], occ[d] if with_occ else None,
                                                    own[d] if with_own else None, window) for d in range(2)]
    return dict(B=B, H=H, W=W, win=list(window or (H, W, 0, 0)), window=window, src=src, own=own, flows=flows, occ=occ,
                want=want)


def _run_op(c, dirs, with_occ, with_own, flows=None, occ=None):
    """The op itself (not the front-end) on fresh output buffers: (warped, photo) on the device."""
    B, (H0, W0) = c["B"], c["win"][:2]
    dev = "cuda"
    flows = c["flows"] if flows is None else flows
    occ = c["occ"].to(torch.uint8) if occ is None else occ
    t = [c["src"][0].to(dev), c["src"][1].to(dev) if dirs == 2 else None,
         c["own"][0].to(dev) if with_own else None, c["own"][1].to(dev) if with_own and dirs == 2 else None,
         flows[0].to(dev), flows[1].to(dev) if dirs == 2 else None,
         occ[:dirs].contiguous().to(dev) if with_occ else None]
    warped = torch.full((dirs, B, H0, W0, 3), 77, dtype=torch.uint8, device=dev)
    photo = torch.zeros((dirs, B, 2), dtype=torch.int64, device=dev) if with_own else None
    nat.ops().warp_frames(t + [warped, photo], [B, c["H"], c["W"]] + c["win"] + [dirs])
    return warped, photo


# --------------------------------------------------------------------- kernel
@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("with_occ", [False, True])
@pytest.mark.parametrize("with_own", [False, True])
def test_kernel_equals_golden_bitwise(case, dirs, with_occ, with_own):
    c = _case(case)
    B, (H0, W0) = c["B"], c["win"][:2]
    want = c["want"][with_occ, with_own]
    # every case holds kept and masked pixels (the counts of the variant with own)
    for d in range(dirs):
        cnt = c["want"][with_occ, True][d][1][:, 1]
        assert (cnt > 0).all() and (cnt < H0 * W0).all(), cnt
    warped, photo = _run_op(c, dirs, with_occ, with_own)
    torch.cuda.synchronize()
    for d in range(dirs):
        assert torch.equal(warped[d].cpu(), want[d][0]), (case, d)
        if with_own:
            assert torch.equal(photo[d].cpu(), want[d][1]), (photo[d].cpu(), want[d][1])
            assert int(want[d][1][:, 0].min()) > 0
    assert with_own or photo is None
    # the front-end: one direction, fresh tensors
    dev = "cuda"
    got = nat.warp_frames(c["src"][0].to(dev), c["flows"][0].to(dev), c["occ"][0].to(dev) if with_occ else None,
                          c["own"][0].to(dev) if with_own else None, c["window"])
    torch.cuda.synchronize()
    assert got[0].dtype == torch.uint8 and got[0].shape == (B, H0, W0, 3) and torch.equal(got[0].cpu(), want[0][0])
    if with_own:
        assert got[1].dtype == torch.int64 and torch.equal(got[1].cpu(), want[0][1])
    else:
        assert got[1] is None


def test_nothing_outside_the_window_is_read():
    c = _case("window_122x150")
    H0, W0, top, left = c["win"]
    inside = torch.zeros(c["H"], c["W"], dtype=torch.bool)
    inside[top:top + H0, left:left + W0] = True
    res = []
    for fill_f, fill_m in ((0.0, 0), (float("nan"), 0xFF)):
        flows = [f.clone() for f in c["flows"]]
        occ = c["occ"].to(torch.uint8)
        for f in flows:
            f[:, ~inside] = fill_f
        occ[:, :, ~inside] = fill_m
        res.append(_run_op(c, 2, True, True, flows, occ))
    torch.cuda.synchronize()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    want = c["want"][True, True]
    assert torch.equal(res[1][0].cpu(), torch.stack([want[0][0], want[1][0]]))
    assert torch.equal(res[1][1].cpu(), torch.stack([want[0][1], want[1][1]]))


def test_same_buffers_twice_and_no_accumulation():
    c = _case("window_122x150")
    dev = "cuda"
    B, (H0, W0) = c["B"], c["win"][:2]
    t = [c["src"][0].to(dev), c["src"][1].to(dev), c["own"][0].to(dev), c["own"][1].to(dev), c["flows"][0].to(dev),
         c["flows"][1].to(dev), c["occ"].to(torch.uint8).to(dev)]
    warped = torch.zeros((2, B, H0, W0, 3), dtype=torch.uint8, device=dev)
    photo = torch.zeros((2, B, 2), dtype=torch.int64, device=dev)
    ints = [B, c["H"], c["W"]] + c["win"] + [2]
    nat.ops().warp_frames(t + [warped, photo], ints)
    w1, p1 = warped.clone(), photo.clone()
    photo.zero_()          # the op adds to the sums: a plan clears them with its memset op
    nat.ops().warp_frames(t + [warped, photo], ints)
    torch.cuda.synchronize()
    assert torch.equal(w1, warped) and torch.equal(p1, photo)
    # the front-end clears its own sums: two calls, the same sums
    args = (t[0], t[4], c["occ"][0].to(dev), t[2], c["window"])
    a, b = nat.warp_frames(*args), nat.warp_frames(*args)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[1], p1[0])
    assert a[0].data_ptr() != b[0].data_ptr() and a[1].data_ptr() != b[1].data_ptr()


def test_maker_checks():
    B, H, W = 1, 8, 16
    dev = "cuda"
    s0, s1, o0, o1 = (torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(4))
    f0, f1 = torch.zeros(B, H, W, 2, device=dev), torch.zeros(B, H, W, 2, device=dev)
    occ = torch.zeros(2, B, H, W, dtype=torch.uint8, device=dev)
    warped = torch.full((2, B, H, W, 3), 9, dtype=torch.uint8, device=dev)
    photo = torch.zeros(2, B, 2, dtype=torch.int64, device=dev)
    slot = torch.zeros(1, dtype=torch.int64, device=dev)
    ints = [B, H, W, H, W, 0, 0, 2]
    good = [s0, s1, o0, o1, f0, f1, occ, warped, photo]
    op = nat.ops().warp_frames

    def rejected(t, i=ints, **put):
        t = list(t)
        for k, v in put.items():
            t[int(k[1:])] = v
        with pytest.raises(RuntimeError, match="warp_frames"):
            op(t, i)

    rejected(good, _0=s0.float())                                                # dtype of a frame
    rejected(good, _2=o0.to(torch.int8))                                         # dtype of own
    rejected(good, _4=f0.half())                                                 # dtype of a flow
    rejected(good, _6=occ.bool())                                                # dtype of occ
    rejected(good, _7=warped.to(torch.int8))                                     # dtype of warped
    rejected(good, _8=photo.int())                                               # dtype of photo
    wide = torch.zeros(B, H, 2 * W, 3, dtype=torch.uint8, device=dev)
    rejected(good, _1=wide[:, :, :W])                                            # a frame that is not contiguous
    rejected(good, _5=torch.zeros(B, H, 2 * W, 2, device=dev)[:, :, :W])         # a flow that is not contiguous
    rejected(good, _0=s0.cpu())                                                  # a host frame
    rejected(good, _4=f0.cpu())                                                  # a host flow
    rejected(good, _0=torch.zeros(B, H, W + 1, 3, dtype=torch.uint8, device=dev))   # frame shape
    rejected(good, _3=torch.zeros(B, H - 1, W, 3, dtype=torch.uint8, device=dev))   # own shape
    rejected(good, _7=warped[:1])                                                # one direction's output for two
    rejected(good, _6=occ[:1])                                                   # one direction's masks for two
    rejected(good, _8=photo[:1])                                                 # one direction's sums for two
    rejected(good, _2=None, _3=None)                                             # photo without own
    rejected(good, _3=None)                                                      # own of one direction only
    rejected(good, [B, H, W, H, W, 1, 0, 2])                                     # window below the map
    rejected(good, [B, H, W, H, W + 1, 0, 0, 2])                                 # window wider than the map
    rejected(good, [B, H, W, 0, W, 0, 0, 2])                                     # empty window
    rejected(good, [B, H, W, H, W, 0, 0, 0])                                     # dirs
    rejected(good, [B, H, W, H, W, 0, 0, 3])
    rejected(good, [B, H, W, H, W, 0, 0, 1])                                     # one direction, two directions' tensors
    big = torch.zeros(B * H * W * 2 + 1, device=dev)
    rejected(good, _4=big[1:].view(B, H, W, 2))                                  # a flow at 4 bytes
    rejected(good, _7=torch.zeros(2, B, H, 2 * W, 3, dtype=torch.uint8, device=dev)[:, :, :, :W])   # warped not contiguous
    both = torch.zeros(3, B, H, W, 3, dtype=torch.uint8, device=dev)
    rejected(good, _0=both[0], _7=both[:2])                                      # warped aliases a frame
    rejected(good, _2=both[2], _3=both[1], _7=both[:2])                          # warped aliases own
    rejected(good, _6=both.view(-1)[:2 * B * H * W].view(2, B, H, W), _7=both[:2])   # warped aliases occ
    al = torch.zeros(B * H * W * 2 + 16, device=dev)
    rejected(good, _4=al[:B * H * W * 2].view(B, H, W, 2), _8=al[:8].view(torch.int64).view(2, B, 2))   # photo aliases a flow
    rejected(good + [slot], ints + [0, 2 * B * H * W])                           # the slot form takes no flow tensors
    rejected(good + [slot], _4=None, _5=None)                                    # ... and two offsets
    rejected(good + [slot], ints + [0, 1], _4=None, _5=None)                     # ... 8-byte aligned
    rejected(good + [slot.int()], ints + [0, 2 * B * H * W], _4=None, _5=None)   # dtype of the slot
    rejected(good, ints + [0, 2 * B * H * W])                                    # offsets without a slot
    torch.cuda.synchronize()
    assert bool((warped == 9).all()) and not photo.any()                        # nothing was launched
    op(good, ints)                                                               # the valid call runs
    op([s0, None, o0, None, f0, None, occ[:1], warped[:1], photo[:1]], [B, H, W, H, W, 0, 0, 1])
    torch.cuda.synchronize()
    assert not warped.any() and photo[:, :, 0].tolist() == [[0], [0]] and photo[:, :, 1].tolist() == [[2 * H * W], [H * W]]
    for bad in ((s0, f0.double()), (s0.float(), f0), (s0[:, 1:], f0), (s0.cpu(), f0)):
        with pytest.raises(ValueError, match="warp_frames"):
            nat.warp_frames(*bad)


# --------------------------------------------------------------------- engine
def _frames(B, seed):
    """uint8 frames 122 x 150 (run at the padded 128 x 152, window (122, 150, 3, 1)): two crops of one
    smooth random image, a few pixels apart."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 3, 18, 22, generator=g)
    big = torch.nn.functional.interpolate(coarse, size=(130, 158), mode="bicubic", align_corners=True)
    big = (big.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
    return big[:, 4:126, 4:154].contiguous().cuda(), big[:, 2:124, 6:156].contiguous().cuda()


def _check_against_own_flows(res, f1, f2):
    """warped_* and photo are bitwise the kernel's and the golden op's on the returned flows and masks."""
    assert isinstance(res, BidirectionalWarp)
    B = f1.shape[0]
    assert res.warped_fw.shape == res.warped_bw.shape == (B, 122, 150, 3) and res.warped_fw.dtype == torch.uint8
    assert res.photo.shape == (2, B, 2) and res.photo.dtype == torch.int64
    for d, (src, own, flow, occ, warped) in enumerate(((f2, f1, res.flows_fw[-1], res.occ_fw, res.warped_fw),
                                                        (f1, f2, res.flows_bw[-1], res.occ_bw, res.warped_bw))):
        kw, kp = nat.warp_frames(src, flow, occ, own)
        gw, gp = warp_frames(src.cpu(), flow.cpu().contiguous(), occ.cpu(), own.cpu())
        assert torch.equal(warped, kw) and torch.equal(res.photo[d], kp)
        assert torch.equal(warped.cpu(), gw) and torch.equal(res.photo[d].cpu(), gp)


@pytest.mark.parametrize("name", ["raft_small", "raft_large"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B", [1, 2])
def test_engine_warp_plan(name, use_graph, B):
    model = FACTORIES[name]()[0].cuda()
    dev = torch.device("cuda")
    eng = RaftEngine(model, dev, use_graph=use_graph)
    f1, f2 = _frames(B, seed=1)
    res = eng.forward(f1, f2, 3, bidirectional=True, warp=True)
    plain = eng.forward(f1, f2, 3, bidirectional=True)
    torch.cuda.synchronize()
    assert isinstance(plain, BidirectionalFlow) and eng.num_plans() == 2
    assert res.flows_fw.shape == (3, B, 122, 150, 2) and res.occ_fw.shape == (B, 122, 150)
    assert all(torch.equal(a, b) for a, b in zip(res[:4], plain))
    _check_against_own_flows(res, f1, f2)
    # thresholds that keep every pixel landing inside: the comparison is not vacuous
    loose = eng.forward(f1, f2, 3, bidirectional=True, warp=True, fb_alpha=0.0, fb_beta=1e6)
    torch.cuda.synchronize()
    assert eng.num_plans() == 2
    assert torch.equal(loose.flows_fw, res.flows_fw) and torch.equal(loose.flows_bw, res.flows_bw)
    assert (loose.photo[:, :, 1] > 0).all() and (loose.photo[:, :, 1] >= res.photo[:, :, 1]).all()
    _check_against_own_flows(loose, f1, f2)
    # a second replay with other frames is consistent with its own flows (the slot is read at run time)
    g1, g2 = _frames(B, seed=2)
    other = eng.forward(g1, g2, 3, return_all_iters=True, bidirectional=True, warp=True, fb_alpha=0.0, fb_beta=1e6)
    torch.cuda.synchronize()
    assert not torch.equal(other.flows_fw, res.flows_fw) and not torch.equal(other.warped_fw, loose.warped_fw)
    assert other.warped_fw.data_ptr() != loose.warped_fw.data_ptr() and other.photo.data_ptr() != loose.photo.data_ptr()
    _check_against_own_flows(other, g1, g2)
    # a plain bidirectional call and a cold call afterwards equal what they return on a fresh engine
    plain2 = eng.forward(f1, f2, 3, bidirectional=True)
    cold = eng.forward(f1, f2, 3)
    fresh = RaftEngine(model, dev, use_graph=use_graph)
    plain_fresh = fresh.forward(f1, f2, 3, bidirectional=True)
    cold_fresh = fresh.forward(f1, f2, 3)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(plain2, plain_fresh)) and all(torch.equal(a, b) for a, b in zip(plain2, plain))
    assert torch.equal(cold, cold_fresh)


def test_final_only_and_the_model_front_door():
    model = raft_small()[0].cuda()
    f1, f2 = _frames(1, seed=3)
    res = model(f1, f2, num_flow_updates=3, return_all_iters=False, bidirectional=True, warp=True, fb_alpha=0.0, fb_beta=1e6)
    torch.cuda.synchronize()
    assert res.flows_fw.shape == (1, 1, 122, 150, 2) and (res.photo[:, :, 1] > 0).all()
    _check_against_own_flows(res, f1, f2)
    # host frames go the same way
    res2 = model(f1.cpu(), f2.cpu(), num_flow_updates=3, return_all_iters=False, bidirectional=True, warp=True,
                 fb_alpha=0.0, fb_beta=1e6)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(res, res2))
    with pytest.raises(ValueError, match="uint8"):
        model(torch.zeros(1, 128, 128, 3, device="cuda"), torch.zeros(1, 128, 128, 3, device="cuda"), bidirectional=True,
              warp=True)
    with pytest.raises(ValueError, match="bidirectional=True"):
        model(f1, f2, warp=True)


def test_warp_call_does_not_synchronise():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    model = raft_small()[0].cuda()
    eng = RaftEngine(model, torch.device("cuda"), use_graph=True)
    f1, f2 = _frames(1, seed=4)
    for _ in range(2):     # warm: the plan, its capture, allocator blocks, the thresholds
        eng.forward(f1, f2, 3, bidirectional=True, warp=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = eng.forward(f1, f2, 3, bidirectional=True, warp=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _check_against_own_flows(res, f1, f2)
