"""Frame interpolation by forward splatting on the GPU: the interp_splat / interp_resolve kernels
(csrc/kernels/interp.hip) bitwise against the golden op (models/reference.py:interpolate_frames),
the accumulator included; their makers' argument checks; and the engine's "interp" plan against the
plain bidirectional plan, the kernels and the golden op applied to the flows and masks it returns."""
import functools

import pytest
import torch

from jax_raft_amd import BidirectionalFlow, BidirectionalInterp, interpolate_frames, raft_large, raft_small
from jax_raft_amd.models import reference as R
from jax_raft_amd.ops import native as nat
from jax_raft_amd.runtime.engine import RaftEngine

pytestmark = pytest.mark.gpu

FACTORIES = {"raft_small": raft_small, "raft_large": raft_large}
NAN, INF = float("nan"), float("inf")
TQS = (1, 77, 128, 255)

# (B, H, W, window): an odd left and a row tail; fewer pixels than a block; several blocks per row
# range; every source of both directions on one cell
KERNEL_CASES = {
    "window_122x150": (2, 128, 152, (122, 150, 3, 1)),
    "tiny_9x5": (2, 9, 5, None),
    "wide_40x300": (1, 40, 300, None),
    "contention_16x16": (2, 16, 16, None),
}
TARGET = (7, 9)   # the contention case's cell (y, x)


def _flow(B, H, W, window, seed):
    """Seeded flows over the map, laid out for tq = 128 (both steps are 1/2, so a flow of 2 d moves a
    pixel by d exactly): sub-pixel noise; rows of exact 1/32 ties of the 1/16 quantisation (at
    tq = 128 along x, at a step of 1/256 along y); 5 % far outside; a planted block whose flows
    diverge, so that nothing lands inside it, but for its centre pixel, which stays; and in the last
    two rows of the frame landings exactly on and just outside the border, NaNs and an inf."""
    g = torch.Generator().manual_seed(seed)
    H0, W0, top, left = window or (H, W, 0, 0)
    f = (torch.rand(B, H, W, 2, generator=g) - 0.5) * 1.8            # |f| < 0.9: a source reaches adjacent cells only
    f[:, top::3, :, 0] = 2.0 / 32                                    # x + 1/32 at tq = 128: a tie
    f[:, top + 1::6, :, 1] = 8.0                                     # y + 1/32 at a step of 1/256: a tie (4 rows at 128)
    far = torch.rand(B, H, W, generator=g) < 0.05
    f[far] = torch.where(torch.rand(int(far.sum()), 2, generator=g) < 0.5, -1e6, 1e6)
    # the diverging block: rows by0 .. by0+bh-1, columns bx0 .. bx0+bw-1 of the frame
    bh, bw = min(6, H0 - 3), min(6, W0 - 2)
    by0, bx0 = (H0 - 2 - bh) // 2, (W0 - bw) // 2
    ys = torch.arange(bh).view(bh, 1).expand(bh, bw)
    xs = torch.arange(bw).view(1, bw).expand(bh, bw)
    blk = f[:, top + by0:top + by0 + bh, left + bx0:left + bx0 + bw]
    blk[..., 0] = torch.where(xs < bw / 2, -3000.0, 3000.0)
    blk[..., 1] = torch.where(ys < bh / 2, -3000.0, 3000.0)
    blk[:, bh // 2, bw // 2] = 0.0                                   # the centre stays: its cell is fed by it alone
    y, x = top + H0 - 1, left                                        # the frame's last row, map coordinates
    f[:, y, x] = torch.tensor([2.0 * (W0 - 1), 0.0])                 # exactly on the last column
    f[:, y, x + 1] = torch.tensor([2.0 * (W0 - 1), 0.0])             # px == W0 exactly: outside
    f[:, y, x + 2] = torch.tensor([-6.0, 0.0])                       # px == -1 exactly: outside
    f[:, y, x + 3] = torch.tensor([2.0 * (-4 + 2.0 ** -10), 0.0])    # just inside -1: a sliver that quantises to 0
    f[:, y - 1, x] = NAN
    f[:, y - 1, x + 1] = torch.tensor([0.0, NAN])
    f[:, y - 1, x + 2] = torch.tensor([INF, 0.0])
    f[:, y - 1, x + 3] = torch.tensor([0.0, 2.0 * (2 - 2.0 ** -10)])  # py just below H0: only the tap outside has weight
    return f, (by0 + bh // 2, bx0 + bw // 2)


def _contention_flow(B, H, W, step):
    """Every pixel lands on TARGET under the step ``step / 256`` (up to the rounding of the product,
    which the 1/16 quantisation absorbs: the whole weight goes to one tap)."""
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1).expand(B, H, W)
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W).expand(B, H, W)
    return (torch.stack([TARGET[1] - xs, TARGET[0] - ys], -1) * 256.0 / float(step)).contiguous()


@functools.lru_cache(maxsize=None)
def _case(name, tq):
    """Inputs and the golden results with and without masks, computed once on the CPU and left
    unchanged: {with_occ: (frame_t, holes, acc)}.  Before anything is launched the golden result
    must hold holes, non-holes, cells fed only by occluded sources and cells fed by both kinds: a
    case that does not is a broken test, not a pass."""
    B, H, W, window = KERNEL_CASES[name]
    H0, W0, top, left = window or (H, W, 0, 0)
    g = torch.Generator().manual_seed(len(name))
    frames = [torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, generator=g) for _ in range(2)]
    occ = torch.rand(2, B, H, W, generator=g) < 0.3
    if name.startswith("contention"):
        flows = [_contention_flow(B, H, W, tq), _contention_flow(B, H, W, 256 - tq)]
        occ[:, -1] = True                        # the last sample's cell is fed by occluded sources only
    else:
        (f0, c), (f1, _) = _flow(B, H, W, window, 1), _flow(B, H, W, window, 2)
        flows = [f0, f1]
        occ[:, :, top + c[0], left + c[1]] = True   # the block's centre pixel, in both directions
    t = tq / 256.0
    want = {w: interpolate_frames(frames[0], frames[1], flows[0], flows[1], t, occ[0] if w else None, occ[1] if w else None,
                                  window, return_acc=True) for w in (False, True)}
    for w in (False, True):
        holes = want[w][1]
        assert 0 < int(holes.sum()) < holes.numel(), (name, tq, w)
    # acc.w = w_occ + 16 w_con with the masks and 16 (w_occ + w_con) without them
    w_occ = (want[False][2][..., 0] - want[True][2][..., 0]) // 15
    w_con = want[False][2][..., 0] // 16 - w_occ
    assert bool(((w_occ > 0) & (w_con == 0)).any()) and bool(((w_occ > 0) & (w_con > 0)).any()), (name, tq)
    if name.startswith("contention"):
        hit = want[False][2][..., 0] != 0
        assert int(hit.sum()) == 2 * B and bool(hit[:, :, TARGET[0], TARGET[1]].all())
        assert int(want[False][2][0, 0, TARGET[0], TARGET[1], 0]) == 256 * 16 * H * W
    return dict(B=B, H=H, W=W, win=list(window or (H, W, 0, 0)), window=window, frames=frames, flows=flows, occ=occ,
                want=want, t=t, par=[tq, R.interp_params(t)[1]])


def _run_ops(c, with_occ, flows=None, occ=None, bufs=None):
    """The two ops themselves (not the front end) after the clear: (frame_t, holes, acc) on the device."""
    B, (H0, W0) = c["B"], c["win"][:2]
    dev = "cuda"
    flows = c["flows"] if flows is None else flows
    occ = c["occ"].to(torch.uint8) if occ is None else occ
    f1, f2 = c["frames"][0].to(dev), c["frames"][1].to(dev)
    par = torch.tensor([[0, 0], c["par"]], dtype=torch.int32, device=dev)      # row 1 is the one in use
    if bufs is None:
        bufs = (torch.full((B, H0, W0, 3), 77, dtype=torch.uint8, device=dev),
                torch.full((B, H0, W0), 77, dtype=torch.uint8, device=dev),
                torch.full((2, B, H0, W0, 4), 77, dtype=torch.int64, device=dev))
    out, holes, acc = bufs
    acc.zero_()
    nat.ops().interp_splat([f1, f2, flows[0].to(dev), flows[1].to(dev), occ.to(dev) if with_occ else None, acc, par],
                           [B, c["H"], c["W"]] + c["win"] + [1])
    nat.ops().interp_resolve([f1, f2, acc, par, out, holes], [B, H0, W0, 1])
    return out, holes, acc


# --------------------------------------------------------------------- kernels
@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
@pytest.mark.parametrize("tq", TQS)
@pytest.mark.parametrize("with_occ", [False, True])
def test_kernels_equal_golden_bitwise(case, tq, with_occ):
    c = _case(case, tq)
    B, (H0, W0) = c["B"], c["win"][:2]
    frame_t, holes, acc = c["want"][with_occ]
    out, hol, a = _run_ops(c, with_occ)
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), acc), (case, tq)
    assert torch.equal(hol.cpu(), holes.to(torch.uint8)), (case, tq)
    assert torch.equal(out.cpu(), frame_t), (case, tq)
    # the front end: fresh tensors, one time and a sequence
    dev = "cuda"
    args = (c["frames"][0].to(dev), c["frames"][1].to(dev), c["flows"][0].to(dev), c["flows"][1].to(dev))
    masks = (c["occ"][0].to(dev), c["occ"][1].to(dev)) if with_occ else (None, None)
    got = nat.interpolate_frames(*args, c["t"], *masks, c["window"])
    seq = nat.interpolate_frames(*args, [0.5, c["t"]], *masks, c["window"])
    torch.cuda.synchronize()
    assert got[0].dtype == torch.uint8 and got[0].shape == (B, H0, W0, 3) and torch.equal(got[0].cpu(), frame_t)
    assert got[1].dtype == torch.bool and got[1].shape == (B, H0, W0) and torch.equal(got[1].cpu(), holes)
    assert seq[0].shape == (2, B, H0, W0, 3) and seq[1].shape == (2, B, H0, W0) and seq[1].dtype == torch.bool
    assert torch.equal(seq[0][1], got[0]) and torch.equal(seq[1][1], got[1])


def test_one_mask_only_and_min_cover():
    c = _case("window_122x150", 77)
    dev = "cuda"
    args = (c["frames"][0].to(dev), c["frames"][1].to(dev), c["flows"][0].to(dev), c["flows"][1].to(dev))
    cpu = (c["frames"][0], c["frames"][1], c["flows"][0], c["flows"][1])
    for masks, mc in (((c["occ"][0], None), 1 / 64), ((None, c["occ"][1]), 0.3), ((c["occ"][0], c["occ"][1]), 1.0)):
        got = nat.interpolate_frames(*args, c["t"], *(m if m is None else m.to(dev) for m in masks), c["window"], mc)
        want = interpolate_frames(*cpu, c["t"], *masks, c["window"], mc)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


def test_nothing_outside_the_window_is_read():
    c = _case("window_122x150", 77)
    H0, W0, top, left = c["win"]
    inside = torch.zeros(c["H"], c["W"], dtype=torch.bool)
    inside[top:top + H0, left:left + W0] = True
    res = []
    for fill_f, fill_m in ((0.0, 0), (NAN, 0xFF)):
        flows = [f.clone() for f in c["flows"]]
        occ = c["occ"].to(torch.uint8)
        for f in flows:
            f[:, ~inside] = fill_f
        occ[:, :, ~inside] = fill_m
        res.append(_run_ops(c, True, flows, occ))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    frame_t, holes, acc = c["want"][True]
    assert torch.equal(res[1][0].cpu(), frame_t) and torch.equal(res[1][1].cpu().bool(), holes) and torch.equal(res[1][2].cpu(), acc)


def test_same_buffers_twice_with_the_clear():
    c = _case("contention_16x16", 128)
    first = _run_ops(c, True)
    kept = tuple(v.clone() for v in first)
    again = _run_ops(c, True, bufs=first)
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(first, again))
    assert all(torch.equal(a, b) for a, b in zip(kept, again))
    assert torch.equal(again[2].cpu(), c["want"][True][2])
    # the front end clears its own accumulator: two calls, the same bits, fresh tensors
    dev = "cuda"
    args = (c["frames"][0].to(dev), c["frames"][1].to(dev), c["flows"][0].to(dev), c["flows"][1].to(dev), c["t"],
            c["occ"][0].to(dev), c["occ"][1].to(dev))
    a, b = nat.interpolate_frames(*args), nat.interpolate_frames(*args)
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], kept[0])
    assert a[0].data_ptr() != b[0].data_ptr() and a[1].data_ptr() != b[1].data_ptr()


def test_maker_checks():
    B, H, W = 1, 8, 16
    dev = "cuda"
    f1, f2 = (torch.zeros(B, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(2))
    w0, w1 = torch.zeros(B, H, W, 2, device=dev), torch.zeros(B, H, W, 2, device=dev)
    occ = torch.zeros(2, B, H, W, dtype=torch.uint8, device=dev)
    acc = torch.zeros(2, B, H, W, 4, dtype=torch.int64, device=dev)
    par = torch.tensor([[128, 16384]], dtype=torch.int32, device=dev)
    out = torch.full((B, H, W, 3), 9, dtype=torch.uint8, device=dev)
    holes = torch.full((B, H, W), 9, dtype=torch.uint8, device=dev)
    slot = torch.zeros(1, dtype=torch.int64, device=dev)
    si, ri = [B, H, W, H, W, 0, 0, 0], [B, H, W, 0]
    splat, resolve = [f1, f2, w0, w1, occ, acc, par], [f1, f2, acc, par, out, holes]

    def rejected(op, t, i, **put):
        t = list(t)
        for k, v in put.items():
            t[int(k[1:])] = v
        with pytest.raises(RuntimeError, match=op):
            getattr(nat.ops(), op)(t, i)

    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)
    # ---- interp_splat
    S = functools.partial(rejected, "interp_splat", splat)
    S(si, _0=f1.float())                                                     # dtype of a frame
    S(si, _2=w0.half())                                                      # dtype of a flow
    S(si, _4=occ.bool())                                                     # dtype of occ
    S(si, _5=acc.int())                                                      # dtype of acc
    S(si, _6=par.long())                                                     # dtype of par
    S(si, _1=u8(B, H, 2 * W, 3)[:, :, :W])                                   # a frame that is not contiguous
    S(si, _3=torch.zeros(B, H, 2 * W, 2, device=dev)[:, :, :W])              # a flow that is not contiguous
    S(si, _5=torch.zeros(2, B, H, W, 8, dtype=torch.int64, device=dev)[..., :4])   # acc not contiguous
    S(si, _0=f1.cpu())                                                       # a host frame
    S(si, _2=w0.cpu())                                                       # a host flow
    S(si, _6=par.cpu())                                                      # host parameters
    S(si, _0=u8(B, H, W + 1, 3))                                             # frame shape
    S(si, _3=torch.zeros(B, H - 1, W, 2, device=dev))                        # flow shape
    S(si, _4=occ[:1])                                                        # one direction's masks
    S(si, _5=acc[:1])                                                        # one direction's accumulator
    S(si, _6=torch.zeros(3, dtype=torch.int32, device=dev))                  # par is not [K][2]
    S(si, _2=None)                                                           # a flow is missing
    S([B, H, W, H, W, 1, 0, 0])                                              # window below the map
    S([B, H, W, H, W + 1, 0, 0, 0])                                          # window wider than the map
    S([B, H, W, 0, W, 0, 0, 0])                                              # empty window
    S([B, H, W, H, W, 0, 0, 1])                                              # the time index past par
    S([B, H, W, H, W, 0, 0, -1])
    S([40000, H, W, H, W, 0, 0, 0])                                          # dirs * B above 65535
    S([B, 1 << 16, 1 << 15, 1 << 16, 1 << 15, 0, 0, 0])                      # H0 * W0 above 2^30
    big = torch.zeros(B * H * W * 2 + 1, device=dev)
    S(si, _2=big[1:].view(B, H, W, 2))                                       # a flow at 4 bytes
    odd = torch.zeros(2 * B * H * W * 4 + 1, dtype=torch.int64, device=dev)
    S(si, _5=odd[1:].view(2, B, H, W, 4))                                    # acc at 8 bytes
    al = torch.zeros(2 * B * H * W * 4, dtype=torch.int64, device=dev)
    S(si, _5=al.view(2, B, H, W, 4), _2=al.view(torch.float32)[:B * H * W * 2].view(B, H, W, 2))    # acc aliases a flow
    S(si, _5=al.view(2, B, H, W, 4), _0=al.view(torch.uint8)[:B * H * W * 3].view(B, H, W, 3))      # acc aliases a frame
    S(si, _5=al.view(2, B, H, W, 4), _4=al.view(torch.uint8)[:2 * B * H * W].view(2, B, H, W))      # acc aliases occ
    S(si, _5=al.view(2, B, H, W, 4), _6=al.view(torch.int32)[:2].view(1, 2))                        # acc aliases par
    rejected("interp_splat", splat + [slot], si + [0, 2 * B * H * W])        # the slot form takes no flow tensors
    rejected("interp_splat", splat + [slot], si, _2=None, _3=None)           # ... and two offsets
    rejected("interp_splat", splat + [slot], si + [0, 1], _2=None, _3=None)  # ... 8-byte aligned
    rejected("interp_splat", splat + [slot.int()], si + [0, 2 * B * H * W], _2=None, _3=None)   # dtype of the slot
    S(si + [0, 2 * B * H * W])                                               # offsets without a slot
    # ---- interp_resolve
    Rz = functools.partial(rejected, "interp_resolve", resolve)
    Rz(ri, _0=f1.float())
    Rz(ri, _2=acc.int())
    Rz(ri, _3=par.float())
    Rz(ri, _4=out.to(torch.int8))                                            # dtype of frame_t
    Rz(ri, _5=holes.bool())                                                  # dtype of holes
    Rz(ri, _4=u8(B, H, 2 * W, 3)[:, :, :W])                                  # frame_t not contiguous
    Rz(ri, _4=out.cpu())
    Rz(ri, _5=u8(B, H, W + 1))                                               # holes shape
    Rz(ri, _2=acc[:1])
    Rz(ri, _2=odd[1:].view(2, B, H, W, 4))
    Rz([B, H, W, 1])
    Rz([B, 0, W, 0])
    Rz([40000, H, W, 0])
    Rz([B, 1 << 16, 1 << 15, 0])                                             # H0 * W0 above 2^30
    Rz(ri, _4=f1)                                                            # frame_t aliases a frame
    Rz(ri, _2=al.view(2, B, H, W, 4), _4=al.view(torch.uint8)[:B * H * W * 3].view(B, H, W, 3))     # frame_t aliases acc
    Rz(ri, _2=al.view(2, B, H, W, 4), _5=al.view(torch.uint8)[:B * H * W].view(B, H, W))            # holes aliases acc
    both = u8(4 * B * H * W)
    Rz(ri, _4=both[:3 * B * H * W].view(B, H, W, 3), _5=both[2 * B * H * W:3 * B * H * W].view(B, H, W))   # holes aliases frame_t
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((holes == 9).all()) and not acc.any()   # nothing was launched
    nat.ops().interp_splat(splat, si)                                        # the valid calls run
    nat.ops().interp_resolve(resolve, ri)
    acc2 = torch.zeros_like(acc)
    big2 = torch.zeros(4 * B * H * W, device=dev)                            # ... the slot form too: zero flows at 0 and 2 M
    slot.fill_(big2.data_ptr())
    nat.ops().interp_splat([f1, f2, None, None, occ, acc2, par, slot], si + [0, 2 * B * H * W])
    torch.cuda.synchronize()
    assert not out.any() and not holes.any() and torch.equal(acc, acc2)
    assert bool((acc[..., 0] == 256 * 16).all()) and not acc[..., 1:].any()
    for bad in ((f1, f2, w0.double(), w1, 0.5), (f1.float(), f2, w0, w1, 0.5), (f1[:, 1:], f2, w0, w1, 0.5),
                (f1.cpu(), f2, w0, w1, 0.5), (f1, f2, w0, w1, 1.0), (f1, f2, w0, w1.cpu(), 0.5)):
        with pytest.raises(ValueError, match="interpolate_frames"):
            nat.interpolate_frames(*bad)


# --------------------------------------------------------------------- engine
def _frames(B, seed):
    """uint8 frames 122 x 150 (run at the padded 128 x 152, window (122, 150, 3, 1)): two crops of one
    smooth random image, a few pixels apart."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand(B, 3, 18, 22, generator=g)
    big = torch.nn.functional.interpolate(coarse, size=(130, 158), mode="bicubic", align_corners=True)
    big = (big.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1)
    return big[:, 4:126, 4:154].contiguous().cuda(), big[:, 2:124, 6:156].contiguous().cuda()


def _check_against_own_flows(res, f1, f2, ts, min_cover=1 / 64):
    """frames and holes are bitwise the kernels' and the golden op's on the returned flows and masks."""
    assert isinstance(res, BidirectionalInterp)
    B, K = f1.shape[0], len(ts)
    assert res.frames.shape == (K, B, 122, 150, 3) and res.frames.dtype == torch.uint8
    assert res.holes.shape == (K, B, 122, 150) and res.holes.dtype == torch.bool
    fw, bw = res.flows_fw[-1], res.flows_bw[-1]
    kf, kh = nat.interpolate_frames(f1, f2, fw, bw, list(ts), res.occ_fw, res.occ_bw, min_cover=min_cover)
    assert torch.equal(res.frames, kf) and torch.equal(res.holes, kh)
    for k, t in enumerate(ts):
        gf, gh = interpolate_frames(f1.cpu(), f2.cpu(), fw.cpu().contiguous(), bw.cpu().contiguous(), t, res.occ_fw.cpu(),
                                    res.occ_bw.cpu(), min_cover=min_cover)
        assert torch.equal(res.frames[k].cpu(), gf) and torch.equal(res.holes[k].cpu(), gh)


@pytest.mark.parametrize("name", ["raft_small", "raft_large"])
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B", [1, 2])
def test_engine_interp_plan(name, use_graph, B):
    model = FACTORIES[name]()[0].cuda()
    dev = torch.device("cuda")
    eng = RaftEngine(model, dev, use_graph=use_graph)
    f1, f2 = _frames(B, seed=1)
    res = eng.forward(f1, f2, 3, bidirectional=True, interpolate=0.5)
    plain = eng.forward(f1, f2, 3, bidirectional=True)
    torch.cuda.synchronize()
    assert isinstance(plain, BidirectionalFlow) and eng.num_plans() == 2
    assert res.flows_fw.shape == (3, B, 122, 150, 2) and res.occ_fw.shape == (B, 122, 150)
    assert all(torch.equal(a, b) for a, b in zip(res[:4], plain))
    _check_against_own_flows(res, f1, f2, [0.5])
    # another time, another cover and other thresholds build no new plan
    other_t = eng.forward(f1, f2, 3, bidirectional=True, interpolate=[0.3], interp_min_cover=0.9, fb_alpha=0.0, fb_beta=1e6)
    torch.cuda.synchronize()
    assert eng.num_plans() == 2
    assert torch.equal(other_t.flows_fw, res.flows_fw) and torch.equal(other_t.flows_bw, res.flows_bw)
    assert not torch.equal(other_t.frames, res.frames)
    _check_against_own_flows(other_t, f1, f2, [0.3], 0.9)
    # a replay with other frames is consistent with its own flows (the slot is read at run time)
    g1, g2 = _frames(B, seed=2)
    other = eng.forward(g1, g2, 3, return_all_iters=True, bidirectional=True, interpolate=0.5)
    torch.cuda.synchronize()
    assert not torch.equal(other.flows_fw, res.flows_fw) and not torch.equal(other.frames, res.frames)
    assert other.frames.data_ptr() != res.frames.data_ptr() and other.holes.data_ptr() != res.holes.data_ptr()
    _check_against_own_flows(other, g1, g2, [0.5])
    # K = 3 in one call (a plan of its own) equals three K = 1 calls
    ts = [0.25, 0.5, 200 / 256]
    three = eng.forward(f1, f2, 3, bidirectional=True, interpolate=ts)
    torch.cuda.synchronize()
    assert eng.num_plans() == 3 and all(torch.equal(a, b) for a, b in zip(three[:4], plain))
    _check_against_own_flows(three, f1, f2, ts)
    for k, t in enumerate(ts):
        one = eng.forward(f1, f2, 3, bidirectional=True, interpolate=t)
        assert torch.equal(one.frames[0], three.frames[k]) and torch.equal(one.holes[0], three.holes[k])
    assert torch.equal(three.frames[1], res.frames[0]) and eng.num_plans() == 3
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
    res = model(f1, f2, num_flow_updates=3, return_all_iters=False, bidirectional=True, interpolate=(0.25, 0.75))
    torch.cuda.synchronize()
    assert res.flows_fw.shape == (1, 1, 122, 150, 2)
    _check_against_own_flows(res, f1, f2, [0.25, 0.75])
    # host frames go the same way
    res2 = model(f1.cpu(), f2.cpu(), num_flow_updates=3, return_all_iters=False, bidirectional=True, interpolate=(0.25, 0.75))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(res, res2))
    with pytest.raises(ValueError, match="uint8"):
        model(torch.zeros(1, 128, 128, 3, device="cuda"), torch.zeros(1, 128, 128, 3, device="cuda"), bidirectional=True,
              interpolate=0.5)
    with pytest.raises(ValueError, match="bidirectional=True"):
        model(f1, f2, interpolate=0.5)
    with pytest.raises(ValueError, match="warp"):
        model(f1, f2, bidirectional=True, warp=True, interpolate=0.5)


def test_interp_call_does_not_synchronise():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no torch.cuda.set_sync_debug_mode")
    model = raft_small()[0].cuda()
    eng = RaftEngine(model, torch.device("cuda"), use_graph=True)
    f1, f2 = _frames(1, seed=4)
    for _ in range(2):     # warm: the plan, its capture, allocator blocks, the thresholds, the times
        eng.forward(f1, f2, 3, bidirectional=True, interpolate=[0.5, 0.75])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = eng.forward(f1, f2, 3, bidirectional=True, interpolate=[0.5, 0.75])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _check_against_own_flows(res, f1, f2, [0.5, 0.75])
