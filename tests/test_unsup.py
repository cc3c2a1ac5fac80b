"""Label-free training on the CPU: the golden op (train/unsup.py) against the explicit-formula fp64
reference of _unsup_refs.py, an fp32 emulation of the kernels' operation order under the same
checks (the tolerances are attainable) and two wrong variants (they are not vacuous), the loss's
conventions on SyntheticFlow, direct optimisation of a flow field, the out-of-frame penalty, the
constancy-safe augmentation records, the frames-only dataset and the trainer switch."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _unsup_refs as R
from _train_refs import U_ACC, ratio
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import FlowPairs, PairLoader, unsup_loss, unsup_loss_reference
from jax_raft_amd.train import augment as A
from jax_raft_amd.train import unsup as U
from jax_raft_amd.train.data import SyntheticFlow
from jax_raft_amd.train.trainer import UNSUP_FIELDS, TrainConfig, Trainer, config_from_args

CPU = torch.device("cpu")
SMALL = [c for c in R.UNSUP_CASES if c[2] * c[3] < 10000]
EPE_KEYS = {"epe", "1px", "3px", "5px"}


# ------------------------------------------------------------------ the golden op
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("case", SMALL, ids=str)
def test_golden_fp64_autograd_equals_the_explicit_formulas(case, with_mask):
    c, ref = R.unsup_inputs(case, with_mask), R.unsup_ref(case, with_mask)
    f = c.pred.double().requires_grad_(True)
    s = U.unsup_sums(f, c.img1.double(), c.img2.double(), c.mask, *R.PRM)
    (g,) = torch.autograd.grad((s[:, :2] * c.scale.double()).sum(), f)
    # fp64 rounding: 2^-40 of the bounds the fp32 tolerances are 2^-16 of
    tiny = 2.0 ** -40 / U_ACC
    finite = torch.isfinite(ref.grad)
    assert torch.equal(torch.isfinite(g), finite)
    assert ratio(g, ref.grad, tiny * ref.tol, finite) <= 1.0
    ok = torch.isfinite(ref.sums)
    assert torch.equal(torch.isfinite(s.detach()), ok)
    assert ratio(s.detach()[:, [0, 1, 3]], ref.sums[:, [0, 1, 3]], tiny * U_ACC * ref.bounds[:, [0, 1, 3]], ok[:, [0, 1, 3]]) <= 1.0
    assert torch.equal(s.detach()[:, 2], ref.sums[:, 2])


class Golden:
    """The fp32 golden op through the CPU path of the native front ends."""
    blocks = False

    def unsup_loss(self, pred, img1, img2, mask, prm):
        return nat.unsup_loss_partials(pred, img1, img2, mask, *prm)

    def unsup_loss_bwd(self, pred, img1, img2, mask, prm, scale):
        return nat.unsup_loss_grad(pred, img1, img2, mask, scale, *prm)


class Emulated:
    """fp32 torch ops in the kernels' operation order (csrc/kernels/unsup.hip), one block of partials.
    ``drop_wy`` and ``left_sign`` make the two wrong variants."""
    blocks = False

    def __init__(self, drop_wy=False, left_sign=1.0):
        self.drop_wy, self.left_sign = drop_wy, left_sign

    @staticmethod
    def _edges(img1, kappa):
        def w(a, b):
            d = (b - a).abs()
            return torch.exp(-kappa * (((d[..., 0] + d[..., 1]) + d[..., 2]) / 3.0))
        return w(img1[:, :, :-1], img1[:, :, 1:]), w(img1[:, :-1], img1[:, 1:])

    @staticmethod
    def _taps(f, img2):
        B, H, W, _ = f.shape
        inside, x0, x1, y0, y1, wx, wy = R.landing32(f)
        flat = img2.reshape(B, H * W, 3)
        tap = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).reshape(B, H * W, 1).expand(-1, -1, 3)).view(B, H, W, 3)
        return inside, tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1), wx.float().unsqueeze(-1), wy.float().unsqueeze(-1)

    def unsup_loss(self, pred, img1, img2, mask, prm):
        eps, eps_s, kappa, pen = prm
        N, B, H, W, _ = pred.shape
        e2, es2 = torch.tensor(eps) ** 2, torch.tensor(eps_s) ** 2
        ax, ay = self._edges(img1, kappa)
        on = torch.ones(B, H, W, dtype=torch.bool) if mask is None else mask >= 0.5
        rho = lambda d, e: torch.sqrt(d * d + e)
        part = torch.full((1, N, 4), float("nan"))
        for i in range(N):
            f = pred[i]
            sm = torch.zeros(B, H, W)
            dx, dy = f[:, :, 1:] - f[:, :, :-1], f[:, 1:] - f[:, :-1]
            sm[:, :, :-1] += ax * (rho(dx[..., 0], es2) + rho(dx[..., 1], es2))
            sm[:, :-1] += ay * (rho(dy[..., 0], es2) + rho(dy[..., 1], es2))
            inside, c00, c01, c10, c11, wx, wy = self._taps(f, img2)
            t, b = c00 + wx * (c01 - c00), c10 + wx * (c11 - c10)
            r = rho(t + wy * (b - t) - img1, e2)
            pix = torch.where(inside, ((r[..., 0] + r[..., 1]) + r[..., 2]) / 3.0, pen + 0.0 * (f[..., 0] + f[..., 1]))
            sel = on & inside
            part[0, i] = torch.stack([(on.float() * pix).sum(), sm.sum(), (on & ~inside).float().sum(),
                                      pix[sel].sum() if i == N - 1 else torch.zeros(())])
        return part

    def unsup_loss_bwd(self, pred, img1, img2, mask, prm, scale):
        eps, eps_s, kappa, _ = prm
        N, B, H, W, _ = pred.shape
        e2, es2 = torch.tensor(eps) ** 2, torch.tensor(eps_s) ** 2
        ax, ay = self._edges(img1, kappa)
        on = torch.ones(B, H, W, dtype=torch.bool) if mask is None else mask >= 0.5
        drho = lambda d, e: d / torch.sqrt(d * d + e)
        grad = torch.full(pred.shape, float("nan"))
        for i in range(N):
            f = pred[i]
            s = torch.zeros(B, H, W, 2)
            gx = ax.unsqueeze(-1) * drho(f[:, :, 1:] - f[:, :, :-1], es2)
            gy = ay.unsqueeze(-1) * drho(f[:, 1:] - f[:, :-1], es2)
            s[:, :, :-1] -= gx
            s[:, :, 1:] += self.left_sign * gx
            s[:, :-1] -= gy
            s[:, 1:] += gy
            inside, c00, c01, c10, c11, wx, wy = self._taps(f, img2)
            t, b = c00 + wx * (c01 - c00), c10 + wx * (c11 - c10)
            r = drho(t + wy * (b - t) - img1, e2)
            dvx = (c01 - c00) if self.drop_wy else (1.0 - wy) * (c01 - c00) + wy * (c11 - c10)
            p = torch.stack([(r * dvx).sum(-1), (r * (b - t)).sum(-1)], -1) / 3.0
            p = torch.where((on & inside).unsqueeze(-1), p, torch.zeros(()))
            grad[i] = scale[i, 1] * s + scale[i, 0] * p
        return grad


@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("case", R.UNSUP_CASES, ids=str)
@pytest.mark.parametrize("impl", [Golden(), Emulated()], ids=["golden", "emulated"])
def test_fp32_implementations_pass_the_kernel_checks(impl, case, with_mask):
    R.check_unsup_loss(impl, case, with_mask)
    R.check_unsup_loss_bwd(impl, case, with_mask)


@pytest.mark.parametrize("wrong", [Emulated(drop_wy=True), Emulated(left_sign=-1.0)], ids=["wy-dropped", "left-sign"])
def test_wrong_variants_fail_the_same_check(wrong):
    case = (3, 2, 13, 37, False)
    R.check_unsup_loss_bwd(Emulated(), case, True)
    with pytest.raises(AssertionError, match="error / tolerance"):
        R.check_unsup_loss_bwd(wrong, case, True)


# ------------------------------------------------------------------ conventions
def test_conventions_on_synthetic_flow():
    """image1(x) = image2(x + f(x)) holds exactly there: the ground truth's photometric error is
    the floor eps, far below the zero flow's, and a 1 px shift raises it."""
    i1, i2, flow, _ = SyntheticFlow((96, 128), seed=3, max_motion=6.0).batch([0, 1])
    eps = U.DEFAULTS["eps"]
    photo = lambda f: float(unsup_loss_reference(f[None], i1, i2)[1]["photo"])
    gt, zero, shifted = photo(flow), photo(torch.zeros_like(flow)), photo(flow + 1.0)
    print(f"photo: ground truth {gt:.4f}, zero flow {zero:.4f}, shifted {shifted:.4f}")
    assert gt <= 1.5 * eps and gt < zero / 3.0 and shifted > gt


def test_direct_optimisation_recovers_the_flow():
    i1, i2, flow, _ = SyntheticFlow((64, 96), seed=5, max_motion=1.0).batch([0, 1])
    f = torch.zeros_like(flow).requires_grad_(True)
    opt = torch.optim.Adam([f], lr=0.05)
    epe = lambda: float((f.detach() - flow).norm(dim=-1).mean())
    start = epe()
    for _ in range(400):
        opt.zero_grad()
        loss, _ = unsup_loss(f[None], i1, i2, smooth_weight=0.05, out_penalty=0.5)
        loss.backward()
        opt.step()
    print(f"EPE {start:.3f} -> {epe():.3f}")
    assert epe() < 0.25 * start


def test_out_penalty():
    i1, i2, _, _ = SyntheticFlow((24, 40), seed=1).batch([0])
    f = torch.full((2, 1, 24, 40, 2), 1000.0, requires_grad=True)
    loss, m = unsup_loss_reference(f, i1, i2, gamma=1.0, smooth_weight=0.0, out_penalty=0.375)
    assert float(loss.detach()) == 2 * 0.375 and float(m["inside"]) == 0.0 and math.isnan(float(m["photo"]))
    loss.backward()
    assert not f.grad.any()
    # a non-finite prediction is not masked away: NaN loss, non-finite gradient at that pixel
    g = torch.zeros(3, 1, 24, 40, 2)
    g[1, 0, 5, 7, 1] = float("inf")
    g.requires_grad_(True)
    loss, _ = unsup_loss_reference(g, i1, i2, mask=torch.zeros(1, 24, 40))
    assert math.isnan(float(loss.detach()))
    loss.backward()
    assert not torch.isfinite(g.grad[1, 0, 5, 7, 1]) and torch.isfinite(g.grad[0]).all() and torch.isfinite(g.grad[2]).all()


def test_front_end_checks_and_exports():
    import jax_raft_amd.train as T

    assert T.unsup_loss is unsup_loss and T.unsup_loss_reference is unsup_loss_reference
    assert "unsup_loss" in T.__all__ and "unsup_loss_reference" in T.__all__
    f, i = torch.zeros(2, 1, 4, 5, 2), torch.zeros(1, 4, 5, 3)
    for bad in ((f[0], i, i), (f, i[:, :3], i), (f, i, i.long()), (f, i, i, torch.zeros(1, 4, 4))):
        with pytest.raises(ValueError, match="unsup_loss"):
            unsup_loss(*bad)
    with pytest.raises(ValueError, match="unsup_loss_bwd"):
        nat.unsup_loss_grad(f, i, i, None, torch.zeros(3, 2))
    assert nat.unsup_loss_blocks(1) == 1 and nat.unsup_loss_blocks(257) == 2 and nat.unsup_loss_blocks(10 ** 7) == 1024
    assert nat.UNSUP_GRID_X * nat.UNSUP_BLOCK == R.UNSUP_GRID


def test_parameter_tensors_share_one_cache():
    dev = torch.device("cpu")
    makers = ((nat.unsup_params, (0.01, 0.001, 10.0, 0.5)), (nat.selfsup_params, (0.001,)), (nat.fb_thresholds, (0.01, 0.5)))
    first = [make(*values, dev) for make, values in makers]
    for (make, values), t in zip(makers, first):
        assert make(*values, dev) is t                                   # a second call uploads nothing
        assert t.dtype == torch.float32 and t.tolist() == torch.tensor(values, dtype=torch.float32).tolist()
        assert sum(v is t for v in nat._floats.values()) == 1           # ... and all live in the one cache
    assert nat.unsup_params(0.01, 0.001, 10.0, 0.25, dev) is not first[0]
    assert nat._cached_floats((0.001,), dev) is first[1]


@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_op_rows():
    for op in ("unsup_loss", "unsup_loss_bwd"):
        assert list(torch.ops.jax_raft_amd.op_arity(op)) == [1, 4, 4]
        for k in (3, 5):
            with pytest.raises(RuntimeError, match=rf"{op}: expected 4 ints, got {k}\b"):
                getattr(torch.ops.jax_raft_amd, op)([None], [1] * k)
        assert hasattr(torch.classes.jax_raft_amd.Plan(), "add_" + op)
        with pytest.raises(RuntimeError, match=op + ":"):          # the builder's own checks name the op
            getattr(torch.ops.jax_raft_amd, op)([None], [1, 4, 4, 33])
        with pytest.raises(RuntimeError, match=op + ":"):
            getattr(torch.ops.jax_raft_amd, op)([torch.zeros(2 * 16 * 2)] + [None] * 6, [1, 4, 4, 2])   # a CPU tensor


# ------------------------------------------------------------------ records
def _words(p):
    return np.concatenate([p.ints, p.floats.view(np.int32)], axis=1)


def test_constancy_records():
    n_ints = {"dense": A.N_INTS, "sparse": A.N_INTS_SPARSE, "mixed": None}
    sizes, dense = [(150, 170), (140, 200), (150, 170), (160, 180)], [True, False, True, False]
    differ = 0
    for step in range(12):
        kw = dict(seed=7, step=step, rank=1)
        pairs = {
            "dense": [A.AugmentParams.sample(4, (150, 170), "chairs", (128, 128), constancy=c, **kw) for c in (False, True)]
                     + [A.AugmentParams.sample(4, (150, 170), "chairs", (128, 128), **kw)],
            "sparse": [A.sample_sparse(4, sizes, "kitti", (128, 128), constancy=c, **kw) for c in (False, True)]
                      + [A.sample_sparse(4, sizes, "kitti", (128, 128), **kw)],
            "mixed": [A.sample_mixed(4, sizes, dense, "sintel", (128, 128), constancy=c, **kw) for c in (False, True)]
                     + [A.sample_mixed(4, sizes, dense, "sintel", (128, 128), **kw)],
        }
        for name, (plain, safe, default) in pairs.items():
            assert plain == default                              # constancy=False: what the sampler returns today
            ni = plain.ints.shape[1]
            assert n_ints[name] in (None, ni)
            free = np.zeros(ni + A.N_FLOATS, dtype=bool)         # the words that may differ
            free[A.I_NRECT:A.N_INTS] = True                      # the rectangle count and the rectangles
            free[ni + A.F_COL2:ni + A.F_COL2 + 12] = True        # colour 2
            w0, w1 = _words(plain), _words(safe)
            assert np.array_equal(w0[:, ~free], w1[:, ~free]), name
            assert not safe.ints[:, A.I_NRECT:A.N_INTS].any(), name
            assert np.array_equal(safe.floats[:, A.F_COL2:A.F_COL2 + 12].view(np.int32),
                                  safe.floats[:, A.F_COL1:A.F_COL1 + 12].view(np.int32)), name
            differ += int(not np.array_equal(w0, w1))
    assert differ > 12                                           # the draws do hold erasers and asymmetric colours


# ------------------------------------------------------------------ frames
def write_frames(root, seqs, h=140, w=150, seed=0):
    """seqs: {sub-directory ('' = the root itself): number of frames}; smooth random frames."""
    from jax_raft_amd.utils.flow_io import write_png

    rng = np.random.default_rng(seed)
    frames = {}
    for sub, n in seqs.items():
        d = os.path.join(root, sub)
        os.makedirs(d, exist_ok=True)
        for k in range(n):
            img = np.kron(rng.integers(0, 256, (h // 10, w // 10, 3)), np.ones((10, 10, 1))).astype(np.uint8)
            write_png(os.path.join(d, f"frame_{k:04d}.png"), img)
            frames[os.path.join(d, f"frame_{k:04d}.png")] = img
    return frames


def test_frames_dataset(tmp_path):
    frames = write_frames(str(tmp_path), {"b_seq": 3, "a_seq": 2, os.path.join("c", "deep"): 4, "empty": 0, "single": 1})
    (tmp_path / "a_seq" / "notes.txt").write_text("not a frame")
    ds = FlowPairs.frames(str(tmp_path))
    assert type(FlowPairs.open(str(tmp_path), "frames")) is type(ds) and FlowPairs.open(str(tmp_path), "frames").items == ds.items
    assert ds.labelled is False and FlowPairs.labelled is True
    pairs = [(os.path.relpath(a, tmp_path), os.path.relpath(b, tmp_path)) for a, b, _ in ds.items]
    j = os.path.join
    assert pairs == [(j("a_seq", "frame_0000.png"), j("a_seq", "frame_0001.png")),
                     (j("b_seq", "frame_0000.png"), j("b_seq", "frame_0001.png")),
                     (j("b_seq", "frame_0001.png"), j("b_seq", "frame_0002.png")),
                     (j("c", "deep", "frame_0000.png"), j("c", "deep", "frame_0001.png")),
                     (j("c", "deep", "frame_0001.png"), j("c", "deep", "frame_0002.png")),
                     (j("c", "deep", "frame_0002.png"), j("c", "deep", "frame_0003.png"))]
    assert all(os.path.dirname(a) == os.path.dirname(b) for a, b in pairs)        # no pair crosses sequences
    a, b, f = ds[2]
    assert np.array_equal(a, frames[ds.items[2][0]]) and np.array_equal(b, frames[ds.items[2][1]])
    assert f.shape == (140, 150, 2) and f.dtype == np.float32 and not f.any() and ds[0][2] is f and not f.flags.writeable
    ld = PairLoader(ds, batch=2)
    i1, i2, fl = ld.fetch(0)
    assert i1.shape == (2, 140, 150, 3) and fl.shape == (2, 140, 150, 2) and not fl.any()
    ld.close()
    with pytest.raises(FileNotFoundError):
        FlowPairs.frames(str(tmp_path / "single"))
    # a frame of another size: the dense loader's error, naming the file
    from jax_raft_amd.utils.flow_io import write_png
    write_png(str(tmp_path / "b_seq" / "frame_0002.png"), np.zeros((140, 160, 3), np.uint8))
    ld = PairLoader(FlowPairs.frames(str(tmp_path)), batch=6)
    with pytest.raises(ValueError, match="frame_0002.png"):
        ld.fetch(0)
    ld.close()
    with pytest.raises(ValueError, match="no ground truth"):
        TrainConfig(data=str(tmp_path), dataset="frames")
    TrainConfig(data=str(tmp_path), dataset="frames", loss="unsup")


# ------------------------------------------------------------------ trainer
KW = dict(arch="raft_small", steps=2, batch=1, iters=2, size=(128, 128), log_every=1, lr=1e-4)


def _params(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


def test_config_rejections_and_cli():
    with pytest.raises(ValueError, match="unknown loss"):
        TrainConfig(loss="census")
    with pytest.raises(ValueError, match="graph_step"):
        TrainConfig(loss="unsup", graph_step=True)
    cfg = TrainConfig()
    assert cfg.loss == "sequence" and [getattr(cfg, k) for k in UNSUP_FIELDS[1:]] == [0.01, 0.001, 10.0, 0.05, 0.5]
    import argparse
    ns = argparse.Namespace(**{**{k: v for k, v in TrainConfig().__dict__.items() if k != "mix_weights"}, "mix": None,
                               "loss": "unsup", "unsup_smooth_weight": 0.1})
    got = config_from_args(ns)
    assert got.loss == "unsup" and got.unsup_smooth_weight == 0.1


def test_trainer_defaults_are_unchanged(tmp_path):
    runs = []
    for k, kw in enumerate(({}, {"loss": "sequence"})):
        tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / str(k)), **KW, **kw), device=CPU)
        logs = []
        tr.fit(log=logs.append)
        runs.append((_params(tr), logs, json.load(open(tmp_path / str(k) / "latest.json"))))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
    assert set(json.loads(runs[0][1][-1])) == {"loss", "grad_norm", "epe", "1px", "3px", "5px", "step", "skipped", "lr",
                                               "elapsed_s", "pairs_per_s"}
    for _, _, latest in runs:
        assert not set(latest["config"]) & set(UNSUP_FIELDS)
        assert set(latest["config"]) == set(TrainConfig.__dataclass_fields__) - set(UNSUP_FIELDS) - {
            "val", "val_every", "val_iters", "val_batch", "val_max_pairs", "chairs_split"}
    # a label-free run records its settings
    tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / "u"), loss="unsup", unsup_smooth_weight=0.1, **KW), device=CPU)
    tr.save(str(tmp_path / "u"))
    config = json.load(open(tmp_path / "u" / "latest.json"))["config"]
    assert config["loss"] == "unsup" and config["unsup_smooth_weight"] == 0.1 and "unsup_eps" not in config


def test_trainer_unsup_cpu():
    tr = Trainer(TrainConfig(loss="unsup", **KW), device=CPU)
    before = _params(tr)
    outs = [tr.train_step(tr.batch_for(s)) for s in range(2)]
    assert all(math.isfinite(float(o["loss"])) for o in outs) and tr.skipped == 0
    assert set(outs[-1]) == {"loss", "grad_norm", "photo", "smooth", "inside"} | EPE_KEYS
    after = _params(tr)
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # the labels take no part in the gradient
    other = Trainer(TrainConfig(loss="unsup", **KW), device=CPU)
    for s in range(2):
        i1, i2, flow, valid = other.batch_for(s)
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(a, b) for a, b in zip(after, _params(other)))


def test_trainer_on_frames_cpu(tmp_path):
    write_frames(str(tmp_path), {"s0": 3, "s1": 3})
    tr = Trainer(TrainConfig(loss="unsup", data=str(tmp_path), dataset="frames", **KW), device=CPU)
    assert tr.labelled is False
    i1, i2, flow, valid = tr.batch_for(0)
    assert i1.shape == (1, 128, 128, 3) and not flow.any()
    # brightness constancy is kept: the step's record has colour 2 = colour 1 and no eraser
    rec = A.AugmentParams.sample(1, (140, 150), "chairs", (128, 128), seed=0, step=0, rank=0, constancy=True)
    from jax_raft_amd.ops import native
    want = native.augment_pairs(*tr.loader.fetch(0), rec, (128, 128))
    assert all(torch.equal(a, b) for a, b in zip((i1, i2, flow, valid), want))
    logs = []
    tr.fit(log=logs.append)
    last = json.loads(logs[-1])
    assert math.isfinite(last["loss"]) and {"photo", "smooth", "inside"} <= set(last) and not EPE_KEYS & set(last)
