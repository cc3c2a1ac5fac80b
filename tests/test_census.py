"""The census photometric term on the CPU: the golden op (train/unsup.py, ``photo="census"``) against
the explicit-formula fp64 reference of _census_refs.py, the fp32 golden op and an fp32 emulation of
the kernels' operation order under the same checks (the tolerances are attainable) and three wrong
variants (they are not vacuous), the term's conventions, its robustness to brightness changes,
direct optimisation of a flow field, ``photo="charbonnier"`` bitwise the old call, and the trainer
switch."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

import _census_refs as CR
import _unsup_refs as R
from _train_refs import U_ACC, bits_equal, ratio
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import census_sums, unsup_loss, unsup_loss_reference
from jax_raft_amd.train import unsup as U
from jax_raft_amd.train.data import SyntheticFlow
from jax_raft_amd.train.trainer import UNSUP_FIELDS, TrainConfig, Trainer, config_from_args

CPU = torch.device("cpu")
MASKS = [False, True]


def test_constants_and_exports():
    import jax_raft_amd.train as T

    assert T.census_sums is census_sums and "census_sums" in T.__all__
    assert (U.CENSUS_R, U.CENSUS_TAU, U.CENSUS_K, U.CENSUS_H, U.CENSUS_POW) == (CR.R, CR.C_TAU, CR.C_K, CR.C_H, CR.C_POW)
    assert (nat.CENSUS_TILE, nat.CENSUS_ITERS) == (CR.CENSUS_TILE, CR.CENSUS_ITERS)
    tx, ty = nat.CENSUS_TILE
    N, B, H, W, _ = CR.TILE_CASE
    assert H // ty >= 3 and H % ty and W // tx >= 3 and W % tx and N > nat.CENSUS_ITERS and N % nat.CENSUS_ITERS
    assert nat.census_tiles(1, 1, 1) == 1 and nat.census_tiles(2, ty + 1, tx) == 4 and nat.census_tiles(B, H, W) == 16
    assert len(CR.offsets()) == 48


# ------------------------------------------------------------------ the golden op
@pytest.mark.parametrize("with_mask", MASKS)
@pytest.mark.parametrize("case", CR.CENSUS_CASES, ids=str)
def test_golden_fp64_autograd_equals_the_explicit_formulas(case, with_mask):
    c, ref = CR.census_inputs(case, with_mask), CR.census_ref(case, with_mask)
    f = c.pred.double().requires_grad_(True)
    s = census_sums(f, c.img1.double(), c.img2.double(), c.mask, CR.PEN)
    (g,) = torch.autograd.grad((s[:, 0] * c.scale[:, 0].double()).sum(), f)
    tiny = 2.0 ** -40 / U_ACC                                        # fp64 rounding, of the fp32 tolerances
    assert bool(torch.isfinite(g).all())
    assert ratio(g, ref.grad, tiny * ref.tol) <= 1.0
    ok = torch.isfinite(ref.sums)
    assert torch.equal(torch.isfinite(s.detach()), ok)
    assert ratio(s.detach()[:, [0, 3]], ref.sums[:, [0, 3]], tiny * ref.sum_tol[:, [0, 3]], ok[:, [0, 3]]) <= 1.0
    assert torch.equal(s.detach()[:, 1:3], ref.sums[:, 1:3])


@pytest.mark.parametrize("with_mask", MASKS)
@pytest.mark.parametrize("case", CR.CENSUS_CASES, ids=str)
def test_the_cases_exercise_the_clamp_path(case, with_mask):
    """Wherever there is a valid masked pixel, some valid pixel's patch holds a neighbour that lands
    outside the frame (and so has the border's grey)."""
    ref = CR.census_ref(case, with_mask)
    N, B, H, W, _ = case
    if H > 2 * CR.R and W > 2 * CR.R:
        assert any(ref.clamp_seen), case
        if B * H * W >= 1000:
            assert all(ref.clamp_seen), case
    else:
        assert not any(ref.clamp_seen) and not ref.coef.any()
    if case == (1, 1, 7, 7, False):
        assert int((ref.coef[0] != 0).sum()) == 1                    # exactly one valid pixel


class Golden:
    """The fp32 golden op through the CPU path of the native front ends."""
    tiles = False

    def census_loss(self, pred, img1, img2, mask, pen):
        return nat.census_loss_partials(pred, img1, img2, mask, pen)

    def census_loss_bwd(self, pred, img1, img2, mask, pen, scale):
        return nat.census_loss_grad(pred, img1, img2, mask, scale, pen)


class Emulated:
    """fp32 torch ops in the kernels' operation order (csrc/kernels/census.hip), one row of partials.
    ``radius``, ``drop_centre`` and ``band`` make the wrong variants."""
    tiles = False

    def __init__(self, radius=CR.R, drop_centre=False, band=CR.R):
        self.radius, self.drop_centre, self.band = radius, drop_centre, band

    @staticmethod
    def _gray(img):
        return 127.5 * ((0.299 * img[..., 0] + 0.587 * img[..., 1]) + 0.114 * img[..., 2])

    @staticmethod
    def _warp(f, G2):
        B, H, W, _ = f.shape
        inside, x0, x1, y0, y1, wx, wy = CR.landing32c(f)
        wx, wy = wx.float(), wy.float()
        flat = G2.reshape(B, H * W)
        tap = lambda yy, xx: torch.gather(flat, 1, (yy * W + xx).reshape(B, H * W)).view(B, H, W)
        c00, c01, c10, c11 = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
        t, b = c00 + wx * (c01 - c00), c10 + wx * (c11 - c10)
        return inside, t + wy * (b - t), (1.0 - wy) * (c01 - c00) + wy * (c11 - c10), b - t

    def _geom(self, B, H, W):
        g, r = torch.zeros(B, H, W, dtype=torch.bool), self.band
        if H > 2 * r and W > 2 * r:
            g[:, r:H - r, r:W - r] = True
        return g

    def _forward(self, f, G1, G2, on):
        """(inside, valid, cen, coef, w, dwx, dwy) of one prediction."""
        B, H, W, _ = f.shape
        inside, w, dwx, dwy = self._warp(f, G2)
        pad = lambda t: F.pad(t, (CR.R, CR.R, CR.R, CR.R))
        G1p, wp = pad(G1), pad(w)
        tau = lambda d: d * torch.rsqrt(CR.C_TAU + d * d)
        h = torch.zeros(B, H, W)
        for dy, dx in CR.offsets(self.radius):
            d = tau(CR.shifted(G1p, dy, dx, H, W) - G1) - tau(CR.shifted(wp, dy, dx, H, W) - w)
            e = d * d
            h = h + e * torch.reciprocal(CR.C_K + e)
        hh = h + CR.C_H
        cen = torch.pow(hh, 0.4)
        valid = inside & self._geom(B, H, W)
        coef = torch.where(on & valid, 0.4 * cen / hh, torch.zeros(()))
        return inside, valid, cen, coef, w, dwx, dwy

    def census_loss(self, pred, img1, img2, mask, pen):
        N, B, H, W, _ = pred.shape
        G1, G2 = self._gray(img1), self._gray(img2)
        on = torch.ones(B, H, W, dtype=torch.bool) if mask is None else mask >= 0.5
        part, coefs = torch.full((1, N, 4), float("nan")), torch.full((N, B, H, W), float("nan"))
        for i in range(N):
            f = pred[i]
            inside, valid, cen, coefs[i], _, _, _ = self._forward(f, G1, G2, on)
            term = torch.where(valid, cen, torch.where(inside, torch.zeros(()), torch.tensor(pen)))
            sel = on & valid
            part[0, i] = torch.stack([(on.float() * term + 0.0 * (f[..., 0] + f[..., 1])).sum(), (on & ~inside).float().sum(),
                                      (on & inside & ~self._geom(B, H, W)).float().sum(),
                                      cen[sel].sum() if i == N - 1 else torch.zeros(())])
        return part, coefs

    def census_loss_bwd(self, pred, img1, img2, mask, pen, scale):
        N, B, H, W, _ = pred.shape
        G1, G2 = self._gray(img1), self._gray(img2)
        on = torch.ones(B, H, W, dtype=torch.bool) if mask is None else mask >= 0.5
        pad = lambda t: F.pad(t, (CR.R, CR.R, CR.R, CR.R))
        G1p = pad(G1)
        grad = torch.full(pred.shape, float("nan"))
        for i in range(N):
            inside, _, _, coef, w, dwx, dwy = self._forward(pred[i], G1, G2, on)
            wp, cp = pad(w), pad(coef)
            a = torch.zeros(B, H, W)
            for dy, dx in CR.offsets(self.radius):
                d1 = CR.shifted(G1p, dy, dx, H, W) - G1
                t1 = d1 * torch.rsqrt(CR.C_TAU + d1 * d1)
                d2 = CR.shifted(wp, dy, dx, H, W) - w
                ri = torch.rsqrt(CR.C_TAU + d2 * d2)
                df = d2 * ri - t1
                ki = torch.reciprocal(CR.C_K + df * df)
                kappa = (CR.C_K * (ki * ki)) * (2.0 * df) * (CR.C_TAU * (ri * ri * ri))
                centre = torch.zeros(()) if self.drop_centre else coef
                a = a - (centre + CR.shifted(cp, dy, dx, H, W)) * kappa
            s = scale[i] * a
            grad[i] = torch.where(inside.unsqueeze(-1), torch.stack([s * dwx, s * dwy], -1), torch.zeros(()))
        return grad


@pytest.mark.parametrize("with_mask", MASKS)
@pytest.mark.parametrize("case", CR.CENSUS_CASES, ids=str)
@pytest.mark.parametrize("impl", [Golden(), Emulated()], ids=["golden", "emulated"])
def test_fp32_implementations_pass_the_kernel_checks(impl, case, with_mask):
    CR.check_census_loss(impl, case, with_mask)
    CR.check_census_loss_bwd(impl, case, with_mask)


WRONG = {"patch-5x5": (Emulated(radius=2), True, True), "centre-dropped": (Emulated(drop_centre=True), False, True),
         "band-off-by-one": (Emulated(band=CR.R - 1), True, True)}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_variants_fail_the_same_checks(wrong):
    impl, fwd_fails, bwd_fails = WRONG[wrong]
    case = (3, 2, 13, 37, False)
    CR.check_census_loss(Emulated(), case, True)
    CR.check_census_loss_bwd(Emulated(), case, True)
    if fwd_fails:
        with pytest.raises(AssertionError, match="error / tolerance|counts|support"):
            CR.check_census_loss(impl, case, True)
    else:
        CR.check_census_loss(impl, case, True)
    if bwd_fails:
        with pytest.raises(AssertionError, match="error / tolerance"):
            CR.check_census_loss_bwd(impl, case, True)


# ------------------------------------------------------------------ conventions
def test_identical_frames_and_zero_flow():
    i1, _, _, _ = SyntheticFlow((24, 40), seed=1).batch([0, 1])
    f = torch.zeros(2, 2, 24, 40, 2, requires_grad=True)
    s = census_sums(f, i1, i1.clone())
    n = 2 * (24 - 6) * (40 - 6)
    floor = torch.tensor(0.01) ** 0.4                                # h = 0 everywhere
    assert torch.allclose(s[:, 0].detach(), n * floor.expand(2), rtol=1e-6, atol=0.0)
    assert s[:, 1].tolist() == [0.0, 0.0] and s[:, 2].tolist() == [2 * 24 * 40 - n] * 2
    assert float(s[0, 3].detach()) == 0.0 and torch.allclose(s[1, 3].detach(), n * floor, rtol=1e-6)
    loss, mets = unsup_loss_reference(f, i1, i1.clone(), photo="census", smooth_weight=0.0)
    loss.backward()
    assert not f.grad.any()
    assert torch.allclose(mets["photo"], floor, rtol=1e-6) and float(mets["inside"]) == 1.0
    assert set(mets) == {"photo", "smooth", "inside"}


def test_brightness_changes_move_census_far_less_than_charbonnier():
    i1, i2, flow, _ = SyntheticFlow((64, 96), seed=3, max_motion=3.0).batch([0, 1])
    base = {p: float(unsup_loss_reference(flow[None], i1, i2, smooth_weight=0.0, photo=p)[0]) for p in U.PHOTO}
    for name, changed in (("additive", i2 + 0.2), ("multiplicative", i2 * 0.7)):
        move = {p: abs(float(unsup_loss_reference(flow[None], i1, changed, smooth_weight=0.0, photo=p)[0]) - base[p])
                for p in U.PHOTO}
        # relative to each loss's own span: what the zero flow pays over the ground truth
        span = {p: abs(float(unsup_loss_reference(torch.zeros_like(flow)[None], i1, i2, smooth_weight=0.0, photo=p)[0])
                       - base[p]) for p in U.PHOTO}
        rel = {p: move[p] / span[p] for p in U.PHOTO}
        print(f"{name}: moved by {move}, relative to the zero flow's excess {rel}")
        assert rel["census"] < rel["charbonnier"] / 4.0, (name, rel)


def test_direct_optimisation_recovers_the_flow():
    i1, i2, flow, _ = SyntheticFlow((64, 96), seed=5, max_motion=1.0).batch([0, 1])
    f = torch.zeros_like(flow).requires_grad_(True)
    opt = torch.optim.Adam([f], lr=0.05)
    inner = (slice(None), slice(3, -3), slice(3, -3))                # the border band has no census term
    epe = lambda: float((f.detach() - flow)[inner].norm(dim=-1).mean())
    start, losses = epe(), []
    for _ in range(300):
        opt.zero_grad()
        loss, _ = unsup_loss(f[None], i1, i2, smooth_weight=0.05, out_penalty=0.5, photo="census")
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"EPE {start:.3f} -> {epe():.3f}, loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    # no rate is claimed (the soft signs saturate: only near-ties of grey levels pull), only the direction
    assert epe() < start and losses[-1] < losses[0]


def test_out_penalty_mask_and_nan():
    i1, i2, _, _ = SyntheticFlow((24, 40), seed=1).batch([0])
    f = torch.full((2, 1, 24, 40, 2), 1000.0, requires_grad=True)
    loss, m = unsup_loss_reference(f, i1, i2, gamma=1.0, smooth_weight=0.0, out_penalty=0.375, photo="census")
    assert float(loss.detach()) == 2 * 0.375 and float(m["inside"]) == 0.0 and math.isnan(float(m["photo"]))
    loss.backward()
    assert not f.grad.any()
    # the mask is honoured ...
    g = torch.randn(1, 1, 24, 40, 2)
    mask = torch.zeros(1, 24, 40)
    assert not census_sums(g, i1, i2, mask).any()
    # ... but a non-finite prediction is not masked away
    g[0, 0, 5, 7, 1] = float("inf")
    s = census_sums(g, i1, i2, mask)
    assert math.isnan(float(s[0, 0])) and not s[0, 1:].any()


# ------------------------------------------------------------------ the switch
def test_photo_argument():
    c = R.unsup_inputs((3, 2, 13, 37, False), True)
    kw = dict(gamma=0.7, eps=0.02, eps_s=0.002, edge_kappa=8.0, smooth_weight=0.08, out_penalty=0.4)
    for fn in (unsup_loss_reference, unsup_loss):
        outs = []
        for extra in ({}, {"photo": "charbonnier"}):
            f = c.pred.clone().requires_grad_(True)
            loss, mets = fn(f, c.img1, c.img2, c.mask, **kw, **extra)
            loss.backward()
            outs.append((loss.detach(), f.grad, mets))
        assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1])
        assert all(bits_equal(outs[0][2][k], outs[1][2][k]) for k in ("photo", "smooth", "inside"))
        census, _ = fn(c.pred, c.img1, c.img2, c.mask, **kw, photo="census")
        assert not torch.equal(census, outs[0][0])
        for bad in ("ssim", "", None, "Census"):
            with pytest.raises(ValueError, match="unknown photo"):
                fn(c.pred, c.img1, c.img2, c.mask, photo=bad)
    # the census loss is the sums assembled as stated, the smoothness term the existing one
    s = census_sums(c.pred, c.img1, c.img2, c.mask, 0.4)
    old = U.unsup_sums(c.pred, c.img1, c.img2, c.mask, 0.02, 0.002, 8.0, 0.4)
    w = 0.7 ** torch.arange(c.N - 1, -1, -1, dtype=torch.float64)
    want = (w.float() * (s[:, 0] / c.P + 0.08 * (old[:, 1] / (2.0 * c.P)))).sum()
    got, mets = unsup_loss_reference(c.pred, c.img1, c.img2, c.mask, **kw, photo="census")
    assert torch.allclose(got, want, rtol=1e-6)
    cnt = float((c.mask >= 0.5).sum())
    assert torch.allclose(mets["photo"], s[-1, 3] / (cnt - s[-1, 1] - s[-1, 2]), rtol=1e-6)
    assert torch.allclose(mets["inside"], (cnt - s[-1, 1]) / cnt, rtol=1e-6)
    assert bits_equal(mets["smooth"], unsup_loss_reference(c.pred, c.img1, c.img2, c.mask, **kw)[1]["smooth"])


def test_front_end_checks():
    f, i = torch.zeros(2, 1, 8, 9, 2), torch.zeros(1, 8, 9, 3)
    for bad in ((f[0], i, i), (f, i[:, :3], i), (f, i, i.long()), (f, i, i, torch.zeros(1, 8, 8))):
        with pytest.raises(ValueError, match="unsup_loss"):
            unsup_loss(*bad, photo="census")
        with pytest.raises(ValueError, match="unsup_loss"):
            nat.census_loss_partials(*bad)
    for bad in (torch.zeros(3), torch.zeros(2, 2)):
        with pytest.raises(ValueError, match="census_loss_bwd"):
            nat.census_loss_grad(f, i, i, None, bad)
    with pytest.raises(ValueError, match="census_gray"):
        nat.census_gray_planes(i, i[:, :3])
    assert torch.equal(nat.census_gray_planes(i + 0.5, i - 0.5)[1], U.census_gray(i - 0.5))
    out = torch.ones_like(f)
    g = nat.census_loss_grad(f, i + 0.1, i, None, torch.ones(2))
    assert nat.census_loss_grad(f, i + 0.1, i, None, torch.ones(2), out=out) is out and torch.equal(out, g + 1.0)


@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_op_rows():
    for op, n in (("census_gray", 3), ("census_loss", 4), ("census_loss_bwd", 5)):
        assert list(torch.ops.jax_raft_amd.op_arity(op)) == [1, n, n]
        for k in (n - 1, n + 1):
            with pytest.raises(RuntimeError, match=rf"{op}: expected {n} ints, got {k}\b"):
                getattr(torch.ops.jax_raft_amd, op)([None], [1] * k)
        assert hasattr(torch.classes.jax_raft_amd.Plan(), "add_" + op)
        with pytest.raises(RuntimeError, match=op + ":"):          # the builder's own checks name the op
            getattr(torch.ops.jax_raft_amd, op)([None], [1, 4, 4, 33, 0][:n] if n > 3 else [0, 4, 4])
        with pytest.raises(RuntimeError, match=op + ":"):
            getattr(torch.ops.jax_raft_amd, op)([torch.zeros(2 * 16 * 2)] + [None] * 6, [1, 4, 4, 2, 0][:n])   # a CPU tensor


# ------------------------------------------------------------------ trainer
KW = dict(arch="raft_small", steps=2, batch=1, iters=2, size=(128, 128), log_every=1, lr=1e-4)


def _params(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


def test_config_and_cli():
    assert TrainConfig().unsup_photo == "charbonnier" and TrainConfig.__dataclass_fields__["unsup_photo"].default == "charbonnier"
    for bad in ("ssim", "", None):
        with pytest.raises(ValueError, match="unsup_photo"):
            TrainConfig(loss="unsup", unsup_photo=bad)
    with pytest.raises(ValueError, match="unsup_photo"):
        TrainConfig(unsup_photo="ssim")
    with pytest.raises(ValueError, match="graph_step"):
        TrainConfig(loss="unsup", unsup_photo="census", graph_step=True)
    import argparse
    ns = argparse.Namespace(**{**{k: v for k, v in TrainConfig().__dict__.items() if k != "mix_weights"}, "mix": None,
                               "loss": "unsup", "unsup_photo": "census"})
    got = config_from_args(ns)
    assert got.loss == "unsup" and got.unsup_photo == "census"


def test_trainer_defaults_are_unchanged(tmp_path):
    """``unsup_photo="charbonnier"`` is the run without the field, bit for bit.  latest.json records the
    field always, at its default too: ``UNSUP_FIELDS``, the fields left out at their defaults, is pinned
    by tests/test_unsup.py (its tail must be the five float parameters, and every field outside it must
    be recorded), so the new field cannot join it; nothing reads the recorded configuration back."""
    runs = []
    for k, kw in enumerate(({}, {"unsup_photo": "charbonnier"})):
        tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / str(k)), loss="unsup", **KW, **kw), device=CPU)
        logs = []
        tr.fit(log=logs.append)
        config = json.load(open(tmp_path / str(k) / "latest.json"))["config"]
        assert config["loss"] == "unsup" and config["unsup_photo"] == "charbonnier" and "unsup_eps" not in config
        runs.append((_params(tr), [json.loads(line)["loss"] for line in logs]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])) and runs[0][1] == runs[1][1]
    tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / "s"), **KW), device=CPU)
    tr.save(str(tmp_path / "s"))
    config = json.load(open(tmp_path / "s" / "latest.json"))["config"]
    assert not set(config) & set(UNSUP_FIELDS) and config["unsup_photo"] == "charbonnier"
    tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / "c"), loss="unsup", unsup_photo="census", **KW), device=CPU)
    tr.save(str(tmp_path / "c"))
    config = json.load(open(tmp_path / "c" / "latest.json"))["config"]
    assert config["unsup_photo"] == "census" and config["loss"] == "unsup" and "unsup_eps" not in config


def test_trainer_census_cpu():
    tr = Trainer(TrainConfig(loss="unsup", unsup_photo="census", **KW), device=CPU)
    before = _params(tr)
    outs = [tr.train_step(tr.batch_for(s)) for s in range(2)]
    assert all(math.isfinite(float(o["loss"])) for o in outs) and tr.skipped == 0
    assert set(outs[-1]) == {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px"}
    after = _params(tr)
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # it is the census loss that trains: the Charbonnier run ends elsewhere
    plain = Trainer(TrainConfig(loss="unsup", **KW), device=CPU)
    first = plain.train_step(plain.batch_for(0))
    assert float(first["loss"]) != float(outs[0]["loss"])
    # the labels take no part in the gradient
    other = Trainer(TrainConfig(loss="unsup", unsup_photo="census", **KW), device=CPU)
    for s in range(2):
        i1, i2, flow, valid = other.batch_for(s)
        other.train_step((i1, i2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(a, b) for a, b in zip(after, _params(other)))
