"""Self-supervision for label-free training on the CPU: the golden ops of train/selfsup.py (crop_resize
against an independent formula and exact properties, the loss against explicit fp64 formulas and under
the derived tolerances of _selfsup_refs.py, wrong variants that must fail them), the geometry on
SyntheticFlow, the front ends' host checks, the three op rows and the trainer switch."""
import argparse
import json
import math

import pytest
import torch
import torch.nn.functional as F

import _selfsup_refs as R
from _train_refs import bits_equal
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import crop_resize, lands_inside, selfsup_loss, selfsup_loss_reference, selfsup_sums, visibility_masks
from jax_raft_amd.train import selfsup as S
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train.data import SyntheticFlow
from jax_raft_amd.train.trainer import UNSUP_FIELDS, TrainConfig, Trainer, config_from_args
from jax_raft_amd.train.unsup import sample_image, unsup_loss

CPU = torch.device("cpu")
NAN = float("nan")


# ------------------------------------------------------------------ crop_resize
@pytest.mark.parametrize("case", R.CROP_CASES)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_crop_resize_against_interpolate_and_fp64(case, C):
    B, H, W, c = case
    x = R.crop_input(case, C)
    got = crop_resize(x, c)
    assert got.shape == x.shape and got.dtype == torch.float32
    # an independent formula: torch's own bilinear resize of the crop.  Its coordinate is scale * (u + 0.5) - 0.5 with
    # scale = float(Wc) / float(W), a correctly rounded fp32 quotient of two exact integers: the same fp32 number as
    # the fp64 quotient rounded once, so the coordinates agree and only the two forms of the blend differ, by a few
    # roundings of values no larger than the range: 8 ulps of the value range.
    crop = x[:, c:H - c, c:W - c]
    want = F.interpolate(crop.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    rng = float(crop.abs().max())
    tol = 8 * 2.0 ** -23 * rng
    err = float((got - want).abs().max())
    print(f"crop_resize{case} C={C}: |golden - interpolate| = {err:.3e} = {err / (2.0 ** -23 * rng):.2f} ulps of the range, "
          f"bound {tol:.3e}")
    assert err <= tol
    ref, bound = R.crop_ref(x, c)
    assert R.ratio(got, ref, R.U_ACC * bound) <= 1.0
    # fp64 in, fp64 out; the coordinates stay the fp32 ones
    assert torch.equal(crop_resize(x.double(), c), ref)


@pytest.mark.parametrize("case", R.CROP_CASES)
def test_crop_resize_exact_properties(case):
    B, H, W, c = case
    Hc, Wc = H - 2 * c, W - 2 * c
    assert bool((crop_resize(torch.ones(B, H, W, 3), c) == 1.0).all())
    # a constant flow comes back as the constant times the scale, one product
    tx, ty = 1.7, -2.3
    flow = torch.tensor([tx, ty]).expand(B, H, W, 2).contiguous()
    sx, sy = S.flow_scale(H, W, c)
    assert (sx, sy) == (float(R.np.float32(W / Wc)), float(R.np.float32(H / Hc)))
    got = crop_resize(flow, c, (sx, sy))
    want = torch.tensor([tx, ty]) * torch.tensor([sx, sy])
    assert bool((got == want).all())
    assert abs(float(got[0, 0, 0, 0]) - tx * W / Wc) < 1e-6 and abs(float(got[0, 0, 0, 1]) - ty * H / Hc) < 1e-6
    # a linear ramp comes back linear: value = ramp(c + xs, c + ys) at the op's own source coordinates
    ys, xs = torch.arange(H, dtype=torch.float32).view(1, H, 1, 1), torch.arange(W, dtype=torch.float32).view(1, 1, W, 1)
    ramp = (0.5 * xs - 0.25 * ys + 3.0).expand(B, H, W, 1).contiguous()
    rx, ry = R.ratios(H, W, c)
    sxs = ((torch.arange(W, dtype=torch.float32) + 0.5) * float(rx) - 0.5).clamp(0, Wc - 1).double()
    sys_ = ((torch.arange(H, dtype=torch.float32) + 0.5) * float(ry) - 0.5).clamp(0, Hc - 1).double()
    lin = 0.5 * (c + sxs).view(1, 1, W, 1) - 0.25 * (c + sys_).view(1, H, 1, 1) + 3.0
    _, bound = R.crop_ref(ramp, c)
    assert R.ratio(crop_resize(ramp, c), lin.expand(B, H, W, 1), R.U_ACC * bound) <= 1.0
    # nothing outside the crop is read
    x = R.crop_input(case, 3, seed=1)
    poisoned = torch.full_like(x, NAN)
    poisoned[:, c:H - c, c:W - c] = x[:, c:H - c, c:W - c]
    got = crop_resize(poisoned, c)
    assert bool(torch.isfinite(got).all()) and bits_equal(got, crop_resize(x, c))


def test_crop_resize_host_checks():
    x = torch.zeros(1, 8, 9, 3)
    for bad_c in (0, -1, 4, 5, 1.0, True):
        with pytest.raises(ValueError, match="crop_resize"):
            nat.crop_resize(x, bad_c)
    for bad in (torch.zeros(8, 9, 3), torch.zeros(1, 8, 9, 5), torch.zeros(1, 8, 9, 3, dtype=torch.int32), None):
        with pytest.raises(ValueError, match="crop_resize"):
            nat.crop_resize(bad, 1)
    with pytest.raises(ValueError, match="scale"):
        nat.crop_resize(x, 1, (1.0, 2.0))
    with pytest.raises(ValueError, match="out"):
        nat.crop_resize(x, 1, out=torch.zeros(1, 8, 9, 2))
    out = torch.full_like(x, NAN)
    assert nat.crop_resize(x + 1.0, 2, out=out) is out and bool((out == 1.0).all())
    assert bits_equal(nat.crop_resize(x, 1), crop_resize(x, 1))            # the CPU front end is the golden op


# ------------------------------------------------------------------ the loss
class Golden:
    """The fp32 golden op behind the front ends (CPU tensors)."""
    blocks = False

    def selfsup_loss(self, stack, target, weight, eps, b0):
        return nat.selfsup_loss_partials(stack, target, weight, eps, batch0=b0)

    def selfsup_loss_bwd(self, stack, target, weight, eps, scale, b0):
        return nat.selfsup_loss_grad(stack, target, weight, scale, eps, batch0=b0)

    def step_loss(self, teacher, Tp, Sp, preds, c, gamma, eps):
        H, W = teacher.shape[1:3]
        target = crop_resize(teacher, c, S.flow_scale(H, W, c))
        weight = crop_resize(Tp.unsqueeze(-1), c).squeeze(-1) * (1.0 - Sp)
        return selfsup_loss_reference(preds, target, weight, gamma, eps)[0]


class Emulated(Golden):
    """The kernels' operation order in fp32: d, d * d + eps^2 with eps^2 one fp32 product, the root, the sum of the
    two components, the product with the weight; the gradient as (scale * weight) * (d / root)."""

    def _parts(self, stack, target, weight, eps, b0):
        B = target.shape[0]
        p = stack[:, b0:b0 + B]
        w = torch.ones(target.shape[:3]) if weight is None else weight
        e2 = torch.tensor(eps, dtype=torch.float32) * torch.tensor(eps, dtype=torch.float32)
        on = w > 0
        d = p - torch.where(on.unsqueeze(-1), target, torch.zeros(()))
        return p, w, on, d, torch.sqrt(d * d + e2)

    def selfsup_loss(self, stack, target, weight, eps, b0):
        p, w, on, d, r = self._parts(stack, target, weight, eps, b0)
        term = torch.where(on, w * (r[..., 0] + r[..., 1]), 0.0 * (p[..., 0] + p[..., 1]))
        part = torch.zeros(1, p.shape[0], 4)
        part[0, :, 0] = term.flatten(1).double().sum(1).float()
        part[0, -1, 1], part[0, -1, 2], part[0, -1, 3] = part[0, -1, 0], w[on].double().sum().float(), float(on.sum())
        return part

    def selfsup_loss_bwd(self, stack, target, weight, eps, scale, b0):
        p, w, on, d, r = self._parts(stack, target, weight, eps, b0)
        sw = scale.view(-1, 1, 1, 1) * w
        return torch.where(on.unsqueeze(-1), sw.unsqueeze(-1) * (d / r), 0.0 * p)


class NotRescaled(Golden):
    def step_loss(self, teacher, Tp, Sp, preds, c, gamma, eps):
        weight = crop_resize(Tp.unsqueeze(-1), c).squeeze(-1) * (1.0 - Sp)
        return selfsup_loss_reference(preds, crop_resize(teacher, c), weight, gamma, eps)[0]


class StudentValid(Golden):
    def step_loss(self, teacher, Tp, Sp, preds, c, gamma, eps):
        H, W = teacher.shape[1:3]
        weight = crop_resize(Tp.unsqueeze(-1), c).squeeze(-1) * Sp
        return selfsup_loss_reference(preds, crop_resize(teacher, c, S.flow_scale(H, W, c)), weight, gamma, eps)[0]


class WeightMean(Golden):
    def step_loss(self, teacher, Tp, Sp, preds, c, gamma, eps):
        H, W = teacher.shape[1:3]
        weight = crop_resize(Tp.unsqueeze(-1), c).squeeze(-1) * (1.0 - Sp)
        loss = selfsup_loss_reference(preds, crop_resize(teacher, c, S.flow_scale(H, W, c)), weight, gamma, eps)[0]
        return loss * weight.numel() / weight.sum()


@pytest.mark.parametrize("impl", [Golden(), Emulated()], ids=["golden", "emulated"])
@pytest.mark.parametrize("case", R.LOSS_CASES_CPU)
def test_loss_under_the_derived_tolerances(impl, case):
    R.check_loss(impl, case)
    R.check_loss_bwd(impl, case)


@pytest.mark.parametrize("impl", [Golden(), Emulated()], ids=["golden", "emulated"])
def test_loss_nan_cases(impl):
    """Weight 0 with a NaN target contributes nothing; weight 0 with a NaN prediction gives a NaN sum in its
    iteration and a non-finite gradient at that pixel only."""
    R.check_loss(impl, R.NAN_CASE, nan=True)
    R.check_loss_bwd(impl, R.NAN_CASE, nan=True)
    c = R.loss_inputs(R.NAN_CASE, True)
    clean = R.loss_inputs(R.NAN_CASE, False)
    i = R.NAN_PRED_AT[0]
    a = impl.selfsup_loss(c.stack, c.target, c.weight, R.EPS, 0)
    w0 = clean.weight.clone()
    w0[R.NAN_TARGET_AT], w0[R.NAN_PRED_AT[1:]] = 0.0, 0.0
    b = impl.selfsup_loss(clean.stack, clean.target, w0, R.EPS, 0)
    keep = [k for k in range(c.N) if k != i]
    assert bits_equal(a[:, keep], b[:, keep])                # the NaN target changed nothing


def test_fp64_autograd_is_the_explicit_formula():
    c = R.loss_inputs(R.NAN_CASE, True)
    f = c.stack.double().requires_grad_(True)
    sums = selfsup_sums(f, c.target.double(), c.weight.double(), R.EPS)
    (sums[:, 0] * c.scale.double()).sum().backward()
    ref = R.loss_ref(R.NAN_CASE, True)
    fin = torch.isfinite(ref.sums)
    assert torch.equal(torch.isfinite(sums), fin) and torch.allclose(sums[fin].detach(), ref.sums[fin], rtol=1e-13, atol=0)
    gfin = torch.isfinite(ref.grad)
    assert torch.equal(torch.isfinite(f.grad), gfin) and int((~gfin).sum()) == 1
    assert torch.allclose(f.grad[gfin], ref.grad[gfin], rtol=1e-12, atol=1e-18)
    loss, mets = selfsup_loss_reference(f.detach()[:2], c.target.double(), c.weight.double(), 0.8, R.EPS)
    s = R.loss_formulas(c.stack[:2], c.target, c.weight, R.EPS)
    assert math.isclose(float(loss), float(0.8 * s[0, 0] + s[1, 0]) / c.P, rel_tol=1e-12)
    assert math.isclose(float(mets["selfsup"]), float(s[1, 0] / s[1, 2]), rel_tol=1e-12)
    assert math.isclose(float(mets["selfsup_w"]), float(s[1, 3]) / c.P, rel_tol=1e-12)
    # no selected pixel: a zero loss, a NaN mean, a zero share
    loss, mets = selfsup_loss_reference(c.stack[:2, :, :3, :3].clamp(-5, 5).nan_to_num(), c.target[:, :3, :3].nan_to_num(),
                                        torch.zeros(2, 3, 3))
    assert float(loss) == 0.0 and math.isnan(float(mets["selfsup"])) and float(mets["selfsup_w"]) == 0.0


def test_step_composition_and_wrong_variants():
    R.check_step(Golden())
    for wrong in (NotRescaled(), StudentValid(), WeightMean()):
        with pytest.raises(AssertionError, match="error / tolerance"):
            R.check_step(wrong)


def test_loss_host_checks_and_front_end():
    p, t, w = torch.zeros(2, 3, 4, 5, 2), torch.zeros(2, 4, 5, 2), torch.zeros(2, 4, 5)
    for args in ((p[0], t[:3], None), (p, t[:, :3], None), (p, t, w[:, :3]), (p, t.long(), None), (p.long(), t, None),
                 (p, t.clone().requires_grad_(True), None)):
        with pytest.raises(ValueError, match="selfsup_loss"):
            selfsup_loss(*args)
    for b0 in (-1, 2, 1.0):
        with pytest.raises(ValueError, match="batch window"):
            nat.selfsup_loss_partials(p, t, None, batch0=b0)
    with pytest.raises(ValueError, match="scale"):
        nat.selfsup_loss_grad(p, t[:1], None, torch.zeros(3), batch0=1)
    # a window of the stack is the same call on its copy
    c = R.loss_inputs(R.LOSS_CASES[6])
    a = nat.selfsup_loss_partials(c.stack, c.target, c.weight, R.EPS, batch0=c.B0)
    b = nat.selfsup_loss_partials(c.stack[:, c.B0:c.B0 + c.B].contiguous(), c.target, c.weight, R.EPS)
    assert bits_equal(a, b)
    # the autograd front end on the CPU is the golden op
    f = c.stack[:, c.B0:c.B0 + c.B].clone().requires_grad_(True)
    loss, mets = selfsup_loss(f, c.target, c.weight, 0.8, R.EPS)
    want, _ = selfsup_loss_reference(f.detach(), c.target, c.weight, 0.8, R.EPS)
    assert bits_equal(loss.detach(), want) and set(mets) == {"selfsup", "selfsup_w"}
    # the batch window of a stack is found without a copy
    stack, b0 = S.batch_window(c.stack[:, c.B0:c.B0 + c.B])
    assert stack.data_ptr() == c.stack.data_ptr() and b0 == c.B0
    assert S.batch_window(c.stack[:, :, 1:]) is None and S.batch_window(c.stack)[1] == 0


@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_op_rows():
    """The three rows of the op table: both forms, the arity, and the builders' own checks (no GPU)."""
    for op, n in (("crop_resize", 5), ("selfsup_loss", 6), ("selfsup_loss_bwd", 6)):
        assert list(torch.ops.jax_raft_amd.op_arity(op)) == [1, n, n]
        assert hasattr(torch.classes.jax_raft_amd.Plan(), "add_" + op)
        for k in (n - 1, n + 1):
            with pytest.raises(RuntimeError, match=rf"{op}: expected {n} ints, got {k}\b"):
                getattr(torch.ops.jax_raft_amd, op)([None], [1] * k)
    for ints in ([1, 8, 8, 4, 1], [1, 8, 8, 3, 0], [1, 8, 8, 3, 4], [70000, 8, 8, 1, 1]):
        with pytest.raises(RuntimeError, match="crop_resize:"):
            torch.ops.jax_raft_amd.crop_resize([None], ints)
    with pytest.raises(RuntimeError, match="crop_resize:"):
        torch.ops.jax_raft_amd.crop_resize([torch.zeros(1, 8, 8, 3), torch.zeros(6), torch.zeros(1, 8, 8, 3)], [1, 8, 8, 3, 1])
    for op in ("selfsup_loss", "selfsup_loss_bwd"):
        for ints in ([0, 1, 4, 4, 1, 0], [33, 1, 4, 4, 1, 0], [1, 2, 4, 4, 3, 2], [1, 1, 4, 4, 1, -1], [1, 1, 1 << 16, 1 << 16, 1, 0]):
            with pytest.raises(RuntimeError, match=op + ":"):
                getattr(torch.ops.jax_raft_amd, op)([None], ints)
        with pytest.raises(RuntimeError, match=op + ":"):      # a CPU tensor
            getattr(torch.ops.jax_raft_amd, op)([torch.zeros(1, 1, 4, 4, 2)] + [None] * 5, [1, 1, 4, 4, 1, 0])


# ------------------------------------------------------------------ geometry
def test_student_frames_agree_under_the_target():
    """The student's image 2 warped by the target reproduces the student's image 1 on the visible interior.
    With I the bilinear interpolant of image 2, both sides approximate I(q + f(q)) at the source point q of
    the student's pixel: image 1 at the (up to) four texels around q is I at points within (1 + L) pixels per
    axis of q + f(q) (L: the flow's largest difference between neighbours), and the warp reads the student's
    image 2 within one student pixel (less than a frame pixel) of a landing that is off by at most L, the
    interpolated flow's error.  I moves by at most G per pixel and axis (G: image 2's largest difference
    between neighbours), so the two sides differ by at most 2 G (1 + L) + 2 G (1 + L)."""
    c, H, W = 16, 96, 128
    i1, i2, flow, valid = SyntheticFlow(size=(H, W), seed=3, max_motion=6.0).batch([0, 1])
    s1, s2 = crop_resize(i1, c), crop_resize(i2, c)
    target = crop_resize(flow, c, S.flow_scale(H, W, c))
    inside, warped = sample_image(target, s2)
    # visible interior: every texel behind the student's pixel is valid, and the landing stays off the border
    ok = (crop_resize(valid.unsqueeze(-1), c).squeeze(-1) == 1.0) & lands_inside(target)
    px = torch.arange(W).view(1, 1, W) + target[..., 0]
    py = torch.arange(H).view(1, H, 1) + target[..., 1]
    ok &= (px >= 1) & (px <= W - 2) & (py >= 1) & (py <= H - 2)
    assert float(ok.float().mean()) > 0.5
    G = max(float((i2[:, 1:] - i2[:, :-1]).abs().max()), float((i2[:, :, 1:] - i2[:, :, :-1]).abs().max()))
    L = max(float((flow[:, 1:] - flow[:, :-1]).abs().max()), float((flow[:, :, 1:] - flow[:, :, :-1]).abs().max()))
    bound = 4.0 * G * (1.0 + L)
    err = (warped - s1).abs().amax(-1)[ok]
    plain = (sample_image(crop_resize(flow, c), s2)[1] - s1).abs().amax(-1)[ok]       # the flow not rescaled
    print(f"selfsup geometry: max error {float(err.max()):.4f}, mean {float(err.mean()):.5f}, bound {bound:.4f} "
          f"(G = {G:.4f}, L = {L:.4f}); without the rescaling: mean {float(plain.mean()):.5f}")
    assert float(err.max()) <= bound
    assert float(err.mean()) < 0.25 * float(plain.mean())


# ------------------------------------------------------------------ trainer
KW = dict(arch="raft_small", steps=2, batch=1, iters=2, size=(128, 128), log_every=1, lr=1e-4)
ON = dict(loss="unsup", unsup_occlusion="range", unsup_selfsup_weight=0.3, unsup_selfsup_crop=16)
OLD_KEYS = {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px", "visible"}
FIELDS = {"unsup_selfsup_weight": 0.0, "unsup_selfsup_crop": 64, "unsup_selfsup_after": 0, "unsup_selfsup_eps": 0.001}


def _params(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


def test_config_and_cli():
    d = TrainConfig()
    assert {k: getattr(d, k) for k in FIELDS} == FIELDS
    for kw in ({"unsup_selfsup_weight": 0.5}, {"unsup_selfsup_crop": 32}, {"unsup_selfsup_after": 5}, {"unsup_selfsup_eps": 0.01}):
        with pytest.raises(ValueError, match="unsup_selfsup"):
            TrainConfig(**kw)
        TrainConfig(loss="unsup", unsup_occlusion="range", **kw)
    with pytest.raises(ValueError, match="unsup_occlusion"):
        TrainConfig(loss="unsup", unsup_selfsup_weight=0.5)
    with pytest.raises(ValueError, match="unsup_selfsup_weight"):
        TrainConfig(loss="unsup", unsup_occlusion="range", unsup_selfsup_weight=-0.1)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="unsup_selfsup_crop"):
            TrainConfig(loss="unsup", unsup_occlusion="range", unsup_selfsup_crop=bad)
    with pytest.raises(ValueError, match="graph_step"):
        TrainConfig(graph_step=True, **ON)
    for bad in (0.0, -0.001, float("nan")):
        with pytest.raises(ValueError, match="unsup_selfsup_eps"):
            TrainConfig(unsup_selfsup_eps=bad, **ON)
    with pytest.raises(ValueError, match="unsup_selfsup_after"):
        TrainConfig(unsup_selfsup_after=-1, **ON)
    with pytest.raises(ValueError, match="unsup_selfsup_crop"):      # 128 - 2 * 40 = 48 pixels are left
        Trainer(TrainConfig(**{**KW, **ON, "unsup_selfsup_crop": 40}), device=CPU)
    assert UNSUP_FIELDS[0] == "loss" and len(UNSUP_FIELDS) == 6
    ap = argparse.ArgumentParser()
    for name, typ in (("weight", float), ("crop", int), ("after", int), ("eps", float)):
        ap.add_argument(f"--unsup-selfsup-{name}", type=typ, default=FIELDS[f"unsup_selfsup_{name}"])
    cli = vars(ap.parse_args(["--unsup-selfsup-weight", "0.25", "--unsup-selfsup-crop", "48", "--unsup-selfsup-after", "7",
                              "--unsup-selfsup-eps", "0.002"]))
    ns = argparse.Namespace(**{**{k: v for k, v in TrainConfig().__dict__.items() if k != "mix_weights"}, "mix": None,
                               "loss": "unsup", "unsup_occlusion": "fb", **cli})
    got = config_from_args(ns)
    assert (got.unsup_selfsup_weight, got.unsup_selfsup_crop, got.unsup_selfsup_after, got.unsup_selfsup_eps) == (0.25, 48, 7, 0.002)
    # the trainer's own parser has the four options: each is parsed, and reaches the config's checks
    for argv in (["--unsup-selfsup-weight", "0.5"], ["--unsup-selfsup-crop", "32"], ["--unsup-selfsup-after", "3"],
                 ["--unsup-selfsup-eps", "0.01"]):
        with pytest.raises(ValueError, match="take loss='unsup'"):
            T.main(argv)
    with pytest.raises(ValueError, match="unsup_selfsup_crop"):
        T.main(["--loss", "unsup", "--unsup-occlusion", "range", "--unsup-selfsup-crop", "0"])


def test_weight_zero_is_the_run_without_the_fields(tmp_path):
    runs = []
    base = dict(loss="unsup", unsup_occlusion="range")
    for k, kw in enumerate(({}, {"unsup_selfsup_weight": 0.0, "unsup_selfsup_crop": 16, "unsup_selfsup_after": 1})):
        tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / str(k)), **KW, **base, **kw), device=CPU)
        logs = []
        tr.fit(log=logs.append)
        lines = [json.loads(line) for line in logs]
        assert all(OLD_KEYS <= set(line) and "selfsup" not in line for line in lines)
        config = json.load(open(tmp_path / str(k) / "latest.json"))["config"]
        assert {f: config[f] for f in FIELDS} == {**FIELDS, **kw}
        runs.append((_params(tr), [line["loss"] for line in lines], [sorted(line) for line in lines]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])) and runs[0][1:] == runs[1][1:]
    # a default (supervised) run records the four fields too
    tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / "s"), **KW), device=CPU)
    tr.save(str(tmp_path / "s"))
    config = json.load(open(tmp_path / "s" / "latest.json"))["config"]
    assert {f: config[f] for f in FIELDS} == FIELDS and not set(config) & set(UNSUP_FIELDS)


def _spies(monkeypatch):
    seen = {"unsup": [], "selfsup": [], "batch": []}
    real_u, real_s = T.unsup_loss, S.selfsup_loss

    def spy_u(preds, a, b, mask, *rest, **k):
        loss, mets = real_u(preds, a, b, mask, *rest, **k)
        seen["unsup"].append((preds.detach().clone(), a, b, None if mask is None else mask.clone(), loss.detach().clone()))
        return loss, mets

    def spy_s(preds, target, weight, *rest):
        loss, mets = real_s(preds, target, weight, *rest)
        seen["selfsup"].append((preds.detach().clone(), target.clone(), weight.clone(), rest, loss.detach().clone()))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy_u)
    monkeypatch.setattr(S, "selfsup_loss", spy_s)
    return seen


def _watch_model(tr, seen):
    real = tr.model.forward

    def forward(image1, image2, *a, **k):
        seen["batch"].append((image1.detach().clone(), image2.detach().clone()))
        return real(image1, image2, *a, **k)

    tr.model.forward = forward


@pytest.mark.parametrize("kind,photo", [("range", "charbonnier"), ("fb", "charbonnier"), ("range", "census")])
def test_trainer_step_cpu(kind, photo, monkeypatch):
    seen = _spies(monkeypatch)
    cfg_kw = {**KW, **ON, "unsup_occlusion": kind, "unsup_photo": photo}
    tr = Trainer(TrainConfig(**cfg_kw), device=CPU)
    _watch_model(tr, seen)
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(2)]
    outs = [tr.train_step(b) for b in batches]
    after = _params(tr)
    assert tr.skipped == 0 and all(math.isfinite(float(o["loss"])) for o in outs)
    assert all(set(o) == OLD_KEYS | {"selfsup", "selfsup_w"} for o in outs)
    assert all(0.0 <= float(o["selfsup_w"]) <= 1.0 for o in outs)
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # step 1: ONE model call over 4B pairs -- the full frames of both directions, then their crops
    B, c, cfg = 1, 16, tr.cfg
    i1, i2 = batches[0][:2]
    assert len(seen["batch"]) == 2 and len(seen["unsup"]) == 2 and len(seen["selfsup"]) == 2
    a, b = torch.cat([i1, i2]), torch.cat([i2, i1])
    m1, m2 = seen["batch"][0]
    assert torch.equal(m1, torch.cat([a, crop_resize(a, c)])) and torch.equal(m2, torch.cat([b, crop_resize(b, c)]))
    full, ua, ub, mask, unsup = seen["unsup"][0]
    student, target, weight, rest, term = seen["selfsup"][0]
    assert full.shape == student.shape == (2, 2 * B, 128, 128, 2) and torch.equal(ua, a) and torch.equal(ub, b)
    assert rest == (cfg.gamma, cfg.unsup_selfsup_eps)
    # the existing half: the masks and the loss of the full frames, as _occlusion_loss computes them
    vis = torch.cat(visibility_masks(full[-1, :B], full[-1, B:], kind, cfg.unsup_occ_thr))
    assert torch.equal(mask, vis) and bits_equal(outs[0]["visible"], vis.mean())
    again, _ = unsup_loss(full, a, b, vis, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s, cfg.unsup_edge_kappa,
                          cfg.unsup_smooth_weight, cfg.unsup_out_penalty, photo=photo)
    assert bits_equal(again, unsup)
    # the target, the weight and the term, recomputed
    H = W = 128
    Tp = vis * lands_inside(full[-1]).float()
    want_t = crop_resize(full[-1], c, S.flow_scale(H, W, c))
    Sp = torch.cat(visibility_masks(student[-1, :B], student[-1, B:], kind, cfg.unsup_occ_thr)) * lands_inside(student[-1]).float()
    want_w = crop_resize(Tp.unsqueeze(-1), c).squeeze(-1) * (1.0 - Sp)
    assert bits_equal(target, want_t) and bits_equal(weight, want_w)
    want_term, want_m = selfsup_loss_reference(student, want_t, want_w, cfg.gamma, cfg.unsup_selfsup_eps)
    assert bits_equal(term, want_term) and bits_equal(outs[0]["loss"], unsup + cfg.unsup_selfsup_weight * want_term)
    assert bits_equal(outs[0]["selfsup_w"], want_m["selfsup_w"])
    # the supervised metrics are the forward direction's of the full frames
    from jax_raft_amd.train.loss import sequence_loss
    _, sup = sequence_loss(full[:, :B], batches[0][2], batches[0][3], cfg.gamma, cfg.max_flow)
    assert bits_equal(outs[0]["epe"], sup["epe"])
    if (kind, photo) != ("range", "charbonnier"):
        return
    # the labels take no part in the gradient
    monkeypatch.undo()
    other = Trainer(TrainConfig(**cfg_kw), device=CPU)
    for j1, j2, flow, valid in batches:
        other.train_step((j1, j2, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(p, q) for p, q in zip(after, _params(other)))


def test_trainer_starts_after(monkeypatch):
    seen = _spies(monkeypatch)
    tr = Trainer(TrainConfig(**{**KW, **ON, "steps": 3, "unsup_selfsup_after": 1, "unsup_occ_after": 2}), device=CPU)
    _watch_model(tr, seen)
    outs = [tr.train_step(tr.batch_for(s)) for s in range(3)]
    assert [m1.shape[0] for m1, _ in seen["batch"]] == [2, 4, 4]              # 2B pairs, then 4B from the step on
    assert "selfsup" not in outs[0] and all("selfsup" in o for o in outs[1:])
    assert len(seen["selfsup"]) == 2
    # step 2 (before unsup_occ_after): no mask, T and S are lands_inside alone
    full, _, _, mask, _ = seen["unsup"][1]
    student, target, weight, _, _ = seen["selfsup"][0]
    assert mask is None
    want_w = crop_resize(lands_inside(full[-1]).float().unsqueeze(-1), 16).squeeze(-1) * (1.0 - lands_inside(student[-1]).float())
    assert bits_equal(weight, want_w)
    assert seen["unsup"][2][3] is not None
