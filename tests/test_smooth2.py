"""Second-order smoothness on the CPU: the golden op (train/unsup.py, ``smooth_order=2``) against the
explicit-formula fp64 reference of _smooth2_refs.py, the fp32 golden op and an fp32 emulation of the
kernels' operation order under the same checks (the tolerances are attainable) and three wrong variants
(they are not vacuous), affine flow, ``smooth_order=1`` bitwise the old call, direct optimisation of a
flow field, and the trainer switch."""
import json
import math

import pytest
import torch

import _smooth2_refs as S
import _unsup_refs as R
from _train_refs import U_ACC, bits_equal, ratio
from jax_raft_amd.ops import native as nat
from jax_raft_amd.train import smooth2_sums, unsup_loss, unsup_loss_reference
from jax_raft_amd.train import trainer as T
from jax_raft_amd.train import unsup as U
from jax_raft_amd.train.data import SyntheticFlow
from jax_raft_amd.train.trainer import UNSUP_FIELDS, TrainConfig, Trainer, config_from_args, main

CPU = torch.device("cpu")
SMALL = [c for c in S.CASES if c[2] * c[3] < 10000]


def test_cases_and_exports():
    import jax_raft_amd.train as TR

    assert TR.smooth2_sums is smooth2_sums and "smooth2_sums" in TR.__all__
    assert U.SMOOTH_ORDERS == (1, 2)
    assert nat.smooth2_loss_blocks(1) == 1 and nat.smooth2_loss_blocks(257) == 2 and nat.smooth2_loss_blocks(10 ** 7) == 1024
    assert nat.UNSUP_GRID_X * nat.UNSUP_BLOCK == S.GRID and nat.UNSUP_BLOCK == S.BLOCK
    # the issue's cases, and the regions the gradient's slope term is about
    assert [c[:4] for c in S.CASES] == [(1, 1, 1, 1), (2, 1, 1, 2), (2, 1, 2, 9), (2, 1, 9, 2), (1, 1, 3, 3), (3, 2, 13, 37),
                                        (5, 2, 40, 72), (32, 1, 24, 40), (12, 2, 40, 72), (5, 1, 516, 512)]
    c = S.inputs((5, 2, 40, 72, False))
    f = c.pred
    D = (f[:, :, :, 2:] - f[:, :, :, 1:-1]) - (f[:, :, :, 1:-1] - f[:, :, :, :-2])
    assert bool((D[:, :, 10:20, 18:52] == 0).all()) and bool((f[:, :, 10:20, 18:54] == torch.round(f[:, :, 10:20, 18:54])).all())
    assert bool((f[:, :, 20:30, :36] == torch.tensor([1.25, -0.75])).all())
    assert torch.equal(c.img1, c.img1.to(torch.bfloat16).float())


# ------------------------------------------------------------------ the golden op
@pytest.mark.parametrize("case", SMALL, ids=str)
def test_golden_fp64_autograd_equals_the_explicit_formulas(case):
    c, ref = S.inputs(case), S.smooth2_ref(case)
    f = c.pred.double().requires_grad_(True)
    s = smooth2_sums(f, c.img1.double(), S.EPS_S, S.KAPPA)
    assert s.shape == (c.N, 2) and s.dtype == torch.float64
    (g,) = torch.autograd.grad((s.sum(-1) * c.scale.double()).sum(), f)
    tiny = 2.0 ** -40 / U_ACC                                        # fp64 rounding, of the fp32 tolerances
    finite = torch.isfinite(ref.grad)
    assert torch.equal(torch.isfinite(g), finite)
    assert ratio(g, ref.grad, tiny * ref.tol, finite) <= 1.0
    ok = torch.isfinite(ref.sums)
    assert torch.equal(torch.isfinite(s.detach()), ok)
    assert ratio(s.detach(), ref.sums, tiny * U_ACC * ref.bounds, ok) <= 1.0


class Golden:
    """The fp32 golden op through the CPU path of the native front ends."""
    blocks = False

    def smooth2_loss(self, pred, img1, prm):
        return nat.smooth2_loss_partials(pred, img1, prm[1], prm[2])

    def smooth2_loss_bwd(self, pred, img1, prm, scale):
        return nat.smooth2_loss_grad(pred, img1, scale, prm[1], prm[2])


class Emulated:
    """fp32 torch ops in the kernels' operation order (csrc/kernels/smooth2.hip), one row of partials.
    ``stride`` (of the image difference in the edge weight), ``centre`` (the centre's coefficient) and ``flat``
    (triples on the flattened index) make the wrong variants."""
    blocks = False

    def __init__(self, stride=2, centre=2.0, flat=False):
        self.stride, self.centre, self.flat = stride, centre, flat

    def _axes(self, f, img1):
        """Per axis: (the flow, its gradient's shape, the image, the axis) as (., n, ., C) grids along whose
        axis the triples run."""
        B, H, W, _ = f.shape
        if self.flat:                                                  # wrong: a row's end runs into the next row
            return ((lambda t: t.reshape(1, 1, B * H * W, -1), 2), (lambda t: t.reshape(1, B * H, W, -1), 1))
        return ((lambda t: t, 2), (lambda t: t, 1))

    @staticmethod
    def _ends(t, axis):
        n = t.shape[axis]
        cut = lambda lo: t.narrow(axis, lo if n >= 3 else 0, max(n - 2, 0))
        return cut(0), cut(1), cut(2)

    def _weight(self, img, axis, kappa):
        p, m, q = self._ends(img, axis)
        d = ((q if self.stride == 2 else m) - p).abs()
        return torch.exp(-kappa * (((d[..., 0] + d[..., 1]) + d[..., 2]) / 3.0)).unsqueeze(-1)

    def smooth2_loss(self, pred, img1, prm):
        _, eps_s, kappa, _ = prm
        N = pred.shape[0]
        es2 = torch.tensor(eps_s) ** 2
        part = torch.full((1, N, 4), float("nan"))
        for i in range(N):
            row = []
            for shape, axis in self._axes(pred[i], img1):
                f0, f1, f2 = self._ends(shape(pred[i]), axis)
                d = (f2 - f1) - (f1 - f0)
                r = torch.sqrt(d * d + es2)
                row.append((self._weight(shape(img1), axis, kappa) * (r[..., :1] + r[..., 1:])).sum())
            part[0, i] = torch.stack(row + [torch.zeros(()), torch.zeros(())])
        return part

    def smooth2_loss_bwd(self, pred, img1, prm, scale):
        _, eps_s, kappa, _ = prm
        N = pred.shape[0]
        es2 = torch.tensor(eps_s) ** 2
        grad = torch.full(pred.shape, float("nan"))
        for i in range(N):
            s = torch.zeros(pred.shape[1:])
            for shape, axis in self._axes(pred[i], img1):
                f0, f1, f2 = self._ends(shape(pred[i]), axis)
                d = (f2 - f1) - (f1 - f0)
                t = self._weight(shape(img1), axis, kappa) * (d / torch.sqrt(d * d + es2))
                left, mid, right = self._ends(shape(s), axis)           # views of s
                left += t
                mid -= self.centre * t
                right += t
            grad[i] = scale[i] * s
        return grad


@pytest.mark.parametrize("case", S.CASES, ids=str)
@pytest.mark.parametrize("impl", [Golden(), Emulated()], ids=["golden", "emulated"])
def test_fp32_implementations_pass_the_kernel_checks(impl, case):
    S.check_partials(impl, case)
    S.check_grad(impl, case)


WRONG = {"stride-1-edge-weight": (Emulated(stride=1), True), "centre-coefficient-1": (Emulated(centre=1.0), False),
         "flattened-triples": (Emulated(flat=True), True)}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_variants_fail_the_same_checks(wrong):
    impl, fwd_fails = WRONG[wrong]
    case = (3, 2, 13, 37, False)
    S.check_partials(Emulated(), case)
    S.check_grad(Emulated(), case)
    if fwd_fails:
        with pytest.raises(AssertionError, match="error / tolerance"):
            S.check_partials(impl, case)
    else:
        S.check_partials(impl, case)
    with pytest.raises(AssertionError, match="error / tolerance"):
        S.check_grad(impl, case)


# ------------------------------------------------------------------ conventions
def test_affine_flow_is_free_at_second_order_only():
    """An affine flow has no second difference: every triple pays the floor ``rho_s(0) = eps_s`` and gives no
    gradient, while the first-order term charges the slope."""
    B, H, W = 2, 12, 17
    ys, xs = torch.arange(H, dtype=torch.float64).view(1, H, 1), torch.arange(W, dtype=torch.float64).view(1, 1, W)
    f = torch.stack([0.25 * xs - 0.5 * ys + 3.0, 0.125 * xs + 0.75 * ys - 1.0], -1).expand(B, H, W, 2)[None].contiguous()
    img = torch.zeros(B, H, W, 3, dtype=torch.float64)                  # every edge weight is 1
    f.requires_grad_(True)
    s2 = smooth2_sums(f, img, S.EPS_S, S.KAPPA)
    triples = torch.tensor([[2.0 * B * H * (W - 2), 2.0 * B * (H - 2) * W]], dtype=torch.float64)
    assert torch.allclose(s2.detach(), S.EPS_S * triples, rtol=1e-9, atol=0.0)
    (g,) = torch.autograd.grad(s2.sum(), f)
    assert float(g.abs().max()) < 1e-9
    s1 = U.smooth_sums(f.detach(), img, S.EPS_S, S.KAPPA)
    pairs = B * H * (W - 1) * (0.25 + 0.125) + B * (H - 1) * W * (0.5 + 0.75)
    assert torch.allclose(s1, torch.tensor([pairs], dtype=torch.float64), rtol=1e-4)
    # ... and through the loss: the smooth metric of either order
    kw = dict(smooth_weight=1.0, eps_s=S.EPS_S)
    _, m2 = unsup_loss_reference(f.detach().float(), img.float(), img.float(), smooth_order=2, **kw)
    _, m1 = unsup_loss_reference(f.detach().float(), img.float(), img.float(), **kw)
    P = B * H * W
    assert torch.allclose(m2["smooth"].double(), S.EPS_S * triples.sum() / (2 * P), rtol=1e-4)
    assert torch.allclose(m1["smooth"].double(), torch.tensor(pairs / (2 * P), dtype=torch.float64), rtol=1e-4)


def test_smooth_order_argument():
    c = R.unsup_inputs((3, 2, 13, 37, False), True)
    kw = dict(gamma=0.7, eps=0.02, eps_s=0.002, edge_kappa=8.0, smooth_weight=0.08, out_penalty=0.4)
    w = 0.7 ** torch.arange(c.N - 1, -1, -1, dtype=torch.float64)
    for photo in U.PHOTO:
        for fn in (unsup_loss_reference, unsup_loss):
            outs = []
            for extra in ({}, {"smooth_order": 1}):
                f = c.pred.clone().requires_grad_(True)
                loss, mets = fn(f, c.img1, c.img2, c.mask, photo=photo, **kw, **extra)
                loss.backward()
                outs.append((loss.detach(), f.grad, mets))
            assert bits_equal(outs[0][0], outs[1][0]) and bits_equal(outs[0][1], outs[1][1])
            assert all(bits_equal(outs[0][2][k], outs[1][2][k]) for k in ("photo", "smooth", "inside"))
            second, m2 = fn(c.pred, c.img1, c.img2, c.mask, photo=photo, **kw, smooth_order=2)
            assert not torch.equal(second, outs[0][0])
            for k in ("photo", "inside"):                            # only the smoothness column changes
                assert bits_equal(m2[k], outs[0][2][k]), k
            for bad in (0, 3, "2", None, 2.0, True):
                with pytest.raises(ValueError, match="smooth_order"):
                    fn(c.pred, c.img1, c.img2, c.mask, photo=photo, smooth_order=bad)
        # the loss is the sums assembled as stated: the photometric column as it was, the smoothness column the new sums
        s2 = smooth2_sums(c.pred, c.img1, 0.002, 8.0)
        if photo == "census":
            col = U.census_sums(c.pred, c.img1, c.img2, c.mask, 0.4)[:, 0]
        else:
            col = U.unsup_sums(c.pred, c.img1, c.img2, c.mask, 0.02, 0.002, 8.0, 0.4)[:, 0]
        want = (w.float() * (col / c.P + 0.08 * (s2.sum(-1) / (2.0 * c.P)))).sum()
        got, mets = unsup_loss_reference(c.pred, c.img1, c.img2, c.mask, photo=photo, smooth_order=2, **kw)
        assert torch.allclose(got, want, rtol=1e-6)
        assert torch.allclose(mets["smooth"], s2[-1].sum() / (2.0 * c.P), rtol=1e-6)


def test_a_non_finite_prediction_makes_the_loss_nan():
    i1, i2, _, _ = SyntheticFlow((24, 40), seed=1).batch([0])
    for shape, at in (((3, 1, 24, 40, 2), (1, 0, 5, 7, 1)), ((3, 1, 24, 40, 2), (1, 0, 23, 39, 0))):
        for photo in U.PHOTO:
            g = torch.zeros(shape)
            g[at] = float("inf")
            loss, _ = unsup_loss_reference(g, i1, i2, mask=torch.zeros(1, 24, 40), photo=photo, smooth_order=2)
            assert math.isnan(float(loss)), (at, photo)
    # ... also where there is no triple at all: the photometric term's 0 * (f.x + f.y)
    g = torch.zeros(1, 1, 2, 2, 2)
    g[0, 0, 1, 1, 0] = float("nan")
    img = torch.zeros(1, 2, 2, 3)
    assert not smooth2_sums(g, img).any()
    assert math.isnan(float(unsup_loss_reference(g, img, img, smooth_order=2)[0]))


def test_direct_optimisation_recovers_the_flow():
    """Measured on the CPU (golden op, fp32): EPE 0.703 -> 0.116 px after 400 Adam steps (the first-order term's
    test, tests/test_unsup.py, reaches 0.703 -> 0.040: a second-order penalty does not pull a noisy field towards
    its neighbours' values, only towards their slope).  The bound is that test's: a quarter of the start, 0.176."""
    i1, i2, flow, _ = SyntheticFlow((64, 96), seed=5, max_motion=1.0).batch([0, 1])
    f = torch.zeros_like(flow).requires_grad_(True)
    opt = torch.optim.Adam([f], lr=0.05)
    epe = lambda: float((f.detach() - flow).norm(dim=-1).mean())
    start = epe()
    for _ in range(400):
        opt.zero_grad()
        loss, _ = unsup_loss(f[None], i1, i2, smooth_weight=0.05, out_penalty=0.5, smooth_order=2)
        loss.backward()
        opt.step()
    print(f"EPE {start:.3f} -> {epe():.3f}")
    assert epe() < 0.25 * start


def test_front_end_checks():
    f, i = torch.zeros(2, 1, 8, 9, 2), torch.zeros(1, 8, 9, 3)
    for bad in ((f[0], i), (f, i[:, :3]), (f, i.long()), (f, None)):
        with pytest.raises(ValueError, match="smooth2_loss:"):
            nat.smooth2_loss_partials(*bad)
        with pytest.raises(ValueError, match="smooth2_loss_bwd:"):
            nat.smooth2_loss_grad(*bad, torch.ones(2))
    for bad in (torch.zeros(3), torch.zeros(2, 2), None):
        with pytest.raises(ValueError, match="smooth2_loss_bwd: scale"):
            nat.smooth2_loss_grad(f, i, bad)
    with pytest.raises(ValueError, match="smooth2_loss_bwd: out"):
        nat.smooth2_loss_grad(f, i, torch.ones(2), out=torch.zeros(2, 1, 8, 8, 2))
    part = nat.smooth2_loss_partials(f + 0.5, i)
    assert part.shape == (1, 2, 4) and part.dtype == torch.float32 and not part[..., 2:].any()
    assert torch.equal(part[0, :, :2], smooth2_sums(f + 0.5, i))
    g0 = torch.randn(2, 1, 8, 9, 2, generator=torch.Generator().manual_seed(0))
    out = torch.ones_like(f)
    g = nat.smooth2_loss_grad(g0, i + 0.1, torch.ones(2))
    assert g.any() and nat.smooth2_loss_grad(g0, i + 0.1, torch.ones(2), out=out) is out and torch.equal(out, g + 1.0)


@pytest.mark.skipif(not nat.available(), reason="native library not built")
def test_op_rows():
    for op, n in (("smooth2_loss", 4), ("smooth2_loss_bwd", 5)):
        assert list(torch.ops.jax_raft_amd.op_arity(op)) == [1, n, n]
        for k in (n - 1, n + 1):
            with pytest.raises(RuntimeError, match=rf"{op}: expected {n} ints, got {k}\b"):
                getattr(torch.ops.jax_raft_amd, op)([None], [1] * k)
        assert hasattr(torch.classes.jax_raft_amd.Plan(), "add_" + op)
        with pytest.raises(RuntimeError, match=op + ":"):          # the builder's own checks name the op
            getattr(torch.ops.jax_raft_amd, op)([None], [1, 4, 4, 33, 0][:n])
        with pytest.raises(RuntimeError, match=op + ":"):
            getattr(torch.ops.jax_raft_amd, op)([torch.zeros(2 * 16 * 2)] + [None] * 4, [1, 4, 4, 2, 0][:n])   # a CPU tensor


# ------------------------------------------------------------------ trainer
KW = dict(arch="raft_small", steps=2, batch=1, iters=2, size=(128, 128), log_every=1, lr=1e-4)


def _params(tr):
    return [p.detach().clone() for p in tr.model.parameters()]


def test_config_and_cli(monkeypatch):
    assert TrainConfig().unsup_smooth_order == 1 and TrainConfig.__dataclass_fields__["unsup_smooth_order"].default == 1
    assert TrainConfig(loss="unsup", unsup_smooth_order=2).unsup_smooth_order == 2
    for bad in (0, 3, "2", None, 2.0, True):
        with pytest.raises(ValueError, match="unsup_smooth_order"):
            TrainConfig(loss="unsup", unsup_smooth_order=bad)
    with pytest.raises(ValueError, match="unsup_smooth_order"):
        TrainConfig(unsup_smooth_order=2)                            # takes loss="unsup"
    with pytest.raises(ValueError, match="unsup_smooth_order"):
        TrainConfig(unsup_smooth_order=3)
    with pytest.raises(ValueError, match="graph_step"):
        TrainConfig(loss="unsup", unsup_smooth_order=2, graph_step=True)
    assert UNSUP_FIELDS[0] == "loss" and len(UNSUP_FIELDS) == 6      # the tuple is left as it is
    import argparse
    ns = argparse.Namespace(**{**{k: v for k, v in TrainConfig().__dict__.items() if k != "mix_weights"}, "mix": None,
                               "loss": "unsup", "unsup_smooth_order": 2})
    got = config_from_args(ns)
    assert got.loss == "unsup" and got.unsup_smooth_order == 2
    # the command line itself
    seen = []
    monkeypatch.setattr(T, "Trainer", lambda cfg: seen.append(cfg) or type("Stub", (), {"fit": lambda self: None})())
    main(["--loss", "unsup", "--unsup-smooth-order", "2"])
    main(["--loss", "unsup"])
    assert [c.unsup_smooth_order for c in seen] == [2, 1] and seen[0].loss == "unsup"
    for bad in ("3", "two"):
        with pytest.raises(SystemExit):
            main(["--loss", "unsup", "--unsup-smooth-order", bad])


def test_trainer_defaults_are_unchanged(tmp_path):
    """``unsup_smooth_order=1`` is the run without the field, bit for bit; latest.json records the field always."""
    runs = []
    for k, kw in enumerate(({}, {"unsup_smooth_order": 1})):
        tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / str(k)), loss="unsup", **KW, **kw), device=CPU)
        logs = []
        tr.fit(log=logs.append)
        config = json.load(open(tmp_path / str(k) / "latest.json"))["config"]
        assert config["loss"] == "unsup" and config["unsup_smooth_order"] == 1 and "unsup_eps" not in config
        runs.append((_params(tr), [json.loads(line)["loss"] for line in logs]))
    assert all(torch.equal(a, b) for a, b in zip(runs[0][0], runs[1][0])) and runs[0][1] == runs[1][1]
    tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / "s"), **KW), device=CPU)
    tr.save(str(tmp_path / "s"))
    config = json.load(open(tmp_path / "s" / "latest.json"))["config"]
    assert not set(config) & set(UNSUP_FIELDS) and config["unsup_smooth_order"] == 1
    tr = Trainer(TrainConfig(ckpt_dir=str(tmp_path / "c"), loss="unsup", unsup_smooth_order=2, **KW), device=CPU)
    tr.save(str(tmp_path / "c"))
    config = json.load(open(tmp_path / "c" / "latest.json"))["config"]
    assert config["unsup_smooth_order"] == 2 and config["loss"] == "unsup" and "unsup_eps" not in config


def _spy(monkeypatch):
    seen = []
    real = T.unsup_loss

    def spy(preds, *a, **k):
        loss, mets = real(preds, *a, **k)
        seen.append((preds.detach().clone(), a, loss.detach().clone(), k))
        return loss, mets

    monkeypatch.setattr(T, "unsup_loss", spy)
    return seen


def test_trainer_second_order_cpu(monkeypatch):
    seen = _spy(monkeypatch)
    tr = Trainer(TrainConfig(loss="unsup", unsup_smooth_order=2, **KW), device=CPU)
    before = _params(tr)
    batches = [tr.batch_for(s) for s in range(2)]
    outs = [tr.train_step(b) for b in batches]
    assert all(math.isfinite(float(o["loss"])) for o in outs) and tr.skipped == 0
    assert set(outs[-1]) == {"loss", "grad_norm", "photo", "smooth", "inside", "epe", "1px", "3px", "5px"}
    after = _params(tr)
    assert not all(torch.equal(a, b) for a, b in zip(before, after))
    # the step-1 loss is the second-order loss of that step's own predictions
    preds, _, loss, k = seen[0]
    assert k == {"smooth_order": 2}
    cfg = tr.cfg
    i1, i2 = batches[0][:2]
    again, mets = unsup_loss_reference(preds, i1, i2, None, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s, cfg.unsup_edge_kappa,
                                       cfg.unsup_smooth_weight, cfg.unsup_out_penalty, smooth_order=2)
    assert bits_equal(again, loss) and bits_equal(outs[0]["loss"], loss) and bits_equal(outs[0]["smooth"], mets["smooth"])
    P = preds[0].numel() // 2
    w = cfg.gamma ** torch.arange(preds.shape[0] - 1, -1, -1, dtype=torch.float64)
    col = U.unsup_sums(preds, i1, i2, None, cfg.unsup_eps, cfg.unsup_eps_s, cfg.unsup_edge_kappa, cfg.unsup_out_penalty)[:, 0]
    s2 = smooth2_sums(preds, i1, cfg.unsup_eps_s, cfg.unsup_edge_kappa).sum(-1)
    assert torch.allclose(loss, (w.float() * (col / P + cfg.unsup_smooth_weight * s2 / (2.0 * P))).sum(), rtol=1e-6)
    # it is the second-order loss that trains: the first-order run ends elsewhere
    monkeypatch.undo()
    plain = Trainer(TrainConfig(loss="unsup", **KW), device=CPU)
    first = plain.train_step(plain.batch_for(0))
    assert float(first["loss"]) != float(outs[0]["loss"]) and float(first["photo"]) == float(outs[0]["photo"])
    # the labels take no part in the gradient
    other = Trainer(TrainConfig(loss="unsup", unsup_smooth_order=2, **KW), device=CPU)
    for s in range(2):
        a, b, flow, valid = other.batch_for(s)
        other.train_step((a, b, flow * -3.0 + 7.0, 1.0 - valid))
    assert all(torch.equal(a, b) for a, b in zip(after, _params(other)))


@pytest.mark.parametrize("extra,want", [({"unsup_photo": "census"}, {"photo": "census", "smooth_order": 2}),
                                        ({"unsup_occlusion": "range"}, {"smooth_order": 2})], ids=["census", "range"])
def test_trainer_second_order_with_the_other_switches_cpu(monkeypatch, extra, want):
    seen = _spy(monkeypatch)
    tr = Trainer(TrainConfig(loss="unsup", unsup_smooth_order=2, **{**KW, "steps": 1}, **extra), device=CPU)
    out = tr.train_step(tr.batch_for(0))
    assert math.isfinite(float(out["loss"])) and tr.skipped == 0 and len(seen) == 1
    preds, a, loss, k = seen[0]
    assert k == want
    again, _ = unsup_loss_reference(preds, *a, **k)
    assert bits_equal(again, loss)
    first, _ = unsup_loss_reference(preds, *a, **{**k, "smooth_order": 1})
    assert not torch.equal(first, loss)
