"""The oracle of tests/test_train_kernels_gpu.py, checked without a GPU.

1. Every fp64 reference of tests/_train_refs.py equals fp64 ``torch.autograd`` of the plain
   forward expression (norm + affine + relu + residual mask, the sequence loss,
   ``R.upsample_flow``, the shifted-taps sum) to 1e-12 relative.
2. The tolerances of the GPU tests are attainable: an emulation of the kernels' arithmetic --
   fp32 for everything, one bf16 rounding of the output, the same inputs -- passes every
   assertion of the GPU tests (the same ``check_*`` functions, which also assert the exclusion
   caps from the reference alone before they look at a result).
"""
import pytest
import torch

import _train_refs as T
from jax_raft_amd.models import reference as R

F32 = torch.float32
F64 = torch.float64


def _close(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    return float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300)


# ============================================================================ 1. the references
def _norm_forward(y, mode, gamma, beta, eps):
    """Plain instance (1) / batch (2) / no (0) norm + affine of y [N, HW, C]."""
    if mode == 0:
        return y * gamma + beta
    dims = (1,) if mode == 1 else (0, 1)
    mean = y.mean(dims, keepdim=True)
    var = ((y - mean) ** 2).mean(dims, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * gamma + beta


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("variant", T.NORM_BWD_VARIANTS)
def test_norm_bwd_ref_is_autograd(mode, variant):
    gen = torch.Generator().manual_seed(11 + mode)
    N, HW, C = 3, 17, 8
    y = (2 * torch.randn(N, HW, C, generator=gen, dtype=F64) + 0.5).requires_grad_(True)
    gamma = (torch.rand(C, generator=gen, dtype=F64) + 0.5).requires_grad_(True)
    beta = (torch.randn(C, generator=gen, dtype=F64) * 0.3).requires_grad_(True)
    other = torch.randn(N, HW, C, generator=gen, dtype=F64).requires_grad_(True)   # the other branch
    g = torch.randn(N, HW, C, generator=gen, dtype=F64)
    if mode == 0:   # no norm has no affine either
        gamma, beta = torch.ones(C, dtype=F64, requires_grad=True), torch.zeros(C, dtype=F64, requires_grad=True)
    z = _norm_forward(y, mode, gamma, beta, T.EPS)
    z.retain_grad()
    relu = 0 if variant == "ds" else 1
    if variant == "relu":      # conv -> norm -> relu
        out, om = torch.relu(z), None
    elif variant == "res":     # relu(relu(norm(y)) + shortcut)
        out = torch.relu(torch.relu(z) + other)
        om = out.detach()
    else:                      # relu(main + norm(y)): the downsample unit
        out = torch.relu(other + z)
        om = out.detach()
    (out * g).sum().backward()
    st = T.stats_ref(y.detach())[0]   # unrounded fp64 statistics
    ref = T.norm_bwd_ref(g, om, y.detach(), st if mode else None, mode, gamma.detach() if mode else None,
                         beta.detach() if mode else None, relu)
    assert not bool(ref.amb.any())
    assert _close(ref.dy, y.grad)
    if om is not None:
        assert _close(ref.gres, other.grad)
    # red = (sum dL/dz, sum dL/dz xhat): summed over n they are the affine's gradients
    mean, rstd = T.norm_mean_rstd(st, mode, N, HW, C)
    xh = (y.detach() - mean) * rstd
    assert _close(ref.red[..., 0], z.grad.sum(1)) and _close(ref.red[..., 1], (z.grad * xh).sum(1))
    assert _close(ref.red[..., 0].sum(0), beta.grad) and _close(ref.red[..., 1].sum(0), gamma.grad)


@pytest.mark.parametrize("relu", [0, 1, 2, 3])
def test_norm_act_ref_is_the_plain_expression(relu):
    gen = torch.Generator().manual_seed(12)
    N, HW, C = 3, 19, 8
    x = 2 * torch.randn(N, HW, C, generator=gen, dtype=F64) + 0.5
    r = torch.randn(N, HW, C, generator=gen, dtype=F64)
    gx, bx, gr, br = (torch.randn(C, generator=gen, dtype=F64) for _ in range(4))
    sx, sr = T.stats_ref(x)[0], T.stats_ref(r)[0]
    one, zero = torch.ones(C, dtype=F64), torch.zeros(C, dtype=F64)

    def act(v, bit):
        return torch.relu(v) if relu & bit else v

    forms = [(1, None, 0, None, None, None, None), (1, r, 0, None, None, None, None),
             (1, r, 1, None, None, gr, br), (2, r, 2, gx, bx, gr, br)]
    for mode_x, res, mode_r, gx_, bx_, gr_, br_ in forms:
        a = act(_norm_forward(x, mode_x, one if gx_ is None else gx_, zero if bx_ is None else bx_, T.EPS), 1)
        if res is not None:
            a = a + _norm_forward(res, mode_r, one if gr_ is None else gr_, zero if br_ is None else br_, T.EPS)
        val, bound, _ = T.norm_act_ref(x, sx, mode_x, gx_, bx_, res, sr if mode_r else None, mode_r, gr_, br_, relu)
        assert _close(val, act(a, 2))
        assert bool((bound >= val.abs() * (1 - 1e-12)).all())
    # the library's own instance norm
    val, _, _ = T.norm_act_ref(x, sx, 1, None, None, None, None, 0, None, None, 0)
    assert _close(val, R.instance_norm_nhwc(x.reshape(N, HW, 1, C)).reshape(N, HW, C), 1e-6)


def test_bn_table_ref_is_the_plain_expression():
    gen = torch.Generator().manual_seed(13)
    N, HW, C = 4, 23, 8
    x = 2 * torch.randn(N, HW, C, generator=gen, dtype=F64) + 0.5
    a0, b0 = torch.randn(C, generator=gen, dtype=F64), torch.rand(C, generator=gen, dtype=F64)
    mom = float(torch.tensor(0.9, dtype=F32))
    (e0, e1), _ = T.bn_table_ref(T.stats_ref(x)[0], N * HW, 0.9, 0, a0, b0)
    assert _close(e0, mom * a0 + (1 - mom) * x.mean((0, 1)))
    assert _close(e1, mom * b0 + (1 - mom) * x.var((0, 1), unbiased=False))
    src = torch.randn(N, C, 2, generator=gen, dtype=F64)
    (e0, e1), _ = T.bn_table_ref(src, 1, 0.0, 1)
    assert _close(e0, src[..., 1].sum(0)) and _close(e1, src[..., 0].sum(0))


@pytest.mark.parametrize("with_valid", [False, True])
def test_seq_loss_ref_is_autograd(with_valid):
    from jax_raft_amd.train.loss import sequence_loss_reference

    c = T.seq_loss_inputs((1000, 5, False), with_valid)
    gamma = 0.8
    # sequence_loss_reference's expression in fp64 (the function itself casts to fp32)
    preds = c.pred.double().requires_grad_(True)
    gt = c.gt.double()
    v = gt.norm(dim=-1) < T.MAX_FLOW
    if c.valid is not None:
        v = v & (c.valid >= 0.5)
    vf = v.unsqueeze(-1).double()
    loss = sum(gamma ** (c.N - i - 1) * (vf * (preds[i] - gt).abs()).mean() for i in range(c.N))
    loss.backward()
    w = torch.tensor([gamma ** (c.N - i - 1) / (2.0 * c.P) for i in range(c.N)], dtype=F64)
    ref = T.seq_loss_ref(c.pred, c.gt, c.valid, T.MAX_FLOW, torch.ones(c.N))
    assert _close((w * ref.l1).sum(), loss.detach())
    assert _close(w[:, None, None] * ref.grad.double(), preds.grad)
    epe = (preds[-1].detach() - gt).norm(dim=-1)[v]
    assert _close(ref.epe, epe.sum())
    assert (ref.c1, ref.c3, ref.c5, ref.cnt) == (int((epe < 1).sum()), int((epe < 3).sum()), int((epe < 5).sum()),
                                                 int(v.sum()))
    # and the fp32 function the kernel was written against
    l32, m32 = sequence_loss_reference(c.pred.reshape(c.N, 1, 1, c.P, 2), c.gt.reshape(1, 1, c.P, 2),
                                       None if c.valid is None else c.valid.reshape(1, 1, c.P), gamma, T.MAX_FLOW)
    assert _close(l32, loss.detach(), 1e-5) and _close(m32["epe"], ref.epe / ref.cnt, 1e-5)
    assert _close(m32["3px"], torch.tensor(ref.c3 / ref.cnt), 1e-6)


def test_seq_loss_ref_nan_and_ties():
    pred = torch.tensor([[[1.0, float("nan")], [2.0, 2.0]], [[1.0, 0.0], [2.0, 5.0]]])
    gt = torch.tensor([[1.0, 1.0], [500.0, 2.0]])
    ref = T.seq_loss_ref(pred, gt, None, T.MAX_FLOW, torch.tensor([2.0, 3.0]))
    assert torch.isnan(ref.l1[0]) and float(ref.l1[1]) == 1.0 and ref.cnt == 1
    assert ref.grad.tolist() == [[[0.0, 0.0], [-0.0, 0.0]], [[0.0, -3.0], [-0.0, 0.0]]]


def _bilinear_matrix(n):
    """[8n, n] fp64 weights of the x8 align-corners linear interpolation along one axis."""
    W = torch.zeros(8 * n, n, dtype=F64)
    for X in range(8 * n):
        pos = X * (n - 1.0) / (8 * n - 1.0)
        i0 = min(max(int(pos // 1), 0), n - 1)
        i1 = min(i0 + 1, n - 1)
        W[X, i0] += 1.0 - (pos - i0)
        W[X, i1] += pos - i0
    return W


@pytest.mark.parametrize("case", T.BILINEAR_CASES[:3] + [(2, 5, 7)], ids=str)
def test_bilinear8_bwd_ref_is_the_weight_matrices(case):
    B, h, w = case
    g = torch.randn(B, 8 * h, 8 * w, 2, generator=torch.Generator().manual_seed(14), dtype=F64)
    val, bound = T.bilinear8_bwd_ref(g, B, h, w)
    Wy, Wx = _bilinear_matrix(h), _bilinear_matrix(w)
    assert _close(val, 8 * torch.einsum("Yy,bYXc,Xx->byxc", Wy, g, Wx).reshape(-1, 2))
    assert _close(bound, 8 * torch.einsum("Yy,bYXc,Xx->byxc", Wy, g.abs(), Wx).reshape(-1, 2))
    # the forward the adjoint belongs to
    flow = torch.randn(B, h, w, 2, generator=torch.Generator().manual_seed(15), dtype=F64)
    assert _close((R.upsample_flow(flow, None) * g).sum(), (val.reshape(B, h, w, 2) * flow).sum())


@pytest.mark.parametrize("case", T.FLOW_GATHER_CASES, ids=str)
def test_flow_gather_ref_is_autograd(case):
    N, h, w = case
    gen = torch.Generator().manual_seed(16)
    taps = torch.randn(N * h * w, 18, generator=gen, dtype=F64)
    flow = torch.zeros(N, h, w, 2, dtype=F64, requires_grad=True)
    # forward: pixel q reads its zero-padded 3x3 neighbourhood, neighbour k = flow(q + d_k)
    fp = torch.nn.functional.pad(flow.permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1)
    t = taps.reshape(N, h, w, 9, 2)
    L = sum((t[:, :, :, ky * 3 + kx] * fp[:, ky:ky + h, kx:kx + w]).sum() for ky in range(3) for kx in range(3))
    L.backward()
    val, bound = T.flow_gather_ref(taps, N, h, w)
    assert _close(val, flow.grad.reshape(-1, 2))
    assert bool((bound >= val.abs() * (1 - 1e-12)).all())


# ============================================================================ 2. fp32 emulation
def _mean_rstd32(st, mode, N, HW, C):
    """train.hip:norm_stat in fp32: [N, C] each."""
    if mode == 0:
        return torch.zeros(N, C), torch.ones(N, C)
    if mode == 1:
        inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(HW), dtype=F32)
        s0, s1 = st[..., 0], st[..., 1]
    else:
        s0, s1 = torch.zeros(C), torch.zeros(C)
        for k in range(N):
            s0, s1 = s0 + st[k, :, 0], s1 + st[k, :, 1]
        s0, s1 = s0.expand(N, C), s1.expand(N, C)
        inv = torch.tensor(1.0, dtype=F32) / (torch.tensor(float(HW), dtype=F32) * torch.tensor(float(N), dtype=F32))
    m = s0 * inv
    r = torch.rsqrt((s1 * inv - m * m).clamp_min(0.0) + T.EPS)
    assert m.dtype == F32 and r.dtype == F32
    return m, r


class Fp32:
    """The kernels' arithmetic on the CPU: fp32 for everything, one bf16 rounding of the output."""

    def norm_bwd(self, g, om, y, st, mode, gamma, beta, relu, gres_dtype):
        N, HW, C = y.shape
        m, r = _mean_rstd32(st, mode, N, HW, C)
        gam = gamma if gamma is not None else torch.ones(C)
        bet = beta if beta is not None else torch.zeros(C)
        xh = (y - m[:, None, :]) * r[:, None, :]
        gr = g if om is None else torch.where(om > 0, g, torch.zeros_like(g))
        gm = torch.where(gam * xh + bet > 0, gr, torch.zeros_like(gr)) if relu & 1 else gr
        red = None
        if mode == 0:
            dy = gm
        else:
            red = torch.stack([gm.sum(1), (gm * xh).sum(1)], -1)
            S, cnt = red, torch.tensor(float(HW), dtype=F32)
            if mode == 2:
                S = torch.zeros(C, 2)
                for k in range(N):
                    S = S + red[k]
                S, cnt = S.expand(N, C, 2), cnt * torch.tensor(float(N), dtype=F32)
            a = (r * gam)[:, None, :]
            dy = a * (gm - (S[..., 0] / cnt)[:, None, :] - xh * (S[..., 1] / cnt)[:, None, :])
        assert dy.dtype == F32
        return T.bf(dy), red, None if gres_dtype is None else gr.to(gres_dtype)

    def stats(self, x):
        return torch.stack([x.sum(1), (x * x).sum(1)], -1)

    def _coeff(self, st, mode, gam, bet, N, HW, C):
        m, a = _mean_rstd32(st, mode, N, HW, C)
        b = -m * a
        if gam is not None:
            a, b = a * gam, b * gam
        if bet is not None:
            b = b + bet
        return a[:, None, :], b[:, None, :]

    def norm_act(self, x, sx, mode_x, gx, bx, r, sr, mode_r, gr, br, relu):
        N, HW, C = x.shape
        a, b = self._coeff(sx, mode_x, gx, bx, N, HW, C)
        v = x * a + b
        if relu & 1:
            v = v.clamp_min(0.0)
        if r is not None:
            a, b = self._coeff(sr, mode_r, gr, br, N, HW, C)
            v = v + (r * a + b)
        if relu & 2:
            v = v.clamp_min(0.0)
        assert v.dtype == F32
        return T.bf(v)

    def bn_table(self, rows):
        outs = []
        for row in rows:
            C = row.C
            s = torch.zeros(C, 2)
            for n in range(row.N):
                s = s + row.src[n]
            d0, d1 = row.d0.clone(), row.d1.clone()
            if row.mode == 0:
                mom = torch.tensor(row.mom, dtype=F32)
                cnt = torch.tensor(float(row.count), dtype=F32)
                m = s[:, 0] / cnt
                v = (s[:, 1] / cnt - m * m).clamp_min(0.0)
                d0[:C] = mom * d0[:C] + (1.0 - mom) * m
                d1[:C] = mom * d1[:C] + (1.0 - mom) * v
            else:
                d0[:C], d1[:C] = s[:, 1], s[:, 0]
            outs.append((d0, d1))
        return outs

    def sum_iters(self, a, b):
        return torch.cat([a.float().cumsum(0)[-1], b.float().cumsum(0)[-1]], -1).to(torch.bfloat16)

    @staticmethod
    def _valid(gt, valid, max_flow):
        ok = torch.sqrt(gt[:, 0] * gt[:, 0] + gt[:, 1] * gt[:, 1]) < max_flow
        return ok if valid is None else ok & (valid >= 0.5)

    def seq_loss(self, pred, gt, valid, max_flow):
        N = pred.shape[0]
        ok = self._valid(gt, valid, max_flow)
        d = pred - gt
        part = torch.zeros(1, 37)
        part[0, :N] = (ok.float()[None, :] * (d[..., 0].abs() + d[..., 1].abs())).sum(1)
        e = torch.sqrt(d[-1, :, 0] * d[-1, :, 0] + d[-1, :, 1] * d[-1, :, 1])[ok]
        part[0, 32:] = torch.stack([e.sum(), (e < 1).sum(), (e < 3).sum(), (e < 5).sum(), ok.sum()])
        return part

    def seq_loss_bwd(self, pred, gt, valid, max_flow, scale):
        ok = self._valid(gt, valid, max_flow)
        s = torch.where(ok[None, :, None], scale[:, None, None], torch.zeros(()))
        return torch.where(pred > gt, s, torch.where(pred < gt, -s, torch.zeros(()))).contiguous()

    def flow_gather_bwd(self, taps, N, h, w, dcs):
        t = taps.reshape(N, h, w, -1)
        out = torch.zeros(N, h, w, dcs)
        for y in range(h):
            for x in range(w):
                for kh in range(3):
                    for kw in range(3):
                        yy, xx = y - (kh - 1), x - (kw - 1)
                        if 0 <= yy < h and 0 <= xx < w:
                            k = 2 * (kh * 3 + kw)
                            out[:, y, x, :2] += t[:, yy, xx, k:k + 2]
        return T.bf(out.reshape(-1, dcs))

    @staticmethod
    def _window_matrix(n):
        """train.hip:src_window in fp32: [8n, n] weights of one axis."""
        X = torch.arange(8 * n, dtype=F32)
        sc = (torch.tensor(float(n - 1), dtype=F32) / torch.tensor(float(8 * n - 1), dtype=F32)) if n > 1 \
            else torch.tensor(0.0, dtype=F32)
        xi = X * sc
        x0 = torch.floor(xi).long().clamp(0, n - 1)
        x1 = (x0 + 1).clamp(max=n - 1)
        f = xi - x0.float()
        W = torch.zeros(8 * n, n)
        W.scatter_add_(1, x0[:, None], (1.0 - f)[:, None])
        W.scatter_add_(1, x1[:, None], f[:, None])
        return W

    def upsample_bilinear_bwd(self, g, B, h, w, dcs):
        Wy, Wx = self._window_matrix(h), self._window_matrix(w)
        out = torch.zeros(B * h * w, dcs)
        out[:, :2] = 8.0 * torch.einsum("Yy,bYXc,Xx->byxc", Wy, g, Wx).reshape(-1, 2)
        return T.bf(out)


EMU = Fp32()


@pytest.mark.parametrize("variant", T.NORM_BWD_VARIANTS)
@pytest.mark.parametrize("case", T.NORM_BWD_CASES, ids=str)
def test_emulated_norm_bwd(case, variant):
    T.check_norm_bwd(EMU, case, variant)


@pytest.mark.parametrize("case", T.STATS_CASES, ids=str)
def test_emulated_stats(case):
    T.check_stats(EMU, case)


@pytest.mark.parametrize("form", T.NORM_ACT_FORMS)
@pytest.mark.parametrize("case", T.NORM_ACT_CASES, ids=str)
def test_emulated_norm_act(case, form):
    T.check_norm_act(EMU, case, form)


def test_emulated_bn_table():
    T.check_bn_table(EMU)


@pytest.mark.parametrize("case", T.SUM_ITERS_CASES, ids=str)
def test_emulated_sum_iters(case):
    T.check_sum_iters(EMU, case)


@pytest.mark.parametrize("with_valid", [False, True], ids=["novalid", "valid"])
@pytest.mark.parametrize("case", T.SEQ_LOSS_CASES, ids=str)
def test_emulated_seq_loss(case, with_valid):
    T.check_seq_loss(EMU, case, with_valid)


@pytest.mark.parametrize("strides", T.FLOW_GATHER_STRIDES, ids=str)
@pytest.mark.parametrize("case", T.FLOW_GATHER_CASES, ids=str)
def test_emulated_flow_gather_bwd(case, strides):
    T.check_flow_gather(EMU, case, strides)


@pytest.mark.parametrize("case", T.BILINEAR_CASES, ids=str)
def test_emulated_upsample_bilinear_bwd(case):
    T.check_bilinear(EMU, case)


def test_a_wrong_divisor_fails():
    """The tolerance is not vacuous either way: the BatchNorm mean taken over HW instead of N HW
    (what a norm_bwd apply kernel without its ``cnt *= N`` computes) fails the dy check."""

    class Wrong(Fp32):
        def norm_bwd(self, g, om, y, st, mode, gamma, beta, relu, gres_dtype):
            dy, red, gres = super().norm_bwd(g, om, y, st, mode, gamma, beta, relu, gres_dtype)
            if mode == 2:
                ref = T.norm_bwd_ref(g, om, y, st, mode, gamma, beta, relu)
                N = y.shape[0]
                S = ref.red.sum(0) / float(y.shape[1])   # not / (N HW)
                mean, rstd = T.norm_mean_rstd(st, mode, N, y.shape[1], y.shape[2])
                xh = (y.double() - mean) * rstd
                gm = ref.gres * ((gamma.double() * xh + beta.double()) > 0) if relu & 1 else ref.gres
                dy = T.bf((rstd * gamma.double() * (gm - S[:, 0] - xh * S[:, 1])).float())
            return dy, red, gres

    with pytest.raises(AssertionError, match="dy error / tolerance"):
        T.check_norm_bwd(Wrong(), (6, 37, 64, 2), "relu")
