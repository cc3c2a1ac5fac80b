"""Per-element fp64 reference tests of the training-only HIP kernels: norm_bwd (partial, final,
apply), the channel statistics and norm_act, bn_table, sum_iters, seq_loss / seq_loss_bwd,
flow_gather_bwd and upsample_bilinear_bwd.

The references, cases, tolerances and assertions live in tests/_train_refs.py and are shared
with tests/test_train_kernel_refs.py, which runs the same assertions on an fp32 CPU emulation
of the kernels.  Every comparison is per element, |got - ref| <= tol everywhere, with the
derived tolerances of that module; exact results (masked gradients, iteration sums, counts,
the loss gradient, repeated calls) are compared bitwise.

norm_bwd cases (N, HW, C, mode) and what they reach:

  (3, 1073, 96, 1)   12 channel groups do not divide 256 (4 idle threads), ragged last block and
                     ragged 4-row unroll
  (2, 5, 24, 1)      fewer rows than row groups (85), 3 channel groups
  (1, 4801, 128, 1)  301 partial blocks: the final kernel's second round and its bb < nb tail
  (6, 37, 64, 2), (4, 300, 32, 2)   BatchNorm: statistics and red summed over the batch
  (512, 2100, 8, 1)  rows per block capped at NB_ROWS (3 blocks), one channel group, 256 row groups
  (2, 333, 64, 0)    no norm: dy is the masked gradient bitwise, no stats / red
"""
import pytest
import torch

import _train_refs as T

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from jax_raft_amd.ops import native

    native.require()
    return native.ops()


def _d(x, dtype=None):
    if x is None:
        return None
    return x.to(DEV, dtype).contiguous() if dtype is not None else x.to(DEV).contiguous()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


class Gpu:
    """The HIP kernels behind the interface of tests/_train_refs.py: CPU tensors in and out;
    every output buffer starts as NaN, so an element the kernel does not write fails its check."""

    def norm_bwd(self, g, om, y, st, mode, gamma, beta, relu, gres_dtype):
        N, HW, C = y.shape
        bf = torch.bfloat16
        dy = _nan(N, HW, C, dtype=bf)
        red = _nan(N, C, 2) if mode else None
        gres = _nan(N, HW, C, dtype=gres_dtype) if gres_dtype is not None else None
        # partial = None: the op sizes its own workspace
        _ops().norm_bwd([_d(g, bf), _d(om, bf), _d(y, bf), _d(st), _d(gamma), _d(beta), red, None, dy, gres],
                        [mode, relu, N, HW, C], T.EPS)
        torch.cuda.synchronize()
        return (dy.float().cpu(), None if red is None else red.cpu(), None if gres is None else gres.cpu())

    def stats(self, x):
        N, HW, C = x.shape
        st = _nan(N, C, 2)
        _ops().stats([_d(x, torch.bfloat16), st], [N, HW, C])
        torch.cuda.synchronize()
        return st.cpu()

    def norm_act(self, x, sx, mode_x, gx, bx, r, sr, mode_r, gr, br, relu):
        N, HW, C = x.shape
        bf = torch.bfloat16
        y = _nan(N, HW, C, dtype=bf)
        _ops().norm_act([_d(x, bf), _d(sx), _d(gx), _d(bx), _d(r, bf), _d(sr), _d(gr), _d(br), y],
                        [mode_x, mode_r, N, HW, C, relu], T.EPS)
        torch.cuda.synchronize()
        return y.float().cpu()

    def bn_table(self, rows):
        # int64 [n][8] = (src, dst0, dst1, N, C, count, fp32 bits of momentum, mode), as
        # train/fused_encoder.py:_bn_table builds it
        dev = [(_d(r.src), _d(r.d0), _d(r.d1)) for r in rows]
        tab = [[s.data_ptr(), a.data_ptr(), b.data_ptr(), r.N, r.C, r.count, T.momentum_bits(r.mom), r.mode]
               for r, (s, a, b) in zip(rows, dev)]
        t = torch.tensor(tab, dtype=torch.int64).to(DEV).contiguous()
        _ops().bn_table([t] + [v for d in dev for v in d], [len(tab), max(r.C for r in rows)])
        torch.cuda.synchronize()
        return [(a.cpu(), b.cpu()) for _, a, b in dev]

    def sum_iters(self, a, b):
        T_, M = a.shape[0], a.shape[1]
        out = _nan(M, a.shape[2] + b.shape[2], dtype=torch.bfloat16)
        _ops().sum_iters([_d(a), _d(b), out], [T_, M])
        torch.cuda.synchronize()
        return out.cpu()

    def seq_loss(self, pred, gt, valid, max_flow):
        N, P = pred.shape[0], pred.shape[1]
        ops = _ops()
        nb = ops.seq_loss_blocks(P)
        assert nb == T.seq_loss_blocks_expected(P)
        part = _nan(nb, 37)
        ops.seq_loss([_d(pred), _d(gt), _d(valid), part], [P, N], max_flow)
        torch.cuda.synchronize()
        return part.cpu()

    def seq_loss_bwd(self, pred, gt, valid, max_flow, scale):
        N, P = pred.shape[0], pred.shape[1]
        grad = _nan(N, P, 2)
        _ops().seq_loss_bwd([_d(pred), _d(gt), _d(valid), _d(scale), grad], [P, N], max_flow)
        torch.cuda.synchronize()
        return grad.cpu()

    def flow_gather_bwd(self, taps, N, h, w, dcs):
        out = _nan(N * h * w, dcs, dtype=torch.bfloat16)
        _ops().flow_gather_bwd([_d(taps), out], [N, h, w])
        torch.cuda.synchronize()
        return out.float().cpu()

    def upsample_bilinear_bwd(self, g, B, h, w, dcs):
        out = _nan(B * h * w, dcs, dtype=torch.bfloat16)
        _ops().upsample_bilinear_bwd([_d(g), out], [B, h, w])
        torch.cuda.synchronize()
        return out.float().cpu()


GPU = Gpu()


@pytest.mark.parametrize("variant", T.NORM_BWD_VARIANTS)
@pytest.mark.parametrize("case", T.NORM_BWD_CASES, ids=str)
def test_norm_bwd(case, variant):
    T.check_norm_bwd(GPU, case, variant)


@pytest.mark.parametrize("case", T.STATS_CASES, ids=str)
def test_stats(case):
    T.check_stats(GPU, case)


@pytest.mark.parametrize("form", T.NORM_ACT_FORMS)
@pytest.mark.parametrize("case", T.NORM_ACT_CASES, ids=str)
def test_norm_act(case, form):
    T.check_norm_act(GPU, case, form)


def test_bn_table():
    T.check_bn_table(GPU)


@pytest.mark.parametrize("case", T.SUM_ITERS_CASES, ids=str)
def test_sum_iters(case):
    T.check_sum_iters(GPU, case)


@pytest.mark.parametrize("with_valid", [False, True], ids=["novalid", "valid"])
@pytest.mark.parametrize("case", T.SEQ_LOSS_CASES, ids=str)
def test_seq_loss(case, with_valid):
    T.check_seq_loss(GPU, case, with_valid)


@pytest.mark.parametrize("strides", T.FLOW_GATHER_STRIDES, ids=str)
@pytest.mark.parametrize("case", T.FLOW_GATHER_CASES, ids=str)
def test_flow_gather_bwd(case, strides):
    T.check_flow_gather(GPU, case, strides)


@pytest.mark.parametrize("case", T.BILINEAR_CASES, ids=str)
def test_upsample_bilinear_bwd(case):
    T.check_bilinear(GPU, case)
