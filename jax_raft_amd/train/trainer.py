"""Data-parallel RAFT training (BASELINE config 5: raft_large, FlyingChairs-
shaped 384x512 pairs, sequence loss over 12 iterations, RCCL gradient
all-reduce).  The reference has no training code; this
follows the original RAFT recipe: AdamW + one-cycle LR (linear anneal, 5%
warm-up), gradient clipping at 1.0, gamma = 0.8, max_flow = 400.

Run (one process per GPU)::

    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 -m jax_raft_amd.train.trainer \\
        --arch raft_large --steps 1000 --batch 6 --iters 12

Without ``--data`` the batches are ``SyntheticFlow``.  ``--data <root> [--dataset chairs |
sintel-clean | sintel-final] [--stage chairs | things | sintel] [--no-augment]`` trains on files:
the raw frames are uploaded as they are and cropped + augmented in one gather on the device
(train/datasets.py, train/augment.py); every batch is a pure function of (seed, step, rank).
``--dataset kitti | hd1k`` (sparse ground truth, frames of several sizes) takes ``--stage kitti``
(crop 288x960) or ``--stage sintel`` and the sparse augmentation op.  ``--dataset things --stage
things`` is FlyingThings3D (both passes; ``things-clean`` / ``things-final``: one).  ``--dataset mix
--stage sintel [--mix name[:weight],...]`` is RAFT's Sintel stage: dense and sparse lists drawn into
the same batches (default ``sintel-clean:100,sintel-final:100,kitti:200,hd1k:5,things-clean:1``, each
part in ``Sintel``, ``KITTI``, ``HD1K`` or ``FlyingThings3D`` under the root) through the mixed op.

Validation on held-out data: ``--val name=root[,name=root...]`` (names ``chairs-val``, ``sintel-clean``,
``sintel-final``, ``kitti``) evaluates the model after every ``--val-every`` steps and after the last one
(``eval/validate.py:evaluate``: inference through the engine, metrics reduced on the device) and logs a JSON
line with a ``"val"`` key; with ``--ckpt-dir`` the lines also go to ``<dir>/val.jsonl``.  ``--chairs-split FILE``
trains ``--dataset chairs`` on the label-1 pairs of FlyingChairs' split file only, which ``chairs-val`` asks for.

Without ground truth: ``--loss unsup`` trains on the photometric + edge-aware smoothness loss of
``train/unsup.py`` (``--unsup-eps``, ``--unsup-eps-s``, ``--unsup-edge-kappa``, ``--unsup-smooth-weight``,
``--unsup-out-penalty``; ``--unsup-photo census`` replaces the colour difference by the soft census term of
UnFlow / SMURF; ``--unsup-smooth-order 2`` penalises second differences of the flow instead of first ones, UFlow's
and SMURF's choice on KITTI; ``--gamma`` weights the iterations as ever), with augmentation records that keep
brightness constancy.  ``--unsup-occlusion fb | range`` runs both directions in the step (2 x batch pairs
through the model) and leaves the occluded pixels out of the photometric term (train/occlusion.py;
``--unsup-occ-thr``: the range map's threshold, ``--unsup-occ-after``: the first step with masks).
``--unsup-selfsup-weight W`` (> 0; with ``--unsup-occlusion``) adds self-supervision (train/selfsup.py): from step
``--unsup-selfsup-after`` on the model also runs on the centre crop (``--unsup-selfsup-crop``: the margin in pixels) of
both directions, 4 x batch pairs in one call, and the cropped student is pulled towards the full frame's flow
(``--unsup-selfsup-eps``: the Charbonnier eps).  ``--dataset frames`` lists the consecutive frames of every directory under ``--data``
(no flow files; ``--loss unsup`` only).  On a labelled set the step also reports ``epe`` / ``1px`` / ``3px`` /
``5px``, which take no part in the gradient.

Checkpoints: ``<dir>/step_<n>.msgpack`` (Flax-format weights, loadable with
``raft_large(weights=...)``) + ``step_<n>.opt.pt`` (optimizer / scheduler
state, tensors only) + ``latest.json``; ``--resume`` continues from latest.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from dataclasses import asdict, dataclass, field
from typing import Dict, Optional

import torch

from .. import raft_large, raft_small
from ..parallel import dp
from ..utils import checkpoint as ckpt
from .data import SyntheticFlow
from .loss import sequence_loss
from .unsup import unsup_loss


@dataclass
class TrainConfig:
    arch: str = "raft_large"
    steps: int = 100
    batch: int = 6                 # per GPU
    iters: int = 12
    size: tuple = (384, 512)
    lr: float = 4e-4
    weight_decay: float = 1e-4
    eps: float = 1e-8
    clip: float = 1.0
    gamma: float = 0.8
    max_flow: float = 400.0
    seed: int = 0
    log_every: int = 10
    ckpt_dir: Optional[str] = None
    ckpt_every: int = 0
    resume: bool = False
    freeze_bn: bool = False
    sync_bn: bool = False          # synchronised BatchNorm statistics across DP ranks
    bucket_mb: float = 32.0
    skip_nonfinite: bool = True    # drop a step whose (all-reduced) gradient is NaN/Inf
    max_skipped: int = 10          # ... but abort after this many consecutive drops
    fault_nan_step: int = -1       # fault injection: poison the loss of this step (tests)
    # GPU, one rank: replay the whole step (fwd + bwd + clip + AdamW) as one captured graph.
    # Bitwise equal to the eager step, but measured slower on MI355X / ROCm 7 (config 5:
    # 259-265 vs 288 pairs/s: the native plans' own hipGraphs + eager PyTorch glue beat
    # one ~2000-node graph), so off by default.
    graph_step: bool = False
    graph_warmup: int = 3          # eager steps before the capture (plan build, autotune, allocator warm-up)
    # Real data (train/datasets.py, train/augment.py).  data=None: SyntheticFlow, as ever.
    data: Optional[str] = None     # dataset root
    # chairs | things[-clean | -final] | sintel-clean | sintel-final | kitti | hd1k (sparse ground truth) | mix
    dataset: str = "chairs"
    # augmentation preset, dense: chairs | things | sintel, sparse: kitti | sintel; sets size when size is left at its default
    stage: str = "chairs"
    augment: bool = True           # False: identity records, i.e. a random crop + normalisation only
    # dataset="mix" (RAFT's Sintel stage): the parts, each in its directory under data (Sintel, KITTI, HD1K,
    # FlyingThings3D), and their integer weights; None: RAFT's (100, 100, 200, 5, 1 for the default parts)
    mix: tuple = ("sintel-clean", "sintel-final", "kitti", "hd1k", "things-clean")
    mix_weights: Optional[tuple] = None
    # Validation on held-out splits (eval/validate.py).  The defaults mean none, as ever.
    val: tuple = ()                # "name=root" strings: chairs-val | sintel-clean | sintel-final | kitti
    val_every: int = 0             # validate after every val_every-th step and after the last; 0: after the last only
    val_iters: int = 0             # 0: the protocol's default of each split
    val_batch: int = 4             # batch size of the dense validation splits
    val_max_pairs: Optional[int] = None
    # a FlyingChairs split file: dataset="chairs" then lists its label-1 (training) pairs only
    chairs_split: Optional[str] = None
    # The training loss: "sequence" (supervised, as ever) | "unsup" (train/unsup.py: photometric + edge-aware
    # smoothness on every iteration's prediction, weighted by gamma; the batch's flow and valid take no part
    # in the gradient).  The unsup_* defaults are placeholders: nothing here to tune them on.
    loss: str = "sequence"
    unsup_eps: float = 0.01
    unsup_eps_s: float = 0.001
    unsup_edge_kappa: float = 10.0
    unsup_smooth_weight: float = 0.05
    unsup_out_penalty: float = 0.5
    unsup_photo: str = "charbonnier"   # the photometric term: "charbonnier" | "census" (7x7 soft census, SMURF's constants)
    # the smoothness term's order: 1 | 2 (second differences over triples, UFlow's / SMURF's choice on KITTI); both use
    # unsup_smooth_weight, whose default is a placeholder for either
    unsup_smooth_order: int = 1
    # Occlusion masks for the photometric term (train/occlusion.py): "none" | "fb" (forward-backward consistency) |
    # "range" (the range map; unsup_occ_thr = the share of a pixel that must map back onto it).  The model then runs
    # both directions as one batch of 2 * batch pairs; the masks apply from step unsup_occ_after on.
    unsup_occlusion: str = "none"
    unsup_occ_thr: float = 0.5
    unsup_occ_after: int = 0
    # Self-supervision (train/selfsup.py): from step unsup_selfsup_after on the model also runs on the centre crop
    # (margin unsup_selfsup_crop, resampled to the frame) of both directions -- 4 * batch pairs in ONE model call --
    # and the cropped "student" is pulled towards the full frame's detached flow where the teacher is valid and the
    # student cannot verify its own flow; the term enters the loss with unsup_selfsup_weight (0: off, as ever).
    unsup_selfsup_weight: float = 0.0
    unsup_selfsup_crop: int = 64
    unsup_selfsup_after: int = 0
    unsup_selfsup_eps: float = 0.001

    def __post_init__(self):
        selfsup = (self.unsup_selfsup_weight, self.unsup_selfsup_crop, self.unsup_selfsup_after, self.unsup_selfsup_eps)
        if self.loss != "unsup" and selfsup != (0.0, 64, 0, 0.001):
            raise ValueError("unsup_selfsup_weight, unsup_selfsup_crop, unsup_selfsup_after and unsup_selfsup_eps take "
                             "loss='unsup'")
        if self.unsup_selfsup_weight < 0:
            raise ValueError(f"unsup_selfsup_weight must not be negative, got {self.unsup_selfsup_weight}")
        if isinstance(self.unsup_selfsup_crop, bool) or not isinstance(self.unsup_selfsup_crop, int) or self.unsup_selfsup_crop < 1:
            raise ValueError(f"unsup_selfsup_crop must be an int of at least 1, got {self.unsup_selfsup_crop!r}")
        if not self.unsup_selfsup_eps > 0:                 # eps = 0 would give 0 / 0 where the student is on the target
            raise ValueError(f"unsup_selfsup_eps must be above 0, got {self.unsup_selfsup_eps}")
        if self.unsup_selfsup_after < 0:
            raise ValueError(f"unsup_selfsup_after must not be negative, got {self.unsup_selfsup_after}")
        if self.unsup_selfsup_weight > 0 and self.unsup_occlusion == "none":
            raise ValueError("unsup_selfsup_weight > 0 takes unsup_occlusion 'fb' or 'range': the teacher's and the "
                             "student's masks need both directions")
        if self.unsup_occlusion not in ("none", "fb", "range"):
            raise ValueError(f"unknown unsup_occlusion {self.unsup_occlusion!r} (none, fb or range)")
        if self.loss != "unsup" and (self.unsup_occlusion, self.unsup_occ_thr, self.unsup_occ_after) != ("none", 0.5, 0):
            raise ValueError("unsup_occlusion, unsup_occ_thr and unsup_occ_after take loss='unsup'")
        if self.unsup_photo not in ("charbonnier", "census"):
            raise ValueError(f"unknown unsup_photo {self.unsup_photo!r} (charbonnier or census)")
        if (isinstance(self.unsup_smooth_order, bool) or not isinstance(self.unsup_smooth_order, int)
                or self.unsup_smooth_order not in (1, 2)):
            raise ValueError(f"unknown unsup_smooth_order {self.unsup_smooth_order!r} (1 or 2)")
        if self.loss != "unsup" and self.unsup_smooth_order != 1:
            raise ValueError("unsup_smooth_order takes loss='unsup'")
        if self.loss not in ("sequence", "unsup"):
            raise ValueError(f"unknown loss {self.loss!r} (sequence or unsup)")
        if self.loss == "unsup" and self.graph_step:
            raise ValueError("loss 'unsup' is not supported together with graph_step")
        if self.data is not None and self.dataset == "frames" and self.loss == "sequence":
            raise ValueError("dataset 'frames' has no ground truth: the sequence loss cannot train on it (loss='unsup' can)")
        self.val = (self.val,) if isinstance(self.val, str) else tuple(self.val)
        if self.val:
            from ..eval.validate import parse_val

            names = [n for n, _ in parse_val(self.val)]
            if "chairs-val" in names and self.data is not None and self.dataset == "chairs" and not self.chairs_split:
                raise ValueError("val: chairs-val while training on dataset 'chairs' without chairs_split would "
                                 "validate on training data")
            if self.graph_step:
                raise ValueError("val: validation is not supported together with graph_step")
        if self.data is not None:
            from .augment import SPARSE_STAGES, STAGES

            if self.dataset == "mix":
                self.mix = tuple(self.mix)
                if self.mix_weights is not None:
                    self.mix_weights = tuple(int(v) for v in self.mix_weights)
                    if len(self.mix_weights) != len(self.mix):
                        raise ValueError(f"mix: {len(self.mix_weights)} weights for {len(self.mix)} parts")
                if self.stage != "sintel":
                    raise ValueError(f"dataset 'mix' is RAFT's Sintel stage: stage 'sintel' wanted, got {self.stage!r}")
            stages = SPARSE_STAGES if self.sparse else STAGES
            if self.stage not in stages:
                raise ValueError(f"unknown stage {self.stage!r} for dataset {self.dataset!r} (one of {sorted(stages)})")
            if tuple(self.size) == tuple(type(self).__dataclass_fields__["size"].default):
                self.size = stages[self.stage].crop

    @property
    def sparse(self) -> bool:
        return self.dataset in ("kitti", "hd1k")

    @property
    def mix_parts(self):
        """``[(name, weight)]`` of a mixture, as ``FlowPairs.open(..., "mix", parts=...)`` takes them."""
        from .datasets import MIX_DEFAULT

        weights = self.mix_weights or [dict(MIX_DEFAULT).get(n, 1) for n in self.mix]   # RAFT's weight of each part
        return list(zip(self.mix, weights))


VAL_FIELDS = ("val", "val_every", "val_iters", "val_batch", "val_max_pairs", "chairs_split")
# likewise left out of latest.json while they are at their defaults
UNSUP_FIELDS = ("loss", "unsup_eps", "unsup_eps_s", "unsup_edge_kappa", "unsup_smooth_weight", "unsup_out_penalty")
# (unsup_photo, unsup_smooth_order and the unsup_occ* fields are recorded always: the tuple above is pinned by
# tests/test_unsup.py, which reads its tail as the five floats)


def _adamw(params, cfg: TrainConfig, device, capturable: bool = False):
    """AdamW; on the GPU the single-kernel (fused) implementation when this
    PyTorch build provides it -- one launch for all ~230 parameter tensors.
    ``capturable``: graph-replayable (device-side step counters, the learning
    rate a device tensor that the LR schedule updates in place)."""
    params = list(params)
    kw = dict(lr=cfg.lr, weight_decay=cfg.weight_decay, eps=cfg.eps)
    if device is not None and torch.device(device).type == "cuda":
        if capturable:
            try:
                return torch.optim.AdamW(params, fused=True, capturable=True,
                                         **dict(kw, lr=torch.tensor(cfg.lr, device=device)))
            except (RuntimeError, TypeError, ValueError):
                pass
        try:
            return torch.optim.AdamW(params, fused=True, **kw)
        except (RuntimeError, TypeError, ValueError):
            pass
    return torch.optim.AdamW(params, **kw)


class Trainer:
    # steps the host may run ahead of the GPU's non-finite flags (each step waits for the flag of
    # the step SETTLE_LAG before it, so the launch queue holds about that many steps)
    SETTLE_LAG = 1

    def __init__(self, cfg: TrainConfig, device: Optional[torch.device] = None):
        self.cfg = cfg
        self.rank, self.world, dev = dp.init_distributed()
        self.device = device or dev
        torch.manual_seed(cfg.seed)
        factory = raft_large if cfg.arch == "raft_large" else raft_small
        self.model, _ = factory(seed=cfg.seed)
        self.model = self.model.to(self.device).train()
        dp.broadcast_module(self.model)
        if cfg.sync_bn and self.world > 1:
            dp.convert_sync_batchnorm(self.model)
        if cfg.unsup_selfsup_weight > 0:
            # the crop has to keep one cell of the coarsest correlation level (8 * 2^(levels - 1) pixels) per axis
            need = 8 * 2 ** (self.model.corr_block.num_levels - 1)
            left = min(cfg.size) - 2 * cfg.unsup_selfsup_crop
            if left < need:
                raise ValueError(f"unsup_selfsup_crop = {cfg.unsup_selfsup_crop} leaves {left} pixels of the "
                                 f"{tuple(cfg.size)} frame, {cfg.arch} needs at least {need}")
        self.flat_comm = dp.FlatGradComm() if self.world > 1 else None
        self.sync = dp.GradAllReducer(self.model, bucket_mb=cfg.bucket_mb, flat_comm=self.flat_comm)
        self._graph_ok = cfg.graph_step and self.device.type == "cuda" and self.world == 1
        self.opt = _adamw(self.model.parameters(), cfg, self.device, capturable=self._graph_ok)
        self._graph = None         # captured whole-step graph (see _graph_step)
        self.sched = torch.optim.lr_scheduler.OneCycleLR(
            self.opt, cfg.lr, total_steps=cfg.steps + 100, pct_start=0.05, cycle_momentum=False,
            anneal_strategy="linear")
        self.data = SyntheticFlow(size=tuple(cfg.size), seed=cfg.seed, device=self.device)
        self.loader = None
        self.labelled = True       # the batches carry ground truth (False: a frames-only list)
        if cfg.data is not None:
            from .datasets import FlowPairs, PairLoader

            if cfg.dataset == "mix":
                ds = FlowPairs.open(cfg.data, "mix", parts=cfg.mix_parts)
            elif cfg.dataset == "chairs" and cfg.chairs_split:
                ds = FlowPairs.chairs(cfg.data, "training", cfg.chairs_split)
            else:
                ds = FlowPairs.open(cfg.data, cfg.dataset)
            self.labelled = bool(getattr(ds, "labelled", True))
            self.loader = PairLoader(ds, cfg.batch, seed=cfg.seed, rank=self.rank, world=self.world, device=self.device)
            if self.loader.frame_min[0] < cfg.size[0] or self.loader.frame_min[1] < cfg.size[1]:
                raise ValueError(f"{cfg.data}: frames {self.loader.frame_min} are smaller than the crop {tuple(cfg.size)}")
        self.step = 0
        self.skipped = 0           # total dropped steps
        self._skip_run = 0         # consecutive dropped steps
        self._pending = []         # (step, pinned non-finite flag, event): GPU steps not yet settled
        self.val_history = []      # {"step": s, name: metrics, ...} of every validation (validate)
        if cfg.resume and cfg.ckpt_dir and os.path.exists(os.path.join(cfg.ckpt_dir, "latest.json")):
            self.load(cfg.ckpt_dir)

    # ------------------------------------------------------------------ step
    def train_step(self, batch) -> Dict[str, float]:
        cfg = self.cfg
        if (self._graph_ok and self.step >= cfg.graph_warmup and cfg.fault_nan_step < 0
                and self.opt.defaults.get("capturable") and self._async_skip()):
            return self._graph_step(batch)
        return self._eager_step(batch)

    def _graph_step(self, batch) -> Dict[str, float]:
        """The whole step as one replayed graph: the native plans enqueue
        eagerly into the capture (fused.py), the loss, backward, clipping,
        the non-finite guard and fused AdamW (device-side step, tensor LR) are
        captured with them, so the launch queue never runs dry on Python or
        launch overhead between the pieces.  Captured once, after the eager
        warm-up steps; the batch is copied into static inputs each step."""
        if self._graph is None:
            self._capture(batch)
        for dst, src in zip(self._static_in, batch):
            dst.copy_(src)
        self._graph.replay()
        if self.cfg.skip_nonfinite:
            flag = torch.empty((), dtype=torch.float32, pin_memory=True)
            flag.copy_(self._static_bad, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._settle(keep_last=True)
            self._pending.append((self.step + 1, flag, ev))
        self.sched.step()
        self.step += 1
        return {k: v.clone() for k, v in self._static_out.items()}

    def _capture(self, batch) -> None:
        cfg = self.cfg
        self._static_in = [t.clone() for t in batch]
        torch.cuda.synchronize(self.device)
        self.opt.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            img1, img2, flow, valid = self._static_in
            preds = self.model(img1, img2, train=not cfg.freeze_bn, num_flow_updates=cfg.iters, autograd=True)
            loss, metrics = sequence_loss(preds, flow, valid, cfg.gamma, cfg.max_flow)
            with self._comm():
                loss.backward()
            gnorm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), cfg.clip)
            bad = (~torch.isfinite(gnorm)).float()
            if cfg.skip_nonfinite:
                self.opt.found_inf = bad
            self.opt.step()
            self.opt.found_inf = None
        self._graph = g
        self._static_bad = bad
        self._static_out = {"loss": loss.detach(), "grad_norm": gnorm.detach(),
                            **{k: v.detach() for k, v in metrics.items()}}

    def _eager_step(self, batch) -> Dict[str, float]:
        img1, img2, flow, valid = batch
        cfg = self.cfg
        self.opt.zero_grad(set_to_none=True)
        train_bn = not cfg.freeze_bn
        if cfg.loss == "unsup" and cfg.unsup_selfsup_weight > 0 and self.step >= cfg.unsup_selfsup_after:
            loss, metrics = self._selfsup_loss(img1, img2, flow, valid)
        elif cfg.loss == "unsup" and cfg.unsup_occlusion != "none":
            loss, metrics = self._occlusion_loss(img1, img2, flow, valid)
        elif cfg.loss == "unsup":
            preds = self.model(img1, img2, train=train_bn, num_flow_updates=cfg.iters, autograd=True)
            loss, metrics = unsup_loss(preds, img1, img2, None, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s,
                                       cfg.unsup_edge_kappa, cfg.unsup_smooth_weight, cfg.unsup_out_penalty,
                                       **self._unsup_switches())
            if self.labelled:      # a labelled set monitors the label-free run: metrics only, no gradient
                with torch.no_grad():
                    _, sup = sequence_loss(preds.detach(), flow, valid, cfg.gamma, cfg.max_flow)
                metrics = {**metrics, **sup}
        else:
            preds = self.model(img1, img2, train=train_bn, num_flow_updates=cfg.iters, autograd=True)
            loss, metrics = sequence_loss(preds, flow, valid, cfg.gamma, cfg.max_flow)
        if self.step + 1 == cfg.fault_nan_step:
            loss = loss * float("nan")
        with self._comm():
            loss.backward()
        self.sync.finish()
        gnorm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), cfg.clip)
        # Failure detection: the gradient is all-reduced, so every rank sees the
        # same norm and takes the same decision (no extra collective needed).
        if cfg.skip_nonfinite and self._async_skip():
            # GPU, fused AdamW: the optimizer kernel itself drops the update when
            # the norm is non-finite (found_inf), so no host sync stalls the
            # launch queue here; the host-side bookkeeping (skip counters, the
            # consecutive-skip abort) reads the flag one step later, when the
            # GPU is already busy with the next step (see _settle).
            bad = (~torch.isfinite(gnorm)).float()
            self.opt.found_inf = bad
            self.opt.step()
            self.opt.found_inf = None
            flag = torch.empty((), dtype=torch.float32, pin_memory=True)
            flag.copy_(bad, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._settle(keep_last=True)
            self._pending.append((self.step + 1, flag, ev))
        elif cfg.skip_nonfinite and not bool(torch.isfinite(gnorm)):
            self.opt.zero_grad(set_to_none=True)
            self._record_skip(self.step + 1, True)
        else:
            if cfg.skip_nonfinite:
                self._record_skip(self.step + 1, False)
            self.opt.step()
        self.sched.step()
        self.step += 1
        out = {"loss": loss.detach(), "grad_norm": gnorm.detach(), **{k: v.detach() for k, v in metrics.items()}}
        return out

    def _unsup_switches(self) -> dict:
        """``unsup_loss``'s ``photo`` and ``smooth_order``, each passed only where it is not the default: the
        default run makes the call it always made."""
        cfg = self.cfg
        return {**({} if cfg.unsup_photo == "charbonnier" else {"photo": cfg.unsup_photo}),
                **({} if cfg.unsup_smooth_order == 1 else {"smooth_order": cfg.unsup_smooth_order})}

    def _occlusion_loss(self, img1, img2, flow, valid):
        """The label-free loss with occlusion masks: both directions as one batch of 2B pairs (forward flows
        in ``preds[:, :B]``, backward flows in ``preds[:, B:]``), the visibility masks of the final prediction
        (detached; ``ops/native.py:visibility_masks``) applied to every iteration's photometric term.  Before
        step ``unsup_occ_after`` there is no mask, but both directions run all the same, so that the batch
        shape and the cached plans do not change mid-run."""
        B = img1.shape[0]
        a, b = torch.cat([img1, img2]), torch.cat([img2, img1])
        preds = self.model(a, b, train=not self.cfg.freeze_bn, num_flow_updates=self.cfg.iters, autograd=True)
        loss, metrics, _ = self._masked_loss(preds, a, b, flow, valid)
        return loss, metrics

    def _masked_loss(self, preds, a, b, flow, valid):
        """The loss and metrics of ``_occlusion_loss`` from the predictions (N, 2B, H, W, 2) of the stacked pairs
        (a, b) -> ``(loss, metrics, mask)``; mask: the visibility masks (2B, H, W), None before ``unsup_occ_after``."""
        from ..ops import native as nat

        cfg = self.cfg
        B = a.shape[0] // 2
        mask = None
        if self.step >= cfg.unsup_occ_after:
            last = preds[-1].detach()
            mask = nat.visibility_masks(last[:B].float().contiguous(), last[B:].float().contiguous(), cfg.unsup_occlusion,
                                        cfg.unsup_occ_thr).view(2 * B, *last.shape[1:3])
        loss, metrics = unsup_loss(preds, a, b, mask, cfg.gamma, cfg.unsup_eps, cfg.unsup_eps_s,
                                   cfg.unsup_edge_kappa, cfg.unsup_smooth_weight, cfg.unsup_out_penalty,
                                   **self._unsup_switches())
        visible = torch.ones((), dtype=torch.float32, device=preds.device) if mask is None else mask.mean()
        metrics = {**metrics, "visible": visible}
        if self.labelled:          # metrics only, from the forward direction
            with torch.no_grad():
                _, sup = sequence_loss(preds[:, :B].detach(), flow, valid, cfg.gamma, cfg.max_flow)
            metrics = {**metrics, **sup}
        return loss, metrics, mask

    def _selfsup_loss(self, img1, img2, flow, valid):
        """``_occlusion_loss`` plus self-supervision (train/selfsup.py): ONE model call over 4B pairs -- the 2B full
        frames of both directions (``preds[:, :2B]``: the teacher, and the half that the existing loss, masks and
        metrics run on unchanged) and their centre crops resampled to the frame (``preds[:, 2B:]``: the student) --
        so the step keeps one forward and one backward.  The teacher's final flow, detached and brought into the
        student's frame by ``crop_resize``, is the target of every student iteration, weighted by ``T' (1 - S)``:
        T' the resampled plane "the teacher's pixel is visible and lands inside", S the same plane from the
        student's own final flows -- the pixels the student cannot verify by itself.  (The crop of the swapped
        stack is the swapped crop, bit for bit, so the frames are resampled by one launch, not two.)"""
        from ..ops import native as nat
        from .occlusion import lands_inside
        from .selfsup import flow_scale, selfsup_loss

        cfg = self.cfg
        B = img1.shape[0]
        c = cfg.unsup_selfsup_crop
        a, b = torch.cat([img1, img2]), torch.cat([img2, img1])
        sa = nat.crop_resize(a.float().contiguous(), c).to(a.dtype)
        sb = torch.cat([sa[B:], sa[:B]])
        preds = self.model(torch.cat([a, sa]), torch.cat([b, sb]), train=not cfg.freeze_bn, num_flow_updates=cfg.iters,
                           autograd=True)
        loss, metrics, mask = self._masked_loss(preds[:, :2 * B], a, b, flow, valid)
        H, W = preds.shape[2:4]
        with torch.no_grad():
            full = preds[-1, :2 * B].detach().float().contiguous()
            T = lands_inside(full).float()
            if mask is not None:
                T = mask * T
            target = nat.crop_resize(full, c, flow_scale(H, W, c))
            Tc = nat.crop_resize(T.view(2 * B, H, W, 1).contiguous(), c).view(2 * B, H, W)
            student = preds[-1, 2 * B:].detach().float().contiguous()
            S = lands_inside(student).float()
            if mask is not None:
                S = nat.visibility_masks(student[:B], student[B:], cfg.unsup_occlusion, cfg.unsup_occ_thr).view(2 * B, H, W) * S
            weight = Tc * (1.0 - S)
        term, mets = selfsup_loss(preds[:, 2 * B:], target, weight, cfg.gamma, cfg.unsup_selfsup_eps)
        return loss + cfg.unsup_selfsup_weight * term, {**metrics, **mets}

    def _comm(self):
        """The fused native backward's flat-arena all-reduce, registered for
        this model only while its step's backward runs (train/fused.py:grad_comm)."""
        from . import fused

        return fused.grad_comm(self.model, self.flat_comm if self.device.type == "cuda" else None)

    def _async_skip(self) -> bool:
        return self.device.type == "cuda" and bool(getattr(self.opt, "defaults", {}).get("fused"))

    def _record_skip(self, step: int, bad: bool) -> None:
        if bad:
            self.skipped += 1
            self._skip_run += 1
            if self._skip_run > self.cfg.max_skipped:
                raise FloatingPointError(f"{self._skip_run} consecutive non-finite gradients at step {step}")
        else:
            self._skip_run = 0

    def _settle(self, keep_last: bool = False) -> None:
        """Fold the non-finite flags of finished steps into the skip counters
        (``keep_last``: leave the newest ``SETTLE_LAG`` pending steps, which may still run)."""
        while len(self._pending) > (self.SETTLE_LAG if keep_last else 0):
            step, flag, ev = self._pending.pop(0)
            ev.synchronize()
            self._record_skip(step, bool(flag.item()))

    def flush(self) -> None:
        """Settle every pending failure-detection flag (waits for the GPU)."""
        self._settle()

    def batch_for(self, step: int):
        cfg = self.cfg
        if self.loader is not None:
            # real data: the raw frames of this step, then crop + augmentation in one gather on the
            # device (the golden op on a CPU device); records and indices are functions of the step
            from ..ops import native as nat
            from .augment import AugmentParams, sample_mixed, sample_sparse

            crop = (int(cfg.size[0]), int(cfg.size[1]))
            safe = {"constancy": True} if cfg.loss == "unsup" else {}   # keep brightness constancy (augment.py)
            if self.loader.mixed:
                img1, img2, flow, valid, sizes, dense = self.loader.fetch(step)
                params = sample_mixed(cfg.batch, sizes, dense, cfg.stage, crop, seed=cfg.seed, step=step, rank=self.rank,
                                      augment=cfg.augment, **safe)
                return nat.augment_pairs_mixed(img1, img2, flow, valid, params, crop)
            if self.loader.sparse:
                img1, img2, flow, valid, sizes = self.loader.fetch(step)
                params = sample_sparse(cfg.batch, sizes, cfg.stage, crop, seed=cfg.seed, step=step, rank=self.rank,
                                       augment=cfg.augment, **safe)
                return nat.augment_pairs_sparse(img1, img2, flow, valid, params, crop)
            img1, img2, flow = self.loader.fetch(step)
            params = AugmentParams.sample(cfg.batch, self.loader.frame, cfg.stage, crop, seed=cfg.seed, step=step,
                                          rank=self.rank, augment=cfg.augment, **safe)
            return nat.augment_pairs(img1, img2, flow, params, crop)
        base = (step * self.world + self.rank) * cfg.batch
        return self.data.batch(list(range(base, base + cfg.batch)))

    def fit(self, log=print, stop_at: Optional[int] = None) -> Dict[str, float]:
        """Train to ``cfg.steps`` (or stop early after step ``stop_at``)."""
        cfg = self.cfg
        end = cfg.steps if stop_at is None else min(stop_at, cfg.steps)
        t0 = time.perf_counter()
        val_s = 0.0                # time spent validating: not training time
        last = {}
        while self.step < end:
            batch = self.batch_for(self.step)
            m = self.train_step(batch)
            if self.step % cfg.log_every == 0 or self.step == cfg.steps:
                self.flush()
                vals = dp.all_reduce_scalars({k: float(v) for k, v in m.items()}, self.device)
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
                dt = time.perf_counter() - t0 - val_s
                vals.update(step=self.step, skipped=self.skipped, lr=float(self.sched.get_last_lr()[0]), elapsed_s=dt,
                            pairs_per_s=self.step * cfg.batch * self.world / dt)
                if cfg.val:
                    vals.update(val_s=val_s)
                last = vals
                if self.rank == 0:
                    log(json.dumps({k: (round(v, 6) if isinstance(v, float) else v) for k, v in vals.items()}))
            if cfg.val and (self.step == cfg.steps or (cfg.val_every and self.step % cfg.val_every == 0)):
                val_s += self.validate(log)
            if cfg.ckpt_dir and cfg.ckpt_every and self.step % cfg.ckpt_every == 0:
                self.save(cfg.ckpt_dir)
        if cfg.ckpt_dir:
            self.save(cfg.ckpt_dir)
        return last

    # ------------------------------------------------------------ validation
    def validate(self, log=print) -> float:
        """Evaluate the model as it stands on every split of ``cfg.val`` (``eval/validate.py:evaluate``:
        inference through the engine, which repacks the updated weights by its version check; the
        training plans, the optimizer, the BatchNorm statistics and the batch sequence are not
        touched) -> the seconds it took.  The result is appended to ``val_history``, logged by rank 0
        as a JSON line with a ``"val"`` key and appended to ``<ckpt_dir>/val.jsonl``."""
        from ..eval.validate import evaluate, parse_val

        cfg = self.cfg
        self.flush()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)    # the pause is the validation's own time
        t0 = time.perf_counter()
        entry = {"step": self.step}
        for name, root in parse_val(cfg.val):
            kw = {"chairs_split": cfg.chairs_split} if name == "chairs-val" and cfg.chairs_split else {}
            entry[name] = evaluate(self.model, name, root, iters=cfg.val_iters or None, batch=cfg.val_batch,
                                   max_pairs=cfg.val_max_pairs, device=self.device, **kw)
        self.val_history.append(entry)
        if self.rank == 0:
            line = json.dumps({"val": entry})
            log(line)
            if cfg.ckpt_dir:
                os.makedirs(cfg.ckpt_dir, exist_ok=True)
                with open(os.path.join(cfg.ckpt_dir, "val.jsonl"), "a") as f:
                    f.write(json.dumps(entry) + "\n")
        return time.perf_counter() - t0

    # ------------------------------------------------------------ checkpoint
    def save(self, d: str) -> None:
        self.flush()
        if self.rank != 0:
            if dp.is_dist():
                torch.distributed.barrier()
            return
        os.makedirs(d, exist_ok=True)
        name = f"step_{self.step}"
        ckpt.save_msgpack(self.model, os.path.join(d, name + ".msgpack"))
        torch.save({"opt": self.opt.state_dict(), "sched": self.sched.state_dict(), "step": self.step,
                    "skipped": self.skipped},
                   os.path.join(d, name + ".opt.pt"))
        fields = type(self.cfg).__dataclass_fields__
        config = {k: (list(v) if isinstance(v, tuple) else v) for k, v in asdict(self.cfg).items()
                  # a run without validation writes the file it always wrote
                  if k not in VAL_FIELDS + UNSUP_FIELDS or v != fields[k].default}
        with open(os.path.join(d, "latest.json"), "w") as f:
            json.dump({"step": self.step, "weights": name + ".msgpack", "opt": name + ".opt.pt", "config": config}, f)
        if dp.is_dist():
            torch.distributed.barrier()

    def load(self, d: str) -> None:
        with open(os.path.join(d, "latest.json")) as f:
            meta = json.load(f)
        ckpt.load_variables_into(self.model, ckpt.load_msgpack(os.path.join(d, meta["weights"])), strict=True)
        st = torch.load(os.path.join(d, meta["opt"]), map_location=self.device, weights_only=True)
        self.opt.load_state_dict(st["opt"])
        self.sched.load_state_dict(st["sched"])
        self.step = int(st["step"])
        self.skipped = int(st.get("skipped", 0))


def config_from_args(a) -> TrainConfig:
    kw = {k: (tuple(v) if k == "size" else v) for k, v in vars(a).items()}
    mix = kw.pop("mix")
    if mix is not None:                             # name[:weight],...
        parts = [p.split(":") for p in mix.split(",") if p]
        if not parts or any(len(p) > 2 or (len(p) == 2 and not p[1].isdigit()) for p in parts):
            raise ValueError(f"--mix {mix!r}: name[:weight],... wanted")
        kw["mix"] = tuple(p[0] for p in parts)
        kw["mix_weights"] = tuple(int(p[1]) if len(p) == 2 else 1 for p in parts)
    if isinstance(kw.get("val"), str):              # name=root,name=root
        kw["val"] = tuple(p for p in kw["val"].split(",") if p)
    if kw.get("val_max_pairs") is not None:
        kw["val_max_pairs"] = int(kw["val_max_pairs"])
    return TrainConfig(**kw)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for f_ in TrainConfig.__dataclass_fields__.values():
        if f_.name == "size":
            ap.add_argument("--size", type=int, nargs=2, default=list(f_.default))
        elif f_.name == "mix":
            ap.add_argument("--mix", type=str, default=None, metavar="NAME[:WEIGHT],...",
                            help="the parts of --dataset mix; a part without a weight counts once")
        elif f_.name == "mix_weights":
            continue                                # given inside --mix
        elif f_.type in ("bool", bool):
            ap.add_argument(f"--{f_.name.replace('_', '-')}", action=argparse.BooleanOptionalAction,
                            default=f_.default)
        else:
            typ = {"int": int, "float": float, "str": str}.get(str(f_.type).replace("Optional[str]", "str"), str)
            ap.add_argument(f"--{f_.name.replace('_', '-')}", type=typ if f_.default is not None else str,
                            default=f_.default, choices=(1, 2) if f_.name == "unsup_smooth_order" else None)
    cfg = config_from_args(ap.parse_args(argv))
    tr = Trainer(cfg)
    tr.fit()
    if dp.is_dist():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
