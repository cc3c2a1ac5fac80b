"""RAFT top-level model, ``raft_large`` / ``raft_small`` factories and the
Flax-style ``apply`` API.

Reference: ``jax_raft/model.py:484-767`` (UpdateCell, RAFT, _raft, raft_large,
raft_small).  API parity:

* ``raft_large(pretrained=False, **kwargs)`` / ``raft_small(...)`` return
  ``(model, variables)``; sub-modules can be injected with the same kwargs
  (``feature_encoder``, ``context_encoder``, ``corr_block``, ``update_block``,
  ``mask_predictor``).
* ``model.apply(variables, image1, image2, train=False, num_flow_updates=12)``
  returns all ``num_flow_updates`` upsampled flows, shape (N, B, H, W, 2),
  NHWC float inputs in [-1, 1].
* ``model(image1, image2, ...)`` is the idiomatic ``nn.Module`` call.

Execution: one implementation per device.  CPU tensors run the golden
PyTorch forward (:mod:`.layers`, :mod:`.reference`); GPU tensors in inference
run the native HIP engine (:mod:`jax_raft_amd.runtime.engine`), and GPU
training runs the autograd path built from the native ops
(:mod:`jax_raft_amd.ops.autograd`).
"""
from __future__ import annotations

from typing import Any, Dict, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import reference as R
from .layers import (
    NORM_BATCH,
    NORM_INSTANCE,
    CorrBlock,
    FeatureEncoder,
    FlowHead,
    MaskPredictor,
    MotionEncoder,
    RecurrentBlock,
    UpdateBlock,
)
from ..utils import checkpoint as ckpt

_BASE_URL = "https://github.com/alebeck/jax-raft/releases/download/checkpoints/"
_MODELS_URLS = {
    "raft_large": _BASE_URL + "raft_large_C_T_SKHT_V2-ff5fadd5.msgpack",
    "raft_small": _BASE_URL + "raft_small_C_T_V2-01064c6d.msgpack",
}


def _as_tensor(x) -> torch.Tensor:
    if isinstance(x, torch.Tensor):
        return x
    a = np.asarray(x)
    if a.dtype == np.uint8:   # raw frames (normalised + padded by the engine / forward)
        return torch.from_numpy(np.ascontiguousarray(a))
    return torch.as_tensor(np.asarray(x, dtype=np.float32))


class RAFT(nn.Module):
    """RAFT (Recurrent All-Pairs Field Transforms), reference ``model.py:513-605``."""

    def __init__(self, feature_encoder: FeatureEncoder, context_encoder: FeatureEncoder, corr_block: CorrBlock,
                 update_block: UpdateBlock, mask_predictor: Optional[MaskPredictor] = None):
        super().__init__()
        self.feature_encoder = feature_encoder
        self.context_encoder = context_encoder
        self.corr_block = corr_block
        self.update_block = update_block
        self.mask_predictor = mask_predictor
        self._engines: Dict[Any, Any] = {}
        self._lowering_error: Optional[str] = None
        self.arch: Optional[str] = None

    # ------------------------------------------------------------ API surface
    def variables(self) -> Dict[str, Dict[str, Any]]:
        return ckpt.variables_from_module(self)

    def forward(self, image1, image2, train: bool = False, num_flow_updates: int = 12, return_all_iters: bool = True,
                flow_init=None, return_flow_low: bool = False, bidirectional: bool = False, fb_alpha: float = 0.01,
                fb_beta: float = 0.5, warp: bool = False, interpolate=None, interp_min_cover: float = 1.0 / 64,
                **engine_kw):
        """Upsampled flows of every refinement iteration, (num_flow_updates, B, H, W, 2)
        (reference semantics, ``model.py:605``).  ``return_all_iters=False`` (inference
        serving mode) upsamples and returns only the final flow, shape (1, B, H, W, 2).

        Warm start (video; not in the reference, original RAFT's ``flow_init``):
        ``flow_init`` (B, H/8, W/8, 2) fp32 NHWC, channel 0 = x, in 1/8-resolution pixels,
        starts the refinement at ``coords1 = coords0 + flow_init`` instead of at zero flow;
        ``flow_init="previous"`` (native engine only) projects the flow of the engine's previous
        call forward in time on the GPU (:func:`reference.forward_project`).
        ``return_flow_low=True`` returns ``(flows, flow_low)``, ``flow_low`` (B, H/8, W/8, 2) the
        final ``coords1 - coords0``.  For uint8 frames of any size both are at the *padded*
        size divided by 8 (``runtime/engine.py:sintel_pad``), not at the frame size.  Inference
        only: with ``train=True`` / ``autograd=True`` they raise ``NotImplementedError``.

        Bidirectional flow (video): ``bidirectional=True`` returns
        :class:`~jax_raft_amd.models.reference.BidirectionalFlow` ``(flows_fw, flows_bw, occ_fw,
        occ_bw)`` -- the flows 1 -> 2 and 2 -> 1 and the (B, H, W) bool occlusion masks of their
        forward-backward consistency check (:func:`reference.fb_consistency`, UnFlow's criterion
        with ``fb_alpha``, ``fb_beta``) -- from one call: one plan of the native engine, or two
        golden passes plus the golden check elsewhere.  For uint8 frames everything is cropped to
        the frame.  Inference only, and not together with ``flow_init`` / ``return_flow_low``.

        ``bidirectional=True, warp=True`` (uint8 frames only; anything else is a ``ValueError``)
        returns :class:`~jax_raft_amd.models.reference.BidirectionalWarp`: the same four fields,
        the motion-compensated frames ``warped_fw`` / ``warped_bw`` (B, H0, W0, 3) uint8 and
        ``photo`` (2, B, 2) int64, the masked photometric sums (:func:`reference.warp_frames`) --
        the last kernel of the same plan, or the golden warp elsewhere.

        ``bidirectional=True, interpolate=t`` (uint8 frames; ``t`` a float or a sequence of 1 to 8
        floats strictly between 0 and 1; not together with ``warp=True``; anything else is a
        ``ValueError``) returns :class:`~jax_raft_amd.models.reference.BidirectionalInterp`: the
        same four fields, ``frames`` (K, B, H0, W0, 3) uint8 -- the frames at the times ``t``
        between frame 1 and frame 2 by forward splatting along both flows -- and ``holes``
        (K, B, H0, W0) bool (:func:`reference.interpolate_frames` with ``min_cover =
        interp_min_cover``) -- the last kernels of the same plan, or the golden op elsewhere."""
        image1, image2 = _as_tensor(image1), _as_tensor(image2)
        if interpolate is not None and not bidirectional:
            raise ValueError("interpolate=t requires bidirectional=True (the splat uses both flows and their "
                             "occlusion masks)")
        if interpolate is not None and warp:
            raise ValueError("bidirectional: interpolate and warp=True exclude each other (one consumer per call)")
        corr = check_corr(engine_kw.get("corr", "volume"))
        if corr == "on_demand":
            # what the on-demand engine does not lower, refused here (an engine's refusal would read
            # as "this model cannot be lowered" and fall back to the golden path)
            if train or engine_kw.get("autograd") or engine_kw.get("fused"):
                raise NotImplementedError("corr='on_demand': inference only (the lookup from the feature maps has "
                                          "no backward; not with train / autograd)")
            if bidirectional:
                raise NotImplementedError("corr='on_demand': not with bidirectional=True (the bidirectional plan "
                                          "is lowered for the all-pairs volume only)")
            if engine_kw.get("precision", "bf16") != "bf16":
                raise NotImplementedError("corr='on_demand': not with precision='fp32' / 'mixed' (the on-demand "
                                          "lookup is lowered for the bf16 engine only)")
            if engine_kw.get("cp_group") is not None:
                raise NotImplementedError("corr='on_demand': not with context parallelism (cp_group splits the "
                                          "volume the on-demand path never builds)")
        if warp and not bidirectional:
            raise ValueError("warp=True requires bidirectional=True (the warp uses both flows' occlusion masks)")
        if bidirectional:
            if train or engine_kw.get("autograd"):
                raise NotImplementedError("bidirectional: inference only (not with train / autograd)")
            if flow_init is not None or return_flow_low:
                raise NotImplementedError("bidirectional: not with flow_init / return_flow_low (the warm seed and "
                                          "the low-resolution output are lowered for one direction)")
            if warp and not (image1.dtype == torch.uint8 and image2.dtype == torch.uint8):
                raise ValueError(f"bidirectional, warp=True requires uint8 frames (the warp samples the frames as "
                                 f"given), got {image1.dtype}")
            times = None
            if interpolate is not None:
                if not (image1.dtype == torch.uint8 and image2.dtype == torch.uint8):
                    raise ValueError(f"bidirectional, interpolate=t requires uint8 frames (the splat reads the frames "
                                     f"as given), got {image1.dtype}")
                _, many = R.interp_times(interpolate, interp_min_cover, R.INTERP_MAX_TIMES)   # ValueError before any work
                times = (list(interpolate) if many else [interpolate], interp_min_cover)
            return self._forward_bidirectional(image1, image2, num_flow_updates, return_all_iters, fb_alpha, fb_beta,
                                               engine_kw, warp, times)
        B, H, W, _ = image1.shape
        assert (H, W) == tuple(image2.shape[-3:-1]), "input images should have the same shape"
        warm = dict(flow_init=flow_init, return_flow_low=return_flow_low)
        if (train or engine_kw.get("autograd")) and (flow_init is not None or return_flow_low):
            raise NotImplementedError("flow_init / return_flow_low: warm start is inference only (not with train / autograd)")
        if image1.dtype == torch.uint8:
            return self._forward_u8(image1, image2, train, num_flow_updates, return_all_iters, engine_kw, warm)
        assert (H % 8 == 0) and (W % 8 == 0), "input image H and W should be divisible by 8"
        if flow_init is not None and not isinstance(flow_init, str):
            flow_init = warm["flow_init"] = check_flow_init(flow_init, B, H, W)
        dev = self._param_device()
        if dev.type == "cuda" and not image1.is_cuda:   # host arrays / tensors for a model on the GPU
            image1, image2 = image1.to(dev), image2.to(dev)
        autograd = engine_kw.pop("autograd", False)
        fused = engine_kw.pop("fused", None)
        if image1.is_cuda:
            if train or autograd:
                from ..ops.autograd import raft_forward_autograd

                out = raft_forward_autograd(self, image1, image2, train, num_flow_updates, fused=fused)
                return out if return_all_iters else out[-1:]
            eng = None if self._lowering_error is not None else self._try_engine(image1.device, engine_kw)
            if eng is not None:
                return eng.forward(image1, image2, num_flow_updates, return_all_iters=return_all_iters, **warm)
            # a model the engine cannot lower (injected sub-modules, custom blocks / norms, channel
            # counts outside the fused kernels' tiling): op by op on the same native kernels
            # (convs, correlation pyramid, lookup: ops/functional.py), no graph
            with torch.no_grad():
                return self.forward_reference(image1, image2, False, num_flow_updates, return_all_iters, **warm,
                                              corr=corr)
        return self.forward_reference(image1, image2, train, num_flow_updates, return_all_iters, **warm, corr=corr)

    def _forward_bidirectional(self, image1, image2, num_flow_updates, return_all_iters, alpha, beta, engine_kw,
                               warp=False, times=None):
        """``forward(bidirectional=True)``: the native engine's bidirectional plan for a model on
        the GPU it can lower (float or uint8 frames); everywhere else two passes of
        :meth:`forward` and the golden check of their final flows (+ the golden warp of both
        frames with ``warp``, or the golden interpolation at ``times = (list of t, min_cover)``)."""
        dev = self._param_device()
        if dev.type == "cuda" and self._lowering_error is None:
            eng = self._try_engine(dev, {k: v for k, v in engine_kw.items() if k not in ("autograd", "fused")})
            if eng is not None:
                if image1.dtype != torch.uint8:
                    assert image1.shape[1] % 8 == 0 and image1.shape[2] % 8 == 0, \
                        "input image H and W should be divisible by 8"
                if not image1.is_cuda and image1.dtype != torch.uint8:
                    image1, image2 = image1.to(dev), image2.to(dev)
                return eng.forward(image1, image2, num_flow_updates, return_all_iters=return_all_iters,
                                   bidirectional=True, fb_alpha=alpha, fb_beta=beta, warp=warp,
                                   **({} if times is None else dict(interpolate=times[0], interp_min_cover=times[1])))
        with torch.no_grad():
            fw = self.forward(image1, image2, False, num_flow_updates, return_all_iters, **engine_kw)
            bw = self.forward(image2, image1, False, num_flow_updates, return_all_iters, **engine_kw)
            occ_fw, occ_bw = R.fb_consistency(fw[-1].contiguous(), bw[-1].contiguous(), alpha, beta)
            if warp:   # the flows are already cropped to the frame: the whole map is the window
                f1, f2 = image1.to(fw.device), image2.to(fw.device)
                warped_fw, photo_fw = R.warp_frames(f2, fw[-1].contiguous(), occ_fw, f1)
                warped_bw, photo_bw = R.warp_frames(f1, bw[-1].contiguous(), occ_bw, f2)
                return R.BidirectionalWarp(fw, bw, occ_fw, occ_bw, warped_fw, warped_bw, torch.stack([photo_fw, photo_bw]))
            if times is not None:   # likewise
                f1, f2 = image1.to(fw.device), image2.to(fw.device)
                res = [R.interpolate_frames(f1, f2, fw[-1].contiguous(), bw[-1].contiguous(), t, occ_fw, occ_bw,
                                            min_cover=times[1]) for t in times[0]]
                return R.BidirectionalInterp(fw, bw, occ_fw, occ_bw, torch.stack([r[0] for r in res]),
                                             torch.stack([r[1] for r in res]))
        return R.BidirectionalFlow(fw, bw, occ_fw, occ_bw)

    def _forward_u8(self, image1, image2, train, num_flow_updates, return_all_iters, engine_kw, warm):
        """Raw uint8 NHWC frames of any size: the reference's input protocol
        (``scripts/validate_sintel.py:177-191``: x / 255 * 2 - 1, InputPadder('sintel') replicate
        padding to /8, unpad of the flows) -- on the GPU inside the engine's prep kernel, elsewhere
        (CPU golden path, training, models the engine cannot lower) with framework ops."""
        dev = self._param_device()
        if dev.type == "cuda" and not (train or engine_kw.get("autograd")) and self._lowering_error is None:
            # host frames go straight into the plan's uint8 input buffers (one H2D copy of 1/4 the
            # bytes of normalised fp32 frames)
            eng = self._try_engine(dev, {k: v for k, v in engine_kw.items() if k not in ("autograd", "fused")})
            if eng is not None:
                return eng.forward(image1, image2, num_flow_updates, return_all_iters=return_all_iters, **warm)
        if dev.type == "cuda" and not image1.is_cuda:
            image1, image2 = image1.to(dev), image2.to(dev)
        from ..runtime.engine import sintel_pad, u8_table

        H0, W0 = image1.shape[1:3]
        pt, pb, pl, pr = sintel_pad(H0, W0)
        lut = u8_table(image1.device)

        def prep(x):
            x = lut[x.long()].permute(0, 3, 1, 2)
            return torch.nn.functional.pad(x, [pl, pr, pt, pb], mode="replicate").permute(0, 2, 3, 1).contiguous()

        out = self.forward(prep(image1), prep(image2), train, num_flow_updates, return_all_iters, **warm, **engine_kw)
        if warm["return_flow_low"]:   # the flows cropped to the frame; flow_low stays at the padded size / 8
            return out[0][:, :, pt:pt + H0, pl:pl + W0], out[1]
        return out[:, :, pt:pt + H0, pl:pl + W0]

    def _param_device(self) -> torch.device:
        p = next(self.parameters(), None)
        return p.device if p is not None else torch.device("cpu")

    def _try_engine(self, device, engine_kw):
        """The native engine, or None (remembering why) when it cannot lower this model."""
        try:
            return self.engine(device, **engine_kw)
        except NotImplementedError as e:
            self._lowering_error = str(e)
            return None

    @property
    def execution_path(self) -> str:
        """"engine" (native plan / hipGraph) or "op-by-op: <why the engine cannot lower it>"."""
        return "engine" if self._lowering_error is None else f"op-by-op: {self._lowering_error}"

    def apply(self, variables: Mapping[str, Any], image1, image2, train: bool = False, num_flow_updates: int = 12,
              mutable=False, **kw):
        """Flax-style ``model.apply(variables, image1, image2, train, num_flow_updates)``
        (``flow_init=`` / ``return_flow_low=`` / ``bidirectional=`` / ``fb_alpha=`` / ``fb_beta=`` pass
        through to :meth:`forward`).

        With ``mutable=['batch_stats']`` (and ``train=True``) returns
        ``(flows, {'batch_stats': updated})`` like Flax."""
        own = self.variables()
        if _same_leaves(own, variables):
            out = self(image1, image2, train=train, num_flow_updates=num_flow_updates, **kw)
            if mutable:
                return out, {"batch_stats": ckpt.variables_from_module(self)["batch_stats"]}
            return out
        # Foreign variables (numpy / torch leaves): validated like Flax's apply
        # (every param present, no unexpected leaf, shapes equal; an absent
        # 'batch_stats' collection keeps the module's own statistics) and bound
        # functionally for this call only -- the module's tensors are untouched.
        # Leaves are copied, so a train-mode BatchNorm update never writes into
        # the caller's arrays; it is returned through ``mutable`` like Flax.
        bound = ckpt.variables_as_tensors(self, variables)
        out = torch.func.functional_call(
            self, bound, (image1, image2), dict(train=train, num_flow_updates=num_flow_updates, **kw))
        if mutable:
            stats = {k: v for k, v in bound.items() if k.endswith(".mean") or k.endswith(".var")}
            if not stats:
                stats = {k: v for k, v in ckpt.flatten_tree(own["batch_stats"]).items()}
            return out, {"batch_stats": ckpt.unflatten_tree(stats)}
        return out

    # ------------------------------------------------------- golden execution
    def forward_reference(self, image1, image2, train: bool, num_flow_updates: int, return_all_iters: bool = True,
                          flow_init: Optional[torch.Tensor] = None, return_flow_low: bool = False,
                          corr: str = "volume"):
        """Reference-semantics forward (``model.py:557-605`` with the scan body
        ``UpdateCell.__call__``, ``model.py:495-510``).  ``flow_init`` (B, H/8, W/8, 2):
        ``coords1 = coords0 + flow_init`` (warm start), everything else unchanged;
        ``return_flow_low``: ``(flows, final coords1 - coords0)``.  ``corr="on_demand"``: every
        lookup is :func:`reference.index_on_demand` on the two feature maps and no correlation
        pyramid is built (inference only); ``"volume"`` (default) is the reference's path."""
        on_demand = check_corr(corr) == "on_demand"
        if on_demand and train:
            raise NotImplementedError("corr='on_demand': inference only (not with train=True)")
        B, H, W, _ = image1.shape
        if isinstance(flow_init, str):
            raise ValueError(f"flow_init={flow_init!r} is a mode of the native engine; this path takes a tensor")
        if flow_init is not None:
            if train:
                raise NotImplementedError("flow_init: warm start is inference only (not with train=True)")
            flow_init = check_flow_init(flow_init, B, H, W).to(image1.device)
        fmaps = self.feature_encoder(torch.cat([image1, image2], dim=0), train)
        fmap1, fmap2 = torch.chunk(fmaps, 2, dim=0)
        assert tuple(fmap1.shape[1:3]) == (H // 8, W // 8), "The feature encoder should downsample H and W by 8"
        pyramid = None if on_demand else self.corr_block.build_pyramid(fmap1, fmap2)
        ctx = self.context_encoder(image1, train)
        assert tuple(ctx.shape[1:3]) == (H // 8, W // 8), "The context encoder should downsample H and W by 8"
        hs = self.update_block.hidden_state_size
        assert ctx.shape[-1] - hs > 0, (
            f"The context encoder outputs {ctx.shape[-1]} channels, but it should have at "
            f"strictly more than hidden_state={hs} channels")
        hidden, context = ctx[..., :hs], ctx[..., hs:]
        hidden = torch.tanh(hidden)
        context = torch.relu(context)
        coords0 = R.make_coords_grid(B, H // 8, W // 8, device=image1.device)
        coords1 = coords0.clone() if flow_init is None else coords0 + flow_init
        preds = []
        for it in range(num_flow_updates):
            coords1 = coords1.detach()  # stop_gradient, model.py:498
            if on_demand:
                corr = R.index_on_demand(fmap1, fmap2, coords1, self.corr_block.radius, self.corr_block.num_levels)
            else:
                corr = self.corr_block.index_pyramid(pyramid, coords1)
            flow = coords1 - coords0
            hidden, delta = self.update_block(hidden, context, corr, flow, train)
            coords1 = coords1 + delta
            if not return_all_iters and it + 1 < num_flow_updates:
                continue
            up_mask = None if self.mask_predictor is None else self.mask_predictor(hidden, train)
            preds.append(R.upsample_flow(coords1 - coords0, up_mask))
        if return_flow_low:
            return torch.stack(preds, dim=0), coords1 - coords0
        return torch.stack(preds, dim=0)

    # -------------------------------------------------------- native engine
    def engine(self, device, **kw):
        """The cached native inference engine for ``device`` (built lazily)."""
        from ..runtime.engine import RaftEngine

        key = (str(device), tuple(sorted(kw.items())))
        eng = self._engines.get(key)
        if eng is None:
            eng = RaftEngine(self, device, **kw)
            eng._hold_model_weakly()   # no model <-> engine cycle: the plans die with the model
            self._engines[key] = eng
        return eng

    def _apply(self, fn, *args, **kwargs):  # drop engines when moved / cast
        self._engines = {}
        self._lowering_error = None
        return super()._apply(fn, *args, **kwargs)

    def __setattr__(self, name, value):
        # a replaced sub-module may make the model lowerable again (or not): re-decide
        if name in ("feature_encoder", "context_encoder", "corr_block", "update_block", "mask_predictor"):
            self.__dict__["_lowering_error"] = None
            if "_engines" in self.__dict__:
                self.__dict__["_engines"] = {}
        super().__setattr__(name, value)


def check_corr(corr) -> str:
    """``corr``: "volume" (the all-pairs correlation pyramid) or "on_demand" (lookups computed from
    the feature maps), else ``ValueError``."""
    if corr not in ("volume", "on_demand"):
        raise ValueError(f"corr must be 'volume' or 'on_demand', got {corr!r}")
    return corr


def check_flow_init(flow_init, B: int, H: int, W: int) -> torch.Tensor:
    """``flow_init`` as an fp32 tensor of the shape a (B, H, W) forward expects, else ``ValueError``."""
    t = flow_init if isinstance(flow_init, torch.Tensor) else torch.as_tensor(np.asarray(flow_init, dtype=np.float32))
    want = (B, H // 8, W // 8, 2)
    if tuple(t.shape) != want:
        raise ValueError(f"flow_init must have shape {want} (B, H/8, W/8, 2; for uint8 frames H, W are the "
                         f"padded size), got {tuple(t.shape)}")
    return t.float()


def _same_leaves(a: Mapping[str, Any], b: Mapping[str, Any]) -> bool:
    fa = {}
    for coll in ("params", "batch_stats"):
        fa.update({f"{coll}.{k}": v for k, v in ckpt.flatten_tree(a.get(coll, {}) or {}).items()})
    fb = {}
    for coll in ("params", "batch_stats"):
        if isinstance(b, Mapping) and coll in b and b[coll]:
            fb.update({f"{coll}.{k}": v for k, v in ckpt.flatten_tree(b[coll]).items()})
    if set(fb) - set(fa):
        return False
    return all(isinstance(v, torch.Tensor) and v is fa[k] for k, v in fb.items())


def _raft(*, feature_encoder_layers, feature_encoder_block, feature_encoder_norm_layer, context_encoder_layers,
          context_encoder_block, context_encoder_norm_layer, corr_block_num_levels, corr_block_radius,
          motion_encoder_corr_layers, motion_encoder_flow_layers, motion_encoder_out_channels,
          recurrent_block_hidden_state_size, recurrent_block_kernel_size, recurrent_block_padding,
          flow_head_hidden_size, use_mask_predictor, pretrained_arch=None, weights: Optional[str] = None,
          seed: int = 0, **kwargs) -> Tuple[RAFT, Dict[str, Any]]:
    """Reference ``_raft``, ``model.py:608-691``."""
    gen = torch.Generator().manual_seed(seed)
    feature_encoder = kwargs.pop("feature_encoder", None) or FeatureEncoder(
        block=feature_encoder_block, layers=feature_encoder_layers, norm=feature_encoder_norm_layer, gen=gen)
    context_encoder = kwargs.pop("context_encoder", None) or FeatureEncoder(
        block=context_encoder_block, layers=context_encoder_layers, norm=context_encoder_norm_layer, gen=gen)
    corr_block = kwargs.pop("corr_block", None) or CorrBlock(num_levels=corr_block_num_levels, radius=corr_block_radius)
    update_block = kwargs.pop("update_block", None)
    if update_block is None:
        hidden = recurrent_block_hidden_state_size
        context_ch = context_encoder.out_channels - hidden
        motion_encoder = MotionEncoder(corr_block.out_channels, corr_layers=motion_encoder_corr_layers,
                                       flow_layers=motion_encoder_flow_layers,
                                       out_channels=motion_encoder_out_channels, gen=gen)
        recurrent_block = RecurrentBlock(context_ch + motion_encoder_out_channels, hidden,
                                         kernel_size=recurrent_block_kernel_size, padding=recurrent_block_padding,
                                         gen=gen)
        flow_head = FlowHead(hidden, flow_head_hidden_size, gen=gen)
        update_block = UpdateBlock(motion_encoder, recurrent_block, flow_head)
    mask_predictor = kwargs.pop("mask_predictor", None)
    if mask_predictor is None and use_mask_predictor:
        mask_predictor = MaskPredictor(update_block.hidden_state_size, hidden_size=256, multiplier=0.25, gen=gen)
    if kwargs:
        raise TypeError(f"unexpected keyword arguments: {sorted(kwargs)}")
    model = RAFT(feature_encoder, context_encoder, corr_block, update_block, mask_predictor)
    model.eval()
    if pretrained_arch is not None or weights is not None:
        arch = pretrained_arch or "raft_large"
        data = ckpt.resolve_pretrained(arch, _MODELS_URLS[arch], weights)
        ckpt.load_variables_into(model, ckpt.msgpack_restore(data), strict=True)
    return model, model.variables()


def raft_large(*, pretrained: bool = False, **kwargs):
    """RAFT large (``model.py:694-729``)."""
    model, variables = _raft(
        feature_encoder_layers=(64, 64, 96, 128, 256),
        feature_encoder_block="residual",
        feature_encoder_norm_layer=NORM_INSTANCE,
        context_encoder_layers=(64, 64, 96, 128, 256),
        context_encoder_block="residual",
        context_encoder_norm_layer=NORM_BATCH,
        corr_block_num_levels=4,
        corr_block_radius=4,
        motion_encoder_corr_layers=(256, 192),
        motion_encoder_flow_layers=(128, 64),
        motion_encoder_out_channels=128,
        recurrent_block_hidden_state_size=128,
        recurrent_block_kernel_size=((1, 5), (5, 1)),
        recurrent_block_padding=((0, 2), (2, 0)),
        flow_head_hidden_size=256,
        use_mask_predictor=True,
        pretrained_arch="raft_large" if pretrained else None,
        **kwargs,
    )
    model.arch = "raft_large"
    return model, variables


def raft_small(*, pretrained: bool = False, **kwargs):
    """RAFT small (``model.py:732-767``)."""
    model, variables = _raft(
        feature_encoder_layers=(32, 32, 64, 96, 128),
        feature_encoder_block="bottleneck",
        feature_encoder_norm_layer=NORM_INSTANCE,
        context_encoder_layers=(32, 32, 64, 96, 160),
        context_encoder_block="bottleneck",
        context_encoder_norm_layer=None,
        corr_block_num_levels=4,
        corr_block_radius=3,
        motion_encoder_corr_layers=(96,),
        motion_encoder_flow_layers=(64, 32),
        motion_encoder_out_channels=82,
        recurrent_block_hidden_state_size=96,
        recurrent_block_kernel_size=((3, 3),),
        recurrent_block_padding=((1, 1),),
        flow_head_hidden_size=128,
        use_mask_predictor=False,
        pretrained_arch="raft_small" if pretrained else None,
        **kwargs,
    )
    model.arch = "raft_small"
    return model, variables
