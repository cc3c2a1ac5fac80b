"""Native MI355X inference engine: lowers a :class:`~jax_raft_amd.models.raft.RAFT`
onto the gfx950 kernels as one :class:`Plan` (prologue = encoders + correlation
pyramid, loop body = one refinement iteration) and runs it eagerly from C++
or as a single captured hipGraph.  The plan executor is ``csrc/runtime/plan.h``; the
``add_<op>`` methods used here are generated from the op table of ``csrc/runtime/binding.cpp``.

Mapping to the reference forward (``jax_raft/model.py:557-605``):

=====================================  ==============================================
reference                              engine
=====================================  ==============================================
concat images, feature encoder :562    prep kernel -> implicit-GEMM convs (+IN stats/apply)
build_pyramid :567, :418-446           ``corr`` (MFMA GEMM, pooling fused, all levels)
context encoder :569 (BN eval)         convs with BN folded into weights, fused relu/residual
split/tanh/relu :582-584               final 1x1 conv epilogue writes tanh(h)|relu(ctx)
                                       straight into the persistent GRU input buffers
scan body :495-510                     loop segment: lookup, 5 motion convs, 2x GRU (A/B),
                                       flow head (+mask), coords update, x8 upsample
=====================================  ==============================================

Persistent buffers replace every concat of the reference:
``hx = [h | motion | flow]`` (GRU z/r input, ``model.py:303,366,290``) and
``qx = [r*h | motion | flow]`` (GRU q input, ``model.py:308``).  The context
features -- the third part of the GRU input ``[h | context | motion]`` -- are
loop-invariant, so their share of every ConvGRU gate (z, r and q, plus the
gate biases) is computed ONCE in the prologue (one conv per GRU over the
context, fp32 output) and added per pixel in the loop convs' epilogues (the
``bmap`` bias map).  That removes a third of the GRU GEMMs' K from every
iteration: K = 5 x 256 instead of 5 x 384 for raft_large.
"""
from __future__ import annotations

import itertools
import operator
import weakref
from collections import OrderedDict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch

from ..models.reference import INTERP_MAX_TIMES, BidirectionalFlow, BidirectionalInterp, BidirectionalWarp, interp_times
from ..models.layers import (
    NORM_BATCH,
    NORM_CUSTOM,
    NORM_INSTANCE,
    BottleneckBlock,
    ConvNormActivation,
    CorrBlock,
    FeatureEncoder,
    FlowHead,
    MaskPredictor,
    MotionEncoder,
    RecurrentBlock,
    ResidualBlock,
    UpdateBlock,
)
from .. import knobs
from ..ops import native as nat
from . import lowering, tunedb
from ..ops.native import (
    ACT_NONE,
    ACT_RELU,
    EPI_STD,
    EPI_TAPS,
    ConvSpec,
    conv_args,
    round_up,
)

BF16 = torch.bfloat16
F32 = torch.float32

_TUNE_CACHE: Dict[tuple, int] = {}


def _tune(spec: ConvSpec, x, N, H, W, y, kw, reps: int = 5) -> int:
    """Time every tile config of one conv problem; return the fastest."""
    ops = nat.ops()
    best, best_t = None, None
    for cfg in _candidates(spec, kw, y):
        args = conv_args(spec, x, N, H, W, y, **dict(kw, cfg=cfg))
        ops.conv(*args)  # warm (and JIT-free: all configs are precompiled)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            ops.conv(*args)
        e.record()
        e.synchronize()
        t = s.elapsed_time(e)
        if best_t is None or t < best_t:
            best, best_t = cfg, t
    return best


def _fused_norm(kw) -> bool:
    """The conv writes channel-statistics partials or normalises its input on load: only the
    halo kernel (conv_halo.hip) does either."""
    return kw.get("stats_part") is not None or kw.get("in_stats") is not None


def _candidates(spec: ConvSpec, kw, y) -> Tuple[int, ...]:
    """Tile configs that can run this conv: the taps-epilogue configs, or the implicit-GEMM
    autotune set plus the halo 3x3 configs (halo only when a norm is fused into the conv)."""
    if kw.get("epi") == nat.EPI_TAPS:
        return nat.TAPS_CFGS
    halo = nat.halo_cfgs_for(spec, dict(kw, y=y))
    return halo if _fused_norm(kw) else nat.TUNE_CFGS + halo


def _fold_bn(cna: ConvNormActivation) -> Tuple[torch.Tensor, torch.Tensor]:
    """Conv kernel/bias with an eval-mode BatchNorm folded in."""
    k = cna.layers_0.kernel.detach().float()
    b = cna.layers_0.bias.detach().float()
    if cna.norm == NORM_BATCH:
        bn = cna.layers_1
        s = bn.scale.detach().float() * torch.rsqrt(bn.var.detach().float() + bn.eps)
        k = k * s  # broadcast over cout (last dim)
        b = (b - bn.mean.detach().float()) * s + bn.bias.detach().float()
    return k, b


@dataclass
class _PlanState:
    plan: object                      # plans[0]
    plans: List[object] = field(default_factory=list)   # one native Plan (one hipGraph) per batch part
    choices: List[object] = field(default_factory=list)   # ... and its lowering.PartChoices
    bufs: Dict[str, torch.Tensor] = field(default_factory=dict)
    inp1: Optional[torch.Tensor] = None
    inp2: Optional[torch.Tensor] = None
    out: Optional[torch.Tensor] = None
    n_iters: int = 0
    # Output indirection: every output writer (convex head / bilinear
    # upsampling) reads its destination base from this device int64, so a
    # replay can write into a fresh tensor (forward with copy_output) instead
    # of the captured buffer + a clone of it.  slot_ok: all writers use it.
    out_slot: Optional[torch.Tensor] = None
    slot_ok: bool = True
    slot_ptr: int = 0
    # context parallelism: {slabs, nq (padded slab pixels per image), local, corr} (see _gather_corr)
    cp: Optional[dict] = None
    # raw uint8 frames (K14): (H0, W0, pt, pl) of the frames inside the padded plan size, else None
    src: Optional[Tuple[int, int, int, int]] = None
    # warm start: the plan's static initial-flow input (B, h, w, 2) fp32 (warm plans only), the key
    # buffer of the "previous" projection, and every plan's final-flow buffers, one
    # (b0, nb, flow32, odd-iteration flow32 or None) per batch part
    flow_init: Optional[torch.Tensor] = None
    keys: Optional[torch.Tensor] = None
    flow_out: List[tuple] = field(default_factory=list)
    # bidirectional plans: the forward-backward check's mask buffer (2, B, H, W) uint8 (0 = 1 -> 2),
    # its device-side thresholds [alpha, beta] and the values they currently hold
    occ: Optional[torch.Tensor] = None
    thr: Optional[torch.Tensor] = None
    thr_vals: Optional[Tuple[float, float]] = None
    # ... with ``warp``: the motion-compensated frames (2, B, H0, W0, 3) uint8 (0 = frame 2 sampled with
    # the flow 1 -> 2) and the photometric sums (2, B, 2) int64 (framewarp.hip)
    warped: Optional[torch.Tensor] = None
    photo: Optional[torch.Tensor] = None
    # ... with ``interpolate`` (K times): the splat accumulator (2, B, H0, W0, 4) int64, shared by the times, the
    # device-side (tq, Dmin) rows (K, 2) int32 and the values they currently hold, the frames (K, B, H0, W0, 3)
    # uint8 and the hole masks (K, B, H0, W0) uint8 (interp.hip)
    acc: Optional[torch.Tensor] = None
    par: Optional[torch.Tensor] = None
    par_vals: Optional[tuple] = None
    interp: Optional[torch.Tensor] = None
    holes: Optional[torch.Tensor] = None


_VERSION = operator.attrgetter("_version")


def sintel_pad(H0: int, W0: int) -> Tuple[int, int, int, int]:
    """InputPadder('sintel') of the reference (``scripts/validate_sintel.py:23-31``): the rows /
    columns (top, bottom, left, right) that replicate-pad an H0 x W0 frame to multiples of 8."""
    ph = (((H0 // 8) + 1) * 8 - H0) % 8
    pw = (((W0 // 8) + 1) * 8 - W0) % 8
    return ph // 2, ph - ph // 2, pw // 2, pw - pw // 2


_U8_LUT: Dict[str, torch.Tensor] = {}


def u8_table(device) -> torch.Tensor:
    """x / 255 * 2 - 1 for x = 0..255, evaluated on the host in fp32 exactly as the reference's
    input protocol (validate_sintel.py:177-178, demo.py:9) -- the device kernel looks values up."""
    key = str(device)
    t = _U8_LUT.get(key)
    if t is None:
        t = _U8_LUT[key] = (torch.arange(256, dtype=torch.float32) / 255.0 * 2.0 - 1.0).to(device)
    return t


class RaftEngine:
    """Inference engine bound to one model and one GPU.

    Args:
        use_graph: capture the whole forward (prologue + N iterations) into one
            hipGraph and replay it (default); otherwise launch from C++ eagerly.
        copy_output: return a fresh tensor (default) instead of the engine's
            static output buffer (which the next call overwrites).
        corr_dtype: storage dtype of the correlation pyramid (bf16 default:
            the lookup output feeding the bf16 MFMA convs is bf16 anyway;
            fp32 for bit-closer parity with the fp32 reference).
        gate_dtype: storage dtype of the ConvGRU z gate and of the folded
            context bias map (bf16 default, fp32 for bit-closer parity); the
            hidden state itself is always carried in fp32.
        autotune: pick every conv's tile config from the persisted table
            (runtime/tunedb.py) or, on a miss, by timing the candidates on the
            real buffers when a plan is built; ``False``: a size heuristic.
        streams: (True / False / "auto") run the model's independent branches
            on concurrent lanes of the plan (parallel branches of the captured
            hipGraph): context encoder || the two feature-encoder halves ||
            correlation pyramid in the prologue; in the loop, iteration i+1's
            flow-feature convs and iteration i's mask head + upsampling on a
            side lane while the critical lane runs lookup -> correlation convs
            -> motion conv -> ConvGRU -> flow head.  "auto" (default) = on at
            batch >= 4 per plan with every iteration upsampled and a
            256 -> 576 mask head (raft_large), where it measured faster.
        split: run the batch as this many independent part-forwards captured
            into ONE hipGraph with no edge between them (when the batch
            divides evenly), so one part's kernels fill CUs another part's
            leave idle.
        cfg_override: fixed tile configs per conv spec name (e.g. {"gru0.b": 27},
            tools/schedule_tune.py); ``JR_CFG_OVERRIDE="name=cfg,..."`` adds entries.
        cp_group: context parallelism of the correlation volume:
            a torch.distributed process group (``True``: the default group) whose
            ranks each hold the pyramid of one slab of query rows
            (``parallel/cp.py:row_slabs``) and all-gather the looked-up
            correlation features every iteration (RCCL over xGMI); the rest of
            the update block runs replicated.  Pyramid memory per rank / world.
            One lane, eager from C++ (the collective sits between the two
            halves of the loop body, ``Plan.run_segment``).
        corr: "volume" (default: the all-pairs correlation pyramid, built in the prologue) or
            "on_demand": no volume -- the prologue pools the target features (``feat_pool``)
            and every iteration's lookup forms the correlations it needs from the two
            feature maps (``lookup_od``, csrc/kernels/corr_od.hip).  Memory O(P * C) instead
            of O(P^2); every other op of the plan is the volume plan's.  Cold and warm
            forwards, float and uint8 frames, both output modes; not with ``bidirectional``,
            :meth:`pipelined`, ``cp_group`` or the fp32 / mixed engines (``NotImplementedError``).
        precision: "bf16" (default: bf16 MFMA operands and activations, fp32
            accumulation, fp32 hidden state / flow / upsampled output) or "fp32"
            (the reference's own precision end to end on the f32 MFMA:
            :class:`~jax_raft_amd.runtime.engine_f32.RaftEngineF32`).

    Schedules (chosen per plan part, ``runtime/lowering.py``: ``PartChoices.schedule`` and the
    ``PartRecorder.schedule_*`` methods): "lanes", the lane schedule above; "one_lane", one
    in-order lane with every iteration upsampled (batch < 4, raft_small); the final-only serving
    mode, "final_merged" below batch 4 and "final"; and "cp" (``cp_group``).  In all of them the flow
    update of iteration i runs inside iteration i+1's lookup kernel and the
    FlowHead's second conv is an MFMA epilogue of its first (raft_large) or a
    skinny taps GEMM (raft_small).  Variants measured and removed in round 3
    (kept in the history): double-buffered flow-head outputs, the 3x3 EPI_FLOW
    and halo-tiled flow heads, the EPI_CONVEX conv epilogue, the side-lane and
    main-lane flow-feature placements, the mask lane forking after convcorr1,
    separate per-part graphs on separate streams, and submit() (the two phases
    as separate graphs on two streams, which serialise on this ROCm).
    """

    def __new__(cls, *args, precision: str = "bf16", **kwargs):
        if precision not in ("bf16", "fp32", "mixed"):
            raise ValueError(f"precision must be 'bf16', 'fp32' or 'mixed', got {precision!r}")
        if precision == "fp32" and cls is RaftEngine:
            from .engine_f32 import RaftEngineF32
            cls = RaftEngineF32
        elif precision == "mixed" and cls is RaftEngine:
            from .engine_f32 import RaftEngineMixed
            cls = RaftEngineMixed
        return super().__new__(cls)

    precision = "bf16"
    fe_external = False   # the feature encoder runs outside the plan (RaftEngineMixed: fp32), fmap filled before it

    # Lowering choices.  Each is the measured winner of an A/B (the profile is cited where the
    # choice is used); they are class attributes rather than environment switches so that tests
    # can cover the alternative lowering against the same oracle (monkeypatch.setattr on the
    # class, before the plan is built).  Operational environment variables: jax_raft_amd/knobs.py.
    GRU = "auto"          # ConvGRU stage lowering: "auto" | "halo" | "fused" | "unfused" (_gru_path)
    GRU_ME = "auto"       # motion conv inside the first fused ConvGRU stage: "auto" | "on" | "off" (_gru_me_ok)
    FLOW_FUSED = "auto"   # lane schedule: the flow branch's two convs as one launch: "auto" | "on" | "off" (_flow_fused_ok)
    PRO_LANES = "auto"    # prologue branches on lanes at one-lane loops: "auto" | "on" | "off"
    HALO_NORM = True      # encoder instance norms fused into the halo 3x3 convs
    MERGED_UP = True      # one-lane loop: 7x7 flow conv merged with the x8 upsampling (merged.hip)
    CONV_GROUP = True     # one-lane loop: last correlation conv + convflow2 as one grouped grid
    MASK_PARITY = False   # lane schedule: parity-buffered h copy for the mask lane (slower at b4)
    CORR_PERSIST_B1 = True   # the persistent blocked pyramid kernel at batch 1 too (plans outside pipelined slots)
    HOST_GATE = True      # host gate of long replays (see GATE_MIN_ITERS)
    WARM_FILL_RADIUS = 4  # flow_init="previous": hole-filling radius of the forward projection (1/8-res cells)

    def __init__(self, model, device, use_graph: bool = True, copy_output: bool = True,
                 corr_dtype: torch.dtype = torch.bfloat16, gate_dtype: torch.dtype = torch.bfloat16,
                 autotune: bool = True, streams="auto", split: int = 1,
                 cfg_override: Optional[Dict[str, int]] = None, cp_group=None, **mode):
        # the two keywords that select the engine's variant: ``precision`` (already consumed by
        # __new__, which picked the class) and ``corr``
        mode.pop("precision", None)
        corr = mode.pop("corr", "volume")
        if mode:
            raise TypeError(f"RaftEngine: unexpected keyword arguments {sorted(mode)}")
        if corr not in ("volume", "on_demand"):
            raise ValueError(f"corr must be 'volume' or 'on_demand', got {corr!r}")
        if corr == "on_demand":
            if self.precision != "bf16":
                raise NotImplementedError(f"corr='on_demand': not with precision={self.precision!r} (the on-demand "
                                          "lookup is lowered for the bf16 engine only)")
            if cp_group is not None:
                raise NotImplementedError("corr='on_demand': not with context parallelism (cp_group splits the "
                                          "volume the on-demand path never builds)")
        self.corr_mode = corr
        nat.require()
        self._init_cp(cp_group)
        assert streams in (True, False, "auto"), streams
        self.streams_mode = streams
        # instance norms of the encoders fused into halo 3x3 convs (statistics partials in the
        # producer's epilogue, normalise + relu in the consumer's footprint load; a residual
        # block's output built -- residual + its norm -- inside the next block's first halo conv;
        # profiles/r4_in_fusion_ab.txt); HALO_NORM = False: the separate statistics / norm_act passes
        self.halo_norm = bool(self.HALO_NORM)
        self.halo_res = self.halo_norm
        # of the most recently built plan (set by runtime/lowering.py:_finish; a plan's own: st.choices)
        self.gru_path = self.corr_blocked = None
        self.gate_dtype = gate_dtype
        self.split = split
        self.cfg_override = dict(cfg_override or {})
        self.cfg_override.update(knobs.cfg_override())
        self._cf1_w = self._cf1_b = None
        self._fh2_b = None
        self._convex_w = self._convex_b = None
        self._taps_w = None
        self._taps_epi_w = None
        self._cc1_w = self._cc1_b = None
        self._halo_w: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}   # GRU gi -> gru_halo (wa, wb)
        # the model: held strongly by an engine built directly, weakly by one the model caches itself
        # (RAFT.engine -> _hold_model_weakly): model._engines -> engine -> model would be a reference
        # cycle, and every plan of a cycle-held engine (hipGraphs, 64 events, lane streams, pyramid
        # buffers) would outlive the model until a full garbage collection
        self._model_strong = model
        self._model_ref = None
        self.device = torch.device(device)
        self.use_graph = use_graph
        self.copy_output = copy_output
        # host gate: the graph replay of a forward with >= GATE_MIN_ITERS iterations is launched
        # only after the previous call's work has finished (the host waits on its completion
        # event).  A long replay enqueued behind a still-running one runs slower on this ROCm:
        # batch 1 raft_large 32 it 208-213 -> 261 pairs/s, raft_small 32 it 334-337 -> 435-436,
        # batch 4 387-393 -> 401-402; short forwards lose (raft_small 12 it 713-754 -> 646-698),
        # where the exposed host launch is a larger share.  profiles/r4_host_gate.txt
        self.host_gate = bool(self.HOST_GATE)
        self._done_ev: Optional[torch.cuda.Event] = None
        self.corr_dtype = corr_dtype
        self.autotune = autotune
        self._specs: Dict[str, ConvSpec] = {}
        self.arch = tunedb.gpu_arch(self.device)
        self.chosen_cfgs: Dict[str, Optional[int]] = {}   # conv spec name -> tile config of the last plan built
        self._sources: Dict[str, callable] = {}
        # built plans, least recently used first; at most max_plans key groups (a forward's plan and
        # its pipelined() slots are one group) -- a long-lived serving / eval process over many input
        # shapes keeps a bounded set; release() drops them all
        self._states: "OrderedDict[tuple, _PlanState]" = OrderedDict()
        self._snap = None    # parameter / module snapshot of the last repack (_snapshot / _stale)
        self._pp = None   # pipelined(): {key, n, pending slot}
        self._last = None   # flow_init="previous": ((B, H, W), n_iters, flow_out) of the last forward()
        self._analyse()
        self._pack()

    @property
    def model(self):
        m = self._model_strong if self._model_strong is not None else self._model_ref()
        if m is None:
            raise ReferenceError("RaftEngine: its model has been garbage-collected")
        return m

    def _hold_model_weakly(self) -> None:
        """Called by the model that caches this engine (``RAFT.engine``): keep a weak reference."""
        if self._model_strong is not None:
            self._model_ref = weakref.ref(self._model_strong)
            self._model_strong = None

    # ------------------------------------------------------------ plan cache
    max_plans = 8   # key groups kept (an instance attribute may lower / raise it)

    @staticmethod
    def _group(key: tuple) -> tuple:
        return key[:-2] if len(key) > 2 and key[-2] == "pslot" else key

    # raw uint8 frames are prepared on the device by the plan's prep kernel (an engine without that
    # path normalises + pads them with framework ops first: the fp32 engine)
    _native_u8 = True

    def _key(self, image1: torch.Tensor, image2: torch.Tensor, n_iters: int, all_iters: bool) -> tuple:
        """Plan key of one call: (B, H, W, n, all) for float NHWC images in [-1, 1] with H, W % 8 == 0;
        + ("u8", H0, W0, pt, pl) for uint8 NHWC frames of any size, whose plan runs at the padded
        size (InputPadder 'sintel' semantics) and returns the flows cropped back to H0 x W0."""
        B, H, W, C = image1.shape
        assert C == 3, "images must be NHWC with 3 channels"
        assert tuple(image2.shape) == tuple(image1.shape), "input images should have the same shape"
        if image1.dtype == torch.uint8:
            assert image2.dtype == torch.uint8, "both frames must be uint8"
            pt, pb, pl, pr = sintel_pad(H, W)
            return (B, H + pt + pb, W + pl + pr, n_iters, bool(all_iters), "u8", H, W, pt, pl)
        assert H % 8 == 0 and W % 8 == 0, "input image H and W should be divisible by 8"
        return (B, H, W, n_iters, bool(all_iters))

    def _build_key(self, key: tuple, *, parts: Optional[int] = None, slot: bool = False) -> _PlanState:
        """Key layout: (B, H, W, n, all)[ + ("u8", H0, W0, pt, pl)][ + ("warm",) | ("bidir",) | ("bidir", "warp") |
        ("bidir", "interp", K)][ + ("pslot", slot)].  ``parts`` / ``slot``: see :meth:`_build` (a bidirectional plan is one part)."""
        src = tuple(key[6:10]) if len(key) >= 10 and key[5] == "u8" else None
        if "bidir" in key[5:]:
            interp = key[key.index("interp") + 1] if "interp" in key[5:] else 0
            return self._build_bidir(*key[:5], src, warp="warp" in key[5:], slot=slot, interp=interp)
        return self._build(*key[:5], src=src, warm="warm" in key[5:], parts=parts, slot=slot)

    @staticmethod
    def _crop(st: _PlanState, out: torch.Tensor) -> torch.Tensor:
        if st.src is None:
            return out
        H0, W0, pt, pl = st.src
        return out[:, :, pt:pt + H0, pl:pl + W0]

    def _host_u8(self, image1, image2):
        """uint8 frames -> float [-1, 1], replicate-padded to /8 with framework ops on the device
        (engines without the native u8 prep); returns (img1, img2, crop)."""
        B, H0, W0, _ = image1.shape
        pt, pb, pl, pr = sintel_pad(H0, W0)
        lut = u8_table(self.device)

        def one(x):
            x = lut[x.to(self.device).long()].permute(0, 3, 1, 2)
            return torch.nn.functional.pad(x, [pl, pr, pt, pb], mode="replicate").permute(0, 2, 3, 1).contiguous()

        return one(image1), one(image2), (H0, W0, pt, pl)

    def _plan_state(self, key: tuple, build) -> _PlanState:
        """The plan of ``key`` (built by ``build()`` on a miss), marked most recently used; a miss
        first evicts the least recently used key groups beyond ``max_plans`` (never the group of a
        batch :meth:`pipelined` left pending)."""
        st = self._states.get(key)
        if st is not None:
            for k in [k for k in self._states if self._group(k) == self._group(key)]:
                self._states.move_to_end(k)
            return st
        self._evict(self._group(key))
        st = build()
        self._states[key] = st
        return st

    def _evict(self, incoming: tuple) -> None:
        groups = list(OrderedDict.fromkeys(self._group(k) for k in self._states))
        pend = self._pp["key"] if self._pp is not None and self._pp["pending"] is not None else None
        n = len(groups) + (incoming not in groups)
        cap = max(1, int(self.max_plans))
        for g in groups:
            if n <= cap:
                break
            if g == incoming or g == pend:
                continue
            self._drop_group(g)
            n -= 1

    def _quiesce(self) -> None:
        """Wait for this engine's launched work before plans are destroyed: Plan::~Plan destroys
        graph execs, events and lane streams, and HIP does not document that destroying a graph
        exec still running is deferred until it finishes.  Eviction / release are rare."""
        if self.device.type == "cuda" and self._states and not torch.cuda.is_current_stream_capturing():
            torch.cuda.synchronize(self.device)

    def _drop_group(self, g: tuple) -> None:
        # a plan's pipelined graph holds the other slot's kernel nodes (its buffers): the whole
        # group goes at once
        self._quiesce()
        for k in [k for k in self._states if self._group(k) == g]:
            del self._states[k]
        if self._pp is not None and self._pp["key"] == g:
            self._pp = None

    def release(self) -> None:
        """Drop every built plan: their hipGraphs, events, lane streams and device buffers are freed
        now (the next forward rebuilds).  Not while a :meth:`pipelined` batch is pending."""
        if self._pp is not None and self._pp["pending"] is not None:
            raise RuntimeError("release(): flush() the pending pipelined batch first")
        self._quiesce()
        self._states.clear()
        self._pp = None
        self._last = None
        self._done_ev = None

    def num_plans(self) -> int:
        return len(self._states)

    # ----------------------------------------------------------- structure
    def _analyse(self):
        m = self.model
        fe, ce = m.feature_encoder, m.context_encoder
        for enc in (fe, ce):
            if not isinstance(enc, FeatureEncoder):
                raise NotImplementedError("native engine supports FeatureEncoder encoders only")
            if enc.block == "custom" or enc.norm_kind == NORM_CUSTOM:
                raise NotImplementedError("native engine lowers residual / bottleneck blocks with batch / "
                                          "instance / no norm only")
        ub = m.update_block
        if not (isinstance(ub, UpdateBlock) and isinstance(ub.motion_encoder, MotionEncoder)
                and isinstance(ub.recurrent_block, RecurrentBlock) and isinstance(ub.flow_head, FlowHead)
                and isinstance(m.corr_block, CorrBlock)
                and (m.mask_predictor is None or isinstance(m.mask_predictor, MaskPredictor))):
            raise NotImplementedError("native engine lowers the reference update block / correlation block / "
                                      "mask predictor classes only")
        me, rb, fh = ub.motion_encoder, ub.recurrent_block, ub.flow_head
        self.hidden = rb.hidden_size
        self.ctx_ch = ce.out_channels - self.hidden
        self.num_levels = m.corr_block.num_levels
        self.radius = m.corr_block.radius
        S = 2 * self.radius + 1
        self.corr_ch = self.num_levels * S * S
        self.corr_cs = round_up(self.corr_ch, 8)
        self.mot_out = me.out_channels
        # loop buffers hold [h | motion | flow]; the context part of the GRU input is folded (see module doc)
        self.hx_real = self.hidden + self.mot_out
        # padded to a multiple of 64 channels when that costs <= 16 zero channels
        # (raft_small: 178 -> 192): the GRU convs' 64-deep K stages then lie inside
        # one tap and take the FAST im2col loader (conv_igemm.h:FastRow)
        hx64 = round_up(self.hx_real, 64)
        self.hx_cs = hx64 if hx64 - self.hx_real <= 16 else round_up(self.hx_real, 8)
        self.mot_off = self.hidden
        self.flow_off = self.mot_off + self.mot_out - 2
        self.gate_cs = round_up(3 * self.hidden, 8)   # fp32 context bias map: [z | r | q] per GRU
        if self.hidden % 16:
            raise NotImplementedError("native engine needs hidden % 16 == 0")
        self.fh_hidden = fh.hidden_size
        self.has_mask = m.mask_predictor is not None
        self.fmap_ch = fe.out_channels
        if self.fmap_ch % 64:
            raise NotImplementedError("native correlation needs feature channels % 64 == 0")

    def _snapshot(self):
        """What a repack saw: every parameter / buffer with its version counter, and every
        module's child list.  Holds the modules' dicts and tensors, never the root module
        itself (a weakly held model stays collectable)."""
        root = self.model
        mods = [root] + [m for n, m in root.named_modules() if n]
        dicts = [d for mod in mods for d in (mod._parameters, mod._buffers, mod._modules)]
        lens = list(map(len, dicts))
        pdicts = [d for mod in mods for d in (mod._parameters, mod._buffers)]
        keys = [(d, k) for d in pdicts for k, t in d.items() if t is not None]
        tensors = [d[k] for d, k in keys]
        kid_dicts = [mod._modules for mod in mods]
        kids = list(itertools.chain.from_iterable(map(dict.values, kid_dicts)))
        return (dicts, lens, [d for d, _ in keys], [k for _, k in keys], tensors,
                list(map(_VERSION, tensors)), kid_dicts, kids)

    def _stale(self) -> bool:
        """Whether any parameter / buffer changed in place (version counter) or was replaced,
        or a submodule was replaced, since the last repack -- checked on every forward with
        C-level map() walks over the snapshot: the tuple signature it replaces cost 0.2-0.7 ms of
        host time per call, which the batch-1 12-iteration stream (~1.2 ms of GPU time per
        pair) pays directly."""
        snap = self._snap
        if snap is None:
            return True
        dicts, lens, pds, pks, tensors, versions, kid_dicts, kids = snap
        if list(map(len, dicts)) != lens or list(map(_VERSION, tensors)) != versions:
            return True
        if not all(map(operator.is_, map(dict.get, pds, pks), tensors)):
            return True
        return not all(map(operator.is_, itertools.chain.from_iterable(map(dict.values, kid_dicts)), kids))

    def _reg(self, name: str, fn):
        """Register a conv spec source: fn() -> (kernel HWIO, bias, stride, padding, cin8)."""
        self._sources[name] = fn

    def _pack(self):
        """(Re)pack every conv into bf16 GEMM layout; BN folded (eval mode).  Packed
        tensors are updated in place so captured graphs stay valid."""
        if not self._sources:
            self._define_specs()
        for name, fn in self._sources.items():
            k, b, stride, pad, cin8 = fn()
            k = k.to(self.device)
            if name in self._specs:
                sp = self._specs[name]
                nat.pack_weight(k, sp.cin8, out=sp.w)
                if sp.wh is not None:
                    nat.pack_halo_conv(k, sp.cin8, out=sp.wh)
                sp.b.copy_(b.float().to(self.device))
            else:
                self._specs[name] = nat.make_spec(k, b.to(self.device), stride, pad, cin8=cin8, device=self.device)
        fh2 = self.model.update_block.flow_head.conv2
        bf = fh2.bias.detach().float().to(self.device).contiguous()
        if self._fh2_b is None:
            self._fh2_b = bf
        else:
            self._fh2_b.copy_(bf)
        # the correlation features' first 1x1 conv on the LDS-resident-weight kernel (conv1x1.hip)
        cc1 = self.model.update_block.motion_encoder.convcorr1.layers_0
        kpad = next((k for k in nat.CONV1X1_KPADS if k >= self.corr_cs), None)
        if kpad is not None and cc1.kernel.shape[:2] == (1, 1) and cc1.kernel.shape[3] % 64 == 0:
            wc = nat.pack_conv1x1(cc1.kernel.to(self.device), kpad)
            bc = cc1.bias.detach().float().to(self.device).contiguous()
            if self._cc1_w is None:
                self._cc1_w, self._cc1_b, self._cc1_kpad = wc, bc, kpad
            else:
                self._cc1_w.copy_(wc)
                self._cc1_b.copy_(bc)
        if fh2.kernel.shape[2] in (128, 256):
            wt = nat.pack_taps(fh2.kernel.to(self.device))
            if self._taps_w is None:
                self._taps_w = wt
            else:
                self._taps_w.copy_(wt)
        if tuple(fh2.kernel.shape) == (3, 3, 256, 2):
            wt = nat.pack_taps_epi(fh2.kernel.to(self.device))
            if self._taps_epi_w is None:
                self._taps_epi_w = wt
            else:
                self._taps_epi_w.copy_(wt)
        mp = self.model.mask_predictor
        if mp is not None and tuple(mp.conv.kernel.shape) == (1, 1, 256, 576):
            wc, bc = nat.pack_convex_head(mp.conv.kernel.to(self.device), mp.conv.bias.to(self.device))
            if self._convex_w is None:
                self._convex_w, self._convex_b = wc, bc
            else:
                self._convex_w.copy_(wc)
                self._convex_b.copy_(bc)
        if self._halo_geom() is not None:   # the halo-tiled fused ConvGRU's weight streams
            for gi in range(len(self.model.update_block.recurrent_block.kernel_size)):
                ka = self._sources[f"gru{gi}.a"]()[0].to(self.device)
                kb = self._sources[f"gru{gi}.b"]()[0].to(self.device)
                old = self._halo_w.get(gi)
                self._halo_w[gi] = (nat.pack_gru_halo(ka, self.hx_cs, out=old[0] if old else None),
                                    nat.pack_gru_halo(kb, self.hx_cs, out=old[1] if old else None))
        cf1 = self.model.update_block.motion_encoder.convflow1.layers_0
        if nat.direct_conv_ok(cf1.kernel, cf1.stride):
            wd = nat.pack_direct_weight(cf1.kernel).to(self.device)
            bd = cf1.bias.detach().float().to(self.device).contiguous()
            if self._cf1_w is None:
                self._cf1_w, self._cf1_b = wd, bd
            else:
                self._cf1_w.copy_(wd)
                self._cf1_b.copy_(bd)
        self._snap = self._snapshot()

    def _define_specs(self):
        m = self.model

        def cna_src(cna: ConvNormActivation, cin8=None):
            def f():
                k, b = _fold_bn(cna)
                c = cna.layers_0
                return k, b, c.stride, c.padding, cin8
            return f

        def conv_src(c, cin8=None):
            return lambda: (c.kernel.detach().float(), c.bias.detach().float(), c.stride, c.padding, cin8)

        def s2d_src(cna: ConvNormActivation):
            def f():
                k, b = _fold_bn(cna)
                return nat.s2d_stem_kernel(k), b, (1, 1), (2, 2), 16
            return f

        for tag, enc in (("fe", m.feature_encoder), ("ce", m.context_encoder)):
            self._reg(f"{tag}.stem", cna_src(enc.convnormrelu, 8))
            c0 = enc.convnormrelu.layers_0
            if tuple(c0.kernel.shape[:3]) == (7, 7, 3) and tuple(c0.stride) == (2, 2) and tuple(c0.padding) == (3, 3):
                # the stem as a 4x4 conv over the 2x2 space-to-depth input (ops/native.py:s2d_stem_kernel)
                self._reg(f"{tag}.stem_s2d", s2d_src(enc.convnormrelu))
            for li in (1, 2, 3):
                layer = getattr(enc, f"layer{li}")
                for bi in range(layer.n):
                    blk = getattr(layer, f"layers_{bi}")
                    names = ["convnormrelu1", "convnormrelu2"] + (["convnormrelu3"] if isinstance(blk, BottleneckBlock) else [])
                    if blk.stride != (1, 1):
                        names.append("downsample")
                    for nm in names:
                        self._reg(f"{tag}.l{li}.b{bi}.{nm}", cna_src(getattr(blk, nm)))
            self._reg(f"{tag}.conv", conv_src(enc.conv))
        ub = m.update_block
        me, rb, fh = ub.motion_encoder, ub.recurrent_block, ub.flow_head
        self._reg("me.convcorr1", cna_src(me.convcorr1, self.corr_cs))
        if len(me.corr_layers) == 2:
            self._reg("me.convcorr2", cna_src(me.convcorr2))
        self._reg("me.convflow1", cna_src(me.convflow1, 8))
        self._reg("me.convflow2", cna_src(me.convflow2))
        self._reg("me.conv", cna_src(me.conv))
        hx_cs = self.hx_cs   # the sources below must not capture the engine (no self-cycle: plans die by refcount)
        for gi in range(len(rb.kernel_size)):
            gru = getattr(rb, f"convgru{gi + 1}")

            H_, C_ = self.hidden, self.ctx_ch

            def loop_part(k):  # input channels [h | context | motion] -> [h | motion]
                k = k.detach().float()
                return torch.cat([k[:, :, :H_], k[:, :, H_ + C_:]], dim=2)

            def gru_a(gru=gru):
                k = torch.cat([loop_part(gru.convz.kernel), loop_part(gru.convr.kernel)], dim=3)
                return k, torch.zeros(2 * H_), (1, 1), gru.padding, hx_cs

            def gru_b(gru=gru):
                return loop_part(gru.convq.kernel), torch.zeros(H_), (1, 1), gru.padding, hx_cs

            def gru_ctx(gru=gru):  # context share of [z | r | q] + the gate biases (prologue, once)
                k = torch.cat([c.kernel.detach()[:, :, H_:H_ + C_] for c in (gru.convz, gru.convr, gru.convq)], dim=3)
                b = torch.cat([c.bias.detach() for c in (gru.convz, gru.convr, gru.convq)])
                return k.float(), b.float(), (1, 1), gru.padding, None

            self._reg(f"gru{gi}.a", gru_a)
            self._reg(f"gru{gi}.b", gru_b)
            self._reg(f"gru{gi}.ctx", gru_ctx)
        if self.has_mask:
            mp = m.mask_predictor

            def fh1():
                k = torch.cat([fh.conv1.kernel.detach(), mp.convrelu.layers_0.kernel.detach()], dim=3).float()
                b = torch.cat([fh.conv1.bias.detach(), mp.convrelu.layers_0.bias.detach()]).float()
                return k, b, (1, 1), (1, 1), None

            self._reg("fh1", fh1)
            self._reg("fh1.flow", conv_src(fh.conv1))  # final-only mode / split mask head: flow head alone
            self._reg("mask.convrelu", cna_src(mp.convrelu))
            self._reg("mask", conv_src(mp.conv))
        else:
            self._reg("fh1", conv_src(fh.conv1))

        def fh2_taps():  # (3,3,cin,2) -> (1,1,cin,18): out channel tap*2 + o
            k = fh.conv2.kernel.detach().float()
            cin = k.shape[2]
            k = k.reshape(9, cin, 2).permute(1, 0, 2).reshape(1, 1, cin, 18)
            return k, torch.zeros(18), (1, 1), (0, 0), None

        self._reg("fh2.taps", fh2_taps)

    # ------------------------------------------------------------- autotune
    def _conv(self, plan, spec: ConvSpec, x, N, H, W, y, x_alt=None, **kw):
        """Append one conv to ``plan``, choosing its tile config (autotuned).  ``x_alt``: the
        input of odd loop iterations (a state that ping-pongs between two buffers)."""
        args = conv_args(spec, x, N, H, W, y, **self._conv_kw(spec, x, N, H, W, y, kw))
        if x_alt is not None:
            plan.add_conv_alt(*args, x_alt)
        else:
            plan.add_conv(*args)

    def _conv_group(self, plan, a: tuple, b: tuple) -> bool:
        """Two independent STD-epilogue convs ``(spec, x, N, H, W, y, kw)`` as ONE grid
        (conv_igemm.h:conv_grouped_kernel) in the tile config tuned for the first, when a
        grouped launch serves that config; returns False (nothing added) otherwise."""
        kwa = self._conv_kw(*a[:6], a[6])
        cfg = kwa.get("cfg")
        if a[6].get("cfg") is None and self.autotune:
            # a measured config for the PAIR (tuned DB key "group" + both problems) beats the
            # first conv's own: profiles/r3_grouped_cfg_ab.txt
            (sa, xa, N, H, W, _), (sb, xb) = a[:6], b[:2]
            gkey = ("group", N * H * W, sa.cout, sa.kh, sa.kw, sa.cin8, xa.shape[-1], sb.cout, sb.kh, sb.kw, sb.cin8,
                    xb.shape[-1])
            gcfg = tunedb.peek(self.arch, gkey)
            name_a = next((k for k, v in self._specs.items() if v is sa), None)
            if gcfg in nat.GROUPED_CFGS and name_a not in self.cfg_override:
                cfg = gcfg
                kwa = dict(kwa, cfg=cfg)
                if name_a is not None:
                    self.chosen_cfgs[name_a] = cfg
        def fast(sp):   # binding.cpp build_conv: the FAST im2col loader (both convs must share it)
            taps = sp.kh * sp.kw
            return taps <= 32 and (taps == 1 or sp.cin8 % 64 == 0)

        if cfg not in nat.GROUPED_CFGS or fast(a[0]) != fast(b[0]):
            return False
        kwb = dict(b[6], cfg=cfg)
        name = next((k for k, v in self._specs.items() if v is b[0]), None)
        if name is not None:
            self.chosen_cfgs[name] = cfg
        ta, ia, aa = conv_args(*a[:6], **kwa)
        tb, ib, ab = conv_args(*b[:6], **kwb)
        plan.add_conv_group(ta, ia, aa, tb, ib, ab)
        return True

    def _conv_kw(self, spec: ConvSpec, x, N, H, W, y, kw):
        """``kw`` with the tile config of this conv (override / persisted / autotuned)."""
        if self.cfg_override and kw.get("cfg") is None:
            name = next((k for k, v in self._specs.items() if v is spec), None)
            if name in self.cfg_override:
                kw = dict(kw, cfg=self.cfg_override[name])
        if kw.get("epi") == EPI_TAPS and not self.autotune and kw.get("cfg") is None:
            kw = dict(kw, cfg=nat.TAPS_CFGS[0])
        if _fused_norm(kw) and not self.autotune and kw.get("cfg") is None:
            kw = dict(kw, cfg=_candidates(spec, kw, y)[0])
        if self.autotune and kw.get("cfg") is None:
            OH, OW = kw["out_hw"] if kw.get("out_hw") is not None else spec.out_hw(H, W)
            valid = _candidates(spec, kw, y)
            key = (N * OH * OW, spec.cout, spec.kh, spec.kw, spec.sh, spec.sw, spec.cin8, x.shape[-1],
                   kw.get("epi", EPI_STD), kw.get("bmap") is not None)
            # problems the halo kernel can run are keyed apart (decisions made before it existed
            # never timed it); a fused norm restricts the choice to the halo configs
            if any(c >= nat.HALO_CFG0 for c in valid):
                key = key + ("halo-norm" if _fused_norm(kw) else "halo",)
            cfg = _TUNE_CACHE.get(key + (str(self.device),))
            if cfg is None:
                cfg = tunedb.lookup(self.arch, key, valid)   # persisted decision (runtime/tunedb.py)
                if cfg is None:
                    cfg = _tune(spec, x, N, H, W, y, kw)
                    tunedb.record(self.arch, key, cfg)
                cfg = self._agree(cfg)
                _TUNE_CACHE[key + (str(self.device),)] = cfg
            kw = dict(kw, cfg=cfg)
        name = next((k for k, v in self._specs.items() if v is spec), None)
        if name is not None:
            self.chosen_cfgs[name] = kw.get("cfg")
        return kw

    # ------------------------------------------------------------- lowering
    def _encoder(self, st: _PlanState, plan, tag: str, enc: FeatureEncoder, x: torch.Tensor, N: int, H: int,
                 W: int, bt: str = ""):
        """Lower a FeatureEncoder up to (not including) its final 1x1 conv.  ``tag``
        names the conv specs ("fe"/"ce"), ``bt`` prefixes the buffers (batch part).
        Instance norms: a two-pass statistics op, then normalise + activation
        (+ residual).  Measured and dropped: the statistics fused into the conv
        kernels (per-tile partials re-read from L2 after the epilogue, only
        configs with one channel tile / image-aligned pixel tiles): 319-320 vs
        321-323 pairs/s; a one-launch statistics kernel with a last-block
        reduction: 0.9 ms/step slower (profiles/r2_pipelined_graph_ab.txt)."""
        inorm = enc.norm_kind == NORM_INSTANCE
        sp = self._specs
        bufs = st.bufs

        def alloc(name, shape, dtype=BF16):
            t = torch.zeros(shape, dtype=dtype, device=self.device)
            bufs[bt + name] = t
            return t

        def conv_raw(name, x, N, H, W, act=ACT_NONE, res=None, res_post=0, out_hw=None):
            s = sp[name]
            OH, OW = out_hw if out_hw is not None else s.out_hw(H, W)
            y = alloc(name + ".y", (N, OH, OW, s.cout))
            self._conv(plan, s, x, N, H, W, y, act=act, res=res, res_post=res_post, out_hw=out_hw)
            return y, OH, OW

        def halo_fusable(name) -> bool:
            return self.halo_norm and bool(nat.halo_cfgs_for(sp[name], {}))

        def conv_stats(name, x, N, H, W, in_stats=None, in_res=None, in_res_stats=None, xn=None):
            """A halo 3x3 conv that writes its output's channel-statistics partials (reduced
            by one small launch) and, given ``in_stats``, instance-normalises + relus its raw
            input as it loads it (no channel_stats pass over the output, no norm_act pass
            over the input); with ``in_res`` (+ its stats) the input is a residual block's
            output relu(IN(x) + [IN](res)), built on the fly and written to ``xn``."""
            s = sp[name]
            y = alloc(name + ".y", (N, H, W, s.cout))
            nb_max = nat.halo_max_blocks(s.cin8, H, W)
            part = alloc(name + ".part", (N, nb_max, s.cout, 2), F32)
            # a residual block's output: relu(res + relu(IN(raw))) (model.py:171-180), in_relu bits 0 + 1
            kw = dict(stats_part=part, in_stats=in_stats, in_relu=3 if in_res is not None else 1, in_hw=H * W,
                      in_res=in_res, in_res_stats=in_res_stats, xn=xn)
            kw = self._conv_kw(s, x, N, H, W, y, kw)
            if kw.get("cfg") is None or kw["cfg"] < nat.HALO_CFG0:   # an override chose another kernel
                return None
            plan.add_conv(*conv_args(s, x, N, H, W, y, **kw))
            c = nat.halo_cfg(kw["cfg"])
            nb = -(-H // c[4]) * -(-W // c[5]) * c[2]
            st_ = alloc(name + ".stats", (N, s.cout, 2), F32)
            plan.add_stats_final([part, st_], [N, nb, s.cout])
            return y, st_

        def stem(act=ACT_NONE):
            if x.shape[-1] == 16:   # space-to-depth input (prep s2d): the 4x4 / stride-1 form of the stem
                return conv_raw(f"{tag}.stem_s2d", x, N, H // 2, W // 2, act=act, out_hw=(H // 2, W // 2))
            return conv_raw(f"{tag}.stem", x, N, H, W, act=act)

        def stats(name, y, N, HW, C):
            t = alloc(name + ".stats", (N, C, 2), F32)
            plan.add_stats([y, t], [N, HW, C])
            return t

        def norm_act(name, x, sx, res=None, sr=None, mode_r=0, relu=3):
            N_, H_, W_, C = x.shape
            y = alloc(name + ".n", (N_, H_, W_, C))
            plan.add_norm_act([x, sx, None, None, res, sr, None, None, y],
                              [1, mode_r, N_, H_ * W_, C, relu], 1e-5)
            return y

        # Instance-norm encoders keep a block's output lazy -- (raw, stats, residual, its stats)
        # -- and build it inside the next block's first conv when that is a stride-1 halo conv
        # (which also writes it out for the next residual); otherwise one norm_act pass
        # materialises it (RaftEngine.HALO_NORM = False: always).
        pend = None

        def materialise(p_):
            return norm_act(p_["name"], p_["raw"], p_["s"], res=p_["res"], sr=p_["rs"],
                            mode_r=1 if p_["rs"] is not None else 0, relu=3 if p_["res"] is not None else 2)

        if inorm:
            y, H, W = stem()
            pend = dict(name=f"{tag}.stem", raw=y, s=stats(f"{tag}.stem", y, N, H * W, y.shape[-1]), res=None, rs=None)
            x = None
        else:
            x, H, W = stem(act=ACT_RELU)
        for li in (1, 2, 3):
            layer = getattr(enc, f"layer{li}")
            for bi in range(layer.n):
                blk = getattr(layer, f"layers_{bi}")
                pre = f"{tag}.l{li}.b{bi}"
                names = ["convnormrelu1", "convnormrelu2"] + (["convnormrelu3"] if isinstance(blk, BottleneckBlock) else [])
                has_ds = blk.stride != (1, 1)
                if inorm:
                    h_, w_ = H, W
                    y, ys = x, None   # ys: stats of a raw conv output y still to be normalised
                    j0 = 0
                    c1 = f"{pre}.{names[0]}"
                    if (pend is not None and self.halo_res and not has_ds and halo_fusable(c1) and sp[c1].out_hw(h_, w_) == (h_, w_)
                            and pend["raw"].shape[-1] == sp[c1].cin8):
                        xb = alloc(f"{pre}.x", tuple(pend["raw"].shape))
                        fused = conv_stats(c1, pend["raw"], N, h_, w_, in_stats=pend["s"], in_res=pend["res"],
                                           in_res_stats=pend["rs"], xn=xb)
                        if fused is not None:
                            x, pend = xb, None
                            (y, ys), j0 = fused, 1
                    if pend is not None:
                        x, pend = materialise(pend), None
                        y = x
                    for j in range(j0, len(names)):
                        nm = names[j]
                        cname = f"{pre}.{nm}"
                        fused = None
                        if halo_fusable(cname) and sp[cname].out_hw(h_, w_) == (h_, w_):
                            fused = conv_stats(cname, y, N, h_, w_, in_stats=ys)
                        if fused is not None:
                            yr, s = fused
                        else:
                            if ys is not None:
                                y = norm_act(f"{pre}.{names[j - 1]}", y, ys, relu=2)
                            yr, h_, w_ = conv_raw(cname, y, N, h_, w_)
                            s = stats(cname, yr, N, h_ * w_, yr.shape[-1])
                        if j + 1 < len(names):
                            y, ys = yr, s
                        else:
                            last, last_s = yr, s
                    if has_ds:
                        dr, _, _ = conv_raw(f"{pre}.downsample", x, N, H, W)
                        ds = stats(f"{pre}.downsample", dr, N, h_ * w_, dr.shape[-1])
                        pend = dict(name=f"{pre}.out", raw=last, s=last_s, res=dr, rs=ds)
                    else:
                        pend = dict(name=f"{pre}.out", raw=last, s=last_s, res=x, rs=None)
                    x = None
                    if not self.halo_norm:
                        x, pend = materialise(pend), None
                    H, W = h_, w_
                else:
                    res = x
                    if has_ds:
                        res, _, _ = conv_raw(f"{pre}.downsample", x, N, H, W)
                    y = x
                    h_, w_ = H, W
                    for j, nm in enumerate(names):
                        if j + 1 < len(names):
                            y, h_, w_ = conv_raw(f"{pre}.{nm}", y, N, h_, w_, act=ACT_RELU)
                        else:
                            y, h_, w_ = conv_raw(f"{pre}.{nm}", y, N, h_, w_, act=ACT_RELU, res=res, res_post=1)
                    x, H, W = y, h_, w_
        if pend is not None:
            x = materialise(pend)
        return x, H, W

    # lanes pay off once the per-iteration kernels fill the chip: measured on
    # MI355X (raft_large, 440x1024, 32 iters) the lane schedule is 17-21 % slower
    # at batch 1, equal at batch 2 and 2 % faster at batch 4 than one in-order
    # lane.  In final-only mode the loop has no mask head to overlap, only the
    # flow-feature convs: one lane measured 13.1 vs 12.7-24.9 ms (lanes,
    # schedule-dependent run to run) at batch 4.  Without a mask predictor
    # (raft_small) one lane measured 562 vs 528 pairs/s at batch 4.
    AUTO_STREAMS_MIN_BATCH = 4

    def _init_cp(self, cp_group) -> None:
        self.cp = cp_group is not None and cp_group is not False
        self.cp_group = None if cp_group is True else cp_group
        self.cp_rank, self.cp_world = 0, 1
        if self.cp:
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized():
                self.cp_rank = dist.get_rank(self.cp_group)
                self.cp_world = dist.get_world_size(self.cp_group)

    def _agree(self, v: int) -> int:
        """Context-parallel ranks build the same plan, so every tuning decision is taken
        from rank 0: ranks timing the candidates themselves (on a shared GPU, or on GPUs
        of different clocks) could pick different tile configs, i.e. flows that differ in
        bf16 rounding between ranks."""
        if not self.cp or self.cp_world == 1:
            return v
        import torch.distributed as dist

        dev = self.device if dist.get_backend(self.cp_group) == "nccl" else torch.device("cpu")
        t = torch.tensor([int(v)], dtype=torch.int64, device=dev)
        src = dist.get_global_rank(self.cp_group, 0) if self.cp_group is not None else 0
        dist.broadcast(t, src=src, group=self.cp_group)
        return int(t.item())

    def _cp_slabs(self, h: int):
        from ..parallel.cp import row_slabs

        return row_slabs(h, self.cp_world)

    def _gather_corr(self, st: _PlanState) -> None:
        """All-gather every rank's looked-up correlation features ``local``
        (B, nq, C) into the full-map ``corr`` (B*h*w, C) (stream-ordered with
        the plan: the eager plan forks from / joins to the current stream)."""
        cp = st.cp
        local, corr, slabs, w = cp["local"], cp["corr"], cp["slabs"], cp["w"]
        B = local.shape[0]
        full = corr.view(B, -1, corr.shape[-1])
        if self.cp_world == 1:
            full[:, : local.shape[1]].copy_(local)
            return
        import torch.distributed as dist

        parts = cp.get("parts")
        if parts is None:
            parts = cp["parts"] = [torch.empty_like(local) for _ in slabs]
        dist.all_gather(parts, local, group=self.cp_group)
        for (r0, r1), part in zip(slabs, parts):
            full[:, r0 * w:r1 * w].copy_(part[:, : (r1 - r0) * w])

    def _forward_cp(self, st: _PlanState, n_iters: int) -> None:
        plan = st.plan
        plan.run_segment(0, 0)
        for it in range(n_iters):
            plan.run_segment(1, it)
            self._gather_corr(st)
            plan.run_segment(3, it)
        plan.run_segment(2, n_iters)

    def _lanes_ok(self, all_iters: bool) -> bool:
        """The lane schedule needs a mask head to overlap (every iteration
        upsampled) and the FlowHead taps epilogue (a 256-channel conv1)."""
        return (all_iters and self.has_mask and self._taps_epi_w is not None and self._convex_w is not None
                and self._specs["fh1.flow"].cout == 256)

    def _halo_geom(self):
        """(hd, [(mode, axis) per ConvGRU stage]) when the halo-tiled fused ConvGRU
        (gru_halo.hip) serves this update block, else None: raft_large's 1x5 + 5x1 stages
        (hidden 128, [h | motion | flow] = 256 loop channels) or raft_small's single 3x3
        GRU (hidden 96, 192 loop channels); bf16 bias map (``gate_dtype``)."""
        rb = self.model.update_block.recurrent_block
        ks = [tuple(k) for k in rb.kernel_size]
        if self.gate_dtype != torch.bfloat16 or self.gate_cs < 3 * self.hidden:
            return None
        if self.hidden == 128 and self.hx_cs == 256 and ks == [(1, 5), (5, 1)]:
            return 128, [(0, 0), (0, 1)]
        if self.hidden == 96 and self.hx_cs == 192 and ks == [(3, 3)]:
            return 96, [(1, 0)]
        return None

    def _gru_path(self, B: int, h: int, w: int) -> str:
        """ConvGRU lowering of a plan: "halo" (gru_halo.hip: one launch per stage, any map
        size and batch), "fused" (gru_fused.hip: whole-row tiles, raft_large at >= 3/4 of
        the CUs' worth of rows) or "unfused" (two implicit-GEMM launches per stage).
        The class attribute ``GRU = "halo" | "fused" | "unfused"`` forces one (where it applies)."""
        env = self.GRU
        assert env in ("auto", "halo", "fused", "unfused"), env
        if env == "unfused":
            return "unfused"
        # auto: the whole-row kernel where it fills the GPU (its own >= 3/4-of-the-CUs rule:
        # raft_large at batch >= 4 on Sintel frames, measured 339 vs 317-334 pairs/s for the
        # halo kernel in the lane schedule, profiles/r4_gru_lowering_ab.txt), the halo kernel
        # everywhere else (batch 1: 215 vs 191 FPS; raft_small; any map size)
        if env in ("auto", "fused") and self._gru_fused_ok(B, h, w):
            return "fused"
        if env in ("auto", "halo") and self._halo_geom() is not None:
            return "halo"
        return "unfused"

    def _halo_tile(self, gi: int, mode: int, axis: int, B: int, h: int, w: int, ops_args) -> Tuple[int, int, int, int]:
        """Tile of one gru_halo stage: the persisted decision (tuned DB key "gru_halo") or
        the fastest candidate (ops/native.py:gru_halo_candidates) timed on the plan's own
        buffers (the prologue re-initialises everything the trial launches write)."""
        cands = nat.gru_halo_candidates(self.hidden, mode, axis, B, h, w)
        enc = {c[0] * 1000000 + c[1] * 1000 + c[2] * 10 + c[3]: c for c in cands}
        key = ("gru_halo", self.hidden, mode, axis, B, h, w)
        if not self.autotune or len(cands) == 1 or self.device.type != "cuda":
            return cands[0]
        code = _TUNE_CACHE.get(key + (str(self.device),))
        if code is None:
            code = tunedb.lookup(self.arch, key, set(enc))
        if code is None:
            t, base = ops_args
            best = None
            for c, tile in enc.items():
                nat.ops().gru_halo(t, base + list(tile))
                s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s_.record()
                for _ in range(5):
                    nat.ops().gru_halo(t, base + list(tile))
                e_.record()
                e_.synchronize()
                el = s_.elapsed_time(e_)
                if best is None or el < best[0]:
                    best = (el, c)
            code = best[1]
            tunedb.record(self.arch, key, code)
        code = self._agree(code)
        _TUNE_CACHE[key + (str(self.device),)] = code
        self.chosen_cfgs[f"gru{gi}.halo"] = code
        return enc[code]

    def _gru_fused_ok(self, B: int, h: int, w: int) -> bool:
        """The fused ConvGRU kernel (gru_fused.hip) serves raft_large's update block:
        hidden 128, [h | motion | flow] = 256 loop channels, a 1x5 then a 5x1 stage,
        and tiles (image rows / column pairs) that fit 128 pixels.  It launches one
        workgroup per tile, so it is used when both stages have >= 3/4 as many tiles
        as the GPU has CUs: measured on MI355X at 440x1024, batch 4 (220 / 256 tiles)
        333-335 vs 320 pairs/s; batch 1 (55 / 64 tiles) 139 vs 158 FPS for the
        two-launch implicit-GEMM path (profiles/r3_gru_fused_ab.txt).
        ``GRU = "fused"`` forces it where it fits."""
        env = "1" if self.GRU == "fused" else "auto"
        rb = self.model.update_block.recurrent_block
        ks = [tuple(k) for k in rb.kernel_size]
        if (self.hidden != 128 or self.hx_cs != 256 or self.gate_cs < 384 or ks != [(1, 5), (5, 1)]
                or self.gate_dtype != torch.bfloat16):
            return False
        tiles = min(nat.gru_fused_tiles(B, h, w, 0), nat.gru_fused_tiles(B, h, w, 1))
        return tiles > 0 and (env == "1" or tiles >= 3 * nat.NUM_CUS // 4)

    def _gru_me_ok(self, B: int, h: int, w: int) -> bool:
        """With the "fused" ConvGRU lowering: whether the motion encoder's output conv runs
        inside the first stage's kernel (gru_fused.hip, op ``gru_fused_me``) instead of as a
        launch of its own.  The row workgroup then does the whole 3x3 conv of its row, so it
        needs a 3x3 / pad-1 conv from 256 to <= 128 channels in front of a 1x5 stage, and it
        pays where the rows fill the GPU (``GRU_ME = "auto"``: the >= 3/4-of-the-CUs rule of
        _gru_fused_ok; with fewer rows the conv's own 64-pixel tiles spread over more CUs).
        ``"on"`` forces it where it fits, ``"off"`` keeps the two launches."""
        assert self.GRU_ME in ("auto", "on", "off"), self.GRU_ME
        if self.GRU_ME == "off" or self.cp:
            return False
        sp = self._specs["me.conv"]
        ks = tuple(self.model.update_block.recurrent_block.kernel_size[0])
        if (not (sp.halo_ks == 3 and sp.cin8 == 256 and sp.cout <= 128 and self.mot_off == 128 and self.hx_cs == 256)
                or ks != (1, 5) or not 1 <= w <= 128):
            return False
        return self.GRU_ME == "on" or nat.gru_fused_tiles(B, h, w, 0) >= 3 * nat.NUM_CUS // 4

    def _flow_fused_ok(self, B: int, h: int, w: int, lanes_on: bool) -> bool:
        """On the lane schedule: whether the motion encoder's flow branch runs as one launch
        (flowfeat.hip, op ``flow_features_fused``) instead of the 7x7 conv and the halo 3x3 conv
        behind it.  The kernel is written for 7x7 / pad 3, 2 -> 128, then 3x3 / pad 1, 128 -> 64,
        on the compact 2-channel flow.  ``FLOW_FUSED = "auto"``: where its 8 x 16 tiles fill the
        GPU (the >= 3/4-of-the-CUs rule of _gru_me_ok); ``"on"`` forces it wherever it fits (the
        tests, at small shapes); ``"off"`` keeps the two launches.  One-lane, final-only and
        context-parallel plans, raft_small, the fp32 / mixed engines and training never take it."""
        assert self.FLOW_FUSED in ("auto", "on", "off"), self.FLOW_FUSED
        if self.FLOW_FUSED == "off" or not lanes_on or self.cp or self.precision != "bf16" or self._cf1_w is None:
            return False
        me = self.model.update_block.motion_encoder
        c1, sp = me.convflow1.layers_0, self._specs["me.convflow2"]
        if (tuple(c1.kernel.shape) != (7, 7, 2, 128) or tuple(c1.padding) != (3, 3)
                or not (sp.halo_ks == 3 and sp.cin8 == 128 and sp.cout == 64 and sp.wh is not None)):
            return False
        return self.FLOW_FUSED == "on" or nat.flow_fused_tiles(B, h, w) >= 3 * nat.NUM_CUS // 4

    def _parts(self, B: int) -> int:
        """Independent part-forwards of a batch-``B`` plan: ``split`` where it divides the batch."""
        return self.split if (self.split > 1 and B % self.split == 0 and not self.cp) else 1

    def uses_lanes(self, B: int, all_iters: bool = True, *, parts: Optional[int] = None) -> bool:
        """Whether the plan for batch ``B`` (in ``parts`` parts; default: :meth:`_parts`) runs the
        model's branches on several lanes (``streams`` / its "auto" rule).  Graph-pipelined steps
        (:meth:`pipelined`) measured faster only on one-lane plans: batch 1
        145 -> 157 pairs/s, raft_small batch 4 559 -> 602, final-only 326 -> 346;
        with lanes (raft_large batch 4) 319 -> 289 (profiles/r2_pipelined_graph_ab.txt)."""
        if self.cp or not self._lanes_ok(all_iters):
            return False
        if self.streams_mode != "auto":
            return bool(self.streams_mode)
        return B // (self._parts(B) if parts is None else parts) >= self.AUTO_STREAMS_MIN_BATCH

    def _build(self, B: int, H: int, W: int, n_iters: int, all_iters: bool = True,
               src: Optional[Tuple[int, int, int, int]] = None, warm: bool = False, *,
               parts: Optional[int] = None, slot: bool = False) -> _PlanState:
        """The cold / warm plan (lowering.build) in ``parts`` parts (default :meth:`_parts`); ``slot``: a pipelined slot's."""
        return lowering.build(self, B, H, W, n_iters, all_iters, src, warm, parts=parts, slot=slot)

    def _build_bidir(self, B: int, H: int, W: int, n_iters: int, all_iters: bool,
                     src: Optional[Tuple[int, int, int, int]], warp: bool = False, *, slot: bool = False,
                     interp: int = 0) -> _PlanState:
        """Record the plan of ``forward(bidirectional=True)`` (runtime/lowering.py:build_bidir)."""
        return lowering.build_bidir(self, B, H, W, n_iters, all_iters, src, warp, slot=slot, interp=interp)

    # --------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, image1: torch.Tensor, image2: torch.Tensor, num_flow_updates: int = 12,
                return_all_iters: bool = True, flow_init=None, return_flow_low: bool = False,
                bidirectional: bool = False, fb_alpha: float = 0.01, fb_beta: float = 0.5, warp: bool = False,
                interpolate=None, interp_min_cover: float = 1.0 / 64):
        """All ``num_flow_updates`` upsampled flows (N, B, H, W, 2), as the reference
        returns; ``return_all_iters=False`` returns only the final one, (1, B, H, W, 2).

        ``bidirectional=True`` returns :class:`BidirectionalFlow` ``(flows_fw, flows_bw, occ_fw,
        occ_bw)``: the flows 1 -> 2 and 2 -> 1, each (N or 1, B, H, W, 2), and the (B, H, W) bool
        occlusion masks of the forward-backward check of the two final flows
        (``models/reference.py:fb_consistency`` with ``fb_alpha``, ``fb_beta``), from one replay
        of a plan of its own (plan key + "bidir", :meth:`_build_bidir`).  The thresholds live in
        a device tensor, so changing them builds no new plan.  Not with ``flow_init`` /
        ``return_flow_low``, :meth:`pipelined`, context parallelism or the fp32 / mixed engines
        (``NotImplementedError``); such a call forgets the engine's "previous" flow.

        ``bidirectional=True, warp=True`` (uint8 frames; anything else is a ``ValueError``)
        returns :class:`BidirectionalWarp`: the same four fields, then ``warped_fw`` / ``warped_bw``
        (B, H0, W0, 3) uint8 -- frame 2 sampled with the flow 1 -> 2 and frame 1 with the flow
        2 -> 1, occluded and outside pixels taken from the frame itself -- and ``photo`` (2, B, 2)
        int64, the masked photometric sums (``models/reference.py:warp_frames``), from one more
        kernel (+ the clear of the sums) at the end of a plan of its own (plan key + "bidir",
        "warp"); every other plan is recorded as before.

        ``bidirectional=True, interpolate=t`` (uint8 frames; ``t`` a float or a sequence of 1 to 8
        floats strictly between 0 and 1; anything else, ``warp=True`` with it included, is a
        ``ValueError``) returns :class:`BidirectionalInterp`: the same four fields, then ``frames``
        (K, B, H0, W0, 3) uint8, the frames at the K times between frame 1 and frame 2 by forward
        splatting along both flows, and ``holes`` (K, B, H0, W0) bool, the pixels nothing reached
        (``models/reference.py:interpolate_frames`` with ``min_cover = interp_min_cover``) -- a clear
        and two kernels per time at the end of a plan of its own (plan key + "bidir", "interp", K).
        The times live in a device tensor, so other times of the same count build no new plan.

        Warm start (video): ``flow_init`` -- a (B, h, w, 2) fp32 tensor in 1/8-resolution
        pixels, channel 0 = x (h, w = the plan's size / 8: the *padded* size for uint8 frames)
        -- starts the refinement at ``coords1 = coords0 + flow_init``.  Such a call runs a plan
        of its own (plan key + "warm") whose seed kernel replaces ``init_coords``;
        ``flow_init=None`` runs today's cold plan, untouched.  ``flow_init="previous"``
        projects the final 1/8-resolution flow of the most recent :meth:`forward` of the same
        (B, H, W) -- any iteration count or output mode -- forward in time
        (``ops/native.py:forward_project``, two small launches on the current stream before
        the replay; no host synchronisation, no host copy) and starts from that; ``ValueError``
        when there is no such call or the weights were repacked since.
        ``return_flow_low=True`` returns ``(flows, flow_low)``: a fresh (B, h, w, 2) fp32 copy
        of the final ``coords1 - coords0``.

        Not with :meth:`pipelined` (a slot's prologue, where the seed runs, is replayed
        concurrently with the previous pair's loop, whose final flow "previous" would need),
        not under context parallelism (its host-driven loop is not lowered for a seed) and
        not in training."""
        if self._stale():
            self._pack()
            self._last = None
        if self.cp and flow_init is not None:
            raise NotImplementedError("forward(flow_init=...): not with context parallelism (cp_group)")
        if warp and not bidirectional:
            raise ValueError("forward(warp=True) requires bidirectional=True (the warp is the last op of the "
                             "bidirectional plan)")
        if interpolate is not None and not bidirectional:
            raise ValueError("forward(interpolate=t) requires bidirectional=True (the splat uses both flows and "
                             "their occlusion masks)")
        if interpolate is not None and warp:
            raise ValueError("forward(bidirectional=True): interpolate and warp=True exclude each other (one consumer "
                             "per plan)")
        if bidirectional and self.corr_mode == "on_demand":
            raise NotImplementedError("forward(bidirectional=True): not with corr='on_demand' (the bidirectional "
                                      "plan is lowered for the all-pairs volume only)")
        if bidirectional:
            return self._forward_bidir(image1, image2, num_flow_updates, return_all_iters, flow_init,
                                       return_flow_low, fb_alpha, fb_beta, warp, interpolate, interp_min_cover)
        if image1.dtype == torch.uint8 and not self._native_u8:
            a, b, src = self._host_u8(image1, image2)
            res = self.forward(a, b, num_flow_updates, return_all_iters, flow_init, return_flow_low)
            H0, W0, pt, pl = src
            if return_flow_low:
                return res[0][:, :, pt:pt + H0, pl:pl + W0], res[1]
            return res[:, :, pt:pt + H0, pl:pl + W0]
        key = self._key(image1, image2, num_flow_updates, return_all_iters)
        B, h, w = key[0], key[1] // 8, key[2] // 8
        prev = None
        if isinstance(flow_init, str):
            if flow_init != "previous":
                raise ValueError(f"flow_init must be a (B, h, w, 2) tensor, None or 'previous', got {flow_init!r}")
            prev = self._last
            if prev is None or prev[0] != key[:3]:
                raise ValueError(f"flow_init='previous': no previous forward() of shape (B, H, W) = {key[:3]} "
                                 "on this engine since its weights were last packed")
        elif flow_init is not None:
            if tuple(flow_init.shape) != (B, h, w, 2):
                raise ValueError(f"flow_init must have shape {(B, h, w, 2)} (B, H/8, W/8, 2; for uint8 frames "
                                 f"H, W are the padded size), got {tuple(flow_init.shape)}")
        if flow_init is not None:
            key = key + ("warm",)
        st = self._plan_state(key, lambda: self._build_key(key))
        st.inp1.copy_(image1)
        st.inp2.copy_(image2)
        if prev is not None:
            # before the replay overwrites the previous call's flow buffers (stream order)
            if st.keys is None:
                st.keys = nat.project_keys(B, h, w, self.device)
            nat.forward_project(self._flow_low(prev[2], prev[1], h, w, copy=False), self.WARM_FILL_RADIUS,
                                keys=st.keys, out=st.flow_init)
        elif flow_init is not None:
            st.flow_init.copy_(flow_init)
        self._pre_launch(st)
        fresh = self.copy_output and st.slot_ok
        out = torch.empty_like(st.out) if fresh else st.out
        self._point_slot(st, out)
        self._gate(num_flow_updates)   # after the host-side preparation: only the launch waits
        if st.cp is not None:
            self._forward_cp(st, num_flow_updates)
        elif len(st.plans) == 1 or not self.use_graph:
            for plan in st.plans:
                self._launch(plan, num_flow_updates)
        else:
            # the parts' captures copied into ONE graph (Plan.merge_*): their chains
            # interleave with no cross-stream edge (separate graphs serialise)
            p0 = st.plans[0]
            if p0.merged_iters() != num_flow_updates:
                p0.merge_reset()
                for plan in st.plans:
                    p0.merge_add(plan, num_flow_updates)
                p0.merge_finish(num_flow_updates)
            p0.replay_pipelined()
        self._mark()
        self._last = (key[:3], num_flow_updates, st.flow_out)
        res = self._crop(st, out) if fresh else self._crop(st, st.out.clone() if self.copy_output else st.out)
        if return_flow_low:
            return res, self._flow_low(st.flow_out, num_flow_updates, h, w)
        return res

    def _forward_bidir(self, image1, image2, n_iters: int, all_iters: bool, flow_init, return_flow_low: bool,
                       alpha: float, beta: float, warp: bool = False, interpolate=None, min_cover: float = 1.0 / 64):
        """``forward(bidirectional=True)`` (weights already repacked where stale)."""
        if flow_init is not None or return_flow_low:
            raise NotImplementedError("forward(bidirectional=True): not with flow_init / return_flow_low (the warm "
                                      "seed and the low-resolution output are lowered for one direction)")
        if self.cp:
            raise NotImplementedError("forward(bidirectional=True): not with context parallelism (its host-driven "
                                      "loop is not lowered for the swapped correlation halves)")
        if self.precision != "bf16":
            raise NotImplementedError(f"forward(bidirectional=True): not with precision={self.precision!r} (the "
                                      "bidirectional plan is lowered for the bf16 engine only)")
        if warp and not (image1.dtype == torch.uint8 and image2.dtype == torch.uint8):
            raise ValueError("forward(bidirectional=True, warp=True) requires uint8 frames (the warp samples the "
                             f"frames as uploaded), got {image1.dtype}")
        rows = None
        if interpolate is not None:
            if not (image1.dtype == torch.uint8 and image2.dtype == torch.uint8):
                raise ValueError("forward(bidirectional=True, interpolate=t) requires uint8 frames (the splat reads "
                                 f"the frames as uploaded), got {image1.dtype}")
            rows = tuple(interp_times(interpolate, min_cover, INTERP_MAX_TIMES)[0])
        # a later flow_init="previous" must not seed from this call's half-batch
        self._last = None
        suffix = ("bidir", "warp") if warp else ("bidir", "interp", len(rows)) if rows else ("bidir",)
        key = self._key(image1, image2, n_iters, all_iters) + suffix
        st = self._plan_state(key, lambda: self._build_key(key))
        st.inp1.copy_(image1)
        st.inp2.copy_(image2)
        if st.thr_vals != (float(alpha), float(beta)):   # stream-ordered, before the replay
            st.thr.copy_(torch.tensor([alpha, beta], dtype=F32))
            st.thr_vals = (float(alpha), float(beta))
        if rows and st.par_vals != rows:   # likewise: another time rewrites two ints, and builds nothing
            st.par.copy_(torch.tensor(rows, dtype=torch.int32))
            st.par_vals = rows
        self._pre_launch(st)
        fresh = self.copy_output and st.slot_ok
        out = torch.empty_like(st.out) if fresh else st.out
        self._point_slot(st, out)
        self._gate(n_iters)
        self._launch(st.plan, n_iters)
        self._mark()
        res = self._crop(st, out) if fresh else self._crop(st, st.out.clone() if self.copy_output else st.out)
        occ = st.occ if st.src is None else st.occ[:, :, st.src[2]:st.src[2] + st.src[0], st.src[3]:st.src[3] + st.src[1]]
        occ = occ.bool()   # a fresh tensor either way (the plan's buffer is uint8)
        B = key[0]
        if warp:   # fresh tensors, copied in stream order
            warped, photo = st.warped.clone(), st.photo.clone()
            return BidirectionalWarp(res[:, :B], res[:, B:], occ[0], occ[1], warped[0], warped[1], photo)
        if rows:   # likewise
            return BidirectionalInterp(res[:, :B], res[:, B:], occ[0], occ[1], st.interp.clone(), st.holes.bool())
        return BidirectionalFlow(res[:, :B], res[:, B:], occ[0], occ[1])

    @staticmethod
    def _flow_low(flow_out, n_iters: int, h: int, w: int, copy: bool = True) -> torch.Tensor:
        """The final 1/8-resolution flow (B, h, w, 2) of a plan that ran ``n_iters`` iterations,
        assembled across its batch parts.  The update of launch index j writes the odd-iteration
        buffer when j is odd (MASK_PARITY) and the last update runs at j = n_iters, so that
        buffer holds the final flow iff ``n_iters`` is odd.  ``copy=False`` may return a view of
        the plan's buffer (a one-part plan)."""
        bufs = [(fb if (fb is not None and n_iters & 1) else f).view(nb, h, w, 2) for _, nb, f, fb in flow_out]
        if len(bufs) == 1:
            return bufs[0].clone() if copy else bufs[0]
        return torch.cat(bufs, dim=0)

    def _pre_launch(self, st: _PlanState) -> None:
        """Work a forward runs before replaying its plan (RaftEngineMixed: the fp32 feature encoder)."""

    GATE_MIN_ITERS = 20

    def _gate(self, n_iters: int) -> None:
        """Wait (host) for the previous forward / pipelined call (see ``host_gate``)."""
        if self.host_gate and self._done_ev is not None and n_iters >= self.GATE_MIN_ITERS:
            self._done_ev.synchronize()

    def _mark(self) -> None:
        if self.host_gate and self.device.type == "cuda":
            if self._done_ev is None:
                self._done_ev = torch.cuda.Event()
            self._done_ev.record()

    @staticmethod
    def _point_slot(st: _PlanState, out: torch.Tensor) -> None:
        """Aim the plan's output writers at ``out`` (stream-ordered: the
        update is a tiny copy on the current stream, before the launch)."""
        if st.slot_ptr != out.data_ptr():
            st.out_slot.fill_(out.data_ptr())
            st.slot_ptr = out.data_ptr()

    # ------------------------------------- software-pipelined graphs (throughput)
    def _slot_state(self, key, slot: int) -> _PlanState:
        """The plan of one :meth:`pipelined` slot: one part, recorded as a slot's plan."""
        return self._plan_state(key + ("pslot", slot), lambda: self._build_key(key, parts=1, slot=True))

    @torch.no_grad()
    def pipelined(self, image1: torch.Tensor, image2: torch.Tensor, num_flow_updates: int = 12,
                  return_all_iters: bool = True, flow_init=None, bidirectional: bool = False) -> Optional[torch.Tensor]:
        """Software-pipelined forward for throughput (batch inference, serving):
        returns the flows of the PREVIOUS call's images (``None`` on the first
        call); :meth:`flush` returns the last pending batch's flows.

        Each call replays ONE hipGraph (``Plan.capture_pipelined``) whose
        independent branches are the previous batch's refinement loop +
        epilogue and this batch's prologue (encoders + correlation pyramid).
        The loop kernels are latency-bound (one workgroup per CU on ~220 of
        256 CUs at batch 4), the encoder convs throughput-bound, so the
        prologue mostly fills SIMD slots the loop leaves idle.  Two plan slots
        (own buffers, own graphs) alternate; every call does one prologue and
        one loop, i.e. one forward's work.  (:meth:`submit` replays the two
        phases as separate graphs on two streams, which serialise on this
        ROCm.)  The result of each batch is bitwise equal to :meth:`forward`
        (tests/test_engine_gpu.py).

        No warm start here (``flow_init`` raises ``NotImplementedError``): a slot's prologue,
        where the seed would run, is replayed concurrently with the previous pair's loop, so
        that pair's final flow -- what "previous" starts from -- does not exist yet."""
        if flow_init is not None:
            raise NotImplementedError("pipelined(flow_init=...): warm start needs the previous pair's final flow, "
                                      "which a pipelined slot's prologue runs concurrently with; use forward()")
        if bidirectional:
            raise NotImplementedError("pipelined(bidirectional=True): the bidirectional plan (its second correlation "
                                      "launch and epilogue check) is not lowered for pipelined slots; use forward()")
        if self.corr_mode == "on_demand":
            raise NotImplementedError("pipelined(): not with corr='on_demand' (a slot's prologue is not lowered for "
                                      "the pooled target features); use forward()")
        if self._stale():
            self._last = None
            if self._pp is not None and self._pp["pending"] is not None:
                # the pending batch's encoders + pyramid ran with the old weights; its loop
                # would run with the new ones (a result matching neither forward)
                raise RuntimeError("pipelined(): the weights changed while a batch is pending; flush() it first")
            self._pack()
        assert self.use_graph, "pipelined() replays captured graphs (use_graph=True)"
        if self.fe_external:
            raise NotImplementedError("pipelined(): not with precision='mixed' (its fp32 encoder runs before the plan)")
        assert not self.cp, "pipelined(): not with context parallelism (a host-driven loop)"
        if image1.dtype == torch.uint8 and not self._native_u8:
            a, b, src = self._host_u8(image1, image2)
            r = self.pipelined(a, b, num_flow_updates, return_all_iters)
            return None if r is None else r[:, :, src[2]:src[2] + src[0], src[3]:src[3] + src[1]]
        n = num_flow_updates
        key = self._key(image1, image2, n, return_all_iters)
        pp = self._pp
        if pp is not None and pp["key"] != key and pp["pending"] is not None:
            raise RuntimeError("pipelined(): flush() the pending batch before changing the input shape / iterations")
        if pp is None or pp["key"] != key:
            pp = self._pp = dict(key=key, n=0, pending=None)
        slot = pp["n"] & 1
        st = self._slot_state(key, slot)
        st.inp1.copy_(image1)
        st.inp2.copy_(image2)
        prev = pp["pending"]
        result = None
        if prev is None:
            if st.plan.captured_part_iters(0) != n:
                st.plan.capture_part(0, n)
            self._gate(n)
            st.plan.replay_part(0)
        else:
            pst = self._slot_state(key, prev)
            fresh = self.copy_output and pst.slot_ok
            out = torch.empty_like(pst.out) if fresh else pst.out
            self._point_slot(pst, out)
            if pst.plan.pipelined_iters(st.plan) != n:
                pst.plan.capture_pipelined(st.plan, n)
            self._gate(n)
            pst.plan.replay_pipelined()
            result = self._crop(pst, out if fresh else (pst.out.clone() if self.copy_output else pst.out))
        self._mark()
        pp["pending"] = slot
        pp["n"] += 1
        return result

    @torch.no_grad()
    def flush(self) -> Optional[torch.Tensor]:
        """Finish the batch :meth:`pipelined` left pending (its refinement loop
        + epilogue as one graph); returns its flows, or ``None`` if none."""
        pp = self._pp
        if pp is None or pp["pending"] is None:
            return None
        key = pp["key"]
        st = self._slot_state(key, pp["pending"])
        n = key[3]
        fresh = self.copy_output and st.slot_ok
        out = torch.empty_like(st.out) if fresh else st.out
        self._point_slot(st, out)
        if st.plan.captured_part_iters(1) != n:
            st.plan.capture_part(1, n)
        st.plan.replay_part(1)
        pp["pending"] = None
        pp["n"] = 0
        return self._crop(st, out if fresh else (st.out.clone() if self.copy_output else st.out))

    def _launch(self, plan, n_iters: int) -> None:
        if self.use_graph:
            if plan.captured_iters() != n_iters:
                plan.capture(n_iters)
            plan.replay()
        else:
            plan.run(n_iters)

    def op_names(self, B: int, H: int, W: int, n_iters: int, return_all_iters: bool = True):
        st = self._plan_state((B, H, W, n_iters, return_all_iters),
                              lambda: self._build(B, H, W, n_iters, return_all_iters))
        return [st.plan.op_names(s) for s in range(3)]
