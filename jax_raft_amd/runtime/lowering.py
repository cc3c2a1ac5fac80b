"""Plan recording of the bf16 inference engine (``RaftEngine._build`` / ``_build_bidir``), in three layers:

* **choices** -- :func:`choose` computes a frozen :class:`PartChoices`, every lowering decision of
  one batch part and the loop ``schedule`` it runs, from the engine and the part's sizes and mode;
  it allocates nothing, touches no plan and leaves the engine as it was.  A plan keeps its parts'
  choices in ``st.choices``.  The measurements behind each decision are cited next to it.
* **emitters** -- :class:`PartRecorder` holds the engine, the plan state, one native plan, the
  choices and the part's buffers; each prologue method and op emitter appends one step's ops.
* **schedules** -- one ``schedule_*`` method per value of ``PartChoices.schedule``: the op order of
  one refinement iteration (``model.py:495-510``) plus the epilogue, read top to bottom.

The number of batch parts and ``slot`` (a :meth:`pipelined` slot's plan) are arguments of a build,
which writes nothing to the engine but the tuning caches and, once done, what :func:`_finish` sets."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ..ops import native as nat
from ..ops.native import ACT_RELU, ACT_SPLIT_TANH_RELU, EPI_GRU_A, EPI_GRU_B, EPI_TAPS, round_up
from . import engine as _engine

BF16, F32 = torch.bfloat16, torch.float32

# events of one part: prep done, context lane done, and the lane schedule's three cross-lane
# edges per iteration (each costs ~6-12 us in a captured graph on this ROCm); image 2's features
E_PREP, E_CTX, E_FLOW, E_FH, E_MASK, E_FE2 = range(6)


@dataclass(frozen=True)
class PartChoices:
    """Every lowering decision of one batch part (see the functions below for the why)."""
    schedule: str                 # "cp" | "lanes" | "one_lane" | "final_merged" | "final"
    all_iters: bool               # every iteration upsampled (else the final flow alone, once, in the epilogue)
    warm: bool                    # the loop starts from the plan's flow_init (init_flow for init_coords)
    bidir: bool                   # both directions in one loop of batch 2 x image pairs
    lanes: Tuple[int, int, int]   # loop lanes (main, side, side2)
    lanes_on: bool                # main != side: the mask lane exists
    pro_on: bool                  # the prologue's branches may run on lanes of their own
    pro_lanes: Tuple[int, int, int]   # prologue lanes: feature encoder + pyramid, context, image 2's features
    fe_split: bool                # the feature encoder per image, image 2's on lane pro_lanes[2]
    s2d: bool                     # 2x2 space-to-depth images, the stems as 4x4 / stride-1 convs
    blocked: int                  # pyramid levels 0 / 1 in the blocked layout (the lookup's flag)
    bl: int                       # ... as the corr op takes it: 2 = the persistent pyramid kernel
    on_demand: bool               # no volume: pooled target features, lookup_od
    split_mask: bool              # the mask predictor's 3x3 conv on its own (else fused into FlowHead conv1)
    s1: str                       # spec of the loop's FlowHead conv1: "fh1" | "fh1.flow"
    taps_epi: bool                # the taps epilogue: the 256 FlowHead features never leave the CU (no ``fm``)
    gru_path: str                 # "halo" | "fused" | "unfused"
    gru_me: bool                  # the motion conv inside the first fused stage's kernel (gru_fused_me)
    halo_pp: bool                 # single halo stage: h ping-pongs between hx and qx
    qx_x: bool                    # qx's [motion | flow] part is written: the unfused GRU-B and the ping-pong read it
    hm: bool                      # the last stage writes the mask head's own copy of h
    parity: bool                  # parity-buffered hm / flow32 for the mask lane (no E_MASK join)
    # The one place that says where the lane schedule's E_MASK join sits: the index of the ConvGRU
    # stage that waits until the previous iteration's mask head has read h / hm (and flow32), or
    # None (one lane; parity buffers).  "halo" / "fused": before that stage's launch -- the last
    # stage, which writes hm (the first, were there no hm copy); "unfused": stage 0, between its
    # two convs (GRU-B is what replaces h).
    mask_wait: Optional[int]
    merged_up: bool               # one lane: 7x7 flow conv + the previous x8 upsampling as one grid (merged.hip)
    c1_merged: bool               # ... which also runs convcorr1 (1x1, K 324 -> 352)
    flow_fused: bool              # lane schedule: the flow branch's two convs as one launch (flow_features_fused; no ``f1``)


def _prologue_choices(eng, Bi: int, h: int, w: int, lanes, slot: bool) -> dict:
    main, side, _ = lanes
    lanes_on = main != side
    # the prologue's branches (context encoder, feature encoder per image) run on their own
    # lanes even when the loop runs on one, up to Sintel-size batch 4 worth of pixels.  At
    # batch 1 ("auto") the feature encoder runs as ONE batch-2 chain next to the context
    # encoder's lane (round 6, profiles/r6_prolanes_ab.txt, r6_ce_lane_b1_ab.txt): per-image
    # lanes of its ~70 short kernels only added dispatch cost (the replayed branches ran one
    # after another, r6_graph_branches.txt); raft_small sync 297 -> 330-344 pairs/s, its
    # 12-iteration stream 662-758 -> 782-805, raft_large sync 216 -> 218-223.  (1088x1920
    # frames: 67.6 -> 63.7 with lanes, round 4, so off there.)
    # PRO_LANES = "off": never, "on": always (per-image feature-encoder lanes at batch 1 too).
    pl = eng.PRO_LANES
    assert pl in ("auto", "on", "off"), pl
    pro_on = pl == "on" or (pl == "auto" and Bi * h * w <= 4 * 55 * 128)
    pro_lanes = tuple(lanes) if lanes_on or eng.cp or not pro_on else (main, 1, 2)
    # the per-image feature-encoder split (lane 2) -- never at batch 1 under "auto", also not in
    # a pipelined slot's multi-lane plan, so that its kernels (tile configs of the batch-2
    # chain) and results equal the synchronous forward's bit for bit
    fe_split = pro_lanes[0] != pro_lanes[1] and not (pl == "auto" and Bi == 1)
    # bf16 levels of /16-wide maps: levels 0 / 1 in the blocked layout (one
    # pyramid tile per block: whole-line writes, 2 x 2 blocks per lookup window)
    blocked = int(eng.corr_dtype == BF16 and w % 16 == 0 and (h * w) % 8 == 0 and not eng.cp)
    # blocked 2: the persistent pyramid kernel (corr_pyr.hip) also at batch 1 -- not in a
    # pipelined slot, whose graph runs it next to the previous pair's loop (there the
    # short-lived tiles interleave better: b1 stream 227 vs 200-204 FPS, round 4)
    bl = 2 if (blocked and eng.CORR_PERSIST_B1 and not slot) else blocked
    return dict(lanes=tuple(lanes), lanes_on=lanes_on, pro_on=pro_on, pro_lanes=pro_lanes, fe_split=fe_split,
                # (the plan's H, W = 8h, 8w are even, as the space-to-depth input needs)
                s2d="fe.stem_s2d" in eng._specs and "ce.stem_s2d" in eng._specs,
                blocked=blocked, bl=bl, on_demand=eng.corr_mode == "on_demand")


def _gru_choices(eng, B: int, h: int, w: int, lanes_on: bool) -> dict:
    ngru = len(eng.model.update_block.recurrent_block.kernel_size)
    # ConvGRU lowering: "halo" (gru_halo.hip, one launch per stage at any size / batch),
    # "fused" (gru_fused.hip, whole-row tiles) or "unfused" (EPI_GRU_A / EPI_GRU_B convs)
    gru_path = eng._gru_path(B, h, w)
    if gru_path == "fused" and eng.cp:
        gru_path = "unfused"
    # the halo kernel cannot update h in place (neighbouring tiles read it): raft_large's
    # stage 1 writes h' into qx, stage 2 reads it there and writes hx; raft_small's single
    # stage ping-pongs h between hx (read on even iterations) and qx (odd), and its FlowHead
    # reads the buffer the stage just wrote
    halo_pp = gru_path == "halo" and ngru == 1
    # with the mask lane, the mask head reads h from its own copy `hm` (written by the last
    # stage), so the first stage can replace h in hx while the mask lane still runs
    # raft_small's ping-pong stage with a mask head (an injected MaskPredictor) also writes the copy:
    # its h' alternates between qx and hx, so the mask head (final-only epilogue, context parallel,
    # mask lane) reads hm instead of a buffer that holds h' only on every other iteration
    hm = gru_path != "unfused" and eng.has_mask and (lanes_on or halo_pp)
    # Parity-buffered mask-lane operands (gru_fused + convex head, MASK_PARITY = True): the last
    # GRU stage writes h into hm / hm2 and the update writes the flow into flow32 / flow32b by
    # iteration parity, so iteration i+1 never overwrites what the lane still reads for iteration
    # i; the lane's next read of a buffer is ordered by the E_FLOW join of the iteration after,
    # and the per-iteration E_MASK join (a ~10 us cross-stream graph edge) goes away.  Measured
    # slower at batch 4 (359-365 vs 372 pairs/s, profiles/r4_mask_parity_ab.txt): unjoined, the
    # mask head overlaps the ConvGRU stages (48 -> 54-56 us each) instead of the motion encoder.
    parity = bool(hm and gru_path == "fused" and eng._convex_w is not None and eng.MASK_PARITY)
    mask_wait = None if not lanes_on or parity else ngru - 1 if (gru_path == "halo" or hm) else 0   # (unfused: no hm)
    return dict(gru_path=gru_path, halo_pp=halo_pp, hm=hm, parity=parity, mask_wait=mask_wait,
                gru_me=gru_path == "fused" and eng._gru_me_ok(B, h, w), qx_x=gru_path != "halo" or halo_pp)


def _head_choices(eng, B: int, h: int, w: int, all_iters: bool, lanes_on: bool) -> dict:
    """The flow head / mask head / flow-feature choices, and from them the schedule."""
    sp = eng._specs
    me = eng.model.update_block.motion_encoder
    split_mask = lanes_on or eng.cp   # (mask lane / context parallel)
    # FlowHead conv1 of the loop: alone (lanes / final-only / no mask head) or
    # fused with the mask predictor's 3x3 conv (one lane, every iteration upsampled)
    s1 = "fh1.flow" if eng.has_mask and not (all_iters and not split_mask) else "fh1"
    taps_epi = eng._taps_epi_w is not None and sp[s1].cout == 256
    flow7 = eng._cf1_w is not None and tuple(me.convflow1.layers_0.kernel.shape[:2]) == (7, 7)
    merged_up = bool(flow7 and not eng.cp and (not eng.has_mask or (eng._convex_w is not None and not taps_epi))
                     and eng.MERGED_UP)
    c1_merged = (merged_up and eng.has_mask and len(me.corr_layers) == 2 and eng._cc1_w is not None
                 and eng._cc1_kpad == 352)
    # "final_merged": final-only below batch 4, the one-lane order of the all-iterations loop: the
    # flow update fused into the next lookup, the 7x7 flow conv in the merged grid (its bilinear
    # half writes the single output slot every iteration; the epilogue's upsampling overwrites
    # it), convflow2 grouped with convcorr2.  Batch 1: 239.5 -> 244.6 pairs/s; batch 4
    # loses (414.8 -> 402.7), keeps the "final" order (profiles/r4_host_gate.txt)
    schedule = ("cp" if eng.cp else "lanes" if lanes_on else "one_lane" if all_iters
                else "final_merged" if flow7 and B < eng.AUTO_STREAMS_MIN_BATCH else "final")
    # The mask lane's chain of four launches (7x7 flow conv, convflow2, mask conv, convex head) ended
    # after the main lane wanted to start the last ConvGRU stage (the E_MASK join: 15-21 us of main-
    # lane idle per iteration, profiles/megru_after.txt); the fused flow features take one launch
    # and the f1 round trip out of it: 17.3 -> 9.2 us alone, +1.2-1.5 % at batch 4, and the join no
    # longer waits for the chain (profiles/masklane_fused.txt)
    flow_fused = schedule == "lanes" and eng._flow_fused_ok(B, h, w, lanes_on)
    return dict(split_mask=split_mask, s1=s1, taps_epi=taps_epi, merged_up=merged_up, c1_merged=c1_merged,
                schedule=schedule, flow_fused=flow_fused)


def choose(eng, Bi: int, B: int, h: int, w: int, all_iters: bool, lanes, *, warm: bool = False,
           bidir: bool = False, slot: bool = False) -> PartChoices:
    """The choices of one batch part of ``Bi`` image pairs whose loop runs at batch ``B`` (2 Bi for
    a bidirectional plan, else Bi) on ``h x w`` feature maps, with the loop on ``lanes``: (0, 1, 2)
    where ``eng.uses_lanes``, else (0, 0, 0).  ``slot``: the plan of a :meth:`pipelined` slot.  Pure."""
    assert not (bidir and (warm or eng.cp)), "bidirectional plans: one part, cold, no context parallelism"
    pro = _prologue_choices(eng, Bi, h, w, lanes, slot)
    assert not (pro["on_demand"] and (bidir or eng.cp)), "on-demand plans: one direction, no context parallelism"
    gru, head = _gru_choices(eng, B, h, w, pro["lanes_on"]), _head_choices(eng, B, h, w, all_iters, pro["lanes_on"])
    return PartChoices(all_iters=bool(all_iters), warm=warm, bidir=bidir, **pro, **gru, **head)


class PartRecorder:
    """Records one forward over the images [b0, b0 + Bi) of ``st`` onto ``plan`` as ``c`` says.
    ``c.warm``: ``init_flow`` from the plan's ``flow_init`` slice in place of ``init_coords``;
    everything else is the cold plan's.  ``c.bidir``: both directions in one loop of batch 2 Bi --
    samples [0, Bi) refine the flow 1 -> 2, samples [Bi, 2 Bi) the flow 2 -> 1.  ``prep`` and the
    feature encoder are the cold plan's (``fmap`` already holds both frames' features); the context
    lane runs over all 2 Bi images of ``x0``, and a second ``corr`` launch fills the levels' second half."""

    def __init__(self, eng, st, plan, c: PartChoices, b0: int, Bi: int, H: int, W: int, pt: str):
        self.eng, self.st, self.plan, self.c, self.pt = eng, st, plan, c, pt
        # Bi image pairs: prep, the feature encoder, each correlation launch; the loop batch B:
        # context encoder, pyramid rows, loop body, upsampling
        self.b0, self.Bi, self.B = b0, Bi, 2 * Bi if c.bidir else Bi
        self.H, self.W, self.h, self.w = H, W, H // 8, W // 8
        self.M, self.L = self.B * self.h * self.w, eng.num_levels
        ub = eng.model.update_block
        self.me, self.ngru = ub.motion_encoder, len(ub.recurrent_block.kernel_size)
        self.inp1, self.inp2 = st.inp1[b0:b0 + Bi], st.inp2[b0:b0 + Bi]
        self.out = st.out[:, b0:b0 + self.B]
        self.out_off = (self.out.data_ptr() - st.out.data_ptr()) // 4   # in floats, from the slot's base
        self.stride = st.out.shape[1] * H * W * 2   # one iteration of the full-batch output

    def alloc(self, name, shape, dtype=BF16):
        t = self.st.bufs[self.pt + name] = torch.zeros(shape, dtype=dtype, device=self.eng.device)
        return t

    def record(self):
        """The prologue, the loop's buffers, then the schedule ``c.schedule`` names."""
        for step in (self.state_buffers, self.prep, self.context, self.features, self.correlation, self.loop_buffers,
                     getattr(self, "schedule_" + self.c.schedule)):
            step()
        self.plan.set_lane(0)
        self.plan.set_segment(2)

    # ---------------- prologue: encoders + correlation pyramid (lanes: c.pro_lanes)
    def state_buffers(self):
        e, p, M = self.eng, self.plan, self.M
        p.set_segment(0)
        p.set_lane(self.c.pro_lanes[0])
        self.hx, self.qx = self.alloc("hx", (M, e.hx_cs)), self.alloc("qx", (M, e.hx_cs))
        self.h32, self.zb = self.alloc("h32", (M, e.hidden), F32), self.alloc("z", (M, e.hidden), e.gate_dtype)
        # bf16 flow for the flow branch: compact 2 channels for the 2-channel conv
        # kernel (4 taps = one 16-B load), 8-channel rows for the implicit GEMM
        self.flow8 = self.alloc("flow8", (M, 2 if e._cf1_w is not None else 8))
        self.coords, self.flow32 = self.alloc("coords", (M, 2), F32), self.alloc("flow32", (M, 2), F32)
        for t in (self.hx, self.qx, self.flow8, self.flow32):
            p.add_memset([t])

    def prep(self):
        p, c, src, Bi, H, W = self.plan, self.c, self.st.src, self.Bi, self.H, self.W
        self.x0 = self.alloc("x0", (2 * Bi, H // 2, W // 2, 16) if c.s2d else (2 * Bi, H, W, 8))
        # s2d: 2x2 space-to-depth images for the 4x4 form of the 7x7 / stride-2 stems; uint8 frames
        # (src = H0, W0, pad top, pad left): normalise + replicate pad + layout in one kernel (K14)
        lut = [] if src is None else [_engine.u8_table(self.eng.device)]
        mode = ([1] if c.s2d else []) if src is None else [int(c.s2d)] + list(src)
        p.add_prep([self.inp1, self.inp2, self.x0] + lut, [Bi, H, W] + mode)
        p.add_record(E_PREP)

    def context(self):
        """Context encoder, the loop-invariant GRU biases and the initial coordinates / seed."""
        e, p, c, sp, B, h, w, M = self.eng, self.plan, self.c, self.eng._specs, self.B, self.h, self.w, self.M
        p.set_lane(c.pro_lanes[1])
        p.add_wait(E_PREP)
        # the context of the loop's first frames: image 1 of every pair; bidirectional: both frames
        ctx_in = self.x0 if c.bidir else self.x0[:self.Bi]
        ctxf, ch_, cw_ = e._encoder(self.st, p, "ce", e.model.context_encoder, ctx_in, B, self.H, self.W, bt=self.pt)
        assert (ch_, cw_) == (h, w), "The context encoder should downsample H and W by 8"
        # [tanh(h) | relu(context)] (model.py:582-584); h also as fp32 state
        ce_out = self.alloc("ce_out", (M, round_up(e.hidden + e.ctx_ch, 8)))
        e._conv(p, sp["ce.conv"], ctxf, B, h, w, ce_out, act=ACT_SPLIT_TANH_RELU, split=e.hidden,
                h32=self.h32, hidden=e.hidden)
        p.add_copy_channels([ce_out, self.hx], [0, 0, M, e.hidden])
        # loop-invariant context share of every GRU gate (+ gate biases)
        self.gbias = []
        for gi in range(self.ngru):
            gb = self.alloc(f"gru{gi}.cbias", (M, e.gate_cs), e.gate_dtype)
            e._conv(p, sp[f"gru{gi}.ctx"], ce_out, B, h, w, gb, x_coff=e.hidden)
            self.gbias.append(gb)
        if c.warm:
            # the seed sits where init_coords sits: on the context lane, which waited for E_PREP
            # (recorded on the main lane after the memsets of hx / qx / flow8 / flow32, so the
            # seed is not zeroed again) and records E_CTX, which the main lane waits for before
            # the lane schedule's iteration-0 flow features and the first lookup.  It writes the
            # state a flow update leaves (flowhead.hip:flow_taps_kernel), qx only where that does.
            p.add_init_flow([self.st.flow_init[self.b0:self.b0 + B], self.coords, self.flow32, self.hx,
                             self.qx if c.qx_x else None, self.flow8], [B, h, w, e.flow_off, e.flow_off])
        else:
            p.add_init_coords([self.coords], [B, h, w])
        p.add_record(E_CTX)

    def features(self):
        """The feature maps of both frames, on the main prologue lane when this returns."""
        self.fmap = self.alloc("fmap", (2 * self.Bi, self.h, self.w, self.eng.fmap_ch))
        if self.c.fe_split and not self.eng.fe_external:
            return self.features_split()
        self.plan.set_lane(self.c.pro_lanes[0])
        if not self.eng.fe_external:   # (else fmap is written before each replay: RaftEngineMixed._pre_launch)
            self.feature_encoder(self.x0, 2 * self.Bi, self.fmap, self.pt)

    def feature_encoder(self, x, N, fmap, bt):
        e = self.eng
        feat, fh_, fw_ = e._encoder(self.st, self.plan, "fe", e.model.feature_encoder, x, N, self.H, self.W, bt=bt)
        assert (fh_, fw_) == (self.h, self.w), "The feature encoder should downsample H and W by 8"
        e._conv(self.plan, e._specs["fe.conv"], feat, N, self.h, self.w, fmap)

    def features_split(self):
        """The feature encoder of image2 on a third lane, concurrent with image1's (and the
        context encoder): per-image instance norms, so the halves are exact, and the sequential
        encoder chain that gates the correlation pyramid is half as long."""
        p, Bi = self.plan, self.Bi
        p.set_lane(self.c.pro_lanes[2])
        p.add_wait(E_PREP)
        self.feature_encoder(self.x0[Bi:], Bi, self.fmap[Bi:], self.pt + "fe2.")
        p.add_record(E_FE2)
        p.set_lane(self.c.pro_lanes[0])
        self.feature_encoder(self.x0[:Bi], Bi, self.fmap[:Bi], self.pt)
        p.add_wait(E_FE2)

    def correlation(self):
        """The correlation pyramid (or, on demand, the pooled target features); joins the context lane."""
        e, p, c, Bi, B, h, w, L = self.eng, self.plan, self.c, self.Bi, self.B, self.h, self.w, self.L
        fmap, pad = self.fmap, [None] * (4 - L)
        # context parallelism: this rank's pyramid holds the query rows [r0, r1) only
        self.slabs = e._cp_slabs(h) if e.cp else [(0, h)]
        self.r0, self.r1 = r0, r1 = self.slabs[e.cp_rank]
        self.nq = nq = (r1 - r0) * w
        # on demand: no volume -- the pooled target features of levels 1 .. L-1 (fp32) instead
        self.pooled = ([self.alloc(f"fpool.l{l}", (Bi, h >> l, w >> l, e.fmap_ch), F32) for l in range(1, L)]
                       if c.on_demand else [])
        self.levels = levels = []
        for l in range(0 if c.on_demand else L):
            shape = ((self.M, -(-h // 8) * (8 >> l), -(-w // 16) * (16 >> l)) if c.blocked and l < 2
                     else (B * nq, h >> l, w >> l))
            levels.append(self.alloc(f"corr.l{l}", shape, e.corr_dtype))
        scale = 1.0 / float(e.fmap_ch) ** 0.5
        if c.on_demand:
            p.add_feat_pool([fmap[Bi:]] + self.pooled, [Bi, h, w, e.fmap_ch, L])
        elif e.cp:
            for b in range(B):
                p.add_corr([fmap[b, r0:r1], fmap[B + b]] + [v[b * nq:(b + 1) * nq] for v in levels] + pad,
                           [1, h, w, e.fmap_ch, L, nq, 0], scale)
        else:
            p.add_corr([fmap[:Bi], fmap[Bi:]] + levels + pad, [Bi, h, w, e.fmap_ch, L, h * w, c.bl], scale)
            if c.bidir:   # 2 -> 1: the halves swapped, into the second B*h*w query rows of every level
                p.add_corr([fmap[Bi:], fmap[:Bi]] + [v[Bi * h * w:] for v in levels] + pad,
                           [Bi, h, w, e.fmap_ch, L, h * w, c.bl], scale)
        p.add_wait(E_CTX)

    def loop_buffers(self):
        e, c, M = self.eng, self.c, self.M
        cl, fl = self.me.corr_layers, self.me.flow_layers
        self.corr = self.alloc("corr", (M, e.corr_cs))
        self.cf = self.alloc("cf", (M, cl[-1] + fl[-1]))
        self.f1 = None if c.flow_fused else self.alloc("f1", (M, fl[0]))   # (the fused flow features keep it on the CU)
        self.c1 = self.alloc("c1", (M, cl[0])) if len(cl) == 2 else None
        self.taps = self.alloc("fh2.taps", (M, 24), F32)
        self.fm = None if c.taps_epi else self.alloc("fm", (M, round_up(e._specs[c.s1].cout, 8)))
        self.mfeat = (self.alloc("mfeat", (M, round_up(e._specs["mask.convrelu"].cout, 8)))
                      if e.has_mask and (c.split_mask or not c.all_iters) else None)
        self.mask = self.alloc("mask", (M, 576)) if e.has_mask and e._convex_w is None else None
        self.hm = self.alloc("hm", (M, e.hidden)) if c.hm else None
        self.hm2 = self.alloc("hm2", (M, e.hidden)) if c.parity else None
        self.flow32b = self.alloc("flow32b", (M, 2), F32) if c.parity else None
        self.st.flow_out.append((self.b0, self.B, self.flow32, self.flow32b))

    # ---------------- op emitters of the loop body (model.py:495-510)
    def flow_features(self):
        e, p, B, h, w = self.eng, self.plan, self.B, self.h, self.w
        if self.c.flow_fused:   # both convs in one launch (flowfeat.hip)
            sp2 = e._specs["me.convflow2"]
            p.add_flow_features_fused([self.flow8, e._cf1_w, e._cf1_b, sp2.wh, sp2.b, self.cf],
                                      [B, h, w, self.me.corr_layers[-1]])
            return
        if e._cf1_w is not None:
            p.add_conv_direct([self.flow8, e._cf1_w, e._cf1_b, self.f1], self._flowin_ints())
        else:
            e._conv(p, e._specs["me.convflow1"], self.flow8, B, h, w, self.f1, act=ACT_RELU)
        e._conv(p, e._specs["me.convflow2"], self.f1, B, h, w, self.cf, y_coff=self.me.corr_layers[-1], act=ACT_RELU)

    def _flowin_ints(self):
        c = self.me.convflow1.layers_0
        kh, kw_, _, co = c.kernel.shape
        return [self.B, self.h, self.w, 2, kh, kw_, c.padding[0], c.padding[1], co, 1, 0]

    def flowin_dual(self, stride: int, convex: bool):
        """The 7x7 flow conv and the previous iteration's x8 upsampling in ONE grid (merged.hip):
        both read the flow the lookup just updated, and at batch 1 neither fills the GPU.
        ``convex``: the convex head reading the fused FlowHead conv1's second half in ``fm``
        (+ convcorr1, the LDS-weight 1x1 kernel, in the same grid: ``c1_merged``), else bilinear."""
        e, cl = self.eng, self.me.corr_layers
        t_ = [self.flow8, e._cf1_w, e._cf1_b, self.f1, self.flow32, self.out, self.st.out_slot]
        if not convex:
            self.plan.add_flowin_dual(t_, self._flowin_ints() + [1, stride, self.out_off, 0], 1.0)
            return
        t_ += [self.fm, e._convex_w, e._convex_b]
        i_ = self._flowin_ints() + [2, stride, self.out_off, e.fh_hidden]
        if self.c.c1_merged:
            t_ += [self.corr, e._cc1_w, e._cc1_b, self.c1]
            i_ += [self.M, e.corr_cs, e._cc1_kpad, cl[0], ACT_RELU, 0]
        self.plan.add_flowin_dual(t_, i_, e.model.mask_predictor.multiplier)

    def flow_head(self):
        """FlowHead conv1 (+ conv2 as per-pixel tap partials into ``taps``)."""
        e, p, c, B, h, w = self.eng, self.plan, self.c, self.B, self.h, self.w
        s1 = e._specs[c.s1]
        if c.taps_epi:
            e._conv(p, s1, self.hx, B, h, w, self.taps, act=ACT_RELU, epi=EPI_TAPS, tapw=e._taps_epi_w)
            return
        if c.halo_pp:   # h' of even iterations is in qx, of odd ones in hx
            e._conv(p, s1, self.qx, B, h, w, self.fm, x_alt=self.hx, act=ACT_RELU)
        else:
            e._conv(p, s1, self.hx, B, h, w, self.fm, act=ACT_RELU)
        if e._taps_w is not None:   # skinny GEMM kernel (flowhead.hip), N = 18
            p.add_taps_gemm([self.fm, e._taps_w, self.taps], [self.M, e.fh_hidden, 0])
        else:
            e._conv(p, e._specs["fh2.taps"], self.fm, B, h, w, self.taps)

    def _update_operands(self, coords=()):
        """The tensors of a flow update: taps in; flow into flow32 (flow32b: the odd iterations') / hx / qx / flow8."""
        return ([self.taps, self.eng._fh2_b] + list(coords)
                + [self.flow32, self.hx, self.qx if self.c.qx_x else None, self.flow8]
                + ([self.flow32b] if self.c.parity else []))

    def flow_update(self):   # ``coords1 += delta`` (model.py:505) from the taps
        off = self.eng.flow_off
        self.plan.add_flow_taps(self._update_operands([self.coords]), [self.B, self.h, self.w, off, off])

    def lookup(self, with_update: bool):
        """The correlation features at ``coords``; ``with_update``: after the previous iteration's flow update."""
        e, p, c, B, h, w, L = self.eng, self.plan, self.c, self.B, self.h, self.w, self.L
        upd = self._update_operands() if with_update else []
        extra = [e.flow_off, e.flow_off] if with_update else []
        if c.on_demand:
            p.add_lookup_od([self.coords, self.corr, self.fmap[:self.Bi], self.fmap[self.Bi:]] + self.pooled
                            + [None] * (4 - L) + upd, [L, B, h, w, e.radius, e.fmap_ch] + extra)
            return
        p.add_lookup([self.coords, self.corr] + self.levels + [None] * (4 - L) + upd,
                     [L, B, h, w, e.radius, h * w, c.blocked] + extra)

    def upsample(self, stride: int, mask_from_fm: bool = False):
        """x8 upsampling of flow32 into the output (model.py:508): convex with the mask head (its
        3x3 conv from hx / hm, or the fused FlowHead conv1's second half in ``fm``), else bilinear."""
        e, p, c, B, h, w = self.eng, self.plan, self.c, self.B, self.h, self.w
        if not e.has_mask:
            p.add_upsample_bilinear([self.flow32, self.out, self.st.out_slot], [B, h, w, stride, self.out_off])
            return
        feat_, coff = self.fm, e.fh_hidden
        if not mask_from_fm:
            e._conv(p, e._specs["mask.convrelu"], self.hm if self.hm is not None else self.hx, B, h, w, self.mfeat,
                    act=ACT_RELU, x_alt=self.hm2)
            feat_, coff = self.mfeat, 0
        mult = e.model.mask_predictor.multiplier
        if e._convex_w is not None:
            p.add_convex_head([feat_, e._convex_w, e._convex_b, self.flow32, self.out, self.st.out_slot]
                              + ([self.flow32b] if c.parity else []), [B, h, w, coff, stride, 0, self.out_off], mult)
        else:   # generic mask head (an injected MaskPredictor): 1x1 conv + convex upsampling
            self.st.slot_ok = False
            e._conv(p, e._specs["mask"], feat_, B, h, w, self.mask, x_coff=coff, alpha=mult)
            p.add_upsample_convex([self.mask, self.flow32, self.out], [B, h, w, stride])

    def corr_convs(self, flow2: bool = False):
        """The correlation branch of the motion encoder.  ``flow2``: convflow2 (the flow branch's
        second conv) is added here, as one grid with the last correlation conv when a grouped
        launch serves its tile config (conv_grouped_kernel; CONV_GROUP = False keeps them separate
        launches) -- and convcorr1 is left out where it ran in the flow conv's merged grid."""
        e, p, sp, B, h, w, cl = self.eng, self.plan, self.eng._specs, self.B, self.h, self.w, self.me.corr_layers
        last = (sp["me.convcorr1"], self.corr, B, h, w, self.cf, dict(act=ACT_RELU))
        if len(cl) == 2:
            if e._cc1_w is None:
                e._conv(p, sp["me.convcorr1"], self.corr, B, h, w, self.c1, act=ACT_RELU)
            elif not (flow2 and self.c.c1_merged):   # LDS-resident-weight 1x1 kernel (conv1x1.hip)
                p.add_conv1x1([self.corr, e._cc1_w, e._cc1_b, self.c1],
                              [self.M, e.corr_cs, e._cc1_kpad, cl[0], ACT_RELU, 0])
            last = (sp["me.convcorr2"], self.c1, B, h, w, self.cf, dict(act=ACT_RELU))
        fl2 = (sp["me.convflow2"], self.f1, B, h, w, self.cf, dict(y_coff=cl[-1], act=ACT_RELU))
        if not (flow2 and e.CONV_GROUP and e._conv_group(p, last, fl2)):
            if flow2:
                e._conv(p, *fl2[:6], **fl2[6])
            e._conv(p, *last[:6], **last[6])

    def motion_conv(self):
        """The motion encoder's output conv into hx (and qx), unless the first fused stage runs it."""
        e, c = self.eng, self.c
        if not c.gru_me:
            e._conv(self.plan, e._specs["me.conv"], self.cf, self.B, self.h, self.w, self.hx, y_coff=e.mot_off,
                    act=ACT_RELU, y2=self.qx if c.qx_x else None, y2_coff=e.mot_off)

    def gru(self):   # one emitter per ConvGRU lowering (looked up per call: a bound method kept on self is a cycle)
        getattr(self, "gru_" + self.c.gru_path)()

    def gru_halo(self):
        e, p, c, hx, qx = self.eng, self.plan, self.c, self.hx, self.qx
        for gi, (mode, axis) in enumerate(e._halo_geom()[1]):
            wa_, wb_ = e._halo_w[gi]
            if c.halo_pp:
                t = [hx, hx, wa_, wb_, self.gbias[gi], self.h32, qx, self.hm, qx, qx, hx]
            else:
                t = [hx if gi == 0 else qx, hx, wa_, wb_, self.gbias[gi], self.h32, qx if gi == 0 else hx,
                     self.hm if gi == self.ngru - 1 else None]
            if c.mask_wait == gi:
                p.add_wait(E_MASK)
            base = [self.B, self.h, self.w, mode, axis]
            p.add_gru_halo(t, base + list(e._halo_tile(gi, mode, axis, self.B, self.h, self.w, (t, base))))

    def gru_fused(self):
        e, p, c, sp, hx, B, h, w = self.eng, self.plan, self.c, self.eng._specs, self.hx, self.B, self.h, self.w
        for gi in range(self.ngru):
            hm = self.hm if gi == self.ngru - 1 else None
            if c.mask_wait == gi:
                p.add_wait(E_MASK)
            if gi == 0 and c.gru_me:   # stage 1 computes its own motion features (nothing reads qx's copy)
                mc = sp["me.conv"]
                p.add_gru_fused_me([hx, sp["gru0.a"].w, sp["gru0.b"].w, self.gbias[0], self.h32, hx, hm, None,
                                    self.cf, mc.w, mc.b], [B, h, w, mc.cout])
                continue
            ks = e.model.update_block.recurrent_block.kernel_size[gi]
            p.add_gru_fused([hx, sp[f"gru{gi}.a"].w, sp[f"gru{gi}.b"].w, self.gbias[gi], self.h32, hx, hm]
                            + ([None, self.hm2] if gi == self.ngru - 1 and c.parity else []),
                            [B, h, w, int(ks[0] > 1)])

    def gru_unfused(self):
        e, p, B, h, w = self.eng, self.plan, self.B, self.h, self.w
        for gi in range(self.ngru):
            # r*h from the bf16 h of the conv's own input hx (no fp32 state read)
            e._conv(p, e._specs[f"gru{gi}.a"], self.hx, B, h, w, self.qx, zbuf=self.zb, hidden=e.hidden,
                    epi=EPI_GRU_A, bmap=self.gbias[gi], bmap_coff=0)
            if self.c.mask_wait == gi:
                p.add_wait(E_MASK)
            e._conv(p, e._specs[f"gru{gi}.b"], self.qx, B, h, w, self.hx, h32=self.h32, zbuf=self.zb,
                    hidden=e.hidden, epi=EPI_GRU_B, bmap=self.gbias[gi], bmap_coff=2 * e.hidden)

    # ---------------- schedules: one iteration (segment 1) + the epilogue (segment 2)
    def schedule_cp(self):
        """Context parallel, one lane, eager from C++.  Segment 1: this rank's slab lookups, one
        per image; the engine all-gathers them into ``corr`` (``_gather_corr``); segment 3: the
        rest of the iteration, replicated."""
        e, p, h, w, hw, nq = self.eng, self.plan, self.h, self.w, self.h * self.w, self.nq
        local = self.alloc("corr.local", (self.B, max(b_ - a_ for a_, b_ in self.slabs) * w, e.corr_cs))
        p.set_segment(1)
        for b in range(self.B):
            p.add_lookup([self.coords[b * hw + self.r0 * w:b * hw + self.r1 * w], local[b]]
                         + [v[b * nq:(b + 1) * nq] for v in self.levels] + [None] * (4 - self.L),
                         [self.L, 1, h, w, e.radius, nq, 0])
        p.set_segment(3)
        self.flow_features()
        self.corr_convs()
        self.motion_conv()
        self.gru()
        self.flow_head()
        self.flow_update()
        if self.c.all_iters:
            self.upsample(self.stride)
        p.set_segment(2)
        if not self.c.all_iters:
            self.upsample(0)
        self.st.cp = dict(slabs=self.slabs, local=local, corr=self.corr, w=w)

    def schedule_lanes(self):
        """The critical lane runs lookup (+ the previous iteration's flow update) -> convcorr1/2
        -> motion conv -> ConvGRU -> FlowHead conv1 with the taps epilogue; the mask lane, forked
        after the lookup, runs the flow-feature convs of this iteration and the mask head + convex
        upsampling of the previous one (deferred ops, skipped in iteration 0).  Three cross-lane
        edges per iteration: E_FH, E_FLOW and E_MASK (``PartChoices.mask_wait``)."""
        p, (main, _, side2) = self.plan, self.c.lanes
        p.set_segment(0)              # iteration 0's flow features (zero flow) run once in the prologue
        p.set_lane(main)
        self.flow_features()
        p.set_segment(1)
        self.lookup(with_update=True)
        p.add_record(E_FH)
        p.set_lane(side2)
        p.set_defer(1)                # skipped in iteration 0
        p.add_wait(E_FH)
        self.flow_features()
        p.add_record(E_FLOW)
        self.upsample(self.stride)    # iteration i-1 (h / hm intact until the E_MASK join)
        p.add_record(E_MASK)
        p.set_defer(0)
        p.set_lane(main)
        self.corr_convs()
        p.add_wait(E_FLOW)
        self.motion_conv()
        self.gru()
        self.flow_head()
        p.set_segment(2)              # epilogue: the last iteration's update, mask head and upsampling
        self.flow_update()
        p.set_defer(1)
        self.upsample(self.stride)
        p.set_defer(0)

    def schedule_one_lane(self):
        """One lane, every iteration upsampled -- the lane schedule's deferral in order: lookup
        (+ update), flow features, upsampling of iteration i-1 (one merged grid under
        ``merged_up``), correlation / motion / GRU convs, FlowHead conv1 (fused with the mask
        predictor's 3x3 conv as one 128 -> 512 GEMM when there is a mask head) + the taps GEMM."""
        p, c = self.plan, self.c
        from_fm = self.fm is not None and self.eng.has_mask
        p.set_segment(1)
        p.set_lane(c.lanes[0])
        self.lookup(with_update=True)
        if c.merged_up:
            self.flowin_dual(self.stride, convex=self.eng.has_mask)
        else:
            self.flow_features()
            p.set_defer(1)
            self.upsample(self.stride, mask_from_fm=from_fm)   # iteration i-1
            p.set_defer(0)
        self.corr_convs(flow2=c.merged_up)
        self.motion_conv()
        self.gru()
        self.flow_head()
        p.set_segment(2)
        self.flow_update()
        p.set_defer(1)
        self.upsample(self.stride, mask_from_fm=from_fm)
        p.set_defer(0)

    def schedule_final_merged(self):
        """Final-only (serving) in the one-lane order: the merged grid's bilinear half writes the
        single output slot every iteration (stride 0); the epilogue's upsampling overwrites it."""
        p = self.plan
        p.set_segment(1)
        p.set_lane(self.c.lanes[0])
        self.lookup(with_update=True)
        self.flowin_dual(0, convex=False)
        self.corr_convs(flow2=True)
        self.motion_conv()
        self.gru()
        self.flow_head()
        p.set_segment(2)              # epilogue: the last update, then the final flow upsampled once
        self.flow_update()
        self.upsample(0)

    def schedule_final(self):
        """Final-only (serving): the loop runs the flow head alone; the mask head + x8 upsampling
        run once in the epilogue on the final hidden state and flow."""
        p = self.plan
        p.set_segment(1)
        p.set_lane(self.c.lanes[0])
        self.flow_features()
        self.lookup(with_update=False)
        self.corr_convs()
        self.motion_conv()
        self.gru()
        self.flow_head()
        self.flow_update()
        p.set_segment(2)              # epilogue: upsample the final flow once (out has one iteration)
        self.upsample(0)


# ---------------- entry points
def new_state(eng, B: int, H: int, W: int, n_iters: int, all_iters: bool, src, parts: int, out_batch: int):
    """What every plan starts from: the size guard of the correlation pyramid, ``parts`` empty native plans,
    the input buffers of ``B`` image pairs and the output of ``out_batch`` flows per iteration with its slot."""
    h, w = H // 8, W // 8
    min_sz = 2 * (2 ** (eng.num_levels - 1))
    assert h >= min_sz and w >= min_sz, (
        f"Feature maps are too small to be down-sampled by the correlation pyramid: need >= {min_sz}, got {(h, w)}; "
        f"input images should be at least {8 * min_sz}.")
    dev = eng.device
    # Each part is an independent forward with its own Plan; with use_graph their captures are
    # copied into ONE hipGraph (Plan.merge_*), so the parts' kernels fill each other's idle CUs.
    plans = [nat.new_plan() for _ in range(parts)]
    st = _engine._PlanState(plan=plans[0], plans=plans, n_iters=n_iters, src=src)
    shape, dtype = ((B, src[0], src[1], 3), torch.uint8) if src is not None else ((B, H, W, 3), F32)   # (src: raw frames)
    st.inp1 = torch.zeros(shape, dtype=dtype, device=dev)
    st.inp2 = torch.zeros(shape, dtype=dtype, device=dev)
    st.out = torch.zeros((n_iters if all_iters else 1, out_batch, H, W, 2), dtype=F32, device=dev)
    st.slot_ptr = st.out.data_ptr()
    st.out_slot = torch.tensor([st.slot_ptr], dtype=torch.int64, device=dev)
    return st


def _finish(eng, st):
    """The one place a build writes plan facts to the engine: ``eng.gru_path`` and
    ``eng.corr_blocked`` are those OF THE MOST RECENTLY BUILT PLAN (tests and tools read them
    right after a build); what a cached plan runs with is in its own ``st.choices``."""
    eng.gru_path, eng.corr_blocked = st.choices[-1].gru_path, bool(st.choices[-1].blocked)
    return st


def build(eng, B: int, H: int, W: int, n_iters: int, all_iters: bool = True, src=None, warm: bool = False,
          parts: Optional[int] = None, slot: bool = False):
    """The cold / warm plan of ``B`` image pairs as ``parts`` independent part-forwards (default:
    the engine's ``split`` where it divides the batch)."""
    if warm and eng.cp:
        raise NotImplementedError("warm start (flow_init) is not lowered under context parallelism")
    parts = eng._parts(B) if parts is None else parts
    nb = B // parts
    lanes = (0, 1, 2) if eng.uses_lanes(B, all_iters, parts=parts) else (0, 0, 0)
    c = choose(eng, nb, nb, H // 8, W // 8, all_iters, lanes, warm=warm, slot=slot)
    st = new_state(eng, B, H, W, n_iters, all_iters, src, parts, B)
    if warm:
        st.flow_init = torch.zeros((B, H // 8, W // 8, 2), dtype=F32, device=eng.device)
    for part, plan in enumerate(st.plans):
        st.choices.append(c)
        PartRecorder(eng, st, plan, c, part * nb, nb, H, W, f"p{part}.").record()
    return _finish(eng, st)


def build_bidir(eng, B: int, H: int, W: int, n_iters: int, all_iters: bool, src, warp: bool = False,
                slot: bool = False, interp: int = 0):
    """The plan of ``forward(bidirectional=True)``: one part (``split`` would lay ``out`` by part)
    whose loop runs both directions at batch 2B, so the lane decision, the ConvGRU lowering and
    every tile choice are those of loop batch 2B; ``out`` is (N, 2B, H, W, 2) with 1 -> 2 in
    ``[:, :B]`` and 2 -> 1 in ``[:, B:]``.  The epilogue ends with the forward-backward check
    (fbcheck.hip) of the final iteration's two flows, on lane 0 after the last upsampling; it
    reads them through the output slot, where that replay wrote them.

    ``warp`` (uint8 frames): the same recording followed, on lane 0 after the check, by the
    ``memset`` of the photometric sums and one ``warp_frames`` over both directions
    (framewarp.hip): it samples the frames as uploaded (``inp1`` / ``inp2``) with the same two
    flows, masked by ``occ``, into the plan's ``warped`` and ``photo``.

    ``interp = K`` (uint8 frames, not with ``warp``): the same recording followed, on lane 0 after
    the check, by ``memset`` of the accumulator, ``interp_splat`` and ``interp_resolve`` for each of
    K times (interp.hip): they splat the frames as uploaded along the same two flows, weighted by
    ``occ``, into the plan's ``acc`` and resolve it into ``interp[k]`` / ``holes[k]``; the times
    are rows of the device tensor ``par``."""
    if eng.cp:
        raise NotImplementedError("bidirectional flow is not lowered under context parallelism")
    assert not warp or src is not None, "warp: uint8 frames only"
    assert not interp or (src is not None and not warp), "interp: uint8 frames only, and not together with warp"
    lanes = (0, 1, 2) if eng.uses_lanes(2 * B, all_iters, parts=1) else (0, 0, 0)
    c = choose(eng, B, 2 * B, H // 8, W // 8, all_iters, lanes, bidir=True, slot=slot)
    st = new_state(eng, B, H, W, n_iters, all_iters, src, 1, 2 * B)
    plan, dev = st.plan, eng.device
    st.occ = torch.zeros((2, B, H, W), dtype=torch.uint8, device=dev)
    st.thr = torch.zeros(2, dtype=F32, device=dev)
    st.choices.append(c)
    PartRecorder(eng, st, plan, c, 0, B, H, W, "p0.").record()
    # the final iteration's flows: the last slice of ``out``, its two batch halves -- through the
    # slot, or the captured buffer itself where a generic mask head writes that (not slot_ok)
    last = st.out[-1]
    off = (last.data_ptr() - st.out.data_ptr()) // 4
    flows, tail = (([None, None], [st.out_slot]) if st.slot_ok else ([last[:B], last[B:]], []))
    ints = [B, H, W] + ([H, W, 0, 0] if src is None else list(src))
    offs = [off, off + B * H * W * 2] if st.slot_ok else []
    plan.add_fb_check(flows + [st.occ, None, st.thr] + tail, ints + offs)
    if warp:
        st.warped = torch.zeros((2, B, src[0], src[1], 3), dtype=torch.uint8, device=dev)
        st.photo = torch.zeros((2, B, 2), dtype=torch.int64, device=dev)
        plan.add_memset([st.photo])
        frames = [st.inp2, st.inp1, st.inp1, st.inp2]   # src (fw, bw), own (fw, bw)
        plan.add_warp_frames(frames + flows + [st.occ, st.warped, st.photo] + tail, ints + [2] + offs)
    if interp:
        H0, W0 = src[0], src[1]
        st.acc = torch.zeros((2, B, H0, W0, 4), dtype=torch.int64, device=dev)
        st.par = torch.zeros((interp, 2), dtype=torch.int32, device=dev)
        st.interp = torch.zeros((interp, B, H0, W0, 3), dtype=torch.uint8, device=dev)
        st.holes = torch.zeros((interp, B, H0, W0), dtype=torch.uint8, device=dev)
        for k in range(interp):
            plan.add_memset([st.acc])
            plan.add_interp_splat([st.inp1, st.inp2] + flows + [st.occ, st.acc, st.par] + tail, ints + [k] + offs)
            plan.add_interp_resolve([st.inp1, st.inp2, st.acc, st.par, st.interp[k], st.holes[k]], [B, H0, W0, k])
    return _finish(eng, st)
