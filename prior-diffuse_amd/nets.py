"""Plan builders: turn reference ``state_dict``s into recorded operator sequences
(include/pdse.h plans) for the networks and signal-processing stages on the path.

  EpsNetPlan     DiffUNet1.forward(x, x_init, t)        model/diff3.py:37-57
  (same builder, ``time_cond=False``)  prior DiffUNet   model/diff.py:23-33
  GcrnPlan       GCRN.forward                           model/gcrn.py:136-166
  StftPlan / IstftPlan   front/back end                 trainer/complex_ddpm_trainer.py:921-937, :1004-1016

Every tensor lives in HBM for the lifetime of the plan (weights packed once, workspaces
allocated once per (B, T)); a plan run is a pure sequence of kernel launches with no
allocation and no host synchronisation, so it can be captured into a hipGraph.

The builders here record descriptors: strides, offsets and buffers of one (B, T).  What a descriptor's weight operands hold -
BatchNorm folds, composed convolutions, f16x2 exponents, fragment layouts - is derived in ``packing.py`` by pure functions from
natural weights to ``{descriptor field: array | scalar}``; ``PlanBase.fields`` uploads such a dict once per weight bank and
``PlanBase.apply`` sets it on a descriptor.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import packing as P

F0 = 161
BIG = 1 << 30

# tags for bench/roofline attribution
TAG_NONE, TAG_EPS_BLOCK, TAG_EPS_CONV1, TAG_TCM, TAG_PRIOR, TAG_LSTM, TAG_SIGNAL, TAG_EW = range(8)


class WeightBank:
    """Packed weights of one set of state_dicts in HBM, shared by every plan built from them.

    A plan is recorded for one (B, T); its weights depend on neither.  The builders therefore route everything that is
    derived from a state_dict through ``PlanBase.memo``: the first plan packs and uploads, every later plan (another
    utterance length in ``generate_wav``, another buffer set of ``PipelinedSampler``) only re-records descriptors
    that point at the same device tensors.  Entries are keyed by (builder namespace, call index) - the builders are
    deterministic, and a site label stored with every entry turns a diverging call sequence into an error."""

    def __init__(self):
        self.items = {}
        self.keep = []      # every device tensor an entry refers to
        self.owners = []    # the state_dicts (and tables) entries were derived from, kept alive: an ``id()`` cannot be recycled

    def token(self, obj):
        """Per-bank identity of a state_dict: its index in ``owners``.  The bank holds a reference, so a bank that
        outlives a checkpoint can never hand that checkpoint's packed weights to a new dict at a recycled address."""
        if obj is None:
            return None
        for i, o in enumerate(self.owners):
            if o is obj:
                return i
        self.owners.append(obj)
        return len(self.owners) - 1

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.keep if torch.is_tensor(t))


class Ctx:
    """Device-memory helper: torch tensors for storage, raw pointers for the ABI."""

    def __init__(self, device, bank=None):
        self.device = torch.device(device)
        self.keep = []                  # per-plan tensors (activations, workspaces, per-step tables)
        self.bank = bank if bank is not None else WeightBank()
        self._banking = 0
        self.scratch = set()            # data_ptr of buffers whose initial contents do not matter (planfile.py saves no bytes for them)

    def alloc(self, *shape, zero=False):
        t = (torch.zeros if zero else torch.empty)(*shape, dtype=torch.float32, device=self.device)
        self.keep.append(t)
        if not zero:
            self.scratch.add(t.data_ptr())
        return t

    def up(self, arr, dtype=np.float32):
        t = torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to(self.device)
        (self.bank.keep if self._banking else self.keep).append(t)
        return t

    def alloc_u16(self, *shape):
        """Zeroed 16-bit storage (bf16 planes travel as integers; torch has no uint16 arithmetic and needs none)."""
        t = torch.zeros(*shape, dtype=torch.int16, device=self.device)
        self.keep.append(t)
        return t

    def all_tensors(self):
        """Everything a descriptor of this context may point at (tests replay descriptors on these)."""
        return list(self.keep) + list(self.bank.keep)

    @staticmethod
    def ptr(t, off=0):
        return 0 if t is None else t.data_ptr() + 4 * int(off)


class PlanBase:
    force_generic = False   # tests: route every convolution through the un-pipelined kernel
    gemm_planes = 3         # operand planes of the GEMM-shaped convolutions (csrc/gconv4.hip): 3 = exact three-way bf16 split
                            # (korder 3), 2 = fp16 hi + lo of the scaled operands (korder 5, f16x2: fp32-equivalent), 1 = plain
                            # bf16, one product (korder 4: the opt-in bf16 mode, its own tolerance)

    def __init__(self, ctx, plan=None, ns=()):
        self.ctx = ctx
        self.descs = []  # python-side copy of every descriptor (tests replay these on the CPU emulator)
        self.plan = plan if plan is not None else (L.Plan(ctx.device) if ctx.device.type == "cuda" else None)
        self.ns = (type(self).__name__, bool(self.force_generic)) + tuple(ns)
        self._mi = 0
        self._audit_ops = {}      # (address, kind) -> f16x2 operand of a recorded launch, in recording order (audited())
        self._audit_names = {}    # data_ptr -> (name, buffer): the buffers audited() may report (named())

    def memo(self, label, fn):
        """Weight-derived value (device tensors, folded scalars), computed once per WeightBank: ``fn`` runs only on
        the first plan built from this state_dict; tensors it uploads through ``ctx.up`` belong to the bank."""
        key = (self.ns, self._mi)
        self._mi += 1
        bank = self.ctx.bank
        hit = bank.items.get(key)
        if hit is None:
            self.ctx._banking += 1
            try:
                hit = (label, fn())
            finally:
                self.ctx._banking -= 1
            bank.items[key] = hit
        if hit[0] != label:
            raise RuntimeError("weight bank: builder call sequence diverged at %r (bank holds %r)" % (label, hit[0]))
        return hit[1]

    def _up(self, a):
        """Upload one weight-derived array.  The one dtype convention of everything ``packing`` returns: uint16 arrays are
        operand planes (bf16 / fp16 bit patterns) and travel as int16 views, int32 stays int32, every other array is fp32."""
        if a.dtype == np.uint16:
            return self.ctx.up(np.ascontiguousarray(a).view(np.int16), np.int16)
        return self.ctx.up(a, np.int32 if a.dtype == np.int32 else np.float32)

    def upw(self, label, fn):
        """Device tensor of a weight-derived array (``fn`` -> numpy, uploaded as ``_up`` states), memoised in the bank."""
        return self.memo(label, lambda: self._up(fn()))

    def fields(self, label, fn):
        """``fn`` -> {descriptor field: array | scalar | tuple} (the pure functions of packing.py), memoised in the bank with every
        array uploaded (``_up``) and replaced by its device pointer; scalars and tuples pass through."""
        return self.memo(label, lambda: {k: self._up(v).data_ptr() if isinstance(v, np.ndarray) else v for k, v in fn().items()})

    @staticmethod
    def apply(d, fields):
        """Set a ``fields`` dict on a descriptor; a key (name, i) is element i of the array field ``name`` (nx_bias)."""
        for k, v in fields.items():
            if isinstance(k, tuple):
                getattr(d, k[0])[k[1]] = v
            else:
                setattr(d, k, v)

    def add(self, desc, tag=TAG_NONE):
        self.descs.append((desc, tag))
        if self.plan is not None:
            self.plan.add(desc, tag)
        for op in self.f16x2_operands(desc):        # noted as recorded (a few comparisons); resolved by audited() only
            self._audit_ops.setdefault((op[0], op[1]), op)

    # ---- range audit of the f16x2 window (csrc/range.hip) -----------------------
    def named(self, name, t):
        """Give a buffer the name it carries in audited() and in range reports; returns the buffer."""
        self._audit_names[t.data_ptr()] = (name, t)
        return t

    @staticmethod
    def f16x2_operands(desc):
        """The activation operands an f16x2 contraction of one recorded launch reads from memory, as
        [(address, kind, layout or None, name suffix)] - empty for every other launch.  kind RANGE_F16HI: a two-plane tensor
        (layout: the packing.hp_box / tcm2_hs_box of its logical elements, address: its first logical vector; suffix: the branch
        of a TCM bottleneck tensor); RANGE_F32: an fp32 tensor the kernel scales by 2^PDSE_F16_ACT_EXP and splits in registers
        (address: anywhere inside it).  This is the one place that knows which launches multiply f16x2 operands: csrc/bglu.hip
        and csrc/tcm2.hip with np 2, csrc/gconv4.hip korder 5, csrc/dense.hip np 2.  Operands that never reach memory (a block's
        gate tensor, the chained 1x1 tiles) cannot be audited."""
        out = []
        if isinstance(desc, L.BgluDesc) and desc.np == 2:
            if desc.hp:
                F_ = desc.hp_Fp - 2 * desc.hp_f0
                box = P.hp_box(desc.B, desc.hp_Tp - desc.hp_t0, F_, 2, par=bool(desc.hp_par))
                out.append((desc.hp + 2 * box["off"], L.RANGE_F16HI, box, ""))
            else:
                out += [(desc.x0.ptr, L.RANGE_F32, None, ""), (desc.x1.ptr, L.RANGE_F32, None, "")]
        elif isinstance(desc, L.Tcm2Desc) and desc.np == 2:
            out.append((desc.x, L.RANGE_F32, None, ""))
            if desc.mode == 0:
                for br, suffix in enumerate((".main", ".mask")):
                    box = P.tcm2_hs_box(desc.B, desc.T, 2, br)
                    out.append((desc.hs + 2 * box["off"], L.RANGE_F16HI, box, suffix))
        elif isinstance(desc, L.Tcm2sDesc):
            for i in range(desc.n):
                out += PlanBase.f16x2_operands(desc.blk[i])
        elif isinstance(desc, L.GconvDesc) and desc.korder == 5:
            out += [(s_.ptr, L.RANGE_F32, None, "") for s_ in (desc.in0, desc.in1) if s_.ptr]
        elif isinstance(desc, L.DenseDesc) and desc.np == 2:
            out.append((desc.D, L.RANGE_F32, None, ""))
        return [o for o in out if o[0]]

    def audited(self):
        """Every activation tensor an f16x2 contraction of the recorded launches reads from memory, as
        [(name, tensor, kind, exp, layout)] in recording order - the contract of the range audit
        (``SamplerPipeline(audit=True)``).  The operands are noted from the descriptors as they are recorded (``add``), so a
        launch cannot be missing; this call resolves them to the buffers the builder named where it allocated them (``named``)
        and raises if an operand lies in a buffer without a name - recording itself never fails for the audit's sake.
        kind / exp / layout are the fields of a pdse_range_row: RANGE_F32 tensors are counted whole (zero padding of the dense
        buffers included: zeros never decide a verdict) with exp = PDSE_F16_ACT_EXP, RANGE_F16HI tensors over the logical box
        ``layout`` (packing.hp_box / tcm2_hs_box; off: uint16 offset in ``tensor``), exp 0; the two branches of a TCM
        bottleneck tensor are two entries (``.main`` / ``.mask``).  Buffers are reused within a pass (both decoders share
        hp_de*, the TCM blocks ping-pong two hs buffers): an audit after a marked range sees their last contents."""
        out, seen = [], set()
        for addr, kind, box, suffix in self._audit_ops.values():
            hit = next(((n, t) for n, t in self._audit_names.values()
                        if t.data_ptr() <= addr < t.data_ptr() + t.numel() * t.element_size()), None)
            if hit is None:
                raise RuntimeError("range audit: the f16x2 operand at 0x%x lies in no buffer the builder named (PlanBase.named)" % addr)
            name, t = hit
            key = (name + suffix, kind)
            if key in seen:
                continue
            seen.add(key)
            out.append((name + suffix, t, kind, P.F16_ACT_EXP if kind == L.RANGE_F32 else 0,
                        None if box is None else dict(box, off=(addr - t.data_ptr()) // 2)))
        return out

    def finish(self):
        if self.plan is not None:
            self.plan.keep(self.ctx.keep, self.ctx.bank)

    # ---- windowed passes (longplan.py) --------------------------
    carries_state = False   # the network's reach into the past is a recurrent state that one window can hand to the next

    def receptive_field(self):
        """(H_left, H_right): the frames before and after frame t that output frame t of this network depends on, when that is
        finite; None when the network looks at all frames (attention, a bidirectional recurrence) and cannot run in windows."""
        return None

    # ---- descriptor helpers -------------------------------------------------
    def src(self, t, C_, sb, sc, st, sf, off=0, act=L.ACT_NONE, blk=0):
        return L.Src(Ctx.ptr(t, off), sb, sc, st, sf, C_, act, blk, 0)

    def gconv(self, *, in0, in1=None, Tin, Fin, taps, sf_in, W, Cout, bias0=None, bias0_sb=0,
              bias1=None, bias1_sb=0, epi=L.EPI_LINEAR, act=L.ACT_NONE, act_slope=0.0,
              padrow=None, padrow_sb=0, padrow_off=0, cin1=False, resid=None, out,
              out_strides, out_off=0, out_cr=1, B, Tout, Fout, tag=TAG_NONE, bias0_off=0, phase1=None, nx=None,
              bias1_off=0, bias_t0=None, label="gconv", s3=False, s3g=False, has_xf=False, flat=False):
        """W: callable -> dict of the launch's natural weight operands (see ``packing.gconv_fields``); evaluated only when the
        weight bank does not hold this launch yet.  bias0 / bias1 / padrow / bias_t0 here are per-plan DEVICE tensors
        (time-conditioned biases); constant biases travel inside W.
        phase1 (dual-phase transposed conv, BIGLU): dict(mask, Fout1) - its weights wk2 / wk3 / ntaps1 come from W.
        nx (BIGLU, C2 == 64): dict(keep, row0, tiles=[dict(bias (device tensor) or None, bias_off, bias_sb, out, strides
        (sb, sc, st, sf), off, add)]) - 1x1 convolutions chained onto the block output (include/pdse.h: nx_*); their
        weights (and constant biases) come from W()["nx"].
        flat (LINEAR GEMM form of one source with Fout == 1, korder 3 / 5): run the launch in the flat form of csrc/gconv4.hip
        (pdse_gconv_desc.flat) - the same result bit for bit."""
        ctx = self.ctx
        d = L.GconvDesc()
        d.in0 = in0
        d.in1 = in1 if in1 is not None else L.Src(0, 0, 0, 0, 0, 0, 0)
        d.Tin, d.Fin = Tin, Fin
        d.padrow, d.padrow_sb = Ctx.ptr(padrow, padrow_off), padrow_sb
        ttaps = tuple((int(a), int(b)) for a, b in taps)
        tkey = ("taps", ttaps)
        tp = ctx.bank.items.get(tkey)
        if tp is None:
            ctx._banking += 1
            tp = ctx.bank.items[tkey] = self._up(P.taps_array(ttaps))
            ctx._banking -= 1
        d.taps, d.ntaps, d.sf_in = tp.data_ptr(), len(ttaps), sf_in
        for i, (dt_, df_) in enumerate(ttaps[:12]):             # by-value copy for the unrolled-tap kernels
            d.tap_dt[i], d.tap_df[i] = dt_, df_
        d.cin1 = 1 if cin1 else 0
        c0, c1 = d.in0.C, d.in1.C
        pipelined_ok = padrow is None and not self.force_generic
        # split-bf16 instantiations (csrc/gconv3.hip): 32-channel blocks with 4 or 6 taps, the composed encoder stage 1
        s3 = bool(s3) and pipelined_ok and epi == L.EPI_BIGLU and (
            ((c0, c1) == (32, 0) and len(ttaps) in (4, 6)) or ((c0, c1, len(ttaps)) == (2, 2, 10) and phase1 is None))
        # split-bf16 GEMM form (csrc/gconv4.hip): LINEAR / GLU, channel counts in multiples of 16, no load transform
        s3g = (bool(s3g) and not s3 and pipelined_ok and epi in (L.EPI_LINEAR, L.EPI_GLU) and not cin1 and not has_xf
               and c0 > 0 and c0 % 16 == 0 and c1 % 16 == 0 and len(ttaps) <= 12)
        site = "%s:%d:%d:%d:%d:%d:%d:%d:%d" % (label, epi, len(ttaps), c0, c1, Cout, pipelined_ok, s3, s3g)
        if s3g:
            pack = lambda: P.gconv_gemm_fields(W(), len(ttaps), c0, c1, self.gemm_planes)   # noqa: E731
        elif s3:
            pack = lambda: P.gconv_s3_fields(W(), len(ttaps), c0 + c1)   # noqa: E731
        else:
            pack = lambda: P.gconv_fields(W(), len(ttaps), c0, c1, epi, cin1, pipelined_ok)   # noqa: E731
        self.apply(d, self.fields(site, pack))
        d.Cout = Cout
        if bias0 is not None:
            d.bias0 = Ctx.ptr(bias0, bias0_off)
        if bias1 is not None:
            d.bias1 = Ctx.ptr(bias1, bias1_off)
        d.bias0_sb, d.bias1_sb = bias0_sb, bias1_sb
        if bias_t0 is not None:                               # (tensor, offset of bias0_t0, offset of bias1_t0)
            d.bias0_t0, d.bias1_t0 = Ctx.ptr(bias_t0[0], bias_t0[1]), Ctx.ptr(bias_t0[0], bias_t0[2])
        d.epi, d.act, d.act_slope = epi, act, float(act_slope)
        if phase1 is not None and d.korder in (1, 2):
            d.p1mask, d.Fout1 = phase1["mask"], phase1["Fout1"]
        elif phase1 is not None and d.korder == 5 and epi == L.EPI_GLU:    # no w2 / w3: the NEXT launch is the odd phase (include/pdse.h)
            d.p1mask, d.Fout1 = phase1["mask"], phase1["Fout1"]
        if nx is not None:
            tiles = nx["tiles"]
            d.nx_n, d.nx_keep, d.nx_row0 = len(tiles), 1 if nx.get("keep") else 0, nx.get("row0", -1)
            for i, tl in enumerate(tiles):
                if tl.get("bias") is not None:
                    d.nx_bias[i] = Ctx.ptr(tl["bias"], tl.get("bias_off", 0))
                d.nx_bias_sb[i] = tl.get("bias_sb", 0)
                d.nx_out[i] = Ctx.ptr(tl["out"])
                d.nx_sb[i], d.nx_sc[i], d.nx_st[i], d.nx_sf[i] = tl["strides"]
                d.nx_off[i] = tl.get("off", 0)
                d.nx_add[i] = Ctx.ptr(tl.get("add"))
        d.resid = Ctx.ptr(resid)
        d.out = Ctx.ptr(out)
        d.out_sb, d.out_sc_hi, d.out_sc_lo, d.out_st, d.out_sf = out_strides
        d.out_off, d.out_cr = out_off, out_cr
        d.B, d.Tout, d.Fout = B, Tout, Fout
        d.flat = 1 if flat and s3g and d.korder in (3, 5) else 0
        self.add(d, tag)
        return d


def nchw(C_, T, F):
    """(sb, sc, st, sf) of a contiguous [B, C, T, F] tensor."""
    return C_ * T * F, T * F, F, 1


def nchw_out(C_, T, F):
    """(out_sb, out_sc_hi, out_sc_lo, out_st, out_sf) of a contiguous [B, C, T, F] output."""
    return C_ * T * F, T * F, 0, F, 1


def nc8(C_, T, F):
    """(sb, sc, st, sf) of a channel-blocked [B, C/8, T, F, 8] tensor (pdse_src.blk = 8: sc is the stride of a block)."""
    return C_ * T * F, T * F * 8, F * 8, 8


def nc8_out(C_, T, F):
    """(out_sb, out_sc_hi, out_sc_lo, out_st, out_sf) of the same tensor as an output (out_cr = 8)."""
    return C_ * T * F, T * F * 8, 1, F * 8, 8


# ==========================================================================
# DiffUNet1 / DiffUNet
# ==========================================================================
class EpsNetPlan(PlanBase):
    """ε-network (``time_cond=True``) or prior DiffUNet (``time_cond=False``).

    Buffers: x, x_init (inputs, [B,2,T,161]); t ([nsteps][B] steps); eps / out ([B,2,T,161]).
    ``build_step(i)`` appends the operators of one forward at diffusion step row i.
    """

    ENC_F = [161, 79, 39, 19, 9, 4]
    fused_tcm = True        # one launch per TCM residual block (csrc/tcm.hip); False: three gather-GEMM launches
    chain_conv1 = True      # every stage's 1x1 input convolution rides on the previous stage's tail (pdse.h: nx_*)
    compose_stage1 = True   # (with chain_conv1) encoder stage 1: conv1 composed into the gather weights
    # BIGLU blocks on the bf16 matrix cores with exact 3-way operand splits (csrc/gconv3.hip): fp32-level accuracy
    # (same goldens, same tolerances) at 16/6 of the fp32 MFMA rate.  False: v_mfma_f32_32x32x2_f32 throughout.
    split_bf16 = True
    split_tcm = True        # (with split_bf16 and fused_tcm) TCM blocks on the bf16 matrix cores too (csrc/tcm2.hip)
    # (with split_bf16, chain_conv1, compose_stage1, DiffUNet1 only, PReLU slopes <= 1) the BIGLU blocks on PLANE tensors
    # (csrc/bglu.hip): the conv1 outputs travel between launches as bf16 split planes written once by their producer.
    # True: every stage (10-20 % faster than csrc/gconv3.hip per launch, profiles/r03_bglu_forms.txt; the only form of the
    # bf16 mode); False: csrc/gconv3.hip throughout (fp32 conv1 tensors, split in every tap).
    plane_h = True
    # the 18 residual blocks of the TCM stack as ONE persistent launch (pdse_tcm2s_desc, csrc/tcm2.hip: tcm2s_kernel) instead of
    # 18: same kernels' arithmetic, bit-identical results, no launch boundary between dependent 16 us blocks.  Used by plans
    # built with exclusive=True (see __init__).
    tcm_stack = True
    parity_planes = True    # the encoders' plane tensors with their bins split by parity (contiguous stride-2 taps; pdse_bglu_desc.hp_par)
    # operand planes of the block kernels (csrc/bglu.hip) and of their plane tensors - 3: exact three-way bf16 split, six bf16 products
    # per multiply-add; 2: fp16 hi + lo of the power-of-two scaled operand ("f16x2": within half an fp32 ulp inside the fp16 window,
    # three f16 products; include/pdse.h PDSE_F16_ACT_EXP) - both fp32-equivalent, held to the same goldens and tolerances;
    # 1: plain bf16 operands (the opt-in bf16 mode, its own tolerance).  Default since round 4: 2 (profiles/r04_*: the same launches
    # in 0.69 of the three-plane form's time, parity margins equal or better)
    planes = 2
    TCM_F16 = True          # with planes 2 the TCM stack runs its two-plane form too (False: it keeps the three-plane split)
    TCM_STACKS, TCM_DILATIONS = 3, (1, 2, 4, 8, 16, 32)   # model/diff3.py:260-277: 3 x residual(d = 1 .. 32)
    NSLOT = 20  # 15 stages + en1 real-row bias + 4 composed encoder-stage-1 biases (l/r x frame >= 1 / frame 0)

    def __init__(self, ctx, sd, B, T, time_cond=True, nsteps=1, plan=None, table=None, with_pre=None, split_bf16=None,
                 planes=None, plane_h=None, exclusive=False, frames=None):
        """with_pre False + time_cond True: ``Nocon`` (model/piror_grad.py), DiffUNet1 without Preprocess.
        frames: device int32 [B] owned by the caller, every utterance's own frame count (exact ragged batches): the TCM launches
        are recorded with the table and zero their bottleneck tensor from an utterance's own end on - the only place where this
        network looks forward in time (the BiConv(Trans)GLU blocks look back one frame).  None: the dense launches.
        exclusive: the plan owns the GPU while it runs (one batch in flight): the TCM stack then runs as one persistent launch
        (``tcm_stack``; bit-identical results).  With several batches in flight the persistent workgroups keep CUs from the other
        batches' block kernels while they wait for their neighbours - measured 17.8 instead of 17.4 ms per pass - so the
        in-flight runners keep one launch per block.
        split_bf16: run the BIGLU blocks on the bf16 matrix cores with exact 3-way operand splits (None: class default).
        planes 1: the opt-in bf16 mode (plain bf16 operands and bf16 block-boundary tensors; implies plane_h True)."""
        with_pre = time_cond if with_pre is None else with_pre
        if split_bf16 is not None:
            self.split_bf16 = bool(split_bf16)
        if planes is not None:
            if int(planes) not in (1, 2, 3):
                raise ValueError("planes is 3 (bf16x3), 2 (f16x2) or 1 (bf16 mode)")
            self.planes = int(planes)
        if plane_h is not None:
            self.plane_h = bool(plane_h)
        if self.planes == 1:
            self.plane_h = True
        self.tcm_planes = 3 if (self.planes == 2 and not self.TCM_F16) else self.planes
        self.use_tcm_stack = bool(self.tcm_stack and exclusive)
        self.frames = frames
        if frames is not None and (self.force_generic or not self.fused_tcm):
            raise ValueError("exact ragged batches need a fused TCM form (csrc/tcm.hip, csrc/tcm2.hip): the three-launch form has no frames table")
        self.sd = sd
        ok = (self.split_bf16 and self.chain_conv1 and self.compose_stage1 and time_cond and with_pre and not self.force_generic
              and all(float(P._np(sd[k])[0]) <= 1.0 for k in sd if k.endswith(".weight") and P._np(sd[k]).shape == (1,)))
        if not ok:
            if self.planes == 1:
                raise ValueError("bf16 mode needs the chained split-bf16 DiffUNet1 path (PReLU slopes <= 1)")
            self.plane_h = False
            if self.planes == 2:       # the csrc/gconv3.hip fallback knows the three-plane split only
                self.planes = self.tcm_planes = 3
        super().__init__(ctx, plan, ns=(ctx.bank.token(sd), bool(time_cond), bool(with_pre), self.fused_tcm, self.chain_conv1,
                                        self.compose_stage1, self.split_bf16, self.split_tcm,
                                        ctx.bank.token(table), str(self.plane_h), self.planes, self.parity_planes))
        self.sd, self.B, self.T, self.time_cond, self.nsteps = sd, B, T, time_cond, nsteps
        self.with_pre = with_pre
        a = ctx.alloc
        self.x = a(B, 2, T, F0)
        self.x_init = a(B, 2, T, F0) if self.with_pre else None
        self.out = a(B, 2, T, F0)
        self.H = a(B, 32, T + 1, F0)                 # conv1 output of the current block (+ explicit pad frame)
        self.H2 = a(B, 32, T + 1, F0)                # ... of the next block, written by the current block's tail (chain_conv1)
        # skip halves of the decoders' conv1 (+ time bias), produced by the encoder tails: [real|imag][stage 1..4]
        self.Pskip = [[None] + [a(B + 1, 32, T, self.ENC_F[k]) for k in range(1, 5)] for _ in range(2)]   # + the dump item of csrc/bglu.hip
        self.zero32 = self.upw("zero32", lambda: np.zeros(32))
        self.en = [a(B, 64, T, f) for f in self.ENC_F[1:5]] + [a(B, 64, 4, T)]  # en5 stored [B,64,4,T]
        self.tcm_a, self.tcm_b = a(B, 256, T), a(B, 256, T)
        self.tcm_h, self.tcm_g = a(B, 64, T), a(B, 64, T)
        # the same bottleneck tensor as the split-bf16 blocks exchange it (pdse_tcm2_desc.hs; its margins stay zero)
        self.tcm_hs = [ctx.alloc_u16(*P.tcm2_hs_shape(B, T, self.tcm_planes)) for _ in range(2)]
        self._tcm_stack = None
        self.tcm_flags = torch.zeros(B * ((T + 31) // 32), dtype=torch.int32, device=ctx.device)   # progress counters of the stack launch
        self.tcm_status = torch.zeros(4, dtype=torch.int32, device=ctx.device)                     # [0]: 0, or block + 1 a workgroup gave up at
        ctx.keep += [self.tcm_flags, self.tcm_status]
        self.dec = [a(B, 64, T, 79), a(B, 64, T, 79)]  # ping-pong decoder activations (largest F=79)
        if self.plane_h:
            # plane tensors of the conv1 outputs (include/pdse.h: hp), one per stage so that their margins stay zero:
            # encoder stages 2..5 (input bins 79, 39, 19, 9), decoder stages 5..1 (4, 9, 19, 39, 79; shared by both decoders)
            # (B + 1 items: item B takes the stores of lanes beyond the last position)
            self.hp_en = {k: ctx.alloc_u16(*P.hp_shape(B + 1, T, self.ENC_F[k - 1], self.planes)) for k in range(2, 6)}
            self.hp_de = {k: ctx.alloc_u16(*P.hp_shape(B + 1, T, self.ENC_F[k], self.planes)) for k in range(1, 6)}
            self.hp_de5b = ctx.alloc_u16(*P.hp_shape(B + 1, T, self.ENC_F[5], self.planes))   # stage 5 of the second decoder (both conv1 are computed by one launch)
            for k, t_ in self.hp_en.items():
                self.named("hp_en%d" % k, t_)
            for k, t_ in self.hp_de.items():
                self.named("hp_de%d" % k, t_)
            self.named("hp_de5b", self.hp_de5b)
        # what the f16x2 kernels read besides the plane tensors: the inputs of encoder stage 1, the TCM residual stream, hs
        for name, t_ in (("x", self.x), ("x_init", self.x_init), ("en5", self.en[4]), ("tcm_a", self.tcm_a), ("tcm_b", self.tcm_b),
                         ("tcm_hs0", self.tcm_hs[0]), ("tcm_hs1", self.tcm_hs[1])):
            if t_ is not None:
                self.named(name, t_)
        if time_cond:
            self.tsteps = a(nsteps, B, zero=True)
            self.tbias = a(nsteps, B, self.NSLOT * 32)
            self.temb = a(nsteps, B, 512)
            self._prep_time(table)

    # ---- weights helpers ------------------------------------------------
    def w(self, k):
        return P._np(self.sd[k])

    def _tcm_names(self):
        """(state_dict prefix, dilation) of every TCM residual block, in the order they run."""
        return [("TCMs.%d.residual%d" % (i, j + 1), dil) for i in range(self.TCM_STACKS) for j, dil in enumerate(self.TCM_DILATIONS)]

    def time_stages(self):
        """Every stage of the network that reaches across frames, in the order they run, as (name, frames back, frames ahead) -
        read from the layer table this builder records and from the kernel shapes in the state_dict:
          encoder stage k    Conv2d (kt, kf) behind one pad frame on top (diff3.py:144-166): kt - 1 frames back
          TCM block (p, d)   Conv1d(kernel K, dilation d, padding (K - 1) / 2 * d) in both branches: (K - 1) / 2 * d either way
          decoder stage k    ConvTranspose2d (kt, kf) and Chomp_T(kt - 1) (diff3.py:298-304): kt - 1 frames back; the two decoders
                             run side by side on the same input, so a stage counts once (the larger of the two)
        The 1x1 convolutions, the folded BatchNorms, PReLU and the gates are per frame."""
        st = []
        for k in range(1, 6):
            kt = max(self.w("en.conv%d.%s.weight" % (k, br)).shape[2] for br in ("l", "r"))
            st.append(("en%d" % k, kt - 1, 0))
        for p, dil in self._tcm_names():
            K = max(self.w("%s.%s.2.weight" % (p, br)).shape[2] for br in ("mainbranch", "maskbranch"))
            if K % 2 != 1:
                raise ValueError("TCM block %s: an even kernel has no symmetric padding" % p)
            st.append((p, (K - 1) // 2 * dil, (K - 1) // 2 * dil))
        for k in (5, 4, 3, 2, 1):
            kt = max(self.w("%s.de%d.0.%s.weight" % (de, k, br)).shape[2] for de in ("de_real", "de_imag") for br in ("l", "r"))
            st.append(("de%d" % k, kt - 1, 0))
        return st

    def receptive_field(self):
        """(H_left, H_right) in frames: the stages run one behind the other, so their reaches add (``time_stages``)."""
        st = self.time_stages()
        return sum(s_[1] for s_ in st), sum(s_[2] for s_ in st)

    def _stage_fold(self):
        """Per stage k: (W1 [32,Cin], b1 [32], Wtp [Cin,512], btp [Cin])."""
        st = []
        for k in range(1, 6):
            W1 = self.w("en.conv%d.conv1.weight" % k)[:, :, 0, 0]
            st.append((W1, self.w("en.conv%d.conv1.bias" % k), "en.tp%d" % k))
        for de in ("de_real", "de_imag"):
            for k in (5, 4, 3, 2, 1):
                p = "%s.de%d.0" % (de, k)
                W1 = self.w(p + ".conv1.weight")[:, :, 0, 0].T
                st.append((W1, self.w(p + ".conv1.bias"), p + ".tp"))
        return st

    def _prep_time(self, table):
        def make():
            ctx = self.ctx
            tb = table
            if tb is None:
                # non-persistent buffer of the reference, rebuilt exactly as model/diff3.py:89-93 does (fp32 torch ops)
                steps = torch.arange(50).unsqueeze(1)
                dims = torch.arange(64).unsqueeze(0)
                tb = steps * 10.0 ** (dims * 4.0 / 63.0)
                tb = torch.cat([torch.sin(tb), torch.cos(tb)], dim=1)
            wf, bf = [], []
            for W1, b1, tp in self._stage_fold():
                Wtp, btp = self.w(tp + ".weight"), self.w(tp + ".bias")
                wf.append(W1 @ Wtp)
                bf.append(b1 + W1 @ btp)
            # slot 15: en1 real rows also carry W1 · b_preprocess (the pad row does not, diff3.py:145-147)
            W1 = self.w("en.conv1.conv1.weight")[:, :, 0, 0]
            wf.append(wf[0])
            bf.append(bf[0] + (W1 @ self.w("preprocess.conv.bias") if self.with_pre else 0.0))
            # slots 16..19: encoder stage 1 with conv1 composed into the two gather convolutions (l, r): their biases become
            #   frame >= 1:  (S0 + S1) b_real + b        frame 0:  S0 b_pad + S1 b_real + b,    S_kt = sum_kf W[:, :, kt, kf]
            # (kt = 0 reads frame t-1; for t = 0 that is the zero pad frame, whose conv1 value is the pad bias, slot 0)
            for br in ("l", "r"):
                Wg = self.w("en.conv1.%s.weight" % br)                                  # [32, 32, 2, 5]
                S0, S1 = Wg[:, :, 0].sum(-1), Wg[:, :, 1].sum(-1)
                bg = self.w("en.conv1.%s.bias" % br)
                wf += [(S0 + S1) @ wf[0], (S0 + S1) @ wf[0]]
                bf += [(S0 + S1) @ bf[15] + bg, S0 @ bf[0] + S1 @ bf[15] + bg]
            WF, BF = np.concatenate(wf, 0), np.concatenate(bf, 0)      # [NSLOT*32, 512], [NSLOT*32]
            return dict(table=ctx.up(tb.numpy()),
                        p1T=ctx.up(self.w("time_embedding.projection1.weight").T),
                        b1=ctx.up(self.w("time_embedding.projection1.bias")),
                        p2T=ctx.up(self.w("time_embedding.projection2.weight").T),
                        b2=ctx.up(self.w("time_embedding.projection2.bias")), wfT=ctx.up(WF.T), bf=ctx.up(BF))

        m = self.memo("time", make)
        self.table = m["table"]
        self.t_p1T, self.t_b1, self.t_p2T, self.t_b2, self.t_wfT, self.t_bf = (m["p1T"], m["b1"], m["p2T"], m["b2"],
                                                                             m["wfT"], m["bf"])

    def build_time(self):
        """One launch computes the folded biases of all recorded diffusion steps."""
        d = L.TimeDesc()
        d.t, d.table = self.tsteps.data_ptr(), self.table.data_ptr()
        d.p1T, d.b1, d.p2T, d.b2 = (self.t_p1T.data_ptr(), self.t_b1.data_ptr(), self.t_p2T.data_ptr(),
                                    self.t_b2.data_ptr())
        d.wfT, d.bf = self.t_wfT.data_ptr(), self.t_bf.data_ptr()
        d.out, d.temb = self.tbias.data_ptr(), self.temb.data_ptr()
        d.B, d.NF, d.max_steps = self.nsteps * self.B, self.NSLOT * 32, 50
        self.time_index = len(self.descs)      # where the launch sits in the plan (a windowed pass runs it alone)
        self.add(d, TAG_EW)

    # ---- blocks -----------------------------------------------------------
    def _bias_for(self, step, slot):
        """(tensor-or-array, element offset, batch stride) of a stage's conv1 bias."""
        return self.tbias, (step * self.B) * self.NSLOT * 32 + slot * 32, self.NSLOT * 32

    def _biconvglu_composed(self, step, src_x, src_init, out_t, out_strides, nx):
        """Encoder stage 1 with its 1x1 conv1 (and the folded Preprocess) composed into the two (2,5) gather
        convolutions: conv1 -> l / r is linear (model/diff3.py:316-319), so l(conv1(u)) is ONE (2,5) convolution over
        the 4 input channels (x, x_init) with W'[o,i] = sum_c Wl[o,c] W1[c,i] - 40 instead of 320 k-rows, no conv1
        launch, no 32-channel H tensor.  conv1's bias (time-conditioned, different for the zero pad frame) moves into
        per-batch-item biases of l / r with a separate value for output frame 0 (slots 16..19 of the folded table)."""
        B, T = self.B, self.T
        p = "en.conv1"
        Fin, Fout = F0, (F0 - 5) // 2 + 1
        kk, taps = P.conv_taps(2, 5, 1)                                     # weight row kt reads frame t + kt - 1
        if self.time_cond:
            tb, o_l, sbb = self._bias_for(step, 16)
            _, o_l0, _ = self._bias_for(step, 17)
            _, o_r, _ = self._bias_for(step, 18)
            _, o_r0, _ = self._bias_for(step, 19)
            bias = dict(bias0=tb, bias0_off=o_l, bias0_sb=sbb, bias1=tb, bias1_off=o_r, bias1_sb=sbb, bias_t0=(tb, o_l0, o_r0))
        else:
            bias = {}

        def W():
            wk0, wk1 = P.compose_stage1(self.sd, p, kk, self.with_pre)
            w = dict(wk0=wk0, wk1=wk1, post=P.bn_fold(self.sd, "en.en1.0"), chain=P.biglu_chain(self.sd, p, 64, False),
                     nx=self._nx_weights(nx))
            if not self.time_cond:
                b1 = self.w(p + ".conv1.bias")                                  # pad frame = conv1(0) = b1 as well
                for key, br in (("bias0", "l"), ("bias1", "r")):
                    Wg = self.w("%s.%s.weight" % (p, br))
                    w[key] = Wg.sum((2, 3)) @ b1 + self.w("%s.%s.bias" % (p, br))
            return w

        self.gconv(in0=src_x, in1=src_init, Tin=T, Fin=Fin, taps=taps, sf_in=2, W=W, Cout=32, epi=L.EPI_BIGLU,
                   act=L.ACT_PRELU, act_slope=self._slope("en.en1.1.weight"), out=out_t, out_strides=out_strides,
                   B=B, Tout=T, Fout=Fout, tag=TAG_EPS_BLOCK, nx=nx, label="en1c", s3=self.split_bf16, **bias)
        return Fout

    def _slope(self, key):
        return self.memo("slope:" + key, lambda: float(self.w(key)[0]))

    @staticmethod
    def _nx_weights(nx):
        """Weight side of the chained tiles: dict(w, bias) per tile, evaluated inside a W() thunk."""
        if nx is None:
            return None
        return [dict(w=tl["wfn"](), bias=tl["bfn"]() if tl.get("bfn") else None) for tl in nx["tiles"]]

    def _biconvglu(self, step, k, src_x, src_init, Fin, out_t, out_strides, H=None, do_conv1=True, nx=None):
        """Encoder stage k (model/diff3.py:144-166 + :307-326 + BN + PReLU).  do_conv1 False: H already holds this
        stage's conv1 output (chained onto the previous stage's tail); nx: 1x1 tiles chained onto this stage's tail."""
        B, T = self.B, self.T
        H = self.H if H is None else H
        p = "en.conv%d" % k
        kw = 5 if k == 1 else 3
        Fout = (Fin - kw) // 2 + 1

        def W1():
            W1 = self.w(p + ".conv1.weight")[:, :, 0, 0]                       # [32, Cin]
            if k == 1 and self.with_pre:
                W1 = W1 @ self.w("preprocess.conv.weight")[:, :, 0, 0]          # [2, 4]: fold Preprocess into conv1
            w = dict(wk0=W1.T)
            if not self.time_cond:
                w["bias0"] = self.w(p + ".conv1.bias")
            return w

        if self.time_cond:
            tb, off_real, sbb = self._bias_for(step, 15 if k == 1 else k - 1)
            _, off_pad, _ = self._bias_for(step, k - 1)
            bias0, pad = tb, tb
        else:
            bias0, pad, off_real, off_pad, sbb = None, None, 0, 0, 0
        # H = conv1 output with an explicit frame -1 in row 0: the reference pads the input with one
        # zero frame on top and THEN adds the time bias (diff3.py:146-147), so that frame is
        # conv1(0 + tp) = the folded bias.  Rows 1..T hold the real frames.
        HT = T + 1
        h_out = (32 * HT * Fin, HT * Fin, 0, Fin, 1)
        if not do_conv1:
            pass
        elif k == 1 and self.time_cond:
            # real frames carry W1*b_preprocess in their bias (slot 15), the pad frame does not (slot 0)
            self.gconv(in0=src_x, in1=src_init, Tin=T, Fin=Fin, taps=[(0, 0)], sf_in=1, W=W1, Cout=32,
                       bias0=bias0, bias0_off=off_real, bias0_sb=sbb, out=H, out_strides=h_out, out_off=Fin,
                       B=B, Tout=T, Fout=Fin, tag=TAG_EPS_CONV1, label="en1.conv1")
            # the pad frame: one output frame whose only tap reads outside the input (zero) -> the folded pad bias
            self.gconv(in0=src_x, in1=src_init, Tin=T, Fin=Fin, taps=[(-(1 << 20), 0)], sf_in=1, W=W1, Cout=32,
                       bias0=pad, bias0_off=off_pad, bias0_sb=sbb, out=H, out_strides=h_out,
                       B=B, Tout=1, Fout=Fin, tag=TAG_EPS_CONV1, label="en1.pad")
        else:
            # same bias for every frame: one launch over T+1 output frames reading input frame r-1
            self.gconv(in0=src_x, in1=src_init, Tin=T, Fin=Fin, taps=[(-1, 0)], sf_in=1, W=W1, Cout=32,
                       bias0=bias0, bias0_off=off_real, bias0_sb=sbb, out=H, out_strides=h_out,
                       B=B, Tout=HT, Fout=Fin, tag=TAG_EPS_CONV1, label="en%d.conv1" % k)
        kk, taps = P.conv_taps(2, kw, 0)            # H row r = frame r-1: weight row kt reads H row t + kt

        def W():
            return dict(wk0=P.conv_kmat(self.sd[p + ".l.weight"], kk), wk1=P.conv_kmat(self.sd[p + ".r.weight"], kk),
                        bias0=self.w(p + ".l.bias"), bias1=self.w(p + ".r.bias"), post=P.bn_fold(self.sd, "en.en%d.0" % k),
                        chain=P.biglu_chain(self.sd, p, 64, False), nx=self._nx_weights(nx))

        self.gconv(in0=self.src(H, 32, *nchw(32, HT, Fin)), Tin=HT, Fin=Fin, taps=taps, sf_in=2, W=W,
                   Cout=32, epi=L.EPI_BIGLU, act=L.ACT_PRELU, act_slope=self._slope("en.en%d.1.weight" % k),
                   out=out_t, out_strides=out_strides, B=B, Tout=T, Fout=Fout, tag=TAG_EPS_BLOCK, nx=nx, label="en%d" % k,
                   s3=self.split_bf16)
        return Fout

    def _biconvtransglu(self, step, slot, p, k, in0, in1, Fin, out_t, out_strides_fn, bn_prefix, prelu_key, out_off=0,
                        H=None, do_conv1=True, nx=None):
        """Decoder stage (model/diff3.py:205-212 + :329-351, last frame chomped, BN, PReLU).  do_conv1 / nx as in
        ``_biconvglu``."""
        B, T = self.B, self.T
        H = self.H if H is None else H
        kw = 5 if k == 1 else 3
        Fout = 2 * (Fin - 1) + kw
        if self.time_cond:
            tb, off, sbb = self._bias_for(step, slot)
            bias0 = tb
        else:
            bias0, off, sbb = None, 0, 0
        if do_conv1:
            def W1():
                w = dict(wk0=self.w(p + ".conv1.weight")[:, :, 0, 0])           # ConvTranspose [in 128, out 32] = k-major
                if not self.time_cond:
                    w["bias0"] = self.w(p + ".conv1.bias")
                return w

            self.gconv(in0=in0, in1=in1, Tin=T, Fin=Fin, taps=[(0, 0)], sf_in=1, W=W1, Cout=32, bias0=bias0,
                       bias0_off=off, bias0_sb=sbb, out=H, out_strides=nchw_out(32, T, Fin), B=B, Tout=T,
                       Fout=Fin, tag=TAG_EPS_CONV1, label=p + ".conv1")
        C2 = 64 if k > 1 else 1
        osb, osc, _, ost, osf = out_strides_fn(Fout)
        common = dict(Cout=32, epi=L.EPI_BIGLU, act=L.ACT_PRELU if prelu_key else L.ACT_NONE,
                      act_slope=self._slope(prelu_key) if prelu_key else 0.0, out=out_t,
                      out_strides=(osb, osc, 0, ost, 2 * osf), B=B, Tout=T, tag=TAG_EPS_BLOCK)
        src_h = self.src(H, 32, *nchw(32, T, Fin))
        kk0, taps0 = P.convT_phase_taps(2, kw, 0)
        kk1, taps1 = P.convT_phase_taps(2, kw, 1)

        def Wph(kk, with_odd, nx_):
            def W():
                w = dict(wk0=P.convT_kmat(self.sd[p + ".l.weight"], kk), wk1=P.convT_kmat(self.sd[p + ".r.weight"], kk),
                         bias0=self.w(p + ".l.bias"), bias1=self.w(p + ".r.bias"),
                         post=P.bn_fold(self.sd, bn_prefix) if bn_prefix else None, chain=P.biglu_chain(self.sd, p, C2, True),
                         nx=self._nx_weights(nx_))
                if with_odd:
                    w.update(wk2=P.convT_kmat(self.sd[p + ".l.weight"], kk1), wk3=P.convT_kmat(self.sd[p + ".r.weight"], kk1),
                             ntaps1=len(taps1))
                return w
            return W

        if not self.force_generic:
            # both output phases in one launch: the odd bins read a subset of the even bins' taps, so the
            # activation loads are shared and every wave stores neighbouring (2j, 2j+1) bins together
            mask = sum(1 << taps0.index(tp) for tp in taps1)
            self.gconv(in0=src_h, Tin=T, Fin=Fin, taps=taps0, sf_in=1, W=Wph(kk0, True, nx), out_off=out_off,
                       Fout=(Fout + 1) // 2, phase1=dict(mask=mask, Fout1=Fout // 2), nx=nx, label=p,
                       s3=self.split_bf16, **common)
        else:
            for phase, (kk, taps) in enumerate(((kk0, taps0), (kk1, taps1))):
                self.gconv(in0=src_h, Tin=T, Fin=Fin, taps=taps, sf_in=1, W=Wph(kk, False, None),
                           out_off=phase * osf + out_off, Fout=(Fout - phase + 1) // 2, label=p, **common)
        return Fout

    def _tcm_conv1(self, p, xin, hout):
        """The 1x1 input convolution of a TCM residual block (diff3.py:223) as its own launch."""
        B, T = self.B, self.T
        self.gconv(in0=self.src(xin, 256, 256 * T, T, 0, 1), Tin=1, Fin=T, taps=[(0, 0)], sf_in=1,
                   W=lambda: dict(wk0=self.w(p + ".conv1.weight")[:, :, 0].T, bias0=self.w(p + ".conv1.bias")), Cout=64,
                   out=hout, out_strides=(64 * T, T, 0, 0, 1), B=B, Tout=1, Fout=T, tag=TAG_TCM, label=p + ".conv1")

    def _residual(self, p, dil, xin, xout):
        """TCM residual block (model/diff3.py:215-257) over [B,256,T] (T on the lanes): three launches."""
        B, T = self.B, self.T
        s64 = (64 * T, T, 0, 1)
        o256 = (256 * T, T, 0, 0, 1)    # out_sb, sc_hi, sc_lo, st, sf
        o64 = (64 * T, T, 0, 0, 1)
        self._tcm_conv1(p, xin, self.tcm_h)
        taps = [(0, (k - 2) * dil) for k in range(5)]

        def Wbr():
            kmain, kmask = P.tcm_branch_kmats(self.sd, p)
            sm, hm = P.bn_fold(self.sd, p + ".mainbranch.1")
            sk, hk = P.bn_fold(self.sd, p + ".maskbranch.1")
            xf = dict(mode=2, scale0=sm, shift0=hm, slope0=self.w(p + ".mainbranch.0.weight")[0],
                      scale1=sk, shift1=hk, slope1=self.w(p + ".maskbranch.0.weight")[0])
            return dict(wk0=kmain, wk1=kmask, bias0=self.w(p + ".mainbranch.2.bias"), bias1=self.w(p + ".maskbranch.2.bias"), xf=xf)

        self.gconv(in0=self.src(self.tcm_h, 64, *s64), Tin=1, Fin=T, taps=taps, sf_in=1, W=Wbr, Cout=64, epi=L.EPI_GLU,
                   out=self.tcm_g, out_strides=o64, B=B, Tout=1, Fout=T, tag=TAG_TCM, label=p + ".br")

        def W2():
            s2, h2 = P.bn_fold(self.sd, p + ".conv2.1")
            xf2 = dict(mode=1, scale0=s2, shift0=h2, slope0=self.w(p + ".conv2.0.weight")[0])
            return dict(wk0=self.w(p + ".conv2.2.weight")[:, :, 0].T, bias0=self.w(p + ".conv2.2.bias"), xf=xf2)

        self.gconv(in0=self.src(self.tcm_g, 64, *s64), Tin=1, Fin=T, taps=[(0, 0)], sf_in=1, W=W2, Cout=256,
                   resid=xin, out=xout, out_strides=o256, B=B, Tout=1, Fout=T, tag=TAG_TCM, label=p + ".conv2")

    def _residual_fused(self, p, dil, xin, xout, hin, hout, p_next):
        """The same block as ONE launch (csrc/tcm.hip): dilated branches + gate + conv2 + residual, and the next
        block's conv1 (``p_next``; None for the last block) chained onto the fresh x in registers (packing.tcm_fields)."""
        d = L.TcmDesc()
        self.apply(d, self.fields(p + ".fused", lambda: P.tcm_fields(self.sd, p, p_next)))
        d.x, d.h, d.x_out = xin.data_ptr(), hin.data_ptr(), xout.data_ptr()
        if p_next is not None:
            d.h_out = hout.data_ptr()
        d.dil, d.B, d.T = dil, self.B, self.T
        d.frames = Ctx.ptr(self.frames)
        self.add(d, TAG_TCM)

    def _residual_split(self, p, dil, xin, xout, hin, hout, p_next, mode=0):
        """``_residual_fused`` in split-bf16 arithmetic (csrc/tcm2.hip): the bottleneck tensor travels as the split
        planes of both branches' BN(PReLU(.)), so a block also carries the NEXT block's input transforms
        (packing.tcm2_fields).  mode 1: only ``p_next``'s conv1 on ``xin`` (the first block of the stack)."""
        npl = self.tcm_planes
        d = L.Tcm2Desc()
        self.apply(d, self.fields("%s.split%d.np%d" % (p if mode == 0 else p_next, mode, npl),
                                  lambda: P.tcm2_fields(self.sd, p, p_next, npl, mode)))
        d.x = xin.data_ptr()
        if mode == 0:
            d.x_out, d.hs = xout.data_ptr(), hin.data_ptr()
        if p_next is not None:
            d.hs_out = hout.data_ptr()
        d.dil, d.B, d.T, d.mode, d.np = dil, self.B, self.T, mode, npl
        d.frames = Ctx.ptr(self.frames)
        if mode == 0 and self._tcm_stack is not None:
            self._tcm_stack.append(d)          # collected: one pdse_tcm2s_desc for the whole stack (build_step)
        else:
            self.add(d, TAG_TCM)

    # ---- the plane path (csrc/bglu.hip) ------------------------------------------------------------------------
    def _plane_stage(self, kind):
        """Does stage ``kind`` ("enc" / "dec") run on plane tensors?  All or none: the encoder leaves the decoders' skip
        halves in the layout of the kernel that reads them (csrc/bglu.hip: groups of four channels)."""
        return self.plane_h is True

    def _bglu(self, label, make, *, hp=None, F_in=None, x0=None, x1=None, taps, sf_in, Fout, p1mask=0, Fout1=0, slope, C2,
              bias, out=None, out_strides=None, out_off=0, nx_hp=None, nx_F=None, nx_row0=False, nx_add=None,
              nx_out=(), nx_bias=(), hp_par=False, nx_par=False, skip_F=0):
        """Record one pdse_bglu_desc.  make(): -> its weight side (packing.bglu_fields; uploaded once per weight bank)."""
        B, T, npl = self.B, self.T, self.planes
        d = L.BgluDesc()
        self.apply(d, self.fields("bglu:%s:%d" % (label, npl), make))
        if hp is not None:
            shp = P.hp_shape(B + 1, T, F_in, npl)
            d.hp, d.hp_sb, d.hp_Tp, d.hp_Fp, d.hp_t0, d.hp_f0 = hp.data_ptr(), int(np.prod(shp[1:])), shp[1], shp[4], P.HP_T0, P.HP_F0
            d.hp_par = 1 if hp_par else 0
        else:
            d.x0, d.x1 = x0, x1
        d.Tin, d.Fin = T, (F_in if F_in is not None else F0)
        d.ntaps, d.sf_in = len(taps), sf_in
        for i, (dt_, df_) in enumerate(taps):
            d.tap_dt[i], d.tap_df[i] = int(dt_), int(df_)
        d.p1mask, d.Fout1 = p1mask, Fout1
        d.B, d.Tout, d.Fout, d.np = B, T, Fout, npl
        tb, o0, o1, o0t, o1t, sb = bias
        if tb is not None:                  # time-conditioned gather biases; constant ones come from make()
            d.bias0, d.bias1, d.bias_sb = Ctx.ptr(tb, o0), Ctx.ptr(tb, o1), sb
            if o0t is not None:
                d.bias0_t0, d.bias1_t0 = Ctx.ptr(tb, o0t), Ctx.ptr(tb, o1t)
        d.slope, d.C2 = float(slope), C2
        if out is not None:
            d.out = Ctx.ptr(out)
            d.out_sb, d.out_sc, d.out_st, d.out_sf = out_strides
            d.out_off = out_off
        d.skip_Fh = (skip_F + 1) // 2 if (skip_F and self.parity_planes) else 0   # bins of the skip halves split by parity
        d.nx_n = (1 if nx_hp is not None else 0) + len(nx_out)
        d.nx_items = B + 1          # what hp_shape(B + 1, ...) and the Pskip tensors hold: item B is the kernel's dump target
        assert all(t_.shape[0] == B + 1 for t_, *_ in nx_out) and (nx_hp is None or nx_hp.shape[0] == B + 1)
        if nx_hp is not None:
            shp = P.hp_shape(B + 1, T, nx_F, npl)
            d.nx_hp, d.nx_hp_sb, d.nx_Tp, d.nx_Fp, d.nx_t0, d.nx_f0 = (nx_hp.data_ptr(), int(np.prod(shp[1:])), shp[1], shp[4],
                                                                      P.HP_T0, P.HP_F0)
            d.nx_row0 = 1 if nx_row0 else 0
            d.nx_par = 1 if nx_par else 0
        if nx_add is not None:
            t_, sb_, sc_, st_, sf_ = nx_add
            d.nx_add, d.add_sb, d.add_sc, d.add_st, d.add_sf = Ctx.ptr(t_), sb_, sc_, st_, sf_
        for i, (t_, sb_, sc_, st_, sf_) in enumerate(nx_out):
            d.nx_out[i] = Ctx.ptr(t_)
            d.nx_sb[i], d.nx_sc[i], d.nx_st[i], d.nx_sf[i] = sb_, sc_, st_, sf_
        for i, (t_, off_, sb_) in enumerate(nx_bias):
            d.nx_bias[i], d.nx_bias_sb[i] = Ctx.ptr(t_, off_), sb_
        self.add(d, TAG_EPS_BLOCK)
        return d

    def _encoder_planes(self, step, x, x_init):
        """Encoder stages 1..5 on plane tensors: stage k's tail writes stage k+1's conv1 output as planes (hp_en[k+1])
        and the skip halves of both decoders' conv1 (Pskip, fp32)."""
        B, T, npl = self.B, self.T, self.planes
        sbb = self.NSLOT * 32
        tb = self.tbias

        def slot(sl):
            return self._bias_for(step, sl)[1]

        for k in range(1, 6):
            p = "en.conv%d" % k
            Fin, Fo = self.ENC_F[k - 1], self.ENC_F[k]
            kw = 5 if k == 1 else 3
            kk, taps = P.conv_taps(2, kw, 1)                                  # weight row kt reads frame t + kt - 1
            chained = k < 5
            pn = "en.conv%d" % (k + 1)

            def nx_weights(k=k, pn=pn):
                if k == 5:
                    return []
                ws = [self.w(pn + ".conv1.weight")[:, :, 0, 0]]
                for de in ("de_real", "de_imag"):
                    ws.append(self.w("%s.de%d.0.conv1.weight" % (de, k))[:, :, 0, 0].T[:, 64:])     # ConvTranspose: [in, out]
                return ws

            if k == 1:
                def make(p=p, kk=kk, nx_weights=nx_weights):
                    g = dict(zip(("w0", "w1"), P.compose_stage1(self.sd, p, kk)))
                    return P.bglu_fields(self.sd, p, False, 64, "en.en1.0", g, nx_weights(), npl, False)
                bias = (tb, slot(16), slot(18), slot(17), slot(19), sbb)
                src = dict(x0=self.src(x, 2, *nchw(2, T, F0)), x1=self.src(x_init, 2, *nchw(2, T, F0)), F_in=F0)
            else:
                def make(p=p, kk=kk, k=k, nx_weights=nx_weights):
                    g = dict(w0=P.conv_kmat(self.sd[p + ".l.weight"], kk), w1=P.conv_kmat(self.sd[p + ".r.weight"], kk))
                    return P.bglu_fields(self.sd, p, False, 64, "en.en%d.0" % k, g, nx_weights(), npl, True)
                bias = None
                src = dict(hp=self.hp_en[k], F_in=Fin, hp_par=self.parity_planes)
            kwargs = dict(taps=taps, sf_in=2, Fout=Fo, slope=self._slope("en.en%d.1.weight" % k), C2=64, **src)
            if chained:
                sk = [(self.Pskip[di][k], 32 * T * Fo, 4 * T * Fo, 4 * Fo, 4) for di in range(2)]   # [B + 1][8 groups][T][F][4]
                kwargs.update(nx_hp=self.hp_en[k + 1], nx_F=Fo, nx_row0=True, nx_out=sk, nx_par=self.parity_planes, skip_F=Fo,
                              nx_bias=[(tb, slot(k), sbb)] + [(tb, slot(5 + 5 * di + (5 - k)), sbb) for di in range(2)])
            else:
                kwargs.update(out=self.en[4], out_strides=(64 * 4 * T, 4 * T, 1, T))          # [B,64,4,T]
            self._bglu("en%d" % k, make, bias=bias or (None, 0, 0, None, None, 0), **kwargs)

    def _decoders_planes(self, step, tcm_out, out):
        """Both decoders on plane tensors.  Stage 5's conv1 (over the TCM output and the encoder's stage-5 output) is its
        own fp32 launch followed by the split into planes; every later conv1 rides on the previous stage's tail."""
        B, T, npl = self.B, self.T, self.planes
        # stage 5's conv1 of BOTH decoders over (TCM output, encoder stage-5 output) and its split into planes: one launch
        # (pdse_planes_desc.w; until round 4: a gather-GEMM launch and a split launch per decoder)
        pd = L.PlanesDesc()
        pd.in_, pd.in1 = tcm_out.data_ptr(), self.en[4].data_ptr()          # [B,64,4,T] read as [B,64,T,4]
        pd.in_sb, pd.in_sc, pd.in_st, pd.in_sf = 256 * T, 4 * T, 1, T
        shp = P.hp_shape(B + 1, T, 4, npl)
        pd.hp, pd.hp1 = self.hp_de[5].data_ptr(), self.hp_de5b.data_ptr()
        pd.hp_sb, pd.hp_Tp, pd.hp_Fp, pd.hp_t0, pd.hp_f0 = int(np.prod(shp[1:])), shp[1], shp[4], P.HP_T0, P.HP_F0
        pd.B, pd.T, pd.F, pd.np, pd.cin0, pd.cin1, pd.nd = B, T, 4, npl, 64, 64, 2
        for di, de in enumerate(("de_real", "de_imag")):
            tb, off, sbb = self._bias_for(step, 5 + 5 * di)
            pd.w[di] = self.upw("%s.de5.0.conv1.kmajor" % de, lambda de=de: self.w("%s.de5.0.conv1.weight" % de)[:, :, 0, 0]).data_ptr()   # ConvTranspose: [in, out]
            pd.bias[di], pd.bias_sb = Ctx.ptr(tb, off), sbb
        self.add(pd, TAG_EPS_CONV1)
        for di, de in enumerate(("de_real", "de_imag")):
            for n, k in enumerate((5, 4, 3, 2, 1)):
                p = "%s.de%d.0" % (de, k)
                Fin = self.ENC_F[k]
                kw = 5 if k == 1 else 3
                Fo = 2 * (Fin - 1) + kw
                kk0, taps0 = P.convT_phase_taps(2, kw, 0)
                kk1, taps1 = P.convT_phase_taps(2, kw, 1)
                mask = sum(1 << taps0.index(tp) for tp in taps1)
                C2 = 64 if k > 1 else 1
                bn = "%s.de%d.2" % (de, k) if k > 1 else None

                def make(p=p, k=k, de=de, kk0=kk0, kk1=kk1, C2=C2, bn=bn):
                    g = dict(w0=P.convT_kmat(self.sd[p + ".l.weight"], kk0), w1=P.convT_kmat(self.sd[p + ".r.weight"], kk0),
                             w2=P.convT_kmat(self.sd[p + ".l.weight"], kk1), w3=P.convT_kmat(self.sd[p + ".r.weight"], kk1))
                    nxw = [self.w("%s.de%d.0.conv1.weight" % (de, k - 1))[:, :, 0, 0].T[:, :64]] if k > 1 else []
                    return P.bglu_fields(self.sd, p, True, C2, bn, g, nxw, npl, True)

                kwargs = dict(hp=self.hp_de5b if (k == 5 and di == 1) else self.hp_de[k], F_in=Fin, taps=taps0, sf_in=1, Fout=(Fo + 1) // 2, p1mask=mask, Fout1=Fo // 2,
                              slope=self._slope("%s.de%d.3.weight" % (de, k)) if k > 1 else 1.0, C2=C2,
                              bias=(None, 0, 0, None, None, 0))
                if k > 1:
                    kwargs.update(nx_hp=self.hp_de[k - 1], nx_F=Fo, nx_add=(self.Pskip[di][k - 1], 32 * T * Fo, 4 * T * Fo, 4 * Fo, 4), skip_F=Fo,
                                  nx_bias=[(self.zero32, 0, 0)])
                else:
                    kwargs.update(out=out, out_strides=(2 * T * F0, T * F0, F0, 2), out_off=di * T * F0)
                self._bglu(p, make, **kwargs)

    def build_step(self, step=0, x=None, x_init=None, out=None):
        """Append one forward.  x / x_init / out default to the plan's own buffers.

        The first call packs and uploads the weights; later calls with the same buffers
        re-use those descriptors and only re-point the per-step time biases."""
        B, T = self.B, self.T
        x = self.x if x is None else x
        out = self.out if out is None else out
        x_init = self.x_init if x_init is None else x_init
        key = (x.data_ptr(), 0 if x_init is None else x_init.data_ptr(), out.data_ptr())
        tmpl = getattr(self, "_tmpl", None)
        if tmpl is not None and tmpl[0] == key and self.time_cond:
            _, step0, items = tmpl
            lo = self.tbias.data_ptr()
            hi = lo + self.tbias.numel() * 4
            delta = (step - step0) * B * self.NSLOT * 32 * 4
            for d, tag in items:
                d2 = type(d).from_buffer_copy(d)
                if isinstance(d2, L.GconvDesc):
                    for f in ("bias0", "bias1", "bias0_t0", "bias1_t0", "padrow"):
                        v = getattr(d2, f)
                        if v and lo <= v < hi:
                            setattr(d2, f, v + delta)
                    for i in range(d2.nx_n):
                        v = d2.nx_bias[i]
                        if v and lo <= v < hi:
                            d2.nx_bias[i] = v + delta
                elif isinstance(d2, L.PlanesDesc):
                    for i in range(2):
                        v = d2.bias[i]
                        if v and lo <= v < hi:
                            d2.bias[i] = v + delta
                elif isinstance(d2, L.BgluDesc):
                    for f in ("bias0", "bias1", "bias0_t0", "bias1_t0"):
                        v = getattr(d2, f)
                        if v and lo <= v < hi:
                            setattr(d2, f, v + delta)
                    for i in range(d2.nx_n):
                        v = d2.nx_bias[i]
                        if v and lo <= v < hi:
                            d2.nx_bias[i] = v + delta
                self.add(d2, tag)
            return out
        begin = len(self.descs)
        self._build_step(step, x, x_init, out)
        self._tmpl = (key, step, list(self.descs[begin:]))
        return out

    def _build_step(self, step, x, x_init, out):
        B, T = self.B, self.T
        s2 = nchw(2, T, F0)
        chained = self.chain_conv1 and not self.force_generic
        # encoder: stage 1 reads (x, x_init) through the folded Preprocess 1x1
        src_x = self.src(x, 2, *s2)
        src_i = self.src(x_init, 2, *s2) if self.with_pre else None
        Fin = F0
        Hc, Hn = self.H, self.H2
        for k in range(1, 6):
            if self._plane_stage("enc"):
                if k == 1:
                    self._encoder_planes(step, x, x_init)
                continue
            if k < 5:
                o, ostr = self.en[k - 1], nchw_out(64, T, self.ENC_F[k])
            else:
                o, ostr = self.en[4], (64 * 4 * T, 4 * T, 0, 1, T)           # [B,64,4,T]: channel c*4+f of [B,256,T]
            nx = None
            if chained and k < 5:
                # this stage's 64-channel output is only ever read by 1x1 convolutions - the next stage's conv1 and the
                # skip half of the two decoders' conv1 (diff3.py:343: conv1(cat(x, skip) + tp), split by linearity) -
                # so its tail evaluates those in registers and the output itself is never written
                Fo, HT = self.ENC_F[k], T + 1
                bias_of = (lambda slot: dict(zip(("bias", "bias_off", "bias_sb"), self._bias_for(step, slot)))) \
                    if self.time_cond else None
                pn = "en.conv%d" % (k + 1)
                t0 = dict(wfn=lambda pn=pn: self.w(pn + ".conv1.weight")[:, :, 0, 0], out=Hn,
                          strides=(32 * HT * Fo, HT * Fo, Fo, 1), off=Fo)
                t0.update(bias_of(k) if self.time_cond else dict(bfn=lambda pn=pn: self.w(pn + ".conv1.bias")))
                tiles = [t0]
                for di, de in enumerate(("de_real", "de_imag")):
                    pd = "%s.de%d.0" % (de, k)
                    tl = dict(wfn=lambda pd=pd: self.w(pd + ".conv1.weight")[:, :, 0, 0].T[:, 64:],   # ConvTranspose: [in, out]
                              out=self.Pskip[di][k], strides=(32 * T * Fo, T * Fo, Fo, 1))
                    tl.update(bias_of(5 + 5 * di + (5 - k)) if self.time_cond else dict(bfn=lambda pd=pd: self.w(pd + ".conv1.bias")))
                    tiles.append(tl)
                nx = dict(keep=False, row0=0, tiles=tiles)
            if chained and k == 1 and self.compose_stage1:
                Fin = self._biconvglu_composed(step, src_x, src_i, o, ostr, nx)
            else:
                Fin = self._biconvglu(step, k, src_x, src_i, Fin, o, ostr, H=Hc, do_conv1=(k == 1 or not chained), nx=nx)
            if chained:
                Hc, Hn = Hn, Hc
            src_x, src_i = self.src(o, 64, *nchw(64, T, Fin)), None
        # TCMs over [B,256,T]
        cur, nxt = self.en[4], self.tcm_a
        names = self._tcm_names()
        if self.force_generic or not self.fused_tcm:
            for p, dil in names:
                self._residual(p, dil, cur, nxt)
                cur, nxt = nxt, (self.tcm_b if nxt is self.tcm_a else self.tcm_a)
        elif self.split_bf16 and self.split_tcm:
            hcur, hnxt = self.tcm_hs
            self._residual_split(None, 1, cur, None, None, hcur, names[0][0], mode=1)
            self._tcm_stack = [] if self.use_tcm_stack else None
            for n, (p, dil) in enumerate(names):
                p_next = names[n + 1][0] if n + 1 < len(names) else None
                self._residual_split(p, dil, cur, nxt, hcur, hnxt, p_next)
                cur, nxt = nxt, (self.tcm_b if nxt is self.tcm_a else self.tcm_a)
                hcur, hnxt = hnxt, hcur
            if self._tcm_stack:
                sd_ = L.Tcm2sDesc()
                for n, blk in enumerate(self._tcm_stack):
                    sd_.blk[n] = blk
                sd_.n = len(self._tcm_stack)
                sd_.flags, sd_.status = self.tcm_flags.data_ptr(), self.tcm_status.data_ptr()
                self.add(sd_, TAG_TCM)
            self._tcm_stack = None
        else:
            # one launch per block; each also produces the next block's conv1 output (h ping-pongs: halo reads)
            hcur, hnxt = self.tcm_h, self.tcm_g
            self._tcm_conv1(names[0][0], cur, hcur)
            for n, (p, dil) in enumerate(names):
                p_next = names[n + 1][0] if n + 1 < len(names) else None
                self._residual_fused(p, dil, cur, nxt, hcur, hnxt, p_next)
                cur, nxt = nxt, (self.tcm_b if nxt is self.tcm_a else self.tcm_a)
                hcur, hnxt = hnxt, hcur
        tcm_out = cur
        # decoders
        if self._plane_stage("dec"):
            self._decoders_planes(step, tcm_out, out)
            return out
        for di, de in enumerate(("de_real", "de_imag")):
            in0 = self.src(tcm_out, 64, 256 * T, 4 * T, 1, T)               # [B,64,4,T] viewed as [B,64,T,4]
            Fin = 4
            Hc, Hn = self.H, self.H2
            for n, k in enumerate((5, 4, 3, 2, 1)):
                skip = self.en[k - 1]
                if k == 5:
                    in1 = self.src(skip, 64, 256 * T, 4 * T, 1, T)
                else:
                    in1 = self.src(skip, 64, *nchw(64, T, self.ENC_F[k]))
                p = "%s.de%d.0" % (de, k)
                if k > 1:
                    o, ooff = self.dec[n & 1], 0
                    fn = lambda Fo: nchw_out(64, T, Fo)  # noqa: E731
                    bn, pr = "%s.de%d.2" % (de, k), "%s.de%d.3.weight" % (de, k)
                else:
                    o, ooff = out, di * T * F0
                    fn = lambda Fo: nchw_out(2, T, Fo)   # noqa: E731
                    bn, pr = None, None
                nx = None
                if chained and k > 1:
                    # stage k-1's conv1 = W[:, :64] * (this stage's output) + the skip half the encoder left in Pskip
                    Fo = 2 * (Fin - 1) + 3
                    wn = lambda de=de, k=k: self.w("%s.de%d.0.conv1.weight" % (de, k - 1))[:, :, 0, 0].T[:, :64]   # noqa: E731  ConvTranspose: [in, out]
                    nx = dict(keep=False, row0=-1, tiles=[dict(wfn=wn, bias=self.zero32, out=Hn, add=self.Pskip[di][k - 1],
                                                                strides=(32 * T * Fo, T * Fo, Fo, 2))])
                Fin = self._biconvtransglu(step, 5 + 5 * di + n, p, k, in0, in1, Fin, o, fn, bn, pr, out_off=ooff, H=Hc,
                                           do_conv1=(k == 5 or not chained), nx=nx)
                if chained:
                    Hc, Hn = Hn, Hc
                in0 = self.src(o, 64, *nchw(64, T, Fin))
        return out


# ==========================================================================
# GCRN prior
# ==========================================================================
class GcrnPlan(PlanBase):
    fused_last = True       # last decoder stage + Linear(161,161) as one persistent launch (pdse_gcrnlast_desc)
    fused_glstm = True      # both LSTM layers + LayerNorm 1 as a layer wavefront, T + 2 launches (pdse_glstm_desc)
    split_bf16 = True       # gated (transposed) convolutions and the LSTM input projection as split-operand GEMMs (csrc/gconv4.hip)
    gemm_planes = 2         # ... in the f16x2 form (korder 5; 3: the three-plane bf16 split, korder 3 - both fp32-equivalent)
    block8 = True           # tensors between those GEMMs in blocks of 8 channels (16-byte gathers and stores)
    fuse_phases = True      # (f16x2 GEMMs, stages of <= 32 channels) a decoder stage's even and odd output bins as ONE launch: the
                            # even-bin descriptor names the next one as its odd phase and a plan runs the two together
                            # (csrc/gconv4.hip, bit-identical); False: the descriptors carry no mark - two launches per stage
    flat_proj = True        # (f16x2 / bf16x3 GEMMs) the LSTM input projections in the flat form (pdse_gconv_desc.flat): columns over
                            # (b, t), one gather and split per workgroup for 32 channel tiles; False: the tiled form every other
                            # GEMM convolution takes (16 channel groups gathering the same tile) - bit-identical, for A/B timing
    persist_lstm = True     # B <= PERSIST_MAX_B and a plan that owns the GPU while it runs: the grouped LSTM as ONE persistent
                            # launch with register-resident weights (pdse_glstmp_desc, csrc/lstmp.hip) instead of T + 2 launches
    chunk_proj = True       # a plan that is NOT exclusive: the layer-2 input projection out of the per-step launches, evaluated per
                            # chunk of CHUNK_TC frames (pdse_glstm_desc.tc; T + TC + 1 two-stage steps + ceil(T / TC) projection
                            # launches).  An exclusive plan keeps the three-stage wavefront: TC more steps lengthen its chain;
                            # so does a plan of fewer than 2 TC frames.
                            # On: headline 13.17 against 13.25 ms, lower in every interleaved pair (profiles/glstm_chunk_ab.md)
    CHUNK_TC = 32
    PERSIST_MAX_B = 4       # measured (tools/time_glstm.py --persist): 3.9 / 6.0 / 9.0 / 21.8 us per step at B = 1 / 2 / 4 / 8 against 11.4-12.0 for the wavefront
    ENC_C = [2, 16, 32, 64, 128, 256]
    ENC_F = [161, 80, 39, 19, 9, 4]
    carries_state = True    # every convolution has a time kernel of 1 (gcrn.py: kernel_size (1, 3)); the grouped LSTM is causal

    def receptive_field(self):
        """(0, 0): no frame of the input but t itself reaches output frame t except through the LSTM's state (``carries_state``)."""
        return 0, 0

    def __init__(self, ctx, sd, B, T, plan=None, split_bf16=None, exclusive=False, planes=None, carry_state=False):
        """planes 3 / 2: the fp32-equivalent operand splits of the GEMM-shaped convolutions (bf16x3: korder 3; f16x2: korder 5, the
        default); planes 1: the opt-in bf16 mode - the gated (transposed) convolutions and the LSTM input projection multiply plain
        bf16 operands (csrc/gconv4.hip, korder 4); tensors, LSTM and the last stage stay fp32.
        exclusive: nothing else runs on the GPU beside this plan (one batch in flight) - the condition under which the
        persistent LSTM may be used (its 256 workgroups wait for each other and must all be resident).  Off by default: a
        plan built with it takes another LSTM kernel at B <= PERSIST_MAX_B than at larger B, so an utterance's result is
        within 1e-5 of, not bit-identical to, the same utterance in a larger batch or shard.
        carry_state: the plan of one window of a long recording: the grouped LSTM takes the wavefront form, whatever
        ``exclusive`` says, and is recorded with ``state_in`` / ``state_out`` (pdse_glstm_desc: h and c of both layers and groups) -
        a run starts from what ``state_in`` holds (zeros: the start of a recording) and leaves its last frame's state in
        ``state_out``; the caller copies one into the other between windows.  False (default): the fields stay NULL."""
        self.carry_state = bool(carry_state)
        if self.carry_state:
            exclusive = False
            if not self.fused_glstm or self.force_generic:
                raise ValueError("carry_state needs the wavefront form of the grouped LSTM (csrc/lstm.hip: glstm_wave_kernel)")
        if split_bf16 is not None:
            self.split_bf16 = bool(split_bf16)
        if planes is not None:
            if planes not in (1, 2, 3) or (planes in (1, 2) and not self.split_bf16):
                raise ValueError("planes is 3 (bf16x3), 2 (f16x2) or 1 (bf16 mode); the one- and two-plane forms run on the GEMM kernels (split_bf16)")
            self.gemm_planes = int(planes)
        self.persist = bool(self.persist_lstm and self.fused_glstm and exclusive and B <= self.PERSIST_MAX_B and not self.force_generic)
        self.exclusive = bool(exclusive)
        # ... from T = 2 TC on.  The rings cost 2 TC frames whatever T is (43 MB at Bp = 32, 34 MB of it gx2): most of a short
        # plan's memory, where a second plan is meant to cost its activations only.  The chain argument points the same way but is
        # an estimate: per-launch times measured with the plan ALONE on the GPU (9.0 against 13.6 us) put the break-even of
        # (T + TC + 1 + T / TC) * 9.0 against (T + 2) * 13.6 at T = 62; the plans concerned share the GPU, where it was not measured.
        # self.chunk is deliberately not part of ns (the weight-bank key): both forms upload the same packed operands
        # (pack_glstm_wavefront).  A packer of the chunked form's own would have to enter the key.
        self.chunk = bool(self.chunk_proj and self.fused_glstm and not exclusive and not self.persist and not self.force_generic
                          and T >= 2 * self.CHUNK_TC)
        super().__init__(ctx, plan, ns=(ctx.bank.token(sd), self.fused_last, self.fused_glstm, self.split_bf16, self.block8, self.persist,
                                        self.gemm_planes))
        self.sd, self.B, self.T = sd, B, T
        a = ctx.alloc
        self.Bp = Bp = (B + 31) // 32 * 32
        self.status = None
        self.x = a(B, 2, T, F0)
        self.out = a(B, 2, T, F0)
        self.e = [a(B, self.ENC_C[i + 1], T, self.ENC_F[i + 1]) for i in range(5)]
        self.gx = a(2, T, 2048, Bp, zero=True)
        R = 2 * self.CHUNK_TC if self.chunk else 2      # chunked form: hT1, gx2 and part are rings of two chunks of frames
        self.hT = a(R, 2, 512, Bp, zero=True)
        self.cst = a(2, 512, Bp, zero=True)
        self.y = a(B, T, 1024)
        if self.persist:
            bq = 1 << (B - 1).bit_length()
            self.gran = torch.zeros(4 * 1024 * bq, dtype=torch.int64, device=ctx.device)   # {tag, value} granules, zeroed by every launch
            self.status = torch.zeros(4, dtype=torch.int32, device=ctx.device)             # [0]: 0 = completed, s + 1 = gave up at step s
            ctx.keep += [self.gran, self.status]
        elif self.fused_glstm and not self.force_generic:
            self.hT2, self.cst2 = a(2, 2, 512, Bp, zero=True), a(2, 512, Bp, zero=True)
            self.gx2, self.part = a(R, 2, 2048, Bp, zero=True), a(R, 2, 64, Bp, 2, zero=True)
            if self.carry_state:     # [4][G][H][Bp]: h1, c1, h2, c2
                self.state_in, self.state_out = a(4, 2, 512, Bp, zero=True), a(4, 2, 512, Bp, zero=True)
        else:
            self.yn = a(B, 1024, T)
        self.glstm = a(B, 256, T, 4)
        self.d = [a(B, 128, T, 9), a(B, 64, T, 19), a(B, 32, T, 39), a(B, 16, T, 80), a(B, 1, T, 161)]
        # inputs of the korder-5 GEMM convolutions (range audit): encoder outputs, the LSTM output, the decoders' stage outputs
        for i, t_ in enumerate(self.e):
            self.named("gcrn.e%d" % (i + 1), t_)
        self.named("gcrn.glstm", self.glstm)
        for i, t_ in enumerate(self.d[:4]):
            self.named("gcrn.d%d" % (5 - i), t_)
        self.named("gcrn.x", self.x)

    def w(self, k):
        return P._np(self.sd[k])

    def _nchw(self, t, blocked):
        if blocked and self.split_bf16 and not self.force_generic and self.block8:
            B, C_, T, F = t.shape
            return t.view(B, C_ // 8, T, F, 8).permute(0, 1, 4, 2, 3).reshape(B, C_, T, F)
        return t

    def enc_out(self, k):
        """Encoder stage k's output (k = 1..5) as [B, C, T, F], whatever layout the plan keeps it in (build())."""
        return self._nchw(self.e[k - 1], k >= 2)

    def glstm_out(self):
        """The grouped LSTM's output after LayerNorm 2 as [B, 256, T, 4]."""
        return self._nchw(self.glstm, True)

    def _lstm_proj(self, layer, proj, gx_lay):
        """The input projections of one LSTM layer's two groups as batched GEMMs into gx.  proj(g) -> (source, Tin, Fin, taps,
        W_ih -> k-major matrix, Tout, Fout, frame stride, bin stride of gx); gx_lay: (batch, gate-row) strides of gx -
        (1, Bp): [G][T][4H][Bp] for the per-frame kernel, (2048, 1): [G][T][Bp][4H] for the fused forms (pdse_glstm_desc.gx1)."""
        B, T, Bp = self.B, self.T, self.Bp
        for g in range(2):
            p = "glstm.%s.%d." % (layer, g)
            in0, Tin, Fin, taps, wk_fn, Tout, Fout, ost, osf = proj(g)
            self.gconv(in0=in0, Tin=Tin, Fin=Fin, taps=taps, sf_in=1, Cout=2048,
                       W=lambda p=p, wk_fn=wk_fn: dict(wk0=wk_fn(self.w(p + "weight_ih_l0")),
                                                       bias0=self.w(p + "bias_ih_l0") + self.w(p + "bias_hh_l0")),
                       out=self.gx, out_strides=gx_lay + (0, ost, osf), out_off=g * T * 2048 * Bp, B=B, Tout=Tout, Fout=Fout,
                       tag=TAG_PRIOR, label=p + "ih", s3g=self.split_bf16,
                       flat=self.flat_proj and Fout == 1 and len(taps) * in0.C <= 512)

    def _lstm_layer(self, layer, xproj_src_fn, y_su, y_sg):
        B, T, Bp = self.B, self.T, self.Bp
        self._lstm_proj(layer, xproj_src_fn, (1, Bp))

        def pack_whh():
            return P.pack_lstm_whh([self.w("glstm.%s.%d.weight_hh_l0" % (layer, g)) for g in range(2)])   # [2048, 512], gate order i,f,g,o

        d = L.LstmDesc()
        d.gx, d.whh = self.gx.data_ptr(), self.upw(layer + ".whh", pack_whh).data_ptr()
        d.hT, d.cst, d.y = self.hT.data_ptr(), self.cst.data_ptr(), self.y.data_ptr()
        d.y_sb, d.y_st, d.y_su, d.y_sg = T * 1024, 1024, y_su, y_sg
        d.B, d.Bp, d.T, d.H, d.G = B, Bp, T, 512, 2
        self.add(d, TAG_LSTM)

    def _glstm_natural(self):
        """The natural weights the fused forms pack (packing.pack_glstm_wavefront / pack_glstm_persistent)."""
        per = lambda key: [self.w("glstm.%s" % (key % g)) for g in range(2)]   # noqa: E731
        return (per("lstm_list1.%d.weight_hh_l0"), per("lstm_list2.%d.weight_ih_l0"), per("lstm_list2.%d.bias_ih_l0"),
                per("lstm_list2.%d.bias_hh_l0"), per("lstm_list2.%d.weight_hh_l0"), self.w("glstm.ln1.weight"), self.w("glstm.ln1.bias"))

    def _glstm_wavefront(self, proj1):
        """gcrn.py:22-35 as one operator (csrc/lstm.hip, glstm_wave_kernel): layer 1 at frame s, LayerNorm 1 + the
        layer-2 input projection at frame s-1, layer 2 at frame s-2, T + 2 launches.  Only the layer-1 input projection
        stays a batched GEMM in front of it."""
        B, T, Bp = self.B, self.T, self.Bp
        self._lstm_proj("lstm_list1", proj1, (2048, 1))
        d = L.GlstmDesc()
        self.apply(d, self.fields("glstm.wavefront", lambda: P.pack_glstm_wavefront(*self._glstm_natural())))
        d.gx1, d.gx2, d.part = self.gx.data_ptr(), self.gx2.data_ptr(), self.part.data_ptr()
        d.hT1, d.cst1, d.hT2, d.cst2 = self.hT.data_ptr(), self.cst.data_ptr(), self.hT2.data_ptr(), self.cst2.data_ptr()
        d.y, d.y_sb, d.y_st, d.y_su, d.y_sg = self.y.data_ptr(), T * 1024, 1024, 1, 512     # cat: index g*512 + u
        d.B, d.Bp, d.T, d.H, d.G, d.eps = B, Bp, T, 512, 2, 1e-5
        d.slices = 2 if self.exclusive else 1     # a plan that owns the GPU: two slices per workgroup share one fetch of the state (bit-identical)
        if self.chunk:                             # same packed operands: the chunk projection walks K in stage B's order
            d.tc, d.lag = self.CHUNK_TC, self.CHUNK_TC + 1
        if self.carry_state:
            d.state_in, d.state_out = self.state_in.data_ptr(), self.state_out.data_ptr()
        self.add(d, TAG_LSTM)

    def _glstm_persistent(self, proj1):
        """gcrn.py:22-35 as ONE persistent launch (csrc/lstmp.hip, pdse_glstmp_desc): layer 1 at frame s, LayerNorm 1 +
        layer 2 at frame s - 1, weights in registers, the state exchanged between the 256 workgroups every step."""
        B, T, Bp = self.B, self.T, self.Bp
        self._lstm_proj("lstm_list1", proj1, (2048, 1))
        d = L.GlstmpDesc()
        self.apply(d, self.fields("glstm.persistent", lambda: P.pack_glstm_persistent(*self._glstm_natural())))
        d.gx1, d.gran, d.status = self.gx.data_ptr(), self.gran.data_ptr(), self.status.data_ptr()
        d.y, d.y_sb, d.y_st, d.y_su, d.y_sg = self.y.data_ptr(), T * 1024, 1024, 1, 512     # cat: index g*512 + u
        d.B, d.Bp, d.T, d.H, d.G, d.eps = B, Bp, T, 512, 2, 1e-5
        self.add(d, TAG_LSTM)

    def _ln(self, name, out_t, osb, os_hi, os_lo, os_t, r, blk=0):
        d = L.LnDesc()
        d.blk = blk
        d.in_, d.out = self.y.data_ptr(), out_t.data_ptr()
        d.gamma = self.upw(name + ".g", lambda: self.w(name + ".weight")).data_ptr()
        d.beta = self.upw(name + ".b", lambda: self.w(name + ".bias")).data_ptr()
        d.osb, d.os_hi, d.os_lo, d.os_t = osb, os_hi, os_lo, os_t
        d.B, d.T, d.N, d.r, d.eps = self.B, self.T, 1024, r, 1e-5
        self.add(d, TAG_PRIOR)

    def build(self, x=None, out=None):
        B, T, Bp = self.B, self.T, self.Bp
        x = self.x if x is None else x
        out = self.out if out is None else out
        # encoder: GluConv2d k(1,3) s(1,2) + BN + ELU (gcrn.py:138-142)
        # Tensors that only the split-bf16 GEMM kernel reads (e2..e5, the decoders' d5..d3) live in blocks of 8 channels,
        # [B][C/8][T][F][8] (pdse_src.blk): its gather was bound by the texture addresser - eight 4-byte loads per lane and
        # K block, 38 memory instructions per wave and chunk at ~12 cycles each - and is two 16-byte loads per K block now.
        # e1 and d2 are also read by gcrnlast_kernel and stay [B][C][T][F].
        blk = self.split_bf16 and not self.force_generic and self.block8

        def lay(k_is_blocked, C_, Fq):
            if k_is_blocked:
                return nc8(C_, T, Fq), nc8_out(C_, T, Fq), 8
            return nchw(C_, T, Fq), nchw_out(C_, T, Fq), 1

        src = self.src(x, 2, *nchw(2, T, F0))
        e_lay = [lay(blk and k >= 2, self.ENC_C[k], self.ENC_F[k]) for k in range(1, 6)]
        for k in range(1, 6):
            ci, co, Fin, Fout = self.ENC_C[k - 1], self.ENC_C[k], self.ENC_F[k - 1], self.ENC_F[k]
            kk, taps = P.conv_taps(1, 3, 0)
            p = "conv%d" % k
            ist, ost_, ocr = e_lay[k - 1]
            self.gconv(in0=src, Tin=T, Fin=Fin, taps=taps, sf_in=2, Cout=co, epi=L.EPI_GLU, act=L.ACT_ELU,
                       W=lambda p=p, k=k, kk=kk: dict(wk0=P.conv_kmat(self.sd[p + ".conv1.weight"], kk),
                                                      wk1=P.conv_kmat(self.sd[p + ".conv2.weight"], kk),
                                                      bias0=self.w(p + ".conv1.bias"), bias1=self.w(p + ".conv2.bias"),
                                                      post=P.bn_fold(self.sd, "bn%d" % k)),
                       out=self.e[k - 1], out_strides=ost_, out_cr=ocr, B=B, Tout=T, Fout=Fout, tag=TAG_PRIOR, label=p,
                       s3g=self.split_bf16)
            src = self.src(self.e[k - 1], co, *ist, blk=8 if ocr == 8 else 0)

        # grouped LSTM (gcrn.py:22-40)
        def proj1(g):
            # group g = channels 128g..128g+127 of e5 [B,256,T,4]; k = f*128 + c'  <->  W_ih column c'*4 + f
            wk = lambda Wih: np.concatenate([Wih[:, f::4].T for f in range(4)], axis=0)   # noqa: E731
            s = self.src(self.e[4], 128, *e_lay[4][0], off=128 * g * T * 4, blk=8 if blk else 0)   # (same offset in both layouts)
            return s, T, 4, [(0, f) for f in range(4)], wk, T, 1, 2048 * Bp, 0

        if self.persist:
            self._glstm_persistent(proj1)
        elif self.fused_glstm and not self.force_generic:
            self._glstm_wavefront(proj1)
        else:
            self._lstm_layer("lstm_list1", proj1, y_su=2, y_sg=1)           # stack(dim=-1)+flatten: index u*2+g
            self._ln("glstm.ln1", self.yn, 1024 * T, T, 0, 1, 1)             # -> [B,1024,T]

            def proj2(g):
                s = self.src(self.yn, 512, 1024 * T, T, 0, 1, off=512 * g * T)
                return s, 1, T, [(0, 0)], (lambda Wih: Wih.T), 1, T, 0, 2048 * Bp

            self._lstm_layer("lstm_list2", proj2, y_su=1, y_sg=512)          # cat: index g*512+u
        if blk:
            self._ln("glstm.ln2", self.glstm, 256 * T * 4, T * 4 * 8, 8, 4 * 8, 4, blk=8)   # j = c*4+f -> [B,32,T,4,8]
        else:
            self._ln("glstm.ln2", self.glstm, 256 * T * 4, T * 4, 1, 4, 4)   # j = c*4+f -> [B,256,T,4]

        # two decoders (gcrn.py:150-164)
        dec = [(5, 512, 128), (4, 256, 64), (3, 128, 32), (2, 64, 16), (1, 32, 1)]
        for br in (1, 2):
            in0 = self.src(self.glstm, 256, *(nc8(256, T, 4) if blk else nchw(256, T, 4)), blk=8 if blk else 0)
            in1 = self.src(self.e[4], 256, *e_lay[4][0], blk=8 if blk else 0)
            Fin = 4
            for n, (k, ci, co) in enumerate(dec):
                p = "conv%d_t_%d" % (k, br)
                Fout = 2 * (Fin - 1) + 3 + (1 if k == 2 else 0)
                if k == 1 and self.fused_last and not self.force_generic:
                    # last stage (one output channel) + Linear(161,161) in one persistent launch (csrc/misc.hip)
                    g = L.GcrnLastDesc()
                    self.apply(g, self.fields(p + ".last", lambda p=p, br=br: P.gcrn_last_fields(self.sd, p, br)))
                    g.in0, g.in1 = self.d[3].data_ptr(), self.e[0].data_ptr()
                    g.out, g.out_sb = Ctx.ptr(out, (br - 1) * T * F0), 2 * T * F0
                    g.B, g.T = B, T
                    self.add(g, TAG_PRIOR)
                    break
                dblk = blk and k >= 3          # d5, d4, d3 (read by the next decoder stage only)
                fuse = self.fuse_phases and self.split_bf16 and self.gemm_planes == 2 and not self.force_generic   # korder 5 only
                ist, (osb, osc, olo, ost, osf), ocr = lay(dblk, co, Fout)
                for phase in (0, 1):
                    kk, taps = P.convT_phase_taps(1, 3, phase)
                    self.gconv(in0=in0, in1=in1, Tin=T, Fin=Fin, taps=taps, sf_in=1, Cout=co, epi=L.EPI_GLU, act=L.ACT_ELU,
                               W=lambda p=p, k=k, br=br, kk=kk: dict(
                                   wk0=P.convT_kmat(self.sd[p + ".conv1.weight"], kk),
                                   wk1=P.convT_kmat(self.sd[p + ".conv2.weight"], kk), bias0=self.w(p + ".conv1.bias"),
                                   bias1=self.w(p + ".conv2.bias"), post=P.bn_fold(self.sd, "bn%d_t_%d" % (k, br))),
                               out=self.d[n], out_strides=(osb, osc, olo, ost, 2 * osf), out_off=phase * osf, out_cr=ocr, B=B,
                               Tout=T, Fout=(Fout - phase + 1) // 2, tag=TAG_PRIOR, label="%s.ph%d" % (p, phase),
                               s3g=self.split_bf16, phase1=dict(mask=1, Fout1=Fout // 2) if phase == 0 and fuse and co <= 32 else None)
                Fin = Fout
                if k > 1:
                    in0 = self.src(self.d[n], co, *ist, blk=8 if dblk else 0)
                    skip = self.e[k - 2]
                    sblk = e_lay[k - 2][2] == 8
                    in1 = self.src(skip, co, *e_lay[k - 2][0], act=L.ACT_ELU, blk=8 if sblk else 0)   # elu(cat(.., skip)) re-applies ELU
            else:   # (no break: the unfused form) Linear(161,161) over the bins (gcrn.py:162-163): taps enumerate the input bin
                self.gconv(in0=self.src(self.d[4], 1, *nchw(1, T, F0)), Tin=T, Fin=F0, taps=[(0, f) for f in range(F0)],
                           sf_in=1, W=lambda br=br: dict(wk0=self.w("fc%d.weight" % br).T, bias0=self.w("fc%d.bias" % br)),
                           Cout=F0, cin1=True, out=out, out_strides=(2 * T * F0, 1, 0, F0, 0), out_off=(br - 1) * T * F0, B=B,
                           Tout=T, Fout=1, tag=TAG_PRIOR, label="fc%d" % br)
        return out


# ==========================================================================
# signal front / back end
# ==========================================================================
def feat_ns(feat_type):
    """The part of a front / back end's ``ns`` that names its compression: empty for "sqrt", whose key is the one it always had."""
    return () if feat_type == "sqrt" else (feat_type,)


class StftPlan(PlanBase):
    """wav [B,L] -> c [B], compressed spectrogram [B,2,T,161]
    (trainer/complex_ddpm_trainer.py:921-937; the compressions beside the square root: :414-435)."""

    def __init__(self, ctx, B, L_, plan=None, normalize=True, split_bf16=False, reflect_own=False, feat_type="sqrt"):
        """split_bf16: the framing GEMM on the bf16 matrix cores with exact three-way operand splits (csrc/gconv4.hip).
        reflect_own: exact ragged batches - the right-hand reflect padding sits at every utterance's own end (``lens``).
        feat_type: the compression of the magnitude behind the framing GEMM, one of ``L.FEAT_TYPES`` (``L.COMPRESS_MODE``);
        "none" records no compand launch: the raw STFT."""
        self.feat_type = L.feat_type_of(feat_type)
        super().__init__(ctx, plan, ns=("stft", bool(split_bf16)) + feat_ns(feat_type))
        self.split_bf16 = bool(split_bf16)
        if L_ <= 160:
            raise ValueError(f"utterance of {L_} samples: the centred STFT reflects 160 samples on each side (torch.stft "
                             "raises for the same input)")
        self.B, self.L = B, L_
        self.T = 1 + L_ // 160
        self.wav = ctx.alloc(B, L_)
        self.xpad = ctx.alloc(B, L_ + 320)
        self.c = ctx.alloc(B)
        self.lens = torch.full((B,), L_, dtype=torch.int32, device=ctx.device)   # true lengths of zero-padded utterances
        ctx.keep.append(self.lens)
        self.feat = ctx.alloc(B, 2, self.T, F0)
        self.normalize = normalize
        self.reflect_own = bool(reflect_own)

    def build(self, feat=None, prep=True):
        """prep False: ``xpad`` is filled by the caller (the label leg of a validation pass: pdse_pair_prep, which a plan cannot
        record) and the plan starts at the framing GEMM."""
        B, L_, T = self.B, self.L, self.T
        feat = self.feat if feat is None else feat
        if prep:
            d = L.WavprepDesc()
            d.wav, d.xpad, d.c, d.lens = self.wav.data_ptr(), self.xpad.data_ptr(), self.c.data_ptr(), self.lens.data_ptr()
            d.B, d.L, d.pad, d.normalize = B, L_, 160, 1 if self.normalize else 0
            d.reflect_own = 1 if self.reflect_own else 0
            self.add(d, TAG_SIGNAL)
        Lp = L_ + 320
        # a frame's 320 samples as 320 "channels" of stride 1 at position 160 j: one GEMM [B T, 320] x [320, 322] (as 320
        # taps of one channel the gather loop ran 320 tap iterations of a 1-deep contraction: 294 us at B=32, 4 s)
        self.gconv(in0=self.src(self.xpad, 320, Lp, 1, 0, 1), Tin=1, Fin=Lp, taps=[(0, 0)],
                   sf_in=160, W=lambda: dict(wk0=P.stft_kmat(320)), Cout=2 * F0, out=feat, label="stft",
                   out_strides=(2 * T * F0, T * F0, 1, 0, F0), out_cr=F0, B=B, Tout=1, Fout=T, tag=TAG_SIGNAL,
                   s3g=self.split_bf16)
        mode = L.COMPRESS_MODE[self.feat_type]
        if mode is not None:
            c = L.CompandDesc()
            c.in_, c.out, c.plane, c.B, c.mode = feat.data_ptr(), feat.data_ptr(), T * F0, B, mode
            self.add(c, TAG_SIGNAL)
        return feat


class IstftPlan(PlanBase):
    """compressed spectrogram [B,2,T,161] -> wav [B,L] * c
    (trainer/complex_ddpm_trainer.py:1004-1016; the decompressions beside the square: utils/metrics.py:534-551)."""

    def __init__(self, ctx, B, T, L_, plan=None, split_bf16=False, frames=None, lens=None, feat_type="sqrt"):
        """frames, lens: device int32 [B] owned by the caller (exact ragged batches): the overlap-add takes an utterance's own
        frames only and writes zeros behind its own samples.
        feat_type: the decompression in front of the GEMM, one of ``L.FEAT_TYPES`` (``L.DECOMPRESS_MODE``); "normal" and "none"
        record the copy mode: nothing is decompressed, but the GEMM reads the frame-major rows the launch writes."""
        self.feat_type = L.feat_type_of(feat_type)
        super().__init__(ctx, plan, ns=("istft", bool(split_bf16)) + feat_ns(feat_type))
        self.frames_tab, self.lens_tab = frames, lens
        self.split_bf16 = bool(split_bf16)
        self.B, self.T, self.L = B, T, L_
        self.spec = ctx.alloc(B, 2, T, F0)
        # decompressed spectrogram, frame-major rows [re 0..160, 7 zeros | im 0..160, 7 zeros]: the GEMM's K axis
        self.dec = ctx.alloc(B, T, 2 * P.ISTFT_ROW, zero=True)
        self.frames = ctx.alloc(B, 320, T)
        self.wav = ctx.alloc(B, L_)
        self.win2 = self.upw("win2", lambda: P.hann_periodic(320) ** 2)

    def build(self, spec=None, c=None):
        B, T = self.B, self.T
        spec = self.spec if spec is None else spec
        cd = L.CompandDesc()
        cd.in_, cd.out, cd.plane, cd.B, cd.mode = spec.data_ptr(), self.dec.data_ptr(), T * F0, B, L.DECOMPRESS_MODE[self.feat_type]
        K = 2 * P.ISTFT_ROW
        cd.out_sb, cd.out_sc, cd.out_st, cd.F = T * K, P.ISTFT_ROW, K, F0
        self.add(cd, TAG_SIGNAL)
        self.gconv(in0=self.src(self.dec, K, T * K, 1, K, 0), Tin=T, Fin=1, taps=[(0, 0)],
                   sf_in=1, W=lambda: dict(wk0=P.istft_kmat_rows(320)), Cout=320, out=self.frames, out_strides=(320 * T, T, 0, 1, 0),
                   B=B, Tout=T, Fout=1, tag=TAG_SIGNAL, label="istft", s3g=self.split_bf16)
        o = L.OlaDesc()
        o.frames, o.win2, o.c, o.out = (self.frames.data_ptr(), self.win2.data_ptr(), Ctx.ptr(c), self.wav.data_ptr())
        o.B, o.T, o.L, o.n_fft, o.hop = B, T, self.L, 320, 160
        o.nframes, o.lens = Ctx.ptr(self.frames_tab), Ctx.ptr(self.lens_tab)
        self.add(o, TAG_SIGNAL)
        return self.wav


# ==========================================================================
# DB-AIAT prior  aia_complex_trans_ri  (model/dbaiat.py:450-478)
# ==========================================================================
class AiaPlan(PlanBase):
    """dense_encoder -> AIA_Transformer (4 x {row over bins, col over frames}) -> AHAM ->
    two dense_decoders.  Convolutions / Linear layers run on the gather-GEMM kernels, the rest
    on the operators of csrc/aia.hip."""

    FH = 80  # bins after the stride-2 encoder conv
    fused_gru_input = True   # d_model 32: W_ih x inside the GRU kernel (csrc/aia.hip, gru_kernel<64, true>)
    split_gru = True         # (with split_bf16 and the fused form) that recurrence on split-bf16 operands (csrc/gru3.hip)
    split_bf16 = True        # dilated dense blocks and the strided / sub-pixel convolutions as split-bf16 GEMMs (csrc/gconv4.hip)
    dense_fused = True       # (with split_bf16) a dense-block layer = ONE launch on a channel-blocked buffer (csrc/dense.hip)
    gemm_planes = 2          # operand form of those GEMMs: f16x2 (csrc/dense.hip np 2, csrc/gconv4.hip korder 5); 3: the three-plane bf16 split
    TPAD, G = 8, 40          # leading zero frames (the largest dilation) and 8-channel groups of the dense buffers

    def __init__(self, ctx, sd, B, T, plan=None, d=32, split_bf16=None, planes=None, frames=None):
        """d: d_model of the transformer layers (32: AIA_Transformer(64, 64); 64: AIA_Transformer_merge(128, 64)).
        frames: exact ragged batches - device int32 [B], every utterance's own frames.  It goes to the four operators through
        which padding frames could reach an utterance's own, and only to their instances that run along the frames: the column
        layers' attention and bidirectional GRU (``seqlen``), the GroupNorm statistics of the layer update and the AHAM average
        pool (``frames``, ``per_frame`` = 80 bins).  Everything else is per frame, per position or causal in time (DESIGN.md
        4.8).  None: every table NULL, the dense plan."""
        if split_bf16 is not None:
            self.split_bf16 = bool(split_bf16)
        if planes is not None:       # 3 / 2: bf16x3 / f16x2 (fp32-equivalent); 1: the opt-in bf16 mode - dense blocks / strided convolutions on plain bf16 operands
            if planes not in (1, 2, 3) or (planes in (1, 2) and not self.split_bf16):
                raise ValueError("planes is 3 (bf16x3), 2 (f16x2) or 1 (bf16 mode); the one- and two-plane forms run on the GEMM kernels (split_bf16)")
            self.gemm_planes = int(planes)
        self.fused = bool(self.dense_fused and self.split_bf16)
        super().__init__(ctx, plan, ns=(ctx.bank.token(sd), d, self.fused_gru_input, self.split_bf16, self.split_gru, self.gemm_planes,
                                        self.fused))
        self.sd, self.B, self.T, self.d = sd, B, T, d
        self.frames = frames
        a = ctx.alloc
        FH = self.FH
        self.x = a(B, 2, T, F0)
        self.out = a(B, 2, T, F0)
        self.tmp161 = a(B, 64, T, F0)
        self.tmp80 = a(B, 64, T, FH)
        if self.fused:
            # dense buffers [out4,out3,out2,out1,x] in blocks of 8 channels, [B][40][T + 8][F + 2][8]: the leading frames and the
            # outer bins are the convolutions' zero padding (never written)
            self.D161 = a(B, self.G, T + self.TPAD, F0 + 2, 8, zero=True)
            self.D80 = a(B, self.G, T + self.TPAD, FH + 2, 8, zero=True)
            self._d80_holds = None
            self.named("aia.D161", self.D161)     # the dense buffers: what csrc/dense.hip np 2 and the korder-5 convolutions read
            self.named("aia.D80", self.D80)
        else:
            self.D161 = a(B, 320, T, F0)            # dense buffer [out4,out3,out2,out1,x]
            self.D80 = a(B, 320, T, FH)
        self.x_ri = a(B, 64, T, FH)
        self.cur = a(B, d, T, FH)                # AIA state ("output" in dbaiat.py:138)
        self.nxt = a(B, d, T, FH)
        self.n_a, self.n_b = a(B, d, T, FH), a(B, d, T, FH)
        self.qkv = a(B, 3 * d, T, FH)
        self.att = a(B, d, T, FH)
        self.gx = a(B, 12 * d, T, FH)            # both directions x (r, z, n) x hidden 2d
        self.gy = a(B, 4 * d, T, FH)
        self.s1, self.s2 = a(B, d, T, FH), a(B, d, T, FH)
        self.br = [a(B, d, T, FH), a(B, d, T, FH)]        # row / col branch outputs
        self.outs = [a(B, 64, T, FH) for _ in range(4)]
        self.merged = a(B, 64, T, FH)
        self.gn_stats = a(B, 64, 4)
        self.means = a(4, B, 64)
        self.dec_up = a(B, 64, T, F0, zero=True)  # sub-pixel output; bin 0 is the left zero pad, never written
        self.t_a, self.t_b, self.t_c = a(B, d, FH, T), a(B, d, FH, T), a(B, d, FH, T)   # "ft" staging (frames innermost)

    def w(self, k):
        return P._np(self.sd[k])

    def _wp(self, key):
        """Device pointer of one state_dict tensor, uploaded as is."""
        return self.upw(key, lambda: self.w(key)).data_ptr()

    def _wf(self, key, idx=0):
        return self.memo("f:" + key, lambda: float(self.w(key).reshape(-1)[idx]))

    # ---- small operators ---------------------------------------------------
    def _rowln(self, src, dst, dst_sb, C_, F_, norm, prelu, dst_off=0):
        d = L.RowlnDesc()
        d.in_, d.out = src.data_ptr(), Ctx.ptr(dst, dst_off)
        d.gamma, d.beta = self._wp(norm + ".weight"), self._wp(norm + ".bias")
        d.slope = self._wp(prelu + ".weight")
        d.out_sb, d.B, d.C, d.T, d.F, d.eps = dst_sb, self.B, C_, self.T, F_, 1e-5
        self.add(d, TAG_PRIOR)

    def _swap(self, src, dst, to_ft):
        """[B,d,T,F] <-> [B,d,F,T] (tile transpose, one read + one write of a d-channel tensor)."""
        d = L.TransposeDesc()
        d.in_, d.out, d.N = src.data_ptr(), dst.data_ptr(), self.B * self.d
        d.R, d.Cc = (self.T, self.FH) if to_ft else (self.FH, self.T)
        self.add(d, TAG_PRIOR)

    def _chln(self, src, dst, norm):
        d = L.ChlnDesc()
        d.in_, d.out = src.data_ptr(), dst.data_ptr()
        d.gamma, d.beta = self._wp(norm + ".weight"), self._wp(norm + ".bias")
        d.plane, d.B, d.C, d.eps = self.T * self.FH, self.B, self.d, 1e-5
        self.add(d, TAG_PRIOR)

    def _pw(self, src_t, Cin, W, out_t, Cout, F_, resid=None, act=L.ACT_NONE, act_slope=0.0,
            in_layout="tf", out_layout="tf", label="pw"):
        """1x1 convolution / Linear over the channel axis of [B,Cin,T,F_]; W: thunk -> dict(wk0 [Cin, Cout], bias0, xf).

        Layouts: "tf" = [B,C,T,F] (bins innermost, the model's own), "ft" = [B,C,F,T] (frames
        innermost).  The row GRU and the column attention walk the axis that is strided in "tf";
        their operands are produced in "ft" so that the 32 lines of a workgroup sit next to each
        other in memory at every step.  A launch whose two sides differ iterates its lanes along t
        (coalesced on the "ft" side — the wide tensors — and scattered on the 32-channel "tf" side)."""
        T, B = self.T, self.B
        plane = T * F_
        if in_layout == "tf" and out_layout == "tf":
            self.gconv(in0=self.src(src_t, Cin, *nchw(Cin, T, F_)), Tin=T, Fin=F_, taps=[(0, 0)], sf_in=1, cin1=Cin == 1,
                       W=W, Cout=Cout, act=act, act_slope=act_slope, resid=resid, out=out_t,
                       out_strides=nchw_out(Cout, T, F_), B=B, Tout=T, Fout=F_, tag=TAG_PRIOR, label=label)
            return
        # lanes along t: the kernel's "frame" index is the bin f, its "bin" index is the frame t
        i_st, i_sf = (1, F_) if in_layout == "tf" else (T, 1)
        o_st, o_sf = (1, F_) if out_layout == "tf" else (T, 1)     # the residual is addressed like the output
        self.gconv(in0=self.src(src_t, Cin, Cin * plane, plane, i_st, i_sf), Tin=F_, Fin=T, taps=[(0, 0)], sf_in=1,
                   W=W, Cout=Cout, act=act, act_slope=act_slope, resid=resid, out=out_t,
                   out_strides=(Cout * plane, plane, 0, o_st, o_sf), B=B, Tout=F_, Fout=T, tag=TAG_PRIOR, label=label)

    # ---- the channel-blocked dense buffers (csrc/dense.hip) ---------------------------------------
    def _d_off(self, F_, g0):
        """Float offset of entry (b 0, group g0, frame 0, bin 0) of a dense buffer with F_ bins."""
        return ((g0 * (self.T + self.TPAD) + self.TPAD) * (F_ + 2) + 1) * 8

    def _d_src(self, D, F_, g0, C_):
        """C_ channels of a dense buffer from group g0 on as a channel-blocked convolution source (pdse_src.blk = 8)."""
        Tp, Fp = self.T + self.TPAD, F_ + 2
        return self.src(D, C_, self.G * Tp * Fp * 8, Tp * Fp * 8, Fp * 8, 8, off=self._d_off(F_, g0), blk=8)

    def _to_dense(self, src, D, F_, g0, norm=None, prelu=None):
        """[B,64,T,F_] channel-major -> groups g0..g0+7 of D, through LayerNorm(F_) + PReLU when ``norm`` is given."""
        Tp, Fp = self.T + self.TPAD, F_ + 2
        d = L.RowlnbDesc()
        d.in_, d.out = src.data_ptr(), Ctx.ptr(D, self._d_off(F_, g0))
        if norm is not None:
            d.gamma, d.beta, d.slope = self._wp(norm + ".weight"), self._wp(norm + ".bias"), self._wp(prelu + ".weight")
        d.in_sb, d.in_sc, d.in_st = 64 * self.T * F_, self.T * F_, F_
        d.out_sb, d.out_sg, d.out_st = self.G * Tp * Fp * 8, Tp * Fp * 8, Fp * 8
        d.B, d.C, d.T, d.F, d.eps = self.B, 64, self.T, F_, 1e-5
        self.add(d, TAG_PRIOR)

    def _dense_block_fused(self, p, D, F_):
        """dbaiat.py:605-631, one launch per layer: convolution, LayerNorm over the bins and PReLU; x is in groups 32..39."""
        kk = [(kt, kf) for kt in range(2) for kf in range(3)]
        npl = self.gemm_planes
        for i in range(1, 5):
            cin = 64 * i
            d = L.DenseDesc()
            d.D = D.data_ptr()
            wk = P.conv_kmat(self.sd["%s.conv%d.weight" % (p, i)], kk)
            qe = P.f16_wexp(wk) if npl == 2 else 0
            d.w = self.upw("%s.conv%d.dense%d" % (p, i, npl), lambda wk=wk, cin=cin, qe=qe: P.pack_dense(wk, cin, npl, qe)).data_ptr()
            d.wexp = qe
            d.bias = self._wp("%s.conv%d.bias" % (p, i))
            d.gamma, d.beta = self._wp("%s.norm%d.weight" % (p, i)), self._wp("%s.norm%d.bias" % (p, i))
            d.slope = self._wp("%s.prelu%d.weight" % (p, i))
            d.B, d.T, d.F, d.G, d.tpad = self.B, self.T, F_, self.G, self.TPAD
            d.g_in, d.cin, d.g_out = (5 - i) * 8, cin, (4 - i) * 8
            d.dil, d.np, d.eps = 2 ** (i - 1), npl, 1e-5
            self.add(d, TAG_PRIOR)

    def _dense_block(self, p, D, F_, tmp):
        """dbaiat.py:605-631.  D [B,320,T,F_] holds [out4,out3,out2,out1,x]; x is already in block 4."""
        if self.fused:
            return self._dense_block_fused(p, D, F_)
        B, T = self.B, self.T
        for i in range(1, 5):
            dil = 2 ** (i - 1)
            cin = 64 * i
            cstart = (5 - i) * 64                                    # skip = channels cstart..319
            kk = [(kt, kf) for kt in range(2) for kf in range(3)]
            taps = [((kt - 1) * dil, kf - 1) for kt, kf in kk]       # pad (1,1,dil,0): causal in time, same in bins
            self.gconv(in0=self.src(D, cin, *nchw(320, T, F_), off=cstart * T * F_), Tin=T, Fin=F_, taps=taps, sf_in=1,
                       W=lambda i=i, kk=kk: dict(wk0=P.conv_kmat(self.sd["%s.conv%d.weight" % (p, i)], kk),
                                                 bias0=self.w("%s.conv%d.bias" % (p, i))), Cout=64,
                       out=tmp, out_strides=nchw_out(64, T, F_), B=B, Tout=T, Fout=F_, tag=TAG_PRIOR,
                       label="%s.conv%d" % (p, i), s3g=self.split_bf16)
            self._rowln(tmp, D, 320 * T * F_, 64, F_, "%s.norm%d" % (p, i), "%s.prelu%d" % (p, i),
                        dst_off=(4 - i) * 64 * T * F_)
        return 0  # out4 sits in channel block 0

    def _encoder_layer(self, p, axis, src_t, dst_t):
        """TransformerEncoderLayer (dbaiat.py:66-88) along bins (axis 0) or frames (axis 1).

        Attention over frames and the GRU over bins run on "ft" operands with the kernels'
        coalesced code path (attention axis 0 / GRU axis 1 on the swapped tensor)."""
        B, T, FH, dm = self.B, self.T, self.FH, self.d
        self._chln(src_t, self.n_a, p + ".norm3")

        def Wqkv():
            Wi, bi = self.w(p + ".self_attn.in_proj_weight").copy(), self.w(p + ".self_attn.in_proj_bias").copy()
            Wi[:dm] *= (dm // 4) ** -0.5                              # q scaled by head_dim^-0.5 inside the projection
            bi[:dm] *= (dm // 4) ** -0.5
            return dict(wk0=Wi.T, bias0=bi)

        att_ft = axis == 1                                            # sequence over frames: operands in "ft"
        lay = "ft" if att_ft else "tf"
        if att_ft:
            # the whole attention sub-block runs frames-innermost: two tile transposes of 32-channel tensors
            # (in: normed input and the residual; out: the sum) instead of lane-scattered 1x1 launches
            self._swap(self.n_a, self.t_a, True)
            self._swap(src_t, self.t_b, True)
            qkv_in, res_in, s1_out = self.t_a, self.t_b, self.t_c
        else:
            qkv_in, res_in, s1_out = self.n_a, src_t, self.s1
        self._pw(qkv_in, dm, Wqkv, self.qkv, 3 * dm, FH, in_layout=lay, out_layout=lay, label=p + ".qkv")
        d = L.AttnDesc()
        d.qkv, d.out, d.B, d.E, d.heads, d.axis = self.qkv.data_ptr(), self.att.data_ptr(), B, dm, 4, 0
        d.T, d.F = (FH, T) if att_ft else (T, FH)                     # "ft": the innermost axis is the sequence either way
        if att_ft:
            d.seqlen = Ctx.ptr(self.frames)                           # keys of an utterance's own frames only
        self.add(d, TAG_PRIOR)
        self._pw(self.att, dm, lambda: dict(wk0=self.w(p + ".self_attn.out_proj.weight").T,
                                            bias0=self.w(p + ".self_attn.out_proj.bias")),
                 s1_out, dm, FH, resid=res_in, in_layout=lay, out_layout=lay, label=p + ".proj")         # src + attention
        if att_ft:
            self._swap(self.t_c, self.s1, False)
        self._chln(self.s1, self.n_b, p + ".norm1")
        g = p + ".gru."
        gru_ft = axis == 0                                            # sequence over bins: lines = frames -> "ft"
        lay = "ft" if gru_ft else "tf"
        if gru_ft:
            self._swap(self.n_b, self.t_a, True)
            gx_in, s2_out = self.t_a, self.t_b
        else:
            gx_in, s2_out = self.n_b, self.s2
        gd = L.GruDesc()
        split_gru = self.split_bf16 and self.split_gru and self.fused_gru_input and dm == 32
        if split_gru:
            # csrc/gru3.hip: the same fused recurrence on split-bf16 operands (six bf16 products per multiply-add)
            def tiles(name, kin):   # [2 dirs][6 gate tiles][kin/16 K blocks][3 planes][64 lanes][8]
                return np.stack([np.stack([P.pack_s3_gather(self.w(g + name + suf)[32 * m:32 * m + 32].T, 1, kin)
                                           for m in range(6)], 0) for suf in ("", "_reverse")], 0)

            gd.split = 1
            gd.x = gx_in.data_ptr()
            gd.wih = self.upw(g + "wih3", lambda: tiles("weight_ih_l0", dm)).data_ptr()
            gd.bih = self.upw(g + "bih", lambda: np.stack([self.w(g + "bias_ih_l0"),
                                                           self.w(g + "bias_ih_l0_reverse")], 0)).data_ptr()
        elif self.fused_gru_input and dm == 32:
            # the input projection runs inside the recurrence kernel: the 12x wider gx tensor never exists
            gd.x = gx_in.data_ptr()
            gd.wih = self.upw(g + "wih", lambda: np.stack([P.pack_a(self.w(g + "weight_ih_l0" + suf).T)
                                                           for suf in ("", "_reverse")], 0)).data_ptr()   # [2, 6, 16, 64]
            gd.bih = self.upw(g + "bih", lambda: np.stack([self.w(g + "bias_ih_l0"),
                                                           self.w(g + "bias_ih_l0_reverse")], 0)).data_ptr()
        else:
            self._pw(gx_in, dm, lambda: dict(
                wk0=np.concatenate([self.w(g + "weight_ih_l0"), self.w(g + "weight_ih_l0_reverse")], 0).T,   # [d, 12d]
                bias0=np.concatenate([self.w(g + "bias_ih_l0"), self.w(g + "bias_ih_l0_reverse")], 0)),
                self.gx, 12 * dm, FH, in_layout=lay, out_layout=lay, label=g + "ih")
        gd.gx, gd.y = self.gx.data_ptr(), self.gy.data_ptr()
        if split_gru:
            gd.whh = self.upw(g + "whh3", lambda: tiles("weight_hh_l0", 2 * dm)).data_ptr()
        else:
            gd.whh = self.upw(g + "whh", lambda: np.stack([P.pack_a(self.w(g + "weight_hh_l0" + suf).T)
                                                           for suf in ("", "_reverse")], 0)).data_ptr()   # [2, 3H/32, H/2, 64]
        gd.bhh = self.upw(g + "bhh", lambda: np.stack([self.w(g + "bias_hh_l0"), self.w(g + "bias_hh_l0_reverse")], 0)).data_ptr()
        gd.B, gd.H, gd.axis = B, 2 * dm, 1                            # lines on the innermost axis, sequence on the outer
        gd.T, gd.F = (FH, T) if gru_ft else (T, FH)
        if not gru_ft:
            gd.seqlen = Ctx.ptr(self.frames)                          # the backward direction starts at the utterance's own last frame
        self.add(gd, TAG_LSTM)
        # relu -> linear2 -> + residual (the normed tensor); ReLU = the load transform with slope 0, identity affine
        self._pw(self.gy, 4 * dm, lambda: dict(wk0=self.w(p + ".linear2.weight").T, bias0=self.w(p + ".linear2.bias"),
                                               xf=dict(mode=1, scale0=np.ones(4 * dm), shift0=np.zeros(4 * dm), slope0=0.0)),
                 s2_out, dm, FH, resid=gx_in, in_layout=lay, out_layout=lay, label=p + ".linear2")
        if gru_ft:
            self._swap(self.t_b, self.s2, False)
        self._chln(self.s2, dst_t, p + ".norm2")

    def _dense_encoder(self, p, src_t, cin, dst):
        """dense_encoder / dense_encoder_mag (dbaiat.py:481-524): src [B,cin,T,161] -> dst [B,64,T,80]."""
        B, T, FH, sd = self.B, self.T, self.FH, self.sd
        self._pw(src_t, cin, lambda: dict(wk0=self.w(p + ".inp_conv.weight")[:, :, 0, 0].T, bias0=self.w(p + ".inp_conv.bias")),
                 self.tmp161, 64, F0, label=p + ".inp")
        if self.fused:
            self._to_dense(self.tmp161, self.D161, F0, 32, p + ".inp_norm", p + ".inp_prelu")
        else:
            self._rowln(self.tmp161, self.D161, 320 * T * F0, 64, F0, p + ".inp_norm", p + ".inp_prelu", dst_off=256 * T * F0)
        self._dense_block(p + ".enc_dense1", self.D161, F0, self.tmp161)
        kk, taps = P.conv_taps(1, 3, 0)
        out4 = self._d_src(self.D161, F0, 0, 64) if self.fused else self.src(self.D161, 64, *nchw(320, T, F0))
        self.gconv(in0=out4, Tin=T, Fin=F0, taps=taps, sf_in=2,
                   W=lambda: dict(wk0=P.conv_kmat(sd[p + ".enc_conv1.weight"], kk), bias0=self.w(p + ".enc_conv1.bias")),
                   Cout=64, out=self.tmp80, out_strides=nchw_out(64, T, FH), B=B, Tout=T, Fout=FH, tag=TAG_PRIOR,
                   label=p + ".enc_conv1", s3g=self.split_bf16)
        self._rowln(self.tmp80, dst, 64 * T * FH, 64, FH, p + ".enc_norm1", p + ".enc_prelu1")

    def _aham(self, p, outs, dst):
        """AHAM / AHAM_ori (dbaiat.py:266-288, :308-330)."""
        ah = L.AhamDesc()
        for i in range(4):
            ah.x[i] = outs[i].data_ptr()
        ah.w = self.upw(p + ".w", lambda: self.w(p + ".conv1.weight").reshape(64)).data_ptr()
        ah.bias = self._wf(p + ".conv1.bias")
        ah.means, ah.out, ah.plane, ah.B, ah.C = self.means.data_ptr(), dst.data_ptr(), self.T * self.FH, self.B, 64
        if self.frames is not None:
            ah.frames, ah.per_frame = self.frames.data_ptr(), self.FH
        self.add(ah, TAG_PRIOR)

    def _dense_decoder(self, de, merged, out, out_C, out_off):
        """dense_decoder (dbaiat.py:527-548) with the sub-pixel up-convolution (:587-602); its 64 -> 1 output goes to
        channel ``out_off // (T*161)`` of ``out`` [B,out_C,T,161].  (The masking decoder :551-584 is the same up to
        its scalar gate, which the CRM operator applies.)"""
        B, T, FH, sd = self.B, self.T, self.FH, self.sd
        if self.fused:
            if self._d80_holds is not merged:     # the decoders of one merge share their input: re-laid out once (layers write groups 0..31)
                self._to_dense(merged, self.D80, FH, 32)
                self._d80_holds = merged
        else:
            for b in range(B):            # merged -> channel block 4 of every batch item (one strided copy per item)
                c = L.EwDesc()
                c.a, c.out = Ctx.ptr(merged, b * 64 * T * FH), Ctx.ptr(self.D80, (b * 320 + 256) * T * FH)
                c.n, c.op = 64 * T * FH, L.EW_COPY
                self.add(c, TAG_EW)
        self._dense_block(de + ".dec_dense1", self.D80, FH, self.tmp80)
        taps = [(0, kf - 1) for kf in range(3)]                   # pad (1,1) in bins
        kk = [(0, kf) for kf in range(3)]
        # co = r*64 + c  ->  channel c, bin 1 + 2w + r   (sub-pixel r = 2, then one zero bin on the left)
        out4 = self._d_src(self.D80, FH, 0, 64) if self.fused else self.src(self.D80, 64, *nchw(320, T, FH))
        self.gconv(in0=out4, Tin=T, Fin=FH, taps=taps, sf_in=1,
                   W=lambda: dict(wk0=P.conv_kmat(sd[de + ".dec_conv1.conv.weight"], kk), bias0=self.w(de + ".dec_conv1.conv.bias")),
                   Cout=128, out=self.dec_up, out_strides=(64 * T * F0, 1, T * F0, F0, 2), out_cr=64, out_off=1, B=B, Tout=T,
                   Fout=FH, tag=TAG_PRIOR, label=de + ".dec_conv1", s3g=self.split_bf16)
        self._rowln(self.dec_up, self.tmp161, 64 * T * F0, 64, F0, de + ".dec_norm1", de + ".dec_prelu1")
        self.gconv(in0=self.src(self.tmp161, 64, *nchw(64, T, F0)), Tin=T, Fin=F0, taps=[(0, 0)], sf_in=1,
                   W=lambda: dict(wk0=self.w(de + ".out_conv.weight")[:, :, 0, 0].T, bias0=self.w(de + ".out_conv.bias")), Cout=1,
                   out=out, out_strides=nchw_out(out_C, T, F0), out_off=out_off, B=B, Tout=T, Fout=F0, tag=TAG_PRIOR,
                   label=de + ".out_conv")

    def _gncomb(self, p, i, base, out):
        g = L.GncombDesc()
        g.base, g.row, g.col, g.out = base.data_ptr(), self.br[0].data_ptr(), self.br[1].data_ptr(), out.data_ptr()
        g.g_row, g.b_row = self._wp("%s.row_norm.%d.weight" % (p, i)), self._wp("%s.row_norm.%d.bias" % (p, i))
        g.g_col, g.b_col = self._wp("%s.col_norm.%d.weight" % (p, i)), self._wp("%s.col_norm.%d.bias" % (p, i))
        g.stats, g.plane, g.B, g.C = self.gn_stats.data_ptr(), self.T * self.FH, self.B, self.d
        g.k1, g.k2, g.eps = self._wf(p + ".k1"), self._wf(p + ".k2"), 1e-8
        if self.frames is not None:
            g.frames, g.per_frame = self.frames.data_ptr(), self.FH
        self.add(g, TAG_PRIOR)

    def build(self, x=None, out=None):
        B, T, FH = self.B, self.T, self.FH
        x = self.x if x is None else x
        out = self.out if out is None else out
        self._dense_encoder("en_ri", x, 2, self.x_ri)
        # ---- AIA_Transformer (dbaiat.py:133-154)
        p = "dual_trans"
        self._pw(self.x_ri, 64, lambda: dict(wk0=self.w(p + ".input.0.weight")[:, :, 0, 0].T, bias0=self.w(p + ".input.0.bias")),
                 self.cur, 32, FH, act=L.ACT_PRELU, act_slope=self._wf(p + ".input.1.weight"), label=p + ".input")
        cur, nxt = self.cur, self.nxt
        for i in range(4):
            self._encoder_layer("%s.row_trans.%d" % (p, i), 0, cur, self.br[0])
            self._encoder_layer("%s.col_trans.%d" % (p, i), 1, cur, self.br[1])
            self._gncomb(p, i, cur, nxt)
            cur, nxt = nxt, cur
            self._pw(cur, 32, lambda: dict(wk0=self.w(p + ".output.1.weight")[:, :, 0, 0].T, bias0=self.w(p + ".output.1.bias"),
                                           xf=dict(mode=1, scale0=np.ones(32), shift0=np.zeros(32),          # PReLU on load
                                                   slope0=float(self.w(p + ".output.0.weight")[0]))),
                     self.outs[i], 64, FH, label=p + ".output")
        self._aham("aham", self.outs, self.merged)
        for ch, de in enumerate(("de1", "de2")):
            self._dense_decoder(de, self.merged, out, 2, ch * T * F0)
        return out


class DualAiaPlan(AiaPlan):
    """dual_aia_trans_merge_crm (model/dbaiat.py:373-413): ri and magnitude encoders -> AIA_Transformer_merge
    (d_model 64, :157-246) -> AHAM_ori x2 -> two dense decoders + the masking decoder -> magnitude/phase recombination.

    The reference runs the merge transformer twice per layer, once per branch; the two runs are the same
    computation: layer 0 of both reads the shared input projection (:206-207), layer i >= 1 of the magnitude
    branch reads mag[i-1] + ri[i-1] (:211) and of the ri branch ri[i-1] + mag[i-1] (:229, ``[-2]`` after the
    append), and IEEE addition commutes.  The golden vectors of the reference module confirm that the two output
    lists are bit-identical (tests/test_oracle_golden.py), so each layer is evaluated once."""

    def __init__(self, ctx, sd, B, T, plan=None, split_bf16=None, planes=None, frames=None):
        super().__init__(ctx, sd, B, T, plan, d=64, split_bf16=split_bf16, planes=planes, frames=frames)
        a = ctx.alloc
        self.mag = a(B, 1, T, F0)
        self.x_mag_en = a(B, 64, T, self.FH)
        self.inp = a(B, 64, T, self.FH)          # shared input projection ("input_mag" == "input_ri")
        self.merged_mag = a(B, 64, T, self.FH)
        self.ri_dec = a(B, 2, T, F0)
        self.o_mask = a(B, 1, T, F0)

    def build(self, x=None, out=None):
        B, T, FH = self.B, self.T, self.FH
        x = self.x if x is None else x
        out = self.out if out is None else out
        c = L.CrmDesc()
        c.x, c.out, c.plane, c.B, c.mode = x.data_ptr(), self.mag.data_ptr(), T * F0, B, 0
        self.add(c, TAG_PRIOR)
        self._dense_encoder("en_ri", x, 2, self.x_ri)
        self._dense_encoder("en_mag", self.mag, 1, self.x_mag_en)
        p = "aia_trans_merge"
        # input projection over cat(mag, ri) (dbaiat.py:205-207): two-source 1x1 + PReLU
        self.gconv(in0=self.src(self.x_mag_en, 64, *nchw(64, T, FH)), in1=self.src(self.x_ri, 64, *nchw(64, T, FH)), Tin=T,
                   Fin=FH, taps=[(0, 0)], sf_in=1, Cout=64,
                   W=lambda: dict(wk0=self.w(p + ".input.0.weight")[:, :, 0, 0].T, bias0=self.w(p + ".input.0.bias")),
                   act=L.ACT_PRELU, act_slope=self._wf(p + ".input.1.weight"),
                   out=self.inp, out_strides=nchw_out(64, T, FH), B=B, Tout=T, Fout=FH, tag=TAG_PRIOR, label=p + ".input")
        u = self.inp
        for i in range(4):
            self._encoder_layer("%s.row_trans.%d" % (p, i), 0, u, self.br[0])
            self._encoder_layer("%s.col_trans.%d" % (p, i), 1, u, self.br[1])
            self._gncomb(p, i, self.inp, self.nxt)                    # input + k1 * row + k2 * col  (:225, :243)
            self._pw(self.nxt, 64, lambda: dict(wk0=self.w(p + ".output.1.weight")[:, :, 0, 0].T, bias0=self.w(p + ".output.1.bias"),
                                                xf=dict(mode=1, scale0=np.ones(64), shift0=np.zeros(64),      # PReLU on load
                                                        slope0=float(self.w(p + ".output.0.weight")[0]))),
                     self.outs[i], 64, FH, label=p + ".output")
            if i < 3:                                                 # next layer reads mag[i] + ri[i] = out + out
                e = L.EwDesc()
                e.a, e.b, e.out = self.outs[i].data_ptr(), self.outs[i].data_ptr(), self.cur.data_ptr()
                e.n, e.op, e.s0 = self.outs[i].numel(), L.EW_ADD_MUL, 1.0
                self.add(e, TAG_EW)
                u = self.cur
        self._aham("aham", self.outs, self.merged)
        self._aham("aham_mag", self.outs, self.merged_mag)
        self._dense_decoder("de1", self.merged, self.ri_dec, 2, 0)
        self._dense_decoder("de2", self.merged, self.ri_dec, 2, T * F0)
        self._dense_decoder("de_mag_mask", self.merged_mag, self.o_mask, 1, 0)
        c = L.CrmDesc()
        c.x, c.o, c.ri, c.out = x.data_ptr(), self.o_mask.data_ptr(), self.ri_dec.data_ptr(), out.data_ptr()
        de = "de_mag_mask."
        c.a1, c.b1 = self._wf(de + "mask1.0.weight"), self._wf(de + "mask1.0.bias")
        c.a2, c.b2 = self._wf(de + "mask2.0.weight"), self._wf(de + "mask2.0.bias")
        c.a3, c.b3 = self._wf(de + "maskconv.weight"), self._wf(de + "maskconv.bias")
        c.plane, c.B, c.mode = T * F0, B, 1
        self.add(c, TAG_PRIOR)
        return out
