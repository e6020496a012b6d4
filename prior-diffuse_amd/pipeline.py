"""The whole sampling path as ONE recorded plan:

    [wav -> RMS normalise -> STFT -> sqrt-compress]            :921-937
    prior(feat) -> X_init; init = X_init / 11                   :939-942
    [--sigma: x_T *= sqrt(mask(init))]                          :951-956
    for n = S-1 .. 0: eps = DiffUNet1(audio, init, T[n]);
                      audio = c1 (audio - c2 eps)               :964-992
    spec = (audio + init) * 11                                  :995-996
    [square-decompress -> ISTFT -> * c]                         :1004-1016

(line numbers: reference trainer/complex_ddpm_trainer.py).  Once built for a (B, T) the
plan owns every buffer in HBM; ``run()`` is a single C call that issues the launches, or
a single hipGraph replay.
"""
import numpy as np
import torch

from . import _lib as L
from . import longplan, nets, packing, rangeaudit
from .params import PRIOR_SCALE_C, params as default_params
from .schedule import inference_schedule, step_coefficients

F0 = 161


RAGGED_PRIORS = ("GCRN", "DiffUNet")
MASKED_PRIORS = ("aia_complex_trans_ri", "dual_aia_trans_merge_crm")    # ragged with the length-masked kernels (masked_prior=True)


def ragged_args(prior_name, L_, masked=False):
    """Argument check of ``SamplerPipeline(ragged=True, masked_prior=masked)``, without a device."""
    if prior_name not in RAGGED_PRIORS and not (masked and prior_name in MASKED_PRIORS):
        raise ValueError("exact ragged batches: prior %r attends and runs a bidirectional GRU over all T frames of the padded batch, "
                         "so padding reaches every frame of an utterance (supported priors: %s)" % (prior_name, ", ".join(RAGGED_PRIORS)))
    if L_ is None:
        raise ValueError("exact ragged batches need the signal front / back end (pass L_)")


def ragged_tables(lens, B, L_):
    """lens (one int for all, or B of them) -> (lens, frames) as int32 arrays, frames = 1 + lens // 160; ValueError for a
    length outside 161 .. L_ (the centred STFT reflects 160 samples) or a list that is not B long.  Host only."""
    lens_h = np.asarray(lens, dtype=np.int64).reshape(-1)
    if lens_h.size == 1 and B != 1:
        lens_h = np.repeat(lens_h, B)
    if lens_h.size != B:
        raise ValueError("lens: expected %d lengths, got %d" % (B, lens_h.size))
    if lens_h.min() < 161 or lens_h.max() > L_:
        raise ValueError("lens: every length must lie in 161 .. %d (the padded length), got %d .. %d" % (L_, lens_h.min(), lens_h.max()))
    return lens_h.astype(np.int32), (1 + lens_h // 160).astype(np.int32)


def _expect(t, like, name):
    """Inputs must have exactly the geometry the plan was recorded for (``copy_`` would silently broadcast)."""
    if tuple(t.shape) != tuple(like.shape) or t.dtype != like.dtype:
        raise ValueError(f"{name}: expected {tuple(like.shape)} {like.dtype}, got {tuple(t.shape)} {t.dtype}")


class SamplerPipeline:
    # the fp32-equivalent operand split of the matrix-core kernels (see ``split``)
    default_split = "f16x2"

    def __init__(self, device, prior_name, prior_sd, ddpm_sd, B, T=None, L_=None, fast_sampling=True,
                 use_sigma=False, params=default_params, with_signal=None, deltamu=False, cond="init", bank=None,
                 split_bf16=None, xT_plus_init=None, dtype="f32", exclusive=False, split=None, audit=False, ragged=False,
                 verdict=False, masked_prior=False, label=False, objective=False, feat_type="sqrt", members=1, window=None,
                 carry_state=False):
        """deltamu: the alternative parameterisation of utils/params.py:36 — ddpm_sd is a ``Nocon`` state_dict,
        x_T = noise + X_init/11 (:947-948), eps = Nocon(x, t) (:970-971), no final ``+ X_init`` (:995).
        cond (deltamu False): what conditions DiffUNet1 — "init": X_init/11 (pirorgrad, :967-969, + X_init at the end,
        :994-995); "feat": the noisy feature / 11 (the branch with neither flag set, :74-75, :972-974; no final add).
        xT_plus_init: x_T = noise + X_init/11 (:946-949 tests ``self.deltamu`` on its own, while model selection :70-73
        and the eps call :967-971 let ``pirorgrad`` win): default = deltamu; True with deltamu False is the reference's
        behaviour when BOTH flags are set (DiffUNet1 conditioned on X_init, start from noise + X_init/11, final + X_init).
        dtype: "f32" (default: fp32 or fp32-equivalent split-bf16 arithmetic, see split_bf16) or "bf16" - the OPT-IN reduced
        precision mode of BASELINE configs 2/4/5: the eps-net's BiConv(Trans)GLU and TCM blocks multiply plain bf16 operands
        (one MFMA product, fp32 accumulate) and exchange their conv1 / bottleneck tensors as bf16 (csrc/bglu.hip, csrc/tcm2.hip,
        one plane); round 4: the priors' GEMM-shaped convolutions (GCRN's gated convolutions and LSTM projection, DB-AIAT's
        dense blocks) multiply plain bf16 operands as well (csrc/gconv4.hip, korder 4); the diffusion state, the skip halves,
        the residual stream of the TCM stack, the recurrences and every tensor of the priors stay fp32.  Its tolerance is its own (stated in
        tests/test_gpu_round2.py::test_bf16_mode_tolerance), it is never the default and never the graded bench line.
        bank: a ``nets.WeightBank`` shared with other pipelines built from the same state_dicts (packed weights are
        uploaded once, every further (B, T) only records descriptors).
        exclusive: this pipeline is the only work on the GPU while it runs (one batch in flight - ``ComplexDDPMTrainer``
        passes True): launches whose workgroups wait for each other may then be used - the TCM stack as one launch
        (csrc/tcm2.hip: tcm2s_kernel, bit-identical) and, for B <= 4, the GCRN prior's LSTM (csrc/lstmp.hip; 1e-5 from, not
        bit-identical to, the kernels large batches take).
        ``ConcurrentSampler`` / ``PipelinedSampler`` and the sharded path keep False.
        split_bf16: the eps-net's BIGLU blocks and the priors' GEMM-shaped convolutions on the bf16 matrix cores with exact three-way
        operand splits - fp32-level accuracy at 16/6 of the fp32 MFMA rate (csrc/gconv3.hip); None: on for fast sampling,
        off (exact fp32 MFMA) for the full 50-step schedule.
        split (with split_bf16, dtype "f32"): which fp32-equivalent operand split the matrix-core kernels use - "bf16x3": the exact
        three-way bf16 split, six bf16 products per multiply-add; "f16x2": fp16 hi + lo of the power-of-two scaled operand (within
        2^-23 |x|, relative, inside the fp16 window, see include/pdse.h PDSE_F16_ACT_EXP), three f16 products, two thirds of the plane
        bytes.  Both are held to the same goldens and tolerances.  None: ``SamplerPipeline.default_split``.
        audit: record the range audit of the f16x2 window with the plan (csrc/range.hip): one launch that clears the histogram
        table at the start of the plan and one accumulate launch at the end of every marked range whose builder has audited
        tensors (``nets.PlanBase.audited()``) - "prior", then every "stepN": the plane buffers are reused by every step, so a
        look after the pass would see the last step only.  Rows are per (range, tensor); the launches only read the tensors, they
        are part of the plan and of its hipGraph.  ``range_report()`` / ``check(audit=True)`` read the table.  Only f16x2 passes
        have a window: with split "bf16x3" (or dtype "bf16", or the exact fp32 arithmetic of the full schedule) the flag is
        accepted and nothing is recorded.  False (default): the plan is launch for launch the one without the feature.
        The audit of a ragged plan sees the padding frames of the shorter utterances too: its histograms are over whole buffers.
        ragged: EXACT ragged batches (needs L_; priors GCRN and DiffUNet).  ``enhance(wav, x_T, lens=..., exact=True)`` then gives
        every utterance b of a zero-padded batch, in samples [0, len_b) and frames [0, T_b = 1 + len_b // 160), exactly what a
        B = 1 pass of length len_b with x_T[b, :, :T_b] gives; samples and frames behind an utterance's own come back as zeros
        (what the intermediate buffers hold there is unspecified, but finite).  The plan records the masked variants of the four
        places where padding could reach an utterance's own frames - the STFT's right-hand reflection (``wavprep``), the TCM
        bottleneck of the eps-net (and of a DiffUNet prior), the overlap-add and the ``--sigma`` maximum - and owns their length
        tables (``lens``, ``frames_tab``, ``valid_tab``: device int32, written by a copy before each pass, so a replayed
        hipGraph sees new lengths).  Everything else on the path is per-frame or looks back in time only.  The
        DB-AIAT priors attend and run a bidirectional GRU over all of T: ValueError, unless ``masked_prior`` records their
        length-masked kernels.  False (default): every table is NULL and
        the plan is launch for launch today's.
        verdict: record the finiteness verdict of a pass with the plan (csrc/range.hip, PDSE_RANGE_NONFINITE): the plan owns
        ``verdict_tab`` (int32 [rows][32], one row per judged tensor: ``spec``, and ``istft.wav`` with the signal back end), clears
        it in its first launch and ends with one launch that counts the Inf / NaN elements of those tensors into column 0 of
        their rows.  Both are ordinary descriptors (marked range "verdict" holds the count), so a hipGraph replay judges its
        own pass.  ``verdict_fetch(stream)`` copies the table to pinned host memory without synchronising and
        ``verdict_counts()`` reads it once an event recorded behind the copy has fired: what ``check()`` learns from a
        reduction over the spectrogram and a device-wide synchronisation, per pass and per stream.  Plan files do not carry it
        (``planfile.save_pipeline`` raises ValueError).  False (default): the plan is launch for launch today's.
        masked_prior (with ``ragged``): record a DB-AIAT prior (``aia_complex_trans_ri``, ``dual_aia_trans_merge_crm``) with the
        length-masked forms of its four operators that reach across frames - attention and the bidirectional GRU along the
        frames, the GroupNorm statistics of the layer update and the AHAM average pool (csrc/aia.hip, csrc/gru3.hip; DESIGN.md
        4.8) - on ``frames_tab``, so that ``ragged=True`` accepts these priors with the same contract.  False (default): they
        are refused as before; for the other priors the flag changes nothing.
        label (needs L_): the label leg of a validation pass (``LabelLeg``, ``self.label``): ``enhance(wav, x_T, clean=...)`` then
        also leaves on the device the clean utterances' compressed spectrogram - scaled by the noisy utterances' c, as
        Collate.collate_fn scales them (utils/dataset.py:45-58) - and the normalised-domain waveforms utils/metrics.py's
        compare_complex compares.  The leg is a second, small plan beside this one: False (default), and every pass without
        ``clean``, records and runs exactly the operators of a pipeline without the flag.
        objective (needs L_): the plan of the denoising objective instead of the sampler's (``ObjectiveLeg``, ``self.objective``;
        ``objective_pass``).  The front is this constructor's own - wav prep, STFT, compression, the prior, and the label leg's
        front for the label spectrogram - and behind the prior the plan holds X_init / 11 (range "scale") and ONE recorded
        eps-net step at a per-utterance ``tsteps`` row (range "step0", ``EpsNetPlan(nsteps=1)``): no x_T, no reverse loop, no
        ISTFT.  ``spec`` is then the eps-net's prediction, which ``check()`` judges.  The parameterisation follows ``deltamu`` and
        ``cond`` as trainer/complex_ddpm_trainer.py:726-733 reads them: DiffUNet1(noisy, init, t), Nocon(noisy, t), or
        DiffUNet1(noisy, feat, t) with feat NOT divided by 11 (:701 is commented out).  Padded batches only (``ragged``:
        ValueError); no verdict.
        feat_type: the spectral compression around the networks, the ``feat_type`` of the reference's configuration files -
        "sqrt" (default), "normal", "cubic", "log_1x" or "none" (include/pdse.h: pdse_compand_desc; any other string:
        ValueError).  The front end and the label leg compress with it, the back end and the label leg's scored waveforms
        decompress with it; the prior, the eps-net, X_init / 11, the sigma mask, the losses and the objective's noising work in
        the compressed domain whatever it is, so nothing else changes.  "sqrt" records, launch for launch and field for field,
        the plan it always recorded.  The fp16 window of the f16x2 split was audited on sqrt-compressed activations only:
        "normal" and "none" feed the networks magnitudes one to two orders above those, and a pass that leaves the window shows
        in the verdict / ``check()`` as before.
        members: K = 1 .. 16 reverse trajectories per utterance behind ONE pass of the front end and the prior - a posterior
        ensemble (any other value: ValueError).  Wav prep, STFT, compression and the prior are recorded at B, the
        eps-net and the reverse loop at K B (``EpsNetPlan(B=K*B)``), member-major: row k B + b is member k of utterance b, so a
        member's block of B rows is an ordinary [B,2,T,161] tensor.  The prologue broadcasts X_init / 11 (and with
        ``cond="feat"`` the feature) to the K B conditioning rows with K launches of the same division; ``xT_in`` is
        [K B,2,T,161]; the last step writes ``members_spec`` [K B,2,T,161]; ``spec`` stays [B,2,T,161] and holds what the ISTFT
        inverts - the ensemble mean, written by ``pdse_ensemble_stats`` (csrc/ensemble.hip; a plain-argument call between the
        ranges "step0" and "istft", so ``graph=True`` is a ValueError), which also leaves ``ensemble``: ``spread`` [B,T,161],
        ``per_utt`` [B,2] and ``per_member`` [K,B] (``ops.ensemble_stats``).  With ``label``, all five ``feat_type`` values,
        ``use_sigma``, the three conditioning branches and every arithmetic; with ``ragged``, ``verdict`` or ``objective``:
        ValueError, and plan files do not carry it.  1 (default): the plan is launch for launch and field for field today's.
        window: W frames (a multiple of ``longplan.FRAME_TILE``; needs L_): recordings of any length through ONE plan of W frames
        (DESIGN.md 4.13).  With T = 1 + L_ // 160 <= W the pipeline is the whole-file one, launch for launch.  With T > W it
        records no whole-file network plan at all: ``self.long`` is a ``LongSampler`` and ``enhance`` runs its windowed pass, whose
        results are the whole-file plan's (built with ``exclusive=False``).  Priors GCRN (its LSTM state carried from window to
        window) and DiffUNet (halos); the DB-AIAT priors attend over all frames: ValueError.  With ``ragged``, ``members`` > 1,
        ``verdict``, ``label``, ``objective`` or ``audit``: ValueError; plan files do not carry it.  None (default): off.
        carry_state: this pipeline is the window plan of a ``LongSampler`` - a GCRN prior is recorded with the LSTM's state
        fields (``nets.GcrnPlan(carry_state=True)``).  False (default): launch for launch today's."""
        objective = bool(objective)
        self.window = longplan.window_arg(window)
        self.long = None
        if self.window is not None:
            if L_ is None:
                raise ValueError("window= needs the signal front / back end (pass L_)")
            longplan.window_conflicts(ragged=ragged, members=members, verdict=verdict, label=label, objective=objective)
            if audit:
                raise ValueError("window= with audit=True: the range audit reads one recorded plan's table")
            LongSampler.prior_check(prior_name)
            if 1 + L_ // 160 > self.window:
                self.long = LongSampler(device, prior_name, prior_sd, ddpm_sd, B, self.window, fast_sampling=fast_sampling,
                                        use_sigma=use_sigma, params=params, deltamu=deltamu, cond=cond, bank=bank, split_bf16=split_bf16,
                                        xT_plus_init=xT_plus_init, dtype=dtype, split=split, feat_type=feat_type)
                self.B, self.T, self.L, self.device, self.members = B, 1 + L_ // 160, L_, torch.device(device), 1
                self.bank, self.split, self.dtype, self.plan = self.long.bank, self.long.win.split, dtype, None
                self.audit = self.audited = self.verdict = False
                self.label = self.objective = self.stft = None
                return
        self.members = K = L.members_arg(members)
        if K > 1:
            for flag, name in ((ragged, "ragged"), (verdict, "verdict"), (objective, "objective")):
                if flag:
                    raise ValueError("members=%d with %s=True: ensembles are built for padded sampler passes verified by check() "
                                     "(exact ragged batches, the in-flight verdict and the objective plan run one trajectory)" % (K, name))
        self.feat_type = L.feat_type_of(feat_type)
        if objective and (L_ is None or ragged or verdict):
            raise ValueError("the objective plan needs the signal front end (pass L_) and is built for padded batches, without the verdict")
        if L_ is not None:
            T = 1 + L_ // 160
        if with_signal is None:
            with_signal = L_ is not None
        if cond not in ("init", "feat"):
            raise ValueError("cond must be 'init' or 'feat'")
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        if dtype == "bf16" and (deltamu or split_bf16 is False):
            raise ValueError("the bf16 mode runs the DiffUNet1 blocks on the bf16 matrix cores (split_bf16 False / Nocon: no)")
        self.dtype = dtype
        split = self.default_split if split is None else split
        if split not in ("bf16x3", "f16x2"):
            raise ValueError("split must be 'bf16x3' or 'f16x2'")
        self.split = split
        if split_bf16 is None:
            # 6-step fast sampling: split-bf16 blocks (2e-6 from the fp32 CPU path, tolerance 1e-4).  The full 50-step
            # schedule amplifies rounding noise ~500x (the fp32 CPU path itself sits 4-7e-5 from the exact answer), so
            # it keeps exact fp32 MFMA arithmetic - BASELINE config 3 is an fp32 configuration anyway.
            split_bf16 = bool(fast_sampling)
        self.ragged = bool(ragged)
        self.masked_prior = bool(masked_prior)
        if self.ragged:
            ragged_args(prior_name, L_, masked=self.masked_prior)
        self.B, self.T, self.L = B, T, L_
        self.device = torch.device(device)
        self.ctx = ctx = nets.Ctx(device, bank)
        self.bank = ctx.bank
        self.plan = L.Plan(self.device) if self.device.type == "cuda" else None
        alpha, beta, alpha_cum, sigmas, Tarr = inference_schedule(params, fast_sampling)
        self.schedule = (alpha, beta, alpha_cum, sigmas, Tarr)
        c1, c2 = step_coefficients(alpha, beta, alpha_cum)
        S = len(alpha)
        self.nsteps = S
        self.ranges = {}
        self.descs = []
        self.audit = bool(audit)
        self.range_rows = []          # (range name, tensor name) of every histogram row, in table order
        self.range_hist = None        # device int32 [RANGE_CAP][32] (the kernel's uint32 counters)

        # ---- builders share one plan object and one descriptor list
        def adopt(pb):
            pb.descs = self.descs
            return pb

        self.frames_tab = self.valid_tab = None
        if self.ragged:
            # the length tables of the masked launches (with stft.lens): every utterance's own frames, and frames x 161 per (b, re|im) plane
            self.frames_tab = torch.full((B,), T, dtype=torch.int32, device=self.device)
            self.valid_tab = torch.full((2 * B,), T * F0, dtype=torch.int32, device=self.device)
            ctx.keep += [self.frames_tab, self.valid_tab]
        self.stft = adopt(nets.StftPlan(ctx, B, L_, plan=self.plan, split_bf16=split_bf16, reflect_own=self.ragged,
                                        feat_type=self.feat_type)) if with_signal else None
        # operand planes of the matrix-core kernels (csrc/planes.h): 1 = plain bf16 (the bf16 mode), 2 = f16x2, 3 = bf16x3
        nplanes = 1 if dtype == "bf16" else (2 if split == "f16x2" else 3)
        # the priors' GEMM-shaped convolutions (csrc/gconv4.hip: korder 4 / 5 / 3) and DB-AIAT's dense blocks (np); None: their fp32 kernels
        pplanes = nplanes if (split_bf16 or dtype == "bf16") else None
        if prior_name == "GCRN":
            self.prior = adopt(nets.GcrnPlan(ctx, prior_sd, B, T, plan=self.plan, split_bf16=split_bf16 or dtype == "bf16", exclusive=exclusive,
                                             planes=pplanes, carry_state=carry_state))
        elif prior_name == "DiffUNet":
            self.prior = adopt(nets.EpsNetPlan(ctx, prior_sd, B, T, time_cond=False, plan=self.plan, split_bf16=split_bf16, exclusive=exclusive,
                                               frames=self.frames_tab))
        elif prior_name == "aia_complex_trans_ri":
            self.prior = adopt(nets.AiaPlan(ctx, prior_sd, B, T, plan=self.plan, split_bf16=split_bf16 or dtype == "bf16", planes=pplanes,
                                            frames=self.frames_tab))
        elif prior_name == "dual_aia_trans_merge_crm":
            self.prior = adopt(nets.DualAiaPlan(ctx, prior_sd, B, T, plan=self.plan, split_bf16=split_bf16 or dtype == "bf16", planes=pplanes,
                                                frames=self.frames_tab))
        else:
            raise ValueError("prior %r not built (GCRN, DiffUNet, aia_complex_trans_ri, dual_aia_trans_merge_crm)" % prior_name)
        if dtype == "bf16":
            split_bf16 = True
        KB = K * B       # rows of the reverse loop: member-major, row k B + b
        self.eps = adopt(nets.EpsNetPlan(ctx, ddpm_sd, KB, T, time_cond=True, nsteps=1 if objective else S, plan=self.plan,
                                         with_pre=not deltamu, split_bf16=split_bf16,
                                         planes=nplanes,
                                         exclusive=exclusive, frames=self.frames_tab))
        self.split_bf16 = self.eps.split_bf16
        # the audit is recorded only where f16x2 operands are multiplied
        self.audited = self.audit and self.windowed and self.plan is not None
        self.deltamu = deltamu
        self.xT_plus_init = xT_plus_init = bool(deltamu if xT_plus_init is None else xT_plus_init)
        self.cond_feat = cond_feat = (cond == "feat") and not deltamu
        self.istft = adopt(nets.IstftPlan(ctx, B, T, L_, plan=self.plan, split_bf16=split_bf16, frames=self.frames_tab,
                                          lens=self.stft.lens if self.ragged else None,
                                          feat_type=self.feat_type)) if with_signal and not objective else None

        self.feat = self.prior.x                     # prior input = compressed spectrogram
        # X_init / 11: the eps-net's conditioning input only in the pirorgrad parameterisation
        self.init = self.eps.x_init if not (deltamu or cond_feat) else ctx.alloc(KB, 2, T, F0)
        self.zero = ctx.alloc(KB, 2, T, F0, zero=True) if (deltamu or cond_feat) and not objective else None
        self.audio = self.eps.x                      # x_t, updated in place
        if objective:
            self.spec, self.xT_in = self.eps.out, None   # the prediction of the one step; nothing is injected
        else:
            self.spec = self.istft.spec if with_signal else ctx.alloc(B, 2, T, F0)
            self.xT_in = ctx.alloc(KB, 2, T, F0)         # injected x_T (kept so a replay starts from it)
        # what the last step writes: ``spec`` itself, or the K members the ensemble kernel reduces into it
        self.members_spec = ctx.alloc(KB, 2, T, F0) if K > 1 else self.spec
        self.ensemble = None                             # the statistics of the last ensemble pass (ops.ensemble_stats)
        n = B * 2 * T * F0

        if self.audited:
            # The clear launch is the plan's first, so the table is sized before the rows are known - by a bound that holds by
            # construction: audited() reports only buffers the builder named (PlanBase.named), each at most twice (the two
            # branches of a TCM bottleneck tensor), once per audited range - the prior's range and one range per step.
            self._range_cap = 2 * (len(self.prior._audit_names) + S * len(self.eps._audit_names))
            self.range_hist = torch.zeros(max(1, self._range_cap), L.RANGE_BINS, dtype=torch.int32, device=self.device)
            ctx.keep.append(self.range_hist)
        self._range_clear = None      # index of the clear launch in the plan
        self._ranges_run = set()      # marked ranges the last run() executed (range_report() reports those)
        self.verdict = bool(verdict)
        self.verdict_tab = self._verdict_host = None
        self._verdict_clear = self._verdict_count = None      # indices of the verdict's two launches in the plan
        if self.verdict:
            # one row per judged tensor, cleared by the same launch the audit clears its histograms with (mode 0 of the operator)
            self.verdict_tab = torch.zeros(2 if with_signal else 1, L.RANGE_BINS, dtype=torch.int32, device=self.device)
            ctx.keep.append(self.verdict_tab)
            if self.device.type == "cuda":
                self._verdict_host = torch.zeros(self.verdict_tab.shape, dtype=torch.int32).pin_memory()

        def range_launch(mode, rows=None, tab=None):
            tab = self.range_hist if tab is None else tab
            d = L.RangeDesc()
            d.out, d.out_rows, d.mode, d.blocks = tab.data_ptr(), tab.shape[0], mode, 1
            if rows:
                dev = ctx.up(rangeaudit.table_of(rows), np.uint8)
                d.rows, d.nrows, d.blocks = dev.data_ptr(), len(rows), rangeaudit.work_blocks(rows)
            elif tab is self.verdict_tab:
                self._verdict_clear = len(self.descs)
            else:
                self._range_clear = len(self.descs)
            self.eps.add(d, nets.TAG_NONE)

        def mark(name, fn):
            b = len(self.descs)
            if self.verdict and not self.ranges:
                range_launch(L.RANGE_CLEAR, tab=self.verdict_tab)   # first launch of the plan
            if self.audited and not self.ranges:
                range_launch(L.RANGE_CLEAR)                     # first launch of the plan (behind the verdict's clear, if any)
            fn()
            if self.audited and (name == "prior" or name.startswith("step")):
                rows = []
                entries = (self.prior if name == "prior" else self.eps).audited()
                # rows in the order of the dataflow at the time of the look: the diffusion state was updated by the step's
                # last launch, so what the audit sees in it is the step's OUTPUT - it goes last (the first ``above`` row of a
                # report is then the tensor that overflowed, not the state it poisoned)
                entries.sort(key=lambda a: a[1].data_ptr() == self.audio.data_ptr())
                for tname, t, kind, e, box in entries:
                    rows.append(rangeaudit.make_row(t, kind, e, box, len(self.range_rows)))
                    self.range_rows.append((name, tname))
                assert len(self.range_rows) <= self._range_cap
                if rows:
                    range_launch(L.RANGE_ACCUMULATE, rows)
            self.ranges[name] = (b, len(self.descs))

        if with_signal:
            mark("stft", lambda: self.stft.build(feat=self.feat))
        if prior_name in ("GCRN", "aia_complex_trans_ri", "dual_aia_trans_merge_crm"):
            mark("prior", lambda: self.prior.build(x=self.feat, out=self.prior.out))
        else:
            mark("prior", lambda: self.prior.build_step(0, x=self.feat, out=self.prior.out))

        def ew(op, a, b=None, c=None, out=None, s0=0.0, s1=0.0, s2=0.0, rows=K, member=0):
            """rows: member blocks the launch covers (K: all K B rows); member: the block of ``out`` a one-block launch writes."""
            d = L.EwDesc()
            d.a, d.b, d.c, d.out = a.data_ptr(), nets.Ctx.ptr(b), nets.Ctx.ptr(c), out.data_ptr() + 4 * n * member
            d.n, d.s0, d.s1, d.s2, d.op = n * rows, s0, s1, s2, op
            self.eps.add(d, nets.TAG_EW)

        def prologue():
            for k in range(K):                    # the prior ran at B: its output / 11 into every member's conditioning rows
                ew(L.EW_DIV, self.prior.out, out=self.init, s0=PRIOR_SCALE_C, rows=1, member=k)
            if cond_feat:
                for k in range(K):
                    ew(L.EW_DIV, self.feat, out=self.eps.x_init, s0=PRIOR_SCALE_C, rows=1, member=k)   # batch_feat /= c  (:943)
            src = self.xT_in
            if xT_plus_init:
                ew(L.EW_ADD_MUL, self.xT_in, b=self.init, out=self.audio, s0=1.0)     # randn_like(init) + init  (:947-948)
                src = self.audio
            if use_sigma:                                                             # audio * sqrt(mask(init))  (:951-956)
                d = L.SigmaDesc()
                d.init, d.a, d.out = self.init.data_ptr(), src.data_ptr(), self.audio.data_ptr()
                d.maxbuf = ctx.alloc(KB * 2).data_ptr()
                d.plane, d.nplanes = T * F0, KB * 2
                d.valid = nets.Ctx.ptr(self.valid_tab)
                self.eps.add(d, nets.TAG_EW)
            elif not xT_plus_init:
                ew(L.EW_COPY, self.xT_in, out=self.audio)
            self.eps.build_time()

        def objective_tail():
            def scale():
                ew(L.EW_DIV, self.prior.out, out=self.init, s0=PRIOR_SCALE_C)        # init_audio /= self.c  (:700)
                if cond_feat:
                    ew(L.EW_COPY, self.feat, out=self.eps.x_init)                     # batch_feat as it is (:701 is commented out)

            def one():
                self.eps.build_time()
                self.eps.build_step(0, x=self.audio, x_init=None if deltamu else (self.eps.x_init if cond_feat else self.init),
                                    out=self.eps.out)

            mark("scale", scale)
            mark("step0", one)                                                       # tsteps row 0: the utterances' own t

        if objective:
            objective_tail()
        else:
            mark("prologue", prologue)
            # diffusion-step rows are stored in loop order: row i is step n = S-1-i
            self.eps.tsteps.copy_(torch.from_numpy(np.ascontiguousarray(Tarr[::-1]))[:, None].expand(S, KB))
        for i in range(0 if objective else S):
            nstep = S - 1 - i

            def one(i=i, nstep=nstep):
                self.eps.build_step(i, x=self.audio, x_init=None if deltamu else (self.eps.x_init if cond_feat else self.init),
                                    out=self.eps.out)
                if nstep > 0:
                    ew(L.EW_UPDATE, self.audio, b=self.eps.out, out=self.audio, s0=float(c1[nstep]), s1=float(c2[nstep]))
                else:
                    ew(L.EW_UPDATE_FINAL, self.audio, b=self.eps.out, c=self.zero if self.zero is not None else self.init,
                       out=self.members_spec,
                       s0=float(c1[0]), s1=float(c2[0]), s2=PRIOR_SCALE_C)

            mark("step%d" % nstep, one)
        if self.istft is not None:
            mark("istft", lambda: self.istft.build(spec=self.spec, c=self.stft.c))
        if self.verdict:
            def count():
                rows = []
                for t in (self.spec,) + ((self.istft.wav,) if with_signal else ()):
                    r = L.RangeRow()                               # an fp32 tensor: pointer and length, nothing else is read
                    r.ptr, r.n = t.data_ptr(), t.numel()
                    rows.append(r)
                self._verdict_count = len(self.descs)
                range_launch(L.RANGE_NONFINITE, rows, tab=self.verdict_tab)

            mark("verdict", count)                                 # last launch of the plan
        self.label = self.objective = None
        if label or objective:
            if not with_signal:
                raise ValueError("the label leg needs the signal front / back end (pass L_)")
            if self.plan is not None:
                self.label = LabelLeg(self, back=not objective)
                if objective:
                    self.objective = ObjectiveLeg(self, "deltamu" if deltamu else ("plain" if cond_feat else "pirorgrad"), use_sigma,
                                                  params.noise_schedule)
        if self.plan is not None:
            self.plan.keep(ctx.keep, ctx.bank)
        self._graph_stream = None

    # ------------------------------------------------------------------
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _whole_file_only(self, what):
        """A pipeline built with ``window=W`` for more than W frames holds a ``LongSampler`` and no whole-file plan."""
        if getattr(self, "long", None) is not None:
            raise ValueError("%s on a pipeline built with window=%d for %d frames: it records no whole-file plan - enhance() and "
                             "check() run the windowed pass (self.long)" % (what, self.window, self.T))

    def run(self, first=None, last=None, graph=False):
        """Run ranges first..last (names from ``self.ranges``), whole plan by default."""
        self._whole_file_only("run")
        if graph:
            self._members_xT(None, True)          # an ensemble plan: ValueError
        if self.plan is None:
            raise L.PdseError("SamplerPipeline built on a CPU context cannot run: there is no CPU fallback")
        if graph:
            if first is not None or last is not None:
                raise ValueError("graph replay always runs the whole plan")
            if not self.plan.has_graph:
                self._graph_stream = torch.cuda.Stream(self.device)
                with torch.cuda.stream(self._graph_stream):
                    self.plan.build_graph(self._graph_stream.cuda_stream)
                self._graph_stream.synchronize()
            self.plan.launch_graph(self._stream())
            self._ranges_run = set(self.ranges)
            return
        b = self.ranges[first][0] if first else 0
        e = self.ranges[last][1] if last else len(self.descs)
        if self.audited and not b <= self._range_clear < e:
            c = self._range_clear                              # a call that starts later still starts from a cleared table
            self.plan.run_range(c, c + 1, self._stream())
        if self.verdict and not b <= self._verdict_clear < e:
            self.plan.run_range(self._verdict_clear, self._verdict_clear + 1, self._stream())
        self.plan.run_range(b, e, self._stream())
        if self.verdict and not b <= self._verdict_count < e:  # a call that ends earlier is judged too: the buffers as it left them
            self.plan.run_range(self._verdict_count, self._verdict_count + 1, self._stream())
        self._ranges_run = {k for k, (rb, re_) in self.ranges.items() if b <= rb and re_ <= e}

    def range_report(self):
        """Synchronises, copies the histogram table of the last pass to the host (a few KB) and returns its
        ``rangeaudit.RangeReport``: per (marked range, audited tensor) ``name``, ``range``, ``count``, ``hist[32]``,
        ``max_binade``, ``below_frac``, ``below``, ``above``; ``ok``, ``worst()`` and a printable table over all of them.  The
        verdicts follow from the format (derivation: the docstring of ``rangeaudit``): an f16x2 pair carries 11 + 11 significand
        bits, |x - hi - lo| <= 2^-23 |x|, only while hi's exponent is >= -2 in scaled units (lo a normal fp16, or its subnormal
        error still inside the bound) - 2^-6 in true scale with PDSE_F16_ACT_EXP = 4.  ``below``: the tensor's largest non-zero
        magnitude is under that edge, no element of it is carried at full precision; ``below_frac``: the share of its non-zero
        elements under the edge; ``above``: an element reached 2^15 scaled, the binade in which hi becomes an infinity (or was
        not finite).  A pipeline built without ``audit=True`` raises ValueError; one built with it whose arithmetic has no
        window (split "bf16x3") returns an empty report.
        The report is that of the last ``run()`` call: every call starts from a cleared table, and only the rows of the marked
        ranges that call executed are reported (a pipeline stepped range by range reports the last range; rows of ranges that
        did not run would be all-zero and read as clean)."""
        self._whole_file_only("range_report")
        if not self.audit:
            raise ValueError("the pipeline was built without the range audit (SamplerPipeline(audit=True))")
        if not self.audited:
            return rangeaudit.RangeReport([])
        hist = self.range_hist[:len(self.range_rows)].cpu().numpy().view(np.uint32)     # synchronises
        return rangeaudit.RangeReport(rangeaudit.ReportRow(tname, rname, hist[i]) for i, (rname, tname) in enumerate(self.range_rows)
                                      if rname in self._ranges_run)

    def verdict_fetch(self, stream=None):
        """Enqueue, on ``stream`` (a ``torch.cuda.Stream``; None: the current one), the copy of the verdict table of the pass
        that stream ran last into the pinned host buffer this pipeline owns.  Asynchronous: nothing is synchronised."""
        if not self.verdict:
            raise ValueError("the pipeline was built without the verdict (SamplerPipeline(verdict=True))")
        if self.plan is None:
            raise L.PdseError("SamplerPipeline built on a CPU context cannot run: there is no CPU fallback")
        with torch.cuda.stream(torch.cuda.current_stream(self.device) if stream is None else stream):
            self._verdict_host.copy_(self.verdict_tab, non_blocking=True)

    def verdict_counts(self):
        """The Inf / NaN counts the last ``verdict_fetch`` brought to the host, as Python ints: (spec,), or (spec, wav) with the
        signal back end.  The caller has waited for an event recorded on the fetch's stream behind it (or synchronised);
        nothing is synchronised here.  All zero: the pass's results are finite."""
        if not self.verdict:
            raise ValueError("the pipeline was built without the verdict (SamplerPipeline(verdict=True))")
        if self._verdict_host is None:
            raise L.PdseError("SamplerPipeline built on a CPU context cannot run: there is no CPU fallback")
        return tuple(int(v) & 0xffffffff for v in self._verdict_host[:, 0].tolist())

    @property
    def init_spec(self):
        """X_init of the last pass, [B,2,T,161], at the scale of the label and of ``spec``: the prior's output as it is (the
        reverse loop runs on ``init`` = X_init / 11; the reference multiplies it back, :495)."""
        return self.prior.out

    @property
    def windowed(self):
        """True where the pass multiplies f16x2 operands: the arithmetic with an fp16 window, which a pass can leave."""
        return self.split == "f16x2" and bool(self.split_bf16) and self.dtype == "f32"

    @staticmethod
    def nonfinite_error(where=""):
        """The ``PdseRangeError`` of an f16x2 pass whose result is not finite (``check()``, and a non-zero verdict)."""
        return L.PdseRangeError("non-finite values in the enhanced spectrogram of an f16x2 pass%s: an activation beyond +-%g left the fp16 "
                                "window (include/pdse.h: PDSE_F16_ACT_EXP), or the input was not finite; build the pipeline with "
                                "split='bf16x3' (ComplexDDPMTrainer does so for this geometry by itself)" % (where, 65504.0 / 2 ** packing.F16_ACT_EXP))

    def check(self, audit=False):
        """Synchronises and raises if a persistent launch of the last run gave up (its workgroups wait for each other
        with bounded polls: another workload on the GPU can keep them from all being resident), or - f16x2 passes - if the
        result is not finite: an activation left the top of the fp16 window (``PdseRangeError``; an audited pipeline names the
        tensor).  audit=True (pipelines built with ``audit=True``): also reads the range report and raises ``PdseRangeError``
        naming the first tensor, and its marked range, that lay wholly below the window - the case that leaves no other trace."""
        if getattr(self, "long", None) is not None:
            return self.long.check()
        for net, field, what in ((self.prior, "status", "persistent LSTM gave up at step %d"), (self.eps, "tcm_status", "TCM stack launch gave up at block %d"),
                                 (self.prior, "tcm_status", "TCM stack launch of the prior gave up at block %d")):
            st = getattr(net, field, None)
            if st is not None:
                code = int(st[0].item())
                if code:
                    st.zero_()
                    raise L.PdseError((what % (code - 1)) + ": its workgroups wait for each other and were not all resident in time (is "
                                      "another workload sharing the GPU?); build the pipeline with exclusive=False")
        if self.windowed and not bool(torch.isfinite(self.spec).all()):
            where = ""
            if self.audited:
                top = self.range_report().above()
                if top:
                    where = " (range audit: first in %s of %s)" % (top[0].name, top[0].range)
            raise self.nonfinite_error(where)
        if audit:
            low = self.range_report().below()
            if low:
                raise L.PdseRangeError("range audit: every non-zero element of %s in %s is below 2^%d, the bottom of the fp16 window of an f16x2 "
                                       "pass (include/pdse.h: PDSE_F16_ACT_EXP): the tensor is not carried at fp32-equivalent precision "
                                       "(%d tensors in all); build the pipeline with split='bf16x3' (ComplexDDPMTrainer(audit=True) does so "
                                       "for this geometry by itself)" % (low[0].name, low[0].range, -2 - packing.F16_ACT_EXP, len(low)))

    def sample(self, feat, x_T, graph=False):
        """feat, x_T [B,2,T,161] -> (enhanced compressed spectrogram, X_init); the
        spectrogram-level body of generate_wav (:939-998)."""
        SamplerPipeline._whole_file_only(self, "sample")
        if self.xT_in is None:
            raise ValueError("an objective plan has no sampler (SamplerPipeline(objective=True): objective_pass)")
        x_T = SamplerPipeline._members_xT(self, x_T, graph)    # not a bound call: the argument checks run on any object with the fields
        _expect(feat, self.feat, "feat")
        _expect(x_T, self.xT_in, "x_T")
        self.feat.copy_(feat)
        self.xT_in.copy_(x_T)
        if self.members > 1:
            self._run_members("prior", None, back=False)
        elif graph and self.stft is None:
            self.run(graph=True)
        else:
            self.run("prior", "step0")
        return self.spec.clone(), self.prior.out.clone()

    def _members_xT(self, x_T, graph):
        """The x_T of a pass as the plan holds it: an ensemble's [K,B,2,T,161] as [K B,2,T,161] (member-major either way);
        ``graph=True`` on an ensemble plan: ValueError."""
        K = getattr(self, "members", 1)
        if graph and K > 1:
            raise ValueError("graph=True with members=%d: the ensemble kernel is a plain-argument launch between the plan's ranges, "
                             "not part of the plan or of its hipGraph" % K)
        if x_T is not None and x_T.dim() == 5 and x_T.shape[0] == K:      # K = 1 too: [1,B,2,T,161] is one member
            x_T = x_T.reshape((-1,) + tuple(x_T.shape[2:]))
        return x_T

    def _run_members(self, first, frames, back=True):
        """An ensemble pass (``members`` > 1): the ranges ``first`` .. "step0", whose last launch leaves the K members in
        ``members_spec``; ``pdse_ensemble_stats`` on them - the mean into ``spec``, the rest into ``ensemble`` (frames: every
        utterance's own frames for the masked sums, None: all T); then, with ``back``, the range "istft" on the mean."""
        from . import ops

        self.run(first, "step0")
        with torch.cuda.device(self.device):
            if self.ensemble is None:
                self._spread = torch.empty(self.B, self.T, F0, dtype=torch.float32, device=self.device)
            self.ensemble = ops.ensemble_stats(self.members_spec, self.members, [self.T] * self.B if frames is None else frames,
                                               out=(self.spec, self._spread))
        if back and self.istft is not None:
            self.plan.run_range(*self.ranges["istft"], self._stream())   # not ``run``: the pass is one, its audit table is cleared once
            self._ranges_run = set(self.ranges)

    def enhance(self, wav, x_T, graph=False, lens=None, exact=False, clean=None):
        """wav [B,L], x_T [B,2,T,161] -> (enhanced wav [B,L], spectrogram [B,2,T,161]).
        lens: true lengths of zero-padded utterances (RMS normalisation over each utterance's own samples,
        utils/dataset.py:45-58); default: every utterance fills L.
        exact (pipelines built with ``ragged=True``, and only those): every utterance as if enhanced alone - see ``ragged`` in
        the constructor; samples behind ``lens[b]`` and frames behind ``1 + lens[b] // 160`` are zeros in both results.
        False on a ragged pipeline: the padding takes part, as on a dense one (its tables are set to the full length).
        clean (pipelines built with ``label=True``): the clean partners of ``wav``, [B,L], zero-padded like it.  The pass then
        also runs the label leg and leaves its results on the device, in buffers the next pass overwrites: ``label.spec`` (the
        label spectrogram), ``spec`` (the final one, as ever), ``init_spec`` (the prior's output at the label's scale, what the
        reference's loop holds after ``init_audio *= self.c``) and the waveforms ``label.wav``, ``label.init_wav`` and
        ``label.est_wav`` - label, X_init and the final spectrogram decompressed and inverted, in the normalised domain (not
        rescaled by c).  The returned pair is what it is without ``clean``.
        Pipelines built with ``members=K`` > 1: x_T is [K,B,2,T,161] or [K B,2,T,161], member-major; the returned pair is the
        ensemble mean's - ``spec`` and the waveform the back end makes of it - and the pass leaves ``members_spec`` and
        ``ensemble`` (its masked sums over ``1 + lens[b] // 160`` frames); ``graph=True``: ValueError.
        Pipelines built with ``window=W`` for more than W frames: the windowed pass (``LongSampler.enhance``); ``graph``, ``lens``,
        ``exact`` and ``clean`` are then refused."""
        if getattr(self, "long", None) is not None:     # (the argument checks below run on any object with the fields)
            longplan.window_conflicts(graph=graph, ragged=exact or lens is not None, label=clean is not None)
            return self.long.enhance(wav, x_T)
        if self.stft is None:
            raise ValueError("pipeline was built without the signal front/back end (pass L_)")
        if self.xT_in is None:
            raise ValueError("an objective plan has no sampler (SamplerPipeline(objective=True): objective_pass)")
        x_T = SamplerPipeline._members_xT(self, x_T, graph)    # not a bound call: the argument checks run on any object with the fields
        _expect(wav, self.stft.wav, "wav")
        _expect(x_T, self.xT_in, "x_T")
        if clean is not None:
            if self.label is None:
                raise ValueError("clean= needs a pipeline recorded with label=True")
            _expect(clean, self.label.clean, "clean")
        if exact:
            if not self.ragged:
                raise ValueError("exact=True needs a pipeline recorded with ragged=True (the dense plan has no length tables)")
            lens_h, frames_h = ragged_tables(self.L if lens is None else lens, self.B, self.L)
        self.stft.wav.copy_(wav)
        self.xT_in.copy_(x_T)
        if lens is None:
            self.stft.lens.fill_(self.L)
        else:
            self.stft.lens.copy_(torch.as_tensor(lens, dtype=torch.int32))
        if self.ragged:
            if exact:
                self.frames_tab.copy_(torch.from_numpy(frames_h))
                self.valid_tab.copy_(torch.from_numpy(np.repeat(frames_h * F0, 2)))
            else:
                self.frames_tab.fill_(self.T)
                self.valid_tab.fill_(self.T * F0)
        if clean is not None:
            self.label.clean.copy_(clean)
            self.label.prepare(self._stream())     # behind the copies of wav, clean and lens, ahead of the pass
        if self.members > 1:      # the masked sums over every utterance's own frames, 1 + len // 160
            self._run_members(None, None if lens is None else [1 + int(n) // 160 for n in lens])
        else:
            self.run(graph=graph)
        if clean is not None:
            self.label.run(self._stream())
        wav_out, spec = self.istft.wav.clone(), self.spec.clone()
        if exact:     # frames behind an utterance's own: zeros in the returned tensor (the overlap-add zeroed the samples itself)
            dead = torch.arange(self.T, device=self.device)[None, :] >= self.frames_tab[:, None]
            spec.masked_fill_(dead[:, None, :, None], 0.0)
        return wav_out, spec


    def objective_pass(self, wav, clean, t, noise, lens=None):
        """One evaluation of the denoising objective (trainer/complex_ddpm_trainer.py:699-733) on a plan recorded with
        ``objective=True``: wav, clean [B,L] zero-padded pairs, lens their own lengths (as for ``enhance``: the padding takes
        part); t [B] integer diffusion steps, a host tensor is range-checked (IndexError), a device tensor is used as it is;
        noise [B,2,T,161].  Front (wav prep, STFT, compression, prior, label spectrogram), X_init / 11 and label / 11, the
        noising at every utterance's own step, one eps-net step with ``tsteps = t``.  Afterwards, in buffers the next pass
        overwrites: ``spec`` (the prediction), ``audio`` (noisy), ``init`` (X_init / 11), ``init_spec`` (X_init), ``label.spec``
        (the label) and ``objective.label`` (label / 11), ``.noise``, ``.target``, ``.maxbuf``, ``.t``.  Returns ``spec``.
        Nothing is synchronised."""
        leg = self.objective
        if leg is None:
            raise ValueError("objective_pass needs a pipeline recorded with objective=True")
        _expect(wav, self.stft.wav, "wav")
        _expect(clean, self.label.clean, "clean")
        _expect(noise, leg.noise, "noise")
        t = torch.as_tensor(t)
        if tuple(t.shape) != (self.B,) or t.dtype.is_floating_point:
            raise ValueError("t: expected %d integer diffusion steps" % self.B)
        if not t.is_cuda and (int(t.min()) < 0 or int(t.max()) >= len(leg.noise_schedule)):
            raise IndexError("diffusion step outside the %d-entry noise schedule" % len(leg.noise_schedule))
        self.stft.wav.copy_(wav)
        self.label.clean.copy_(clean)
        leg.noise.copy_(noise)
        leg.t.copy_(t)
        self.eps.tsteps.copy_(leg.t.view(1, self.B))     # the step embedding's row, as floats
        if lens is None:
            self.stft.lens.fill_(self.L)
        else:
            self.stft.lens.copy_(torch.as_tensor(lens, dtype=torch.int32))
        stream = self._stream()
        self.label.prepare(stream)             # behind the copies of wav, clean and lens, ahead of the pass
        self.run("stft", "scale")
        self.label.plan.run(stream)
        leg.run(stream)
        self.plan.run_range(*self.ranges["step0"], stream)     # not ``run``: the pass is one, its audit table is cleared once
        self._ranges_run = set(self.ranges)
        return self.spec


class LabelLeg:
    """The label leg of a validation pass (``SamplerPipeline(label=True)``): what the reference's validation loop needs beside
    the enhancement (trainer/complex_ddpm_trainer.py:408-559, utils/dataset.py:45-74, utils/metrics.py:528-566), as direct
    calls and two small plans beside the pipeline's:

        prepare   pdse_pair_prep (csrc/valid.hip; a plain-argument call, not recordable): the noisy rows' c, both rows / c,
                  reflect-padded.  The noisy outputs go where the pipeline's own wavprep launch writes the same bits (its
                  ``stft.xpad``, ``stft.c``); the clean rows into this leg's STFT input.
        front     (plan) STFT GEMM + compression (the pipeline's ``feat_type``) of the clean rows -> ``spec`` (the label).
        frames    pdse_spec_frames (pdse_spec_frames_mode for a feat_type other than "sqrt"; csrc/valid.hip, plain arguments) on the label, on the prior's output and on the final
                  spectrogram: decompression and windowed inverse DFT in double, frames rounded to fp32 once.
        back      (plan) the overlap-add operator on the three frame tensors, without the rescale by c -> ``wav`` (label),
                  ``init_wav``, ``est_wav``.

    All waveforms are in the normalised domain, as compare_complex compares them.  They do not reuse the pipeline's own ISTFT
    frames: its fp32 decompression and GEMM lie 2e-6 from a double transform, which a score of 20 - 27 dB over a few frames
    shows in its fifth decimal.  On a ragged pipeline the leg uses its length tables: the clean rows reflect
    at their own end and the overlap-adds stop at an utterance's own frames and samples in an exact pass."""

    def __init__(self, pipe, back=True):
        """back False: ``prepare`` and the front only - the label spectrogram, which is all the objective plan needs of the leg."""
        from . import ops

        ctx, B, T, L_ = pipe.ctx, pipe.B, pipe.T, pipe.L
        self.pipe = pipe
        self.plan = L.Plan(pipe.device)
        self.stft = nets.StftPlan(ctx, B, L_, plan=self.plan, split_bf16=pipe.stft.split_bf16, reflect_own=pipe.ragged,
                                  feat_type=pipe.feat_type)
        self.clean, self.spec = self.stft.wav, self.stft.feat
        self.stft.build(prep=False)
        self.plan.keep(ctx.keep, ctx.bank)
        self.descs = self.stft.descs
        if not back:
            return
        self.basis, win2 = ops.frame_tables(pipe.device)
        lens = pipe.stft.lens if pipe.ragged else None
        self.back = nets.PlanBase(ctx, L.Plan(pipe.device))
        self.frames, wavs = [], []
        for _ in range(3):
            fr, wav = ctx.alloc(B, 320, T), ctx.alloc(B, L_)
            o = L.OlaDesc()
            o.frames, o.win2, o.c, o.out = fr.data_ptr(), win2.data_ptr(), 0, wav.data_ptr()
            o.B, o.T, o.L, o.n_fft, o.hop = B, T, L_, 320, 160
            o.nframes, o.lens = nets.Ctx.ptr(pipe.frames_tab), nets.Ctx.ptr(lens)
            self.back.add(o, nets.TAG_SIGNAL)
            self.frames.append(fr)
            wavs.append(wav)
        self.wav, self.init_wav, self.est_wav = wavs
        self.back.plan.keep(ctx.keep, win2, self.basis)
        self.descs = self.stft.descs + self.back.descs

    def prepare(self, stream):
        p = self.pipe.stft
        L.pair_prep(p.wav.data_ptr(), self.clean.data_ptr(), p.lens.data_ptr(), p.xpad.data_ptr(), self.stft.xpad.data_ptr(),
                    p.c.data_ptr(), p.B, p.L, 160, 1 if p.reflect_own else 0, stream, device=self.pipe.device)

    def run(self, stream):
        pipe = self.pipe
        self.plan.run(stream)
        mode = L.DECOMPRESS_MODE[pipe.feat_type]
        for spec, fr in zip((self.spec, pipe.prior.out, pipe.spec), self.frames):
            if mode == L.COMPAND_SQUARE:
                L.spec_frames(spec.data_ptr(), self.basis.data_ptr(), fr.data_ptr(), pipe.B, pipe.T, F0, stream, device=pipe.device)
            else:
                L.spec_frames_mode(spec.data_ptr(), self.basis.data_ptr(), fr.data_ptr(), pipe.B, pipe.T, F0, mode, stream,
                                   device=pipe.device)
        self.back.plan.run(stream)


class ObjectiveLeg:
    """What the objective plan (``SamplerPipeline(objective=True)``) holds beside the shared front: the buffers of the forward
    noising of trainer/complex_ddpm_trainer.py:699-733 and one small plan.

        scale     (plan) label / 11 (:699) on the label leg's spectrogram -> ``label``; X_init / 11 is the pipeline's own range
                  "scale", written where the eps-net reads its conditioning input.
        noising   pdse_objective_noise (csrc/objective.hip; a plain-argument call, not recordable) on ``label``, the pipeline's
                  ``init``, ``noise`` and the step row ``t`` -> the eps-net's input (``pipe.audio``), ``target``, ``maxbuf``.

    mode: "pirorgrad", "deltamu" or "plain" (``ops.NOISING_MODES``); sigma: the --sigma mask and target."""

    def __init__(self, pipe, mode, sigma, noise_schedule):
        ctx, B, T = pipe.ctx, pipe.B, pipe.T
        if len(noise_schedule) > 50:
            raise ValueError("the objective draws t below len(noise_schedule) = %d, the step embedding has 50 entries" % len(noise_schedule))
        self.pipe, self.sigma, self.noise_schedule = pipe, bool(sigma), list(noise_schedule)
        self.mode = mode
        self.label, self.noise, self.target = ctx.alloc(B, 2, T, F0), ctx.alloc(B, 2, T, F0), ctx.alloc(B, 2, T, F0)
        self.maxbuf = ctx.alloc(2 * B)
        self.t = torch.zeros(B, dtype=torch.int32, device=pipe.device)
        ctx.keep.append(self.t)
        self.scale = nets.PlanBase(ctx, L.Plan(pipe.device))
        d = L.EwDesc()
        d.a, d.out, d.n, d.s0, d.op = pipe.label.spec.data_ptr(), self.label.data_ptr(), self.label.numel(), PRIOR_SCALE_C, L.EW_DIV
        self.scale.add(d, nets.TAG_EW)
        self.scale.plan.keep(ctx.keep)
        self.descs = self.scale.descs

    def run(self, stream):
        """Behind the pipeline's ranges "stft" .. "scale" and the label leg's front: label / 11, then the noising."""
        from . import ops

        pipe = self.pipe
        self.scale.plan.run(stream)
        ops.noising(self.label, pipe.init, self.t, self.noise, mode=self.mode, sigma=self.sigma, noise_schedule=self.noise_schedule,
                    out=(pipe.audio, self.target, self.maxbuf))


class ConcurrentSampler:
    """The same path with the batch cut into ``nsplit`` contiguous sub-batches, each a complete
    ``SamplerPipeline`` replayed on its own HIP stream.

    Why: the path alternates MFMA-bound phases (BiConvGLU blocks) with strictly sequential,
    latency-bound ones (401 LSTM frames x 2 layers, 18 dilated TCM residuals x 6 steps) that
    leave most of the 256 CUs idle.  Utterances are independent, so while one sub-batch walks
    its LSTM/TCM chain the other's convolutions fill the chip.  Results are bit-identical to
    the single-pipeline run (tiling never crosses a batch item)."""

    def __init__(self, device, prior_name, prior_sd, ddpm_sd, B, T=None, L_=None, nsplit=2, **kw):
        from .shard import shard_range

        self.device = torch.device(device)
        self.B, self.nsplit = B, max(1, min(nsplit, B))
        self.spans = [shard_range(B, self.nsplit, r) for r in range(self.nsplit)]
        kw.setdefault("bank", nets.WeightBank())    # one packed copy of the weights for all sub-batch pipelines
        kw["exclusive"] = False                     # the sub-batches share the GPU: no launch may wait for its own workgroups
        self.pipes = [SamplerPipeline(device, prior_name, prior_sd, ddpm_sd, hi - lo, T=T, L_=L_, **kw)
                      for lo, hi in self.spans]
        self.T, self.L = self.pipes[0].T, self.pipes[0].L
        self.nsteps = self.pipes[0].nsteps
        self.streams = [torch.cuda.Stream(self.device) for _ in self.pipes]
        self._graphs = False

    def _run_all(self, graph, first=None, last=None):
        cur = torch.cuda.current_stream(self.device)
        start = torch.cuda.Event()
        start.record(cur)
        for p, s in zip(self.pipes, self.streams):
            s.wait_event(start)
            with torch.cuda.stream(s):
                if graph:
                    if not p.plan.has_graph:
                        p.plan.build_graph(s.cuda_stream)
                    p.plan.launch_graph(s.cuda_stream)
                else:
                    b = p.ranges[first][0] if first else 0
                    e = p.ranges[last][1] if last else len(p.descs)
                    p.plan.run_range(b, e, s.cuda_stream)
            done = torch.cuda.Event()
            done.record(s)
            cur.wait_event(done)

    def enhance(self, wav, x_T, graph=False):
        for p, (lo, hi) in zip(self.pipes, self.spans):
            p.stft.wav.copy_(wav[lo:hi])
            p.xT_in.copy_(x_T[lo:hi])
        self._run_all(graph)
        return (torch.cat([p.istft.wav for p in self.pipes], 0), torch.cat([p.spec for p in self.pipes], 0))

    def sample(self, feat, x_T, graph=False):
        for p, (lo, hi) in zip(self.pipes, self.spans):
            p.feat.copy_(feat[lo:hi])
            p.xT_in.copy_(x_T[lo:hi])
        if graph and self.pipes[0].stft is None:
            self._run_all(True)
        else:
            self._run_all(False, "prior", "step0")
        return (torch.cat([p.spec for p in self.pipes], 0), torch.cat([p.prior.out for p in self.pipes], 0))


class PipelinedSampler:
    """Throughput mode for a stream of batches: two ``SamplerPipeline`` instances (ping-pong
    buffers) and two HIP streams.  Stage 1 of batch n+1 (STFT + prior — dominated by the
    latency-bound LSTM frame chain, which leaves most CUs idle) runs on the *prior* stream
    while stage 2 of batch n (reverse loop + ISTFT — MFMA-bound) runs on the *loop* stream.
    Per-batch results are bit-identical to ``SamplerPipeline.enhance``; only the schedule
    differs.  ``submit`` returns immediately; ``result`` waits for that batch."""

    # measurement switch (bench.py --inflight-stack): let the in-flight pipelines use the launches that wait for their own workgroups
    # (the TCM stack as one launch; at B = 32 nothing else).  Measured slower in rounds 4 (17.8 vs 17.4 ms) - see DESIGN.md 4.1b.
    stack_in_flight = False

    def __init__(self, device, prior_name, prior_sd, ddpm_sd, B, L_, depth=2, by_batch=False, graph=True, **kw):
        """depth: batches in flight (= buffer sets).  by_batch False: two stage streams (prior | loop);
        True: every batch runs start to end on its own stream, ``depth`` streams round-robin."""
        self.device = torch.device(device)
        self.depth, self.by_batch, self.graph = depth, by_batch, graph
        kw.setdefault("bank", nets.WeightBank())    # the in-flight buffer sets share one packed copy of the weights
        kw["exclusive"] = bool(self.stack_in_flight)   # batches in flight share the GPU: no launch may wait for its own workgroups
        self.pipes = [SamplerPipeline(device, prior_name, prior_sd, ddpm_sd, B, L_=L_, **kw) for _ in range(depth)]
        self.s_prior = torch.cuda.Stream(self.device, priority=-1)   # tiny dependent launches: schedule them first
        self.s_loop = torch.cuda.Stream(self.device)
        self.s_batch = [torch.cuda.Stream(self.device) for _ in range(depth)] if by_batch else []
        self.n = 0
        self.done = [None] * depth      # event: batch in slot finished
        self.nsteps = self.pipes[0].nsteps
        if by_batch and graph:          # capture every buffer set's graph now, not inside somebody's timed region
            for p, st in zip(self.pipes, self.s_batch):
                with torch.cuda.stream(st):
                    p.plan.build_graph(st.cuda_stream)
            torch.cuda.synchronize(self.device)

    def submit(self, wav, x_T):
        slot = self.n % self.depth
        p = self.pipes[slot]
        if self.by_batch:
            cur = torch.cuda.current_stream(self.device)
            ready = torch.cuda.Event()
            ready.record(cur)
            st = self.s_batch[slot]
            with torch.cuda.stream(st):
                st.wait_event(ready)                              # same stream as the slot's previous batch: ordered
                for src in (wav, x_T):                            # inputs were allocated on the caller's stream: tell
                    if src.is_cuda:                               # the caching allocator this stream still reads them
                        src.record_stream(st)
                p.stft.wav.copy_(wav, non_blocking=True)
                p.xT_in.copy_(x_T, non_blocking=True)
                if self.graph:        # one hipGraph per in-flight buffer set: ~8000 launches become one host call
                    if not p.plan.has_graph:
                        p.plan.build_graph(st.cuda_stream)
                    p.plan.launch_graph(st.cuda_stream)
                else:
                    p.plan.run_range(0, len(p.descs), st.cuda_stream)
                self.done[slot] = torch.cuda.Event()
                self.done[slot].record(st)
            self.n += 1
            return slot
        cur = torch.cuda.current_stream(self.device)
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(self.s_prior):
            self.s_prior.wait_event(ready)
            if self.done[slot] is not None:
                self.s_prior.wait_event(self.done[slot])      # the slot's buffers are free again
            for src in (wav, x_T):
                if src.is_cuda:
                    src.record_stream(self.s_prior)
            p.stft.wav.copy_(wav, non_blocking=True)
            p.xT_in.copy_(x_T, non_blocking=True)
            p.plan.run_range(p.ranges["stft"][0], p.ranges["prior"][1], self.s_prior.cuda_stream)
            staged = torch.cuda.Event()
            staged.record(self.s_prior)
        with torch.cuda.stream(self.s_loop):
            self.s_loop.wait_event(staged)
            p.plan.run_range(p.ranges["prologue"][0], len(p.descs), self.s_loop.cuda_stream)
            self.done[slot] = torch.cuda.Event()
            self.done[slot].record(self.s_loop)
        self.n += 1
        return slot

    def result(self, slot):
        torch.cuda.current_stream(self.device).wait_event(self.done[slot])
        p = self.pipes[slot]
        return p.istft.wav, p.spec

    def drain(self):
        cur = torch.cuda.current_stream(self.device)
        for e in self.done:
            if e is not None:
                cur.wait_event(e)


class LongSampler:
    """Recordings of any length through ONE window plan (``SamplerPipeline(window=W)``, ``ComplexDDPMTrainer(window=W)``).

    What grows with the frame count T and is small stays whole-file, in buffers re-made when the length changes: the waveforms, the
    [B,2,T,161] spectrograms (feature, X_init, X_init / 11, x_T, two copies of x_t, the result) and the front / back end with its
    frame GEMMs, recorded per length exactly as ``SamplerPipeline`` records them.  The two networks exist once, as ``win``: a
    ``SamplerPipeline`` of W frames without the signal ends, ``exclusive=False``, whose activation set serves every window, every
    step and every file.  One pass:

        front      wav prep, STFT, compression                          whole-file plan, as ever
        prior      GCRN: consecutive windows (``longplan.carried``), the LSTM's h and c handed from each to the next
                   (pdse_glstm_desc.state_in / state_out; zeros at the start of the file)
                   DiffUNet: windows with halos (``longplan.windows`` at the prior's receptive field)
        prologue   X_init / 11, x_T (+ X_init / 11), the --sigma mask   whole-file launches of the operators the one-plan pass
                   records: the mask's per-utterance maximum is taken over the whole file, once
        steps      step-major: for n = S-1 .. 0, for every window (``longplan.windows`` at the eps-net's receptive field):
                   gather x_n and the condition, one eps-net step and the update on the window, scatter of the kept frames of
                   x_{n-1} into the second whole-file buffer; then the buffers swap.  The field is two-sided, so a window needs
                   x_n of frames a later window owns: no window may run ahead of the others.
        back       decompression, inverse frames, overlap-add            whole-file plan, as ever

    pdse_window_gather / pdse_window_scatter (csrc/window.hip) move the frames.  The priors that attend over all frames have no
    receptive field (``prior_check``: ValueError)."""

    @staticmethod
    def prior_check(prior_name):
        if prior_name not in ("GCRN", "DiffUNet"):
            raise ValueError("window=: prior %r attends and runs a bidirectional GRU over all T frames, it has no finite receptive "
                             "field and no state to carry (supported priors: GCRN, DiffUNet)" % prior_name)

    def __init__(self, device, prior_name, prior_sd, ddpm_sd, B, window, fast_sampling=True, use_sigma=False, params=default_params,
                 deltamu=False, cond="init", bank=None, split_bf16=None, xT_plus_init=None, dtype="f32", split=None, feat_type="sqrt"):
        self.prior_check(prior_name)
        self.W = W = longplan.window_arg(window)
        if W is None:
            raise ValueError("LongSampler needs a window length")
        self.device = torch.device(device)
        self.B, self.prior_name, self.use_sigma, self.feat_type = B, prior_name, bool(use_sigma), L.feat_type_of(feat_type)
        self.win = win = SamplerPipeline(device, prior_name, prior_sd, ddpm_sd, B, T=W, with_signal=False, fast_sampling=fast_sampling,
                                         use_sigma=False, params=params, deltamu=deltamu, cond=cond, bank=bank, split_bf16=split_bf16,
                                         xT_plus_init=xT_plus_init, dtype=dtype, exclusive=False, split=split, carry_state=True)
        self.bank = win.bank
        sb = bool(fast_sampling) if split_bf16 is None else split_bf16      # as SamplerPipeline hands it to its front and back end
        self._split_front, self._split_back = sb, True if dtype == "bf16" else sb
        self.eps_field = win.eps.receptive_field()
        self.prior_field = win.prior.receptive_field()
        self.carried = bool(win.prior.carries_state)
        longplan.windows(W + 1, W, *self.eps_field)                          # ValueError: W does not exceed the field
        if not self.carried:
            longplan.windows(W + 1, W, *self.prior_field)
        self.nsteps = win.nsteps
        self._time = win.eps.time_index                                       # the launch of the steps' folded time biases
        self.L = self.T = None
        self.spec = None

    # ------------------------------------------------------------------
    def _whole(self, L_):
        """The whole-file side for recordings of L_ samples: buffers and the front / back end, re-made when the length changes."""
        if self.L == L_:
            return
        win, B = self.win, self.B
        T = 1 + L_ // 160
        ctx = nets.Ctx(self.device, self.bank)
        self.stft = nets.StftPlan(ctx, B, L_, split_bf16=self._split_front, feat_type=self.feat_type)
        self.istft = nets.IstftPlan(ctx, B, T, L_, split_bf16=self._split_back, feat_type=self.feat_type)
        a = ctx.alloc
        self.feat, self.xinit, self.init, self.xT_in = a(B, 2, T, F0), a(B, 2, T, F0), a(B, 2, T, F0), a(B, 2, T, F0)
        self.x = [a(B, 2, T, F0), a(B, 2, T, F0)]
        self.featc = a(B, 2, T, F0) if win.cond_feat else None
        self.spec = self.istft.spec
        self.stft.build(feat=self.feat)
        self.istft.build(spec=self.spec, c=self.stft.c)
        # the prologue of the one-plan pass (SamplerPipeline.__init__: prologue) on the whole-file tensors
        pro = self.pro = nets.PlanBase(ctx)
        n = B * 2 * T * F0

        def ew(op, a_, b=None, out=None, s0=0.0):
            d = L.EwDesc()
            d.a, d.b, d.c, d.out = a_.data_ptr(), nets.Ctx.ptr(b), 0, out.data_ptr()
            d.n, d.s0, d.s1, d.s2, d.op = n, s0, 0.0, 0.0, op
            pro.add(d, nets.TAG_EW)

        ew(L.EW_DIV, self.xinit, out=self.init, s0=PRIOR_SCALE_C)
        if win.cond_feat:
            ew(L.EW_DIV, self.feat, out=self.featc, s0=PRIOR_SCALE_C)
        src = self.xT_in
        if win.xT_plus_init:
            ew(L.EW_ADD_MUL, self.xT_in, b=self.init, out=self.x[0], s0=1.0)
            src = self.x[0]
        if self.use_sigma:
            d = L.SigmaDesc()
            d.init, d.a, d.out = self.init.data_ptr(), src.data_ptr(), self.x[0].data_ptr()
            d.maxbuf = ctx.alloc(B * 2).data_ptr()
            d.plane, d.nplanes, d.valid = T * F0, B * 2, 0
            pro.add(d, nets.TAG_EW)
        elif not win.xT_plus_init:
            ew(L.EW_COPY, self.xT_in, out=self.x[0])
        for pb in (self.stft, self.istft, pro):
            pb.finish()
        self.ctx, self.L, self.T = ctx, L_, T
        self.eps_windows = longplan.windows(T, self.W, *self.eps_field)
        self.prior_windows = longplan.carried(T, self.W) if self.carried else longplan.windows(T, self.W, *self.prior_field)

    def activation_bytes(self):
        """(window plan, whole-file side) bytes of per-plan device memory - weights excluded; the second grows with T."""
        size = lambda ctx: sum(t.numel() * t.element_size() for t in ctx.keep if torch.is_tensor(t))   # noqa: E731
        return size(self.win.ctx), size(self.ctx) if self.L is not None else 0

    def _gather(self, whole, winbuf, a, stream):
        L.window_gather(whole.data_ptr(), winbuf.data_ptr(), self.B, 2, self.T, F0, self.W, a, stream, device=self.device)

    def _scatter(self, winbuf, whole, a, lo, hi, stream):
        L.window_scatter(winbuf.data_ptr(), whole.data_ptr(), self.B, 2, self.T, F0, self.W, a, lo, hi, stream, device=self.device)

    def enhance(self, wav, x_T):
        """wav [B,L], x_T [B,2,T,161] with T = 1 + L // 160 > W -> (enhanced wav [B,L], spectrogram [B,2,T,161]): what a
        whole-file ``SamplerPipeline(exclusive=False)`` of that length returns.  Nothing is synchronised."""
        win = self.win
        if wav.dim() != 2 or wav.shape[0] != self.B:
            raise ValueError("wav: expected [%d, L], got %s" % (self.B, tuple(wav.shape)))
        L_ = int(wav.shape[1])
        if 1 + L_ // 160 <= self.W:
            raise ValueError("a recording of %d frames fits the window of %d: it takes the whole-file plan" % (1 + L_ // 160, self.W))
        self._whole(L_)
        _expect(wav, self.stft.wav, "wav")
        _expect(x_T, self.xT_in, "x_T")
        self.stft.wav.copy_(wav)
        self.xT_in.copy_(x_T)
        self.stft.lens.fill_(L_)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        self.stft.plan.run(stream)
        # ---- prior
        prior = win.prior
        if self.carried:
            prior.state_in.zero_()
        for a, lo, hi in self.prior_windows:
            self._gather(self.feat, win.feat, a, stream)
            win.plan.run_range(*win.ranges["prior"], stream)
            self._scatter(prior.out, self.xinit, a, lo, hi, stream)
            if self.carried:
                prior.state_in.copy_(prior.state_out)
        # ---- prologue on the whole file, and the steps' time biases
        self.pro.plan.run(stream)
        win.plan.run_range(self._time, self._time + 1, stream)
        cond = None if win.deltamu else (self.featc if win.cond_feat else self.init)
        # the last step adds X_init / 11 back where the window plan does (win.zero None): it is the gathered condition
        cur, nxt = self.x
        for nstep in range(self.nsteps - 1, -1, -1):
            rng = win.ranges["step%d" % nstep]
            dst = nxt if nstep else self.spec
            for a, lo, hi in self.eps_windows:
                self._gather(cur, win.audio, a, stream)
                if cond is not None:
                    self._gather(cond, win.eps.x_init, a, stream)
                win.plan.run_range(*rng, stream)
                self._scatter(win.audio if nstep else win.members_spec, dst, a, lo, hi, stream)
            cur, nxt = nxt, cur
        self.istft.plan.run(stream)
        return self.istft.wav.clone(), self.spec.clone()

    def check(self):
        """Synchronises; raises ``PdseRangeError`` if an f16x2 pass left a non-finite spectrogram (``SamplerPipeline.check``).
        (``SamplerPipeline.windowed`` is the older name of "has an fp16 range to leave" and has nothing to do with frame windows.)"""
        if self.win.windowed and not bool(torch.isfinite(self.spec).all()):
            raise SamplerPipeline.nonfinite_error()
