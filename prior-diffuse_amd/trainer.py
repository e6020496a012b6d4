"""Drop-in for the sampling half of the reference's ``ComplexDDPMTrainer``
(trainer/complex_ddpm_trainer.py): same constructor arguments, same
``inference_schedule()`` return tuple, same ``generate_wav()`` behaviour, plus the batched
entry points the reference lacks (it can only read wav files from a directory):

    enhance(wav[B,L], x_T=None)      -> wav[B,L]         whole path, batched
    enhance_batch(wavs, exact=True)  -> [wav_b]          ragged batch, every utterance as if enhanced alone
    sample(feat[B,2,T,161], x_T)     -> spectrogram      :939-998 on a given spectrogram

Training (train_ddpm/train_step/train/draw_audio) is out of scope.
Deliberate differences from the reference, all recorded in SURVEY.md §0/§2:
  * both networks run with eval-mode BatchNorm (the reference's generate_wav forgets
    ``model_ddpm.eval()``, :914 — a bug, not a target);
  * no ``exit()`` after generation (:1021), no wandb, no CUDA_VISIBLE_DEVICES override.
"""
import glob
import logging
import os
from collections import OrderedDict, deque, namedtuple
from copy import deepcopy
from functools import partial
from itertools import chain

import torch

from . import _lib as L
from . import longplan, nets, ops, raggedplan, wavdev, wavio
from .params import PRIOR_SCALE_C, params as default_params
from .pipeline import RAGGED_PRIORS, LongSampler, SamplerPipeline, _expect, ragged_args
from .schedule import inference_schedule as _inference_schedule


# one item of ``enhance_stream`` in flight: the event behind its pass, clones and verdict copy; what a repeat needs
_Job = namedtuple("_Job", "event pipe key wav x_T out")


class _PlanCache(OrderedDict):
    """Recorded plans of some geometries, key -> plan, least recently used first.  At most ``capacity`` plans - and so
    activation sets - are alive at any moment: the least recently used one is dropped BEFORE a new one is built.
    ``hits[key]``: how often the key was met again since its plan was built (0 for a fresh plan, a rebuilt one included)."""

    def __init__(self, capacity):
        super().__init__()
        self.capacity, self.hits = capacity, {}

    def take(self, key, build):
        """-> (plan of ``key``, met_before); ``build()`` makes the plan where the cache does not hold one."""
        met = key in self
        self.hits[key] = self.hits.get(key, 0) + 1 if met else 0
        if met:
            self.move_to_end(key)
        else:
            while len(self) >= self.capacity:
                self.popitem(last=False)
            self[key] = build()
        return self[key], met


class _Slot:
    """One slot of ``enhance_stream``: a HIP stream and the recorded geometries it keeps ((geometry, split) -> pipeline, LRU)."""

    def __init__(self, stream, capacity):
        self.stream, self.pipes = stream, _PlanCache(capacity)
        self.hits = self.pipes.hits


def _inflight_arg(inflight):
    inflight = int(inflight)
    if not 1 <= inflight <= 4:
        raise ValueError("inflight must be 1 .. 4 (a process has four hardware queues), got %d" % inflight)
    return inflight


class ComplexDDPMTrainer(object):
    MAX_PLANS = 3   # recorded (B, T) geometries kept alive (least recently used first out); weights are shared by all
    masked_prior = False   # exact ragged batches of the DB-AIAT priors on the length-masked kernels (constructor)
    wav_formats = "pcm"    # what generate_wav opens: "pcm" (the wave module's integer PCM) or "all" (constructor)
    wav_out = "pcm16"      # what generate_wav writes: "pcm16" (16 kHz, 16-bit, mono) or "source" (the file's own rate and format)
    channels = "mix"       # what generate_wav enhances of a multichannel file: "mix" (the mono mix) or "each" (every channel)

    def __init__(self, args, config, device=None, prior_state_dict=None, ddpm_state_dict=None, params=None, exclusive=None,
                 dtype=None, split=None, audit=None, masked_prior=None, wav_formats=None, wav_out=None, channels=None, window=None):
        """args: .retrain .joint .draw .sigma .checkpoint .generated_wav
        config: .model.name, .train.{fft_num, win_size, win_shift, feat_type}.  feat_type: the spectral compression the
        checkpoint was trained with - "sqrt", "normal", "cubic", "log_1x" or "none" (``SamplerPipeline(feat_type=...)``; any other
        string: ValueError).  Every entry point honours it without an argument of its own: the front end and the label leg
        compress with it, the back end and the scored waveforms decompress with it, everything between them works in the
        compressed domain whatever it is.
        Weights come from ``<args.checkpoint>/best_checkpoint.pth`` under the reference's
        rules (:91-97) or from the two state_dict arguments (synthetic runs).
        exclusive: this trainer is the only work on its GPU (the reference's situation: one process, one batch at a
        time), so small batches may take the persistent LSTM launch (csrc/lstmp.hip).  None: True unless the process is
        one rank of a torch.distributed job - a sharded run keeps the kernels that make an utterance's result
        bit-identical whatever the number of ranks (prior-diffuse_amd/shard.py).
        dtype: "f32" (default: the reference's arithmetic - fp32, or an fp32-equivalent operand split of the matrix-core kernels,
        see ``split``) or "bf16",
        the OPT-IN reduced-precision mode BASELINE configs 2/4/5 name (``SamplerPipeline(dtype="bf16")``: plain bf16 operands
        and bf16 block-boundary tensors in the eps-net, tolerance 3e-2 rel-L2; never the default).  None: ``args.bf16`` when the
        CLI set it (``main.py --bf16``), else "f32".
        split: the fp32-equivalent operand split every plan of this trainer is built with, handed to ``SamplerPipeline`` as is -
        "f16x2" (fp16 hi + lo of the scaled operand: fp32-equivalent inside the fp16 window of include/pdse.h) or "bf16x3" (the
        exact three-way bf16 split: no window, 1.45 x the time); None: ``args.split`` when the CLI set it (``main.py --split``),
        else ``SamplerPipeline.default_split`` ("f16x2").  A geometry whose f16x2 pass leaves the window is repeated on
        "bf16x3" whatever this says (``_checked``).
        audit: build the plans with the range audit of the f16x2 window (``SamplerPipeline(audit=True)``) and let ``_checked``
        treat a tensor that lies wholly BELOW the window - finite output, no other trace - like one that overflowed it: warn,
        repeat the geometry on "bf16x3".  None: ``args.audit_range`` when the CLI set it (``main.py --audit-range``), else False.
        masked_prior: let ``enhance_batch(exact=True)`` and ``generate_wav(batch=N)`` take the DB-AIAT priors
        (``aia_complex_trans_ri``, ``dual_aia_trans_merge_crm``): their ragged plans are recorded with the length-masked attention,
        GRU, GroupNorm and AHAM kernels (``SamplerPipeline(ragged=True, masked_prior=True)``), and every utterance comes out as
        if enhanced alone, as for the other priors.  Dense passes are not touched.  None: ``args.masked_prior`` when the CLI set
        it (``main.py --masked-prior``), else False: exact ragged batches of these priors raise ValueError as before.
        wav_formats: what ``generate_wav`` opens, in all three modes.  "pcm": 8-, 16- and 32-bit integer PCM in a plain header, as
        the ``wave`` module reads it; everything else is skipped with a warning.  "all": also 24-bit PCM, IEEE float (32 and
        64 bits), G.711 A-law and mu-law and WAVE_FORMAT_EXTENSIBLE headers, decoded on the device
        (``wavdev.load(formats="all")``, the waveform of ``wavio.read_any``); a float file with a non-finite sample is skipped
        with the same warning before its x_T is drawn.  None: "all" when the CLI set ``args.all_wav`` (``main.py --all-wav``),
        else "pcm".
        wav_out: what ``generate_wav`` writes, in all three modes.  "pcm16": 16 kHz, 16-bit, mono, whatever the source was
        (``wavio.write_wav``, as ever).  "source": every file at its source's rate, frame count and channel count, in the source's
        encoding where that holds an enhanced signal - 16-, 24- and 32-bit PCM as themselves, binary32 and binary64 as binary32,
        8-bit PCM and G.711 as 16-bit PCM (``wavio.target_of``) - converted, clamped, encoded and interleaved on the device
        (``wavdev.encode``: ``wavio.resample`` + ``wavio.encode`` byte for byte).  The network enhances the mono mix, so every
        channel of a written file carries the same signal.  A file in which the integer clamp changed samples - an enhancer's
        output is not bounded by +-1 - is written and logged with one warning that names it and the count.  None: "source" when
        the CLI set ``args.keep_format`` (``main.py --keep-format``), else "pcm16".
        channels: what ``generate_wav`` enhances of a file with 2 .. 8 channels, in all three modes.  "mix": the mono mix, as
        above.  "each": every channel on its own - the file is decoded with its channels kept apart (``wavdev.load(channels=
        "each")``: the rows of ``wavio.read_channels``), channel c gets its own x_T (and its ``rng_fidelity`` discards), drawn in
        channel order where the file's single draw stood, and the C channels are enhanced as C utterances of equal length: one
        exact ragged pass of B = C (``batch=1``; the DB-AIAT priors need ``masked_prior=True`` for it, else the first
        multichannel file raises their ValueError), rows of the ragged windows (``batch=N``), or one item [C, L] in flight
        (``inflight=N``; GCRN and DiffUNet priors).  The file is written with C different channels through
        ``wavdev.encode_channels``: at its source's rate, length and encoding with ``wav_out="source"``, at 16 kHz and 16 bits
        with "pcm16".  Contract: channel c of every written file is what the same trainer writes for a mono file holding that
        channel, given the same x_T - byte for byte on an ``exclusive=False`` trainer, whose kernels do not depend on the batch
        size, and within the persistent-LSTM difference (1e-5, see ``enhance_stream``) on the default trainer, where ``enhance``
        at B <= 4 may take the persistent launch.  A seeded run on a stereo file draws what the same run draws on its two
        channels stored as mono files that sort next to each other.  Mono files behave exactly as under "mix"; a source with
        more than 8 channels is enhanced as the mix and written as under "mix" (logged).  No x_T is shared between channels, and
        the metrics score the mix.  None: "each" when the CLI set ``args.per_channel`` (``main.py --per-channel``), else "mix".
        window: W frames (a multiple of ``longplan.FRAME_TILE``): ``enhance`` and ``generate_wav`` send a recording of more than W
        frames through the windowed pass (``pipeline.LongSampler``) - one window plan per batch size, whatever the
        lengths - with the results of an ``exclusive=False`` trainer's whole-file pass; shorter recordings take today's path.
        Priors GCRN and DiffUNet; with ``channels="each"`` or ``audit=True``: ValueError.  None: ``args.window``
        (``main.py --window``), else off."""
        self.window = longplan.window_arg(getattr(args, "window", None) if window is None else window)
        if channels is None:
            channels = "each" if getattr(args, "per_channel", False) else "mix"
        if channels not in ("mix", "each"):
            raise ValueError("channels must be 'mix' or 'each'")
        self.channels = channels
        if wav_out is None:
            wav_out = "source" if getattr(args, "keep_format", False) else "pcm16"
        if wav_out not in ("pcm16", "source"):
            raise ValueError("wav_out must be 'pcm16' or 'source'")
        self.wav_out = wav_out
        if wav_formats is None:
            wav_formats = "all" if getattr(args, "all_wav", False) else "pcm"
        if wav_formats not in ("pcm", "all"):
            raise ValueError("wav_formats must be 'pcm' or 'all'")
        self.wav_formats = wav_formats
        self.masked_prior = bool(getattr(args, "masked_prior", False) if masked_prior is None else masked_prior)
        if split is None:
            split = getattr(args, "split", None)
        if split not in (None, "f16x2", "bf16x3"):
            raise ValueError("split must be 'f16x2' or 'bf16x3'")
        self.split = split
        self.audit = bool(getattr(args, "audit_range", False) if audit is None else audit)
        if dtype is None:
            dtype = "bf16" if getattr(args, "bf16", False) else "f32"
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        self.dtype = dtype
        if exclusive is None:
            import torch.distributed as dist

            exclusive = not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)
        self.exclusive = bool(exclusive)
        self.c = PRIOR_SCALE_C                                        # :30
        self.args = deepcopy(args)
        self.config = deepcopy(config)
        self.params = default_params if params is None else params    # :34 (override: synthetic runs / deltamu)
        self.pirorgrad = bool(self.params.pirorgrad)
        # :70-75 / :967-974: pirorgrad wins over deltamu for the model and the eps call; neither flag = DiffUNet1
        # conditioned on the noisy feature.  The x_T prologue (:946-949) tests deltamu on its own: with both flags set
        # the reference starts from randn + X_init/11 and still adds X_init at the end.
        self.deltamu = bool(self.params.deltamu) and not self.pirorgrad
        self.xT_plus_init = bool(self.params.deltamu)
        self.cond = "init" if (self.pirorgrad or self.deltamu) else "feat"
        tr = self.config.train
        if (tr.fft_num, tr.win_size, tr.win_shift) != (320, 320, 160):
            raise NotImplementedError("STFT 320/320/160 is baked into every model of the path")
        # the spectral compression around the networks (:414-435, utils/metrics.py:534-551): one of L.FEAT_TYPES, else ValueError
        self.feat_type = L.feat_type_of(tr.feat_type)
        if device is None:
            rank = int(os.environ.get("LOCAL_RANK", "0"))
            device = "cuda:%d" % rank
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise L.PdseError("ComplexDDPMTrainer needs an MI355X (device %s unavailable); no CPU fallback" % device)
        L.load()
        self.prior_name = self.config.model.name
        if self.prior_name not in ops.PRIOR_OPS:
            raise NotImplementedError("prior %r: built priors are %s" % (self.prior_name, sorted(ops.PRIOR_OPS)))
        self.prior_sd, self.ddpm_sd = prior_state_dict, ddpm_state_dict
        self._streaming = False           # enhance_stream: one stream per trainer at a time
        if self.window is not None:
            LongSampler.prior_check(self.prior_name)
            longplan.window_conflicts(per_channel=self.channels == "each")
            if self.audit:
                raise ValueError("window= with audit=True: the range audit reads one recorded plan's table")
        if getattr(self.args, "retrain", False):                      # :91-97
            self._load_checkpoint()
        else:
            self._install_weights()

    # ---- A8 checkpoint rules (:91-97, :906-913) ---------------------------
    def _load_checkpoint(self):
        path = os.path.join(self.args.checkpoint, "best_checkpoint.pth")
        data = torch.load(path, map_location="cpu")
        if isinstance(data, (list, tuple)):
            self.prior_sd = data[0]
            if getattr(self.args, "draw", False) or getattr(self.args, "joint", False):
                self.ddpm_sd = data[2]
        else:
            self.prior_sd = data
        logging.info("loaded %s", path)
        self._install_weights()

    def _install_weights(self):
        """Pack ``prior_sd`` / ``ddpm_sd`` for the device, once: the constructor's weights and every checkpoint loaded later."""
        if self.prior_sd is None or self.ddpm_sd is None:
            raise ValueError("no weights: pass state_dicts or use --retrain with a best_checkpoint.pth")
        self._forget_plans()
        self.bank = nets.WeightBank()     # packed weights in HBM: uploaded once, shared by every plan of this trainer
        self.model = ops.PRIOR_OPS[self.prior_name](self.prior_sd, self.device, bank=self.bank, exclusive=self.exclusive)       # :69
        self.model_ddpm = (ops.NoconOp if self.deltamu else ops.DiffUNet1Op)(self.ddpm_sd, self.device, bank=self.bank, exclusive=self.exclusive)   # :70-73

    def _forget_plans(self):
        """New weights: every recorded plan is stale, and so is every verdict on the fp16 window."""
        self._pipes = _PlanCache(self.MAX_PLANS)   # the trainer's own plans; ``_hits``: uses of a recorded geometry after the first
        self._slots = []                  # enhance_stream: one stream and a few recorded geometries per item in flight
        self._range_fallback = set()      # geometries whose f16x2 pass left the fp16 window once: they run on the three-plane bf16 split (_checked)
        self._audit_clean = set()         # geometries whose audited f16x2 pass came back clean once: their report is not read again
        self._long = {}                   # windowed passes: ("long", B, W, sigma, fast sampling, split) -> LongSampler

    _hits = property(lambda self: self._pipes.hits)

    # ---- A1 ---------------------------------------------------------------
    def inference_schedule(self, fast_sampling=False):
        return _inference_schedule(self.params, fast_sampling)

    # ---- batched entry points ----------------------------------------------
    def _key(self, B, T=None, L_=None, ragged=False, label=False, objective=False, members=1):
        """The key of a geometry in the plan caches and in ``_range_fallback`` / ``_audit_clean``."""
        return ((B, T, L_, bool(getattr(self.args, "sigma", False)), bool(self.params.fast_sampling)) + ((True,) if ragged else ())
                + (("label",) if label else ()) + (("objective",) if objective else ())
                + ((("members", members),) if members != 1 else ())              # plans are cached per K; K = 1: the key it always had
                + ((self.feat_type,) if self.feat_type != "sqrt" else ()))       # a trainer has one; the key names it all the same

    def _split_of(self, key, split):
        """The operand split a plan of the geometry ``key`` is built with, where ``split`` is what it was asked for."""
        return "bf16x3" if key in self._range_fallback else split

    def _build(self, key, split, **kw):
        """A new plan of the geometry ``key`` against the weights already packed in ``self.bank``: re-recording the descriptors
        takes milliseconds.  split: ``_split_of(key, ...)``; kw: what the trainer's own plans and the stream's slots set apart."""
        return SamplerPipeline(
            self.device, self.prior_name, self.prior_sd, self.ddpm_sd, key[0], T=key[1], L_=key[2],
            fast_sampling=self.params.fast_sampling, use_sigma=key[3], params=self.params, deltamu=self.deltamu,
            cond=self.cond, bank=self.bank, xT_plus_init=self.xT_plus_init, dtype=self.dtype, split=split,
            feat_type=self.feat_type, **kw)

    def _plan(self, **geom):
        """-> (plan, key, met_before) of one geometry (``_key``'s arguments).  ``generate_wav`` meets a new utterance length
        with almost every file; only ``MAX_PLANS`` geometries keep their activation buffers, the least recently used one is
        dropped.  met_before: the geometry came back (a directory of equally long files, a serving loop) - the callers that
        replay a plan from its hipGraph, one host call instead of ~770 launches, do so then; a length seen once is not worth
        the capture."""
        key = self._key(**geom)
        ragged = True in key[5:]
        legs = {name: True for name in ("label", "objective") if name in key[5:]}      # the plans with a leg beside the sampler's
        legs.update(m for m in key[5:] if isinstance(m, tuple))                       # ("members", K): an ensemble plan
        build = partial(self._build, key, self._split_of(key, self.split), exclusive=self.exclusive, audit=self.audit,
                        ragged=ragged, masked_prior=ragged and self.masked_prior, **legs)
        pipe, met = self._pipes.take(key, build)
        return pipe, key, met

    def _pipe(self, B, T=None, L_=None, ragged=False, label=False, objective=False, members=1):
        """The recorded plan of one geometry."""
        return self._plan(B=B, T=T, L_=L_, ragged=ragged, label=label, objective=objective, members=members)[0]

    def _checked(self, run, **geom):
        """``run(pipe, graph) -> result`` on the plan of a geometry, verified (``SamplerPipeline.check``: synchronises); graph:
        the geometry was met before (``_plan``), for the callers that replay.  A pass on f16x2 operands whose activations left
        the fp16 window shows as non-finite output (include/pdse.h: PDSE_F16_ACT_EXP): the geometry is then rebuilt on the exact
        three-plane bf16 split - no window - and the pass repeated, launch by launch; later calls stay on it.
        With ``audit`` the range report of the pass is read as well and a tensor wholly below the window is handled the same
        way.  The audit is read on a geometry's passes until one comes back clean; after that the geometry keeps its audited
        plan (re-recording it would cost more than the launches do) and stops reading the report - a geometry is judged on the
        first inputs it sees, at the price of one small device-to-host copy per pass until then and of the audit launches for
        as long as the plan lives."""
        pipe, key, met = self._plan(**geom)
        res = run(pipe, met)
        try:
            read = self.audit and pipe.audited and key not in self._audit_clean
            pipe.check(audit=read)
            if read:
                self._audit_clean.add(key)
        except L.PdseRangeError as e:
            logging.warning("%s - repeating this geometry with split='bf16x3'", e)
            self._range_fallback.add(key)
            del self._pipes[key]
            pipe, _, met = self._plan(**geom)
            res = run(pipe, met)
            pipe.check()
        return res

    # ---- utterances in flight -------------------------------------------------
    STREAM_PLANS = 2   # recorded geometries every slot of ``enhance_stream`` keeps alive (least recently used first out; <= MAX_PLANS)

    def enhance_stream(self, items, inflight=3):
        """A stream of independent items, ``inflight`` of them on the GPU at a time; a generator of ``(wav_out [B, L], spec
        [B, 2, T, 161])``, one pair per item, in the order of the items.  items: an iterable of ``wav`` or ``(wav, x_T)``; wav
        [B, L] or 1-D (B = 1), any scale, as for ``enhance``; x_T None or [B, 2, 1 + L // 160, 161].  The iterable is consumed
        as slots come free, at most ``inflight`` items ahead of the one handed out.

        Item i runs start to end on slot ``i % inflight`` (the ``by_batch`` form of ``PipelinedSampler``).  A slot is one HIP
        stream and a cache of ``STREAM_PLANS`` = 2 recorded geometries, least recently used first out, built with this
        trainer's weights (``bank``), ``split`` and ``dtype``, with ``verdict=True`` and with ``exclusive=False``: the items in
        flight share the GPU, so no launch may wait for its own workgroups.  Memory is therefore bounded by ``inflight`` x 2
        activation sets beside the trainer's own ``MAX_PLANS``; the slots live as long as the trainer (or its weights), so a
        second stream of the same lengths re-records nothing.  ``1 <= inflight <= 4`` (a process has four hardware queues),
        else ValueError.  A geometry a slot meets again is replayed from its hipGraph, one seen once runs launch by launch -
        ``enhance``'s rule.

        x_T None is drawn on the caller's stream at submission, in item order: the generator sees the draws of the
        one-at-a-time loop.  A slot's results are cloned on the slot's stream ahead of its event, so what is handed out is never
        overwritten by a later item.

        Verification costs no device-wide synchronisation: the plan ends with the finiteness verdict of its own pass
        (``SamplerPipeline(verdict=True)``), the counters travel to pinned host memory behind the pass, and before item i is
        handed out the host waits for item i's event only.  Counts of zero: the item is handed out.  Otherwise (an activation
        left the f16x2 window, or the input was not finite) every submitted item is waited for, ``_checked``'s warning is logged,
        the geometry joins ``_range_fallback``, and THAT item is repeated through ``_checked`` on a "bf16x3" plan, synchronously
        and with the same x_T, and handed out in its place; items already in flight keep their own verdicts, later items of the
        geometry are built on "bf16x3".  Where the arithmetic has no window to leave (split "bf16x3", dtype "bf16", the exact fp32
        of the full schedule) a non-zero count raises ``PdseRangeError`` from the generator at that item.

        Closing the generator early (``close()``, garbage collection, an exception in the consumer) waits for the slots' events.
        One stream per trainer at a time (RuntimeError), and on a trainer with ``exclusive=True`` no other entry point between
        two items: its own plans assume the GPU to themselves.  ``audit=True`` trainers: ValueError (the audit reads a report
        per pass).  All four priors; nothing here is ragged.

        Every item's tensors equal, bit for bit, what ``ComplexDDPMTrainer(..., exclusive=False).enhance(wav, x_T)`` and its
        plan's spectrogram give: the kernels the in-flight plans take do not depend on the batch size.  The default trainer
        (``exclusive=True``) takes the persistent LSTM at B <= 4 in ``enhance``, which is 1e-5 from these kernels and not
        bit-identical to them.  (Measured limit, DESIGN.md 4.9: at T = 401 three B = 1 graph replays sharing the GPU differed from
        the sequential pass in a few of 192 passes, with and without the verdict; the tests hold T <= 21 to ``torch.equal``.)"""
        self._no_window("enhance_stream")
        inflight = _inflight_arg(inflight)
        if self.audit:
            raise ValueError("enhance_stream on a trainer built with audit=True: the range audit reads a report per pass")
        return self._enhance_stream(items, inflight)

    def _stream_slots(self, inflight):
        while len(self._slots) < inflight:
            self._slots.append(_Slot(torch.cuda.Stream(self.device), self.STREAM_PLANS))
        return self._slots[:inflight]

    def _enhance_stream(self, items, inflight):
        if self._streaming:
            raise RuntimeError("enhance_stream: this trainer already has a stream open (its slots are in use)")
        self._streaming = True
        pending = deque()
        try:
            slots = self._stream_slots(inflight)
            it, n, more = iter(items), 0, True

            def refill():
                nonlocal n, more
                while more and len(pending) < inflight:
                    try:
                        item = next(it)
                    except StopIteration:
                        more = False
                        return
                    pending.append(self._stream_submit(slots[n % inflight], item))
                    n += 1

            while True:
                refill()
                if not pending:
                    return
                res = self._stream_collect(pending.popleft(), pending)
                refill()                       # the slot is free: it gets the next item before the consumer gets this one
                yield res
        finally:
            for job in pending:                # closed early, or an exception: the slots' buffers are not reused before their work is done
                job.event.synchronize()
            self._streaming = False

    def _stream_submit(self, slot, item):
        """Enqueue one item on a slot (whose previous item has been collected: its stream is idle); returns the job."""
        wav, x_T = item if isinstance(item, (tuple, list)) else (item, None)
        wav = torch.as_tensor(wav).to(self.device, torch.float32)
        if wav.dim() == 1:
            wav = wav[None]
        B, L_ = wav.shape
        cur = torch.cuda.current_stream(self.device)
        x_T = self._x_T((B, 2, 1 + L_ // 160, 161), x_T)          # :947-950: the caller's stream, item order
        key = self._key(B, L_=L_)
        split = self._split_of(key, self.split or SamplerPipeline.default_split)      # resolved: the split is part of a slot's cache key
        pipe, met = slot.pipes.take((key, split), partial(self._build, key, split, exclusive=False, verdict=True))
        _expect(x_T, pipe.xT_in, "x_T")
        ready = torch.cuda.Event()
        ready.record(cur)                                          # behind the draw, the upload of the inputs and the recording of a new plan
        st = slot.stream
        with torch.cuda.stream(st):
            st.wait_event(ready)
            for src in (wav, x_T):                                 # allocated on the caller's stream: tell the caching allocator
                src.record_stream(st)                              # this stream still reads them
            pipe.stft.wav.copy_(wav, non_blocking=True)
            pipe.xT_in.copy_(x_T, non_blocking=True)
            pipe.stft.lens.fill_(L_)
            if met:                                                # met again: one host call instead of ~770 launches
                if not pipe.plan.has_graph:
                    pipe.plan.build_graph(st.cuda_stream)
                pipe.plan.launch_graph(st.cuda_stream)
            else:
                pipe.plan.run_range(0, len(pipe.descs), st.cuda_stream)
            out = (pipe.istft.wav.clone(), pipe.spec.clone())      # ahead of the event: a later item of the slot cannot overwrite them
            pipe.verdict_fetch(st)
            event = torch.cuda.Event()
            event.record(st)
        return _Job(event, pipe, key, wav, x_T, out)

    def _stream_collect(self, job, pending):
        """Wait for one item's own event, read its verdict, and return its result - or that of its repeat on "bf16x3"."""
        job.event.synchronize()
        if not any(job.pipe.verdict_counts()):
            cur = torch.cuda.current_stream(self.device)
            for t in job.out:                                      # allocated on the slot's stream, read on the caller's from here on
                t.record_stream(cur)
            return job.out
        err = SamplerPipeline.nonfinite_error()
        if not job.pipe.windowed:
            raise err
        for other in pending:                                      # the repeat may take launches that want the GPU to themselves
            other.event.synchronize()
        logging.warning("%s - repeating this geometry with split='bf16x3'", err)
        self._range_fallback.add(job.key)
        self._pipes.pop(job.key, None)                             # f16x2 plans of the geometry: not used again
        for slot in self._slots:
            slot.pipes.pop((job.key, job.pipe.split), None)
        return self._checked(lambda pipe, graph: pipe.enhance(job.wav, job.x_T, graph=graph), B=job.wav.shape[0], L_=job.wav.shape[1])

    def _x_T(self, shape, x_T, members=1):
        """The x_T of a pass of ``shape`` [B,2,T,161].  members K > 1: [K B,2,T,161], member-major - drawn as K consecutive draws
        of ``shape`` (what K one-member passes draw), or a given [K,B,2,T,161] / [K B,2,T,161] tensor."""
        if x_T is None:                                            # :947-950 randn_like(init)
            draws = [torch.randn(*shape, device=self.device, dtype=torch.float32) for _ in range(members)]
            return draws[0] if members == 1 else torch.cat(draws)
        x_T = x_T.to(self.device)
        if x_T.dim() == 5 and x_T.shape[0] == members:                   # members = 1 too: [1,B,2,T,161] is one member
            x_T = x_T.reshape((-1,) + tuple(x_T.shape[2:]))
        return x_T

    def sample(self, feat, x_T=None, verify=True, members=1):
        """feat [B,2,T,161] compressed spectrogram -> enhanced compressed spectrogram.  verify, members: see ``enhance``."""
        self._no_window("sample")
        members = L.members_arg(members)
        feat = feat.to(self.device)
        B, _, T, _ = feat.shape
        x_T = self._x_T(feat.shape, x_T, members)
        if not verify:
            return self._pipe(B, T=T, members=members).sample(feat, x_T)[0]
        return self._checked(lambda pipe, graph: pipe.sample(feat, x_T)[0], B=B, T=T, members=members)     # never replayed

    def _no_window(self, entry):
        """A trainer built with ``window=W`` runs windowed passes through ``enhance`` and ``generate_wav`` only: every other entry
        point records whole-file plans and would silently ignore the option - ValueError instead, as ``members`` does it."""
        if getattr(self, "window", None) is not None:
            raise ValueError("%s on a trainer built with window=%d: windowed passes enhance one padded batch, one trajectory, one file "
                             "at a time through enhance() and generate_wav(); build a trainer without window= for %s"
                             % (entry, self.window, entry))

    def _long_sampler(self, B, W):
        """The windowed sampler of batch size B and window W: one per trainer and operand split, whatever the lengths
        (``pipeline.LongSampler``).  A geometry whose f16x2 pass left the fp16 range once stays on "bf16x3" (``_range_fallback``)."""
        geom = ("long", B, W, bool(getattr(self.args, "sigma", False)), bool(self.params.fast_sampling))
        key = geom + (self._split_of(geom, self.split),)
        if key not in self._long:
            self._long[key] = LongSampler(self.device, self.prior_name, self.prior_sd, self.ddpm_sd, B, W,
                                          fast_sampling=self.params.fast_sampling, use_sigma=geom[3], params=self.params,
                                          deltamu=self.deltamu, cond=self.cond, bank=self.bank, xT_plus_init=self.xT_plus_init,
                                          dtype=self.dtype, split=key[-1], feat_type=self.feat_type)
        return self._long[key], geom

    def _enhance_long(self, wav, x_T, W, verify):
        long, geom = self._long_sampler(wav.shape[0], W)
        out = long.enhance(wav, x_T)[0]
        if verify:
            try:
                long.check()
            except L.PdseRangeError as e:
                logging.warning("%s - repeating the windowed pass with split='bf16x3'", e)
                self._range_fallback.add(geom)
                long, _ = self._long_sampler(wav.shape[0], W)
                out = long.enhance(wav, x_T)[0]
                long.check()
        return out

    def enhance(self, wav, x_T=None, verify=True, members=1, window=None):
        """wav [B,L] (any scale; RMS-normalised internally like :922-923) -> enhanced [B,L].
        verify (default): the pass is checked before its result is handed out (one synchronisation: persistent launches that
        gave up, and - f16x2 operands - an activation outside the fp16 window, in which case the geometry is repeated on the
        three-plane bf16 split, see ``_checked``); False: asynchronous, the caller answers for ``SamplerPipeline.check()``.
        members: K = 1 .. 16 reverse trajectories per utterance behind one pass of the front end and the prior
        (``SamplerPipeline(members=K)``); the result is the ensemble mean - taken in the compressed domain, then decompressed
        and inverted by the back end as ever.  x_T: [K,B,2,T,161] or [K B,2,T,161], member-major; None: K consecutive draws of
        [B,2,T,161], what K one-member calls draw.  Never replayed from a hipGraph.  1 (default): today's pass.
        ``enhance_members`` returns the members, the spread map and the sums as well.
        window: W frames (None: the trainer's ``window``): a recording of more than W frames takes the windowed pass - see the
        constructor; x_T is drawn for the whole file as ever.  With ``members`` > 1: ValueError."""
        members = L.members_arg(members)
        window = getattr(self, "window", None) if window is None else longplan.window_arg(window)
        wav = wav.to(self.device, torch.float32)
        B, L_ = wav.shape
        T = 1 + L_ // 160
        if window is not None:
            longplan.window_conflicts(members=members, per_channel=self.channels == "each")
            LongSampler.prior_check(self.prior_name)
            if self.audit:
                raise ValueError("window= with audit=True: the range audit reads one recorded plan's table")
        x_T = self._x_T((B, 2, T, 161), x_T, members)
        if window is not None and T > window:
            return self._enhance_long(wav, x_T, window, verify)
        # a geometry that comes back is replayed (``_plan``); an ensemble pass never is
        run = lambda pipe, graph: pipe.enhance(wav, x_T, graph=graph and members == 1)[0]   # noqa: E731
        if not verify:
            pipe, _, met = self._plan(B=B, L_=L_, members=members)
            return run(pipe, met)
        return self._checked(run, B=B, L_=L_, members=members)

    def enhance_members(self, wav, x_T=None, members=2):
        """``enhance(wav, x_T, members=K)`` with everything the ensemble pass leaves, as a dictionary of tensors on the device:
        ``wav`` [B,L] and ``spec`` [B,2,T,161] (the ensemble mean and its waveform, what ``enhance`` returns), ``members_spec``
        [K B,2,T,161] (row k B + b: member k of utterance b), ``spread`` [B,T,161] (the sample standard deviation of every complex
        bin), ``per_utt`` [B,2] and ``per_member`` [K,B] (float64 sums, ``ops.ensemble_stats``) and ``relative_spread`` [B] =
        sqrt(per_utt[b][0] / (K - 1) / per_utt[b][1]), the ensemble's standard deviation over the norm of its mean (zeros for
        K = 1).  Verified like ``enhance``.  members 1 is allowed: one member, zero spread."""
        self._no_window("enhance_members")
        members = L.members_arg(members)
        wav = wav.to(self.device, torch.float32)
        B, L_ = wav.shape
        x_T = self._x_T((B, 2, 1 + L_ // 160, 161), x_T, members)

        def run(pipe, graph):
            out, spec = pipe.enhance(wav, x_T)                                                  # never replayed
            if members == 1:
                with torch.cuda.device(self.device):
                    ens = ops.ensemble_stats(spec, 1, [pipe.T] * B)
            else:
                ens = pipe.ensemble
            return dict(wav=out, spec=spec, members_spec=pipe.members_spec.clone(), spread=ens["spread"].clone(), per_utt=ens["per_utt"],
                        per_member=ens["per_member"], relative_spread=ops.relative_spread(ens["per_utt"], members))

        return self._checked(run, B=B, L_=L_, members=members)

    def enhance_batch(self, wavs, x_T=None, trim_to_frames=False, exact=False, members=1):
        """Ragged batch.  Returns a list of 1-D tensors (rescaled by c), each of its utterance's own length.
        exact False (default), the validation loop's convention: every utterance is RMS-normalised
        over its own samples, zero-padded to the longest (utils/dataset.py:45-58), enhanced in one batch
        (:408-494) - the padding takes part - and cut back — to its own length, or with ``trim_to_frames`` to
        ``(frame_num - 1) * 160`` samples as utils/metrics.py:562-563 does.
        exact True: every utterance exactly as ``enhance(wav_b[None], x_T_b)`` gives it alone (``generate_wav``'s per-file
        result) - the STFT reflects at, the TCM pads at and the ISTFT sums up to the utterance's own end, ``--sigma`` takes
        the maximum over its own frames (``SamplerPipeline(ragged=True)``; priors GCRN and DiffUNet, ValueError for the
        DB-AIAT priors, which attend over all frames of the batch - unless the trainer was built with ``masked_prior=True``).  x_T: one padded [B, 2, T, 161] tensor, or a list of
        per-utterance [2, T_b, 161] (or [1, 2, T_b, 161]) tensors, T_b = 1 + len_b // 160; None: one draw per utterance at its
        own shape, in list order - the draws of the B = 1 calls.
        members: K > 1 returns the ensemble mean of K trajectories of the padded batch (``enhance``; x_T [K,B,2,T,161] or
        [K B,2,T,161]); with exact=True: ValueError (an exact ragged plan runs one trajectory)."""
        self._no_window("enhance_batch")
        members = L.members_arg(members)
        wavs = [torch.as_tensor(w, dtype=torch.float32).flatten() for w in wavs]
        lens = [int(w.numel()) for w in wavs]
        if min(lens) < 161:
            raise ValueError("utterances must be longer than the reflect padding (160 samples)")
        if exact and members > 1:
            raise ValueError("enhance_batch(exact=True, members=%d): an exact ragged plan runs one trajectory per utterance; ensembles "
                             "take the padded pass (exact=False)" % members)
        if exact:
            out = self._enhance_ragged(wavs, x_T, max(lens))
            return [o[:(n // 160) * 160].clone() if trim_to_frames else o for o, n in zip(out, lens)]
        batch = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True).to(self.device)
        B, L_ = batch.shape
        T = 1 + L_ // 160
        x_T = self._x_T((B, 2, T, 161), x_T, members)
        out = self._checked(lambda pipe, graph: pipe.enhance(batch, x_T, lens=lens)[0], B=B, L_=L_, members=members)    # never replayed
        cut = [(n // 160) * 160 if trim_to_frames else n for n in lens]
        return [out[i, :cut[i]].clone() for i in range(B)]

    def _enhance_ragged(self, wavs, x_T, L_):
        """``enhance_batch(exact=True)`` on 1-D utterances, padded to ``L_`` samples; returns the list of enhanced utterances."""
        ragged_args(self.prior_name, L_, masked=self.masked_prior)
        lens = [int(w.numel()) for w in wavs]
        B, T = len(wavs), 1 + L_ // 160
        batch = torch.zeros(B, L_, dtype=torch.float32, device=self.device)
        for b, w in enumerate(wavs):
            batch[b, :lens[b]] = w.to(self.device)
        if x_T is None:
            x_T = [self._x_T((1, 2, 1 + n // 160, 161), None) for n in lens]          # :947-950, one draw per utterance
        if isinstance(x_T, (list, tuple)):
            if len(x_T) != B:
                raise ValueError("x_T: expected %d per-utterance tensors, got %d" % (B, len(x_T)))
            xp = torch.zeros(B, 2, T, 161, dtype=torch.float32, device=self.device)
            for b, (x, n) in enumerate(zip(x_T, lens)):
                x = torch.as_tensor(x, dtype=torch.float32)
                x = x[0] if x.dim() == 4 else x
                if tuple(x.shape) != (2, 1 + n // 160, 161):
                    raise ValueError("x_T[%d]: expected (2, %d, 161) for an utterance of %d samples, got %s" % (b, 1 + n // 160, n, tuple(x.shape)))
                xp[b, :, :x.shape[1]] = x.to(self.device)
            x_T = xp
        else:
            x_T = x_T.to(self.device)
        out = self._checked(lambda pipe, graph: pipe.enhance(batch, x_T, lens=lens, exact=True, graph=graph)[0], B=B, L_=L_, ragged=True)
        return [out[b, :lens[b]].clone() for b in range(B)]

    def evaluate_batch(self, noisy_wavs, clean_wavs, x_T=None, stoi=False):
        """The validation loop's enhancement and scoring in one call (:408-494 with utils/metrics.py: compare_complex, less
        PESQ and STOI): ``enhance_batch(noisy_wavs, trim_to_frames=True)``, the clean references cut to the same
        ``(frame_num - 1) * 160`` samples (utils/metrics.py:562-563), then ``metrics.quality`` on the device-resident result.
        Returns (enhanced_list, scores): ``scores`` holds the per-utterance device tensors ``ssnr``, ``llr``, ``wss``,
        ``fwsnrseg`` and, as compare_complex returns means, ``mean_ssnr`` ... ``mean_fwsnrseg`` (0-dim device tensors).
        One synchronisation in total: the pass's own check (``_checked``); the scores are asynchronous.
        stoi=True: ``metrics.quality(..., stoi=True)``, so ``scores`` also holds ``stoi``, ``estoi``, ``mean_stoi`` and
        ``mean_estoi`` - every figure of the reference's loop except PESQ."""
        from . import metrics

        clean_wavs = [torch.as_tensor(w, dtype=torch.float32).flatten() for w in clean_wavs]
        noisy_lens = [int(torch.as_tensor(w).numel()) for w in noisy_wavs]
        if len(clean_wavs) != len(noisy_lens) or any(c.numel() != n for c, n in zip(clean_wavs, noisy_lens)):
            raise ValueError("every noisy utterance needs a clean reference of its own length")
        cut = [(n // 160) * 160 for n in noisy_lens]
        if min(cut) < metrics.MIN_LEN:
            raise ValueError("utterances must keep at least %d samples after trimming to frames" % metrics.MIN_LEN)
        enhanced = self.enhance_batch(noisy_wavs, x_T=x_T, trim_to_frames=True)
        pad = torch.nn.utils.rnn.pad_sequence
        clean = pad([c[:n] for c, n in zip(clean_wavs, cut)], batch_first=True).to(self.device)
        with torch.cuda.device(self.device):
            scores = metrics.quality(clean, pad(enhanced, batch_first=True), lens=cut, stoi=stoi)
        for k in ("ssnr", "llr", "wss", "fwsnrseg") + (("stoi", "estoi") if stoi else ()):
            scores["mean_" + k] = scores[k].mean()
        return enhanced, scores

    # ---- A2..A7: the reference's entry point --------------------------------
    def generate_wav(self, load_pre_train=True, data_path="data/noisy_testset_wav", rng_fidelity=True, batch=1, inflight=1, members=1,
                     window=None):
        """Per-file B=1 enhancement of ``data_path/*.wav`` into ``args.generated_wav``
        (:903-1018).  Returns the list of written paths instead of calling exit().

        feat_type: the reference's own generate_wav defines its compressed magnitude for "sqrt" only and stops with a NameError
        for every other value; for those this method follows the statements of the validation loop (:414-435 to compress,
        utils/metrics.py:534-551 to decompress), as every other entry point does.

        One loop (``_file_loop``) serves the three modes: the sorted paths are read, every readable file's x_T is drawn in path
        order at its own shape and followed at once by its ``rng_fidelity`` discards, the files are enhanced, and the results
        are written under the sources' names, in path order.  The modes differ only in how the files are enhanced, so file k's
        noise, the names and the state the generator is left in are the same whatever ``batch`` and ``inflight`` are.

        batch (default 1: one file per pass, ``enhance``, verified): N > 1 enhances N files per pass as exact ragged batches
        (``enhance_batch(exact=True)``; ``raggedplan``): the sorted paths are taken in windows of 8 N, a window is decoded at
        once and drawn as above; the window is then sorted by length and enhanced N at a time, padded to a multiple of 2560
        samples.

        rng_fidelity: the reference draws ``randn_like(audio)`` after every reverse step n > 0 (:986-987) and multiplies
        it by ``newsigma == 0``; the draws change nothing in a file's output but advance the generator, so file k's
        x_T depends on them.  With the flag set the same number of same-shaped draws is made (and discarded) for each
        file - behind its x_T and, as no pass draws from the generator, ahead of its pass instead of after it - which keeps a
        seeded ``--generate`` run on the reference's generator stream file for file.
        Files that cannot be read (unsupported encoding) are logged and skipped instead of aborting the run.
        A file's PCM frames are decoded, mixed to mono and converted to 16 kHz on the device (``wavdev.load``); the waveform
        is ``wavio.read_wav``'s bit for bit, so the written files do not depend on which of the two produced it.

        inflight (default 1: one file at a time): N = 2 .. 4 with ``batch`` 1 sends the files through
        ``enhance_stream(inflight=N)``: they are read, decoded, drawn and skipped as in the default mode, file by file as the
        stream asks for them, and the same files are written under the same names; every file is verified by its plan's
        own verdict instead of a synchronisation per file.  The bits are those of an ``exclusive=False`` trainer (see
        ``enhance_stream``).  With ``batch`` > 1: ValueError (streams of ragged windows are not built).

        members (default 1): K = 2 .. 16 writes every file from the mean of a K-member posterior ensemble (``enhance_members``:
        one pass of the front end and the prior, K reverse trajectories).  Member k's x_T is the file's k-th draw, each followed by
        its own ``rng_fidelity`` discards: a seeded run draws for a file what K consecutive one-member runs of it would draw.
        ``<args.log>/ensemble.json`` (``args.log``: ``<assets>/log/<doc>``; beside the written files where the arguments have
        none) then holds, per file, ``relative_spread`` and ``medoid``, the index of the member nearest the mean (the argmin of
        ``per_member``).  One file per pass: with ``batch`` > 1, ``inflight`` > 1, ``channels="each"`` or an ``audit=True``
        trainer: ValueError.

        window (default None: the trainer's ``window``): W frames - a file of more than W frames takes the windowed pass
        (``enhance(window=W)``): one window plan serves a directory of recordings of any lengths.  Same draws, same names.  One
        file per pass: with ``batch`` > 1, ``inflight`` > 1, ``members`` > 1 or ``channels="each"``: ValueError."""
        inflight = _inflight_arg(inflight)
        members = L.members_arg(members)
        window = getattr(self, "window", None) if window is None else longplan.window_arg(window)
        if window is not None:
            longplan.window_conflicts(ragged=int(batch) > 1, inflight=inflight, members=members, per_channel=self.channels == "each")
            LongSampler.prior_check(self.prior_name)
        if inflight > 1 and int(batch) > 1:
            raise ValueError("generate_wav: inflight > 1 runs one file per pass (batch=1); streams of ragged windows are not built")
        if members > 1:
            for on, what in ((int(batch) > 1, "batch > 1 (exact ragged batches run one trajectory per file)"),
                             (inflight > 1, "inflight > 1 (the in-flight plans are verified by the verdict, which an ensemble plan lacks)"),
                             (self.channels == "each", "channels='each' (a file's channels share an exact ragged pass)"),
                             (self.audit, "audit=True (the range audit reads one trajectory's report)")):
                if on:
                    raise ValueError("generate_wav(members=%d) with %s: ensembles are built for one file per pass" % (members, what))
        if load_pre_train and getattr(self.args, "retrain", False):
            self._load_checkpoint()
        os.makedirs(self.args.generated_wav, exist_ok=True)
        if int(batch) > 1:
            return self._generate_wav_batched(data_path, rng_fidelity, int(batch))
        one_by_one = lambda n: [(k, k + 1) for k in range(n)]   # noqa: E731  (a file is read when its turn comes)
        if members > 1:
            report = {}
            written = self._file_loop(data_path, rng_fidelity, one_by_one, partial(self._enhance_ensembles, members=members, report=report),
                                      members=members)
            import json

            log = getattr(self.args, "log", None) or self.args.generated_wav
            os.makedirs(log, exist_ok=True)
            with open(os.path.join(log, "ensemble.json"), "w") as f:
                json.dump({"members": members, "files": report}, f, indent=1)
            return written
        return self._file_loop(data_path, rng_fidelity, one_by_one, partial(self._enhance_files, inflight=inflight, window=window))

    def _enhance_ensembles(self, windows, members, report):
        """``_file_loop``'s files one per pass as K-member ensembles: the file from the mean, its figures into ``report``."""
        for path, wav, x_T in chain.from_iterable(windows):
            res = self.enhance_members(wav[None], x_T=x_T, members=members)
            report[os.path.basename(path)] = {"relative_spread": float(res["relative_spread"][0]),
                                              "medoid": int(torch.argmin(res["per_member"][:, 0]))}
            yield path, res["wav"][0]

    def _generate_wav_batched(self, data_path, rng_fidelity, batch):
        ragged_args(self.prior_name, 161, masked=self.masked_prior)
        return self._file_loop(data_path, rng_fidelity, partial(raggedplan.windows, batch=batch), partial(self._enhance_windows, batch=batch))

    def _file_loop(self, data_path, rng_fidelity, windows, enhance, members=1):
        """The file loop of ``generate_wav``.  windows(n) -> [(lo, hi)]: the slices of the sorted paths that are read at once.
        enhance: a generator function; it is handed an iterator of windows, each an iterator of the window's readable files as
        ``(path, wav [len], x_T)``, and yields ``(path, enhanced [len])`` in path order (``channels="each"``, a file of C > 1
        channels: wav [C, len], x_T [C, 2, T, 161], enhanced [C, len]).  Nothing is read or drawn before
        ``enhance`` asks for it, and x_T and discards are drawn in the order it asks: path order."""
        paths = sorted(glob.glob(data_path + "/*.wav"))
        ndiscard = len(self.inference_schedule(self.params.fast_sampling)[0]) - 1 if rng_fidelity else 0   # a plan's steps less one

        def drawn(window):
            for path, wav in self._load_window(window):
                shape = (1, 2, 1 + wav.shape[-1] // 160, 161)
                x_T = []
                # channels="each": a draw per channel, in channel order; members=K (mono rows only): a draw per member, in member order
                for _ in range(members if wav.dim() == 1 else wav.shape[0]):
                    x_T.append(self._x_T(shape, None))                        # :947-950 randn_like(init): the file's draw, kept for a repeat
                    for _ in range(ndiscard):
                        torch.randn(*shape, device=self.device, dtype=torch.float32)     # :986 randn_like, scaled by 0
                yield path, wav, x_T[0] if wav.dim() == 1 and members == 1 else torch.cat(x_T)

        written = []
        with torch.no_grad():
            for path, out in enhance(drawn(paths[lo:hi]) for lo, hi in windows(len(paths))):
                dst = os.path.join(self.args.generated_wav, path.split("/")[-1])
                self._write_wav(dst, out, path)
                written.append(dst)
        print("success!")
        return written

    def _enhance_files(self, windows, inflight, window=None):
        """``_file_loop``'s files one per pass: through ``enhance`` (verified: ``SamplerPipeline.check()``, f16x2 window fallback)
        or, ``inflight`` > 1, through ``enhance_stream``, which asks for a file as a slot comes free."""
        files = chain.from_iterable(windows)
        if inflight == 1:
            for path, wav, x_T in files:
                if wav.dim() == 1:
                    # window None: the call as it always was
                    yield path, (self.enhance(wav[None], x_T=x_T) if window is None else self.enhance(wav[None], x_T=x_T, window=window))[0]
                else:                                # a file's channels: one exact ragged pass of equal lengths, nothing padded
                    yield path, torch.stack(self._enhance_ragged(list(wav), list(x_T), wav.shape[1]))
            return
        paths = deque()                              # (path, mono) of the files handed to the stream and not yet handed back

        def items():
            for path, wav, x_T in files:
                if wav.dim() == 2 and self.prior_name not in RAGGED_PRIORS:
                    raise ValueError("generate_wav(inflight=%d) with channels='each': the channels of %s would share a dense pass "
                                     "of prior %r, which is built for %s only" % (inflight, path, self.prior_name, ", ".join(RAGGED_PRIORS)))
                paths.append((path, wav.dim() == 1))
                yield (wav[None] if wav.dim() == 1 else wav), x_T

        for out, _ in self.enhance_stream(items(), inflight=inflight):
            path, mono = paths.popleft()
            yield path, out[0] if mono else out

    def _enhance_windows(self, windows, batch):
        """``_file_loop``'s files ``batch`` per pass: a window sorted by length, in exact ragged batches (``raggedplan.buckets``)."""
        for window in windows:
            files = list(window)                     # path order: the generator sees what the B = 1 loop shows it
            # the rows of the window: a file's waveform, or (channels="each") each of its channels, with its own x_T
            rows = [(w, x) for _, wav, x_T in files for w, x in ([(wav, x_T)] if wav.dim() == 1 else zip(wav, x_T))]
            outs = [None] * len(rows)
            for idx, L_pad in raggedplan.buckets([w.numel() for w, _ in rows], batch):
                res = self._enhance_ragged([rows[i][0] for i in idx], [rows[i][1] for i in idx], L_pad)
                for i, r in zip(idx, res):
                    outs[i] = r
            r = 0
            for path, wav, _ in files:               # regrouped per file
                n = 1 if wav.dim() == 1 else wav.shape[0]
                yield path, outs[r] if wav.dim() == 1 else torch.stack(outs[r:r + n])
                r += n

    def _load_window(self, paths):
        """[(path, wav [len] on the device)] of the readable files of ``paths``, in order, decoded in one call ([B, Lmax] on the
        device, ``read_wav``'s bits); where that fails at least one file cannot be read: they are then read one by one, and the
        unreadable ones are logged and skipped."""
        try:
            if self.channels == "each":
                return self._load_channels(paths)
            wav, lens = wavdev.load(paths, self.device, 16000, formats=self.wav_formats)
            return [(p, wav[i, :lens[i]]) for i, p in enumerate(paths)]
        except (ValueError, EOFError, wavio.wave.Error) as e:
            if len(paths) == 1:
                logging.warning("skipping %s: %s", paths[0], e)
                return []
        return [f for p in paths for f in self._load_window([p])]

    def _load_channels(self, paths):
        """``_load_window``'s decode under ``channels="each"``: [(path, wav)] with wav [len] for a mono file and [C, len] for one
        of C = 2 .. 8 channels, the rows of ``wavio.read_channels``.  A source with more channels (or a header ``wavio.probe``
        does not take) goes through the mix's loader and is enhanced as the mix."""
        def wide(path):
            try:
                return wavio.probe(path)[1] > L.WAV_MAX_CH
            except (ValueError, OSError):
                return True

        mix = [p for p in paths if wide(p)]
        each = [p for p in paths if p not in mix]
        found = {}
        if each:
            wav, lens, chans = wavdev.load(each, self.device, 16000, formats=self.wav_formats, channels="each")
            r = 0
            for p, ch in zip(each, chans):
                found[p] = wav[r, :lens[r]] if ch == 1 else wav[r:r + ch, :lens[r]]
                r += ch
        if mix:
            wav, lens = wavdev.load(mix, self.device, 16000, formats=self.wav_formats)
            for i, p in enumerate(mix):
                logging.warning("%s: more than %d channels, enhanced as the mix", p, L.WAV_MAX_CH)
                found[p] = wav[i, :lens[i]]
        return [(p, found[p]) for p in paths]

    def _write_channels(self, dst, out, src):
        """The writer of a file whose C = 2 .. 8 channels were enhanced apart (``channels="each"``).  out: [C, len] at 16 kHz.
        "source": ``_write_wav``'s steps with ``wavdev.encode_channels`` - the source's rate, frame count and encoding, channel
        c from row c.  "pcm16" (or a header ``wavio.probe`` refuses): 16 kHz, 16-bit, C channels through the same encoder at
        ratio 1 - per channel the payload ``wavio.write_wav`` writes.  One warning for a file that clipped, with the counts per
        channel."""
        out = torch.as_tensor(out, dtype=torch.float32).to(self.device)
        C, n = int(out.shape[0]), int(out.shape[1])
        rate, fmt, width, keep = 16000, wavio.WAV_INT, 2, n
        if self.wav_out == "source":
            try:
                rate, _, tag, width, n_src = wavio.probe(src)
                tag, width = wavio.target_of((tag, width))
                fmt = wavio.WAV_FLOAT if tag == 3 else wavio.WAV_INT
                keep = min(n_src, wavio.out_len(n, 16000, rate))
            except ValueError as e:
                logging.warning("%s: written at 16 kHz, 16-bit: %s", dst, e)
                rate, fmt, width, keep = 16000, wavio.WAV_INT, 2, n
        (payload,), (clipped,) = wavdev.encode_channels(out, [n] * C, [C], self.device, rate, fmt, width, n_keep=[keep])
        wavio.write_payload(dst, payload, rate, fmt, width, C)
        if any(clipped):
            logging.warning("%s: %s of %d samples per channel clipped at the %d-bit range", dst, "/".join(str(c) for c in clipped), keep, 8 * width)

    def _write_wav(self, dst, out, src):
        """The writer of the file loop.  out: the enhanced waveform of the file ``src`` at 16 kHz, 1-D - a numpy array or a
        tensor.  "pcm16": ``wavio.write_wav``.  "source": the header of ``src`` is read again (``wavio.probe``), the waveform goes
        through ``wavdev.encode`` at the source's rate, cut to the source's frame count, and the frames are written behind a plain
        header (``wavio.write_payload``).  A source with more channels than the encoder interleaves (8) is written mono.
        A 2-D ``out`` - [C, len], the channels of a file enhanced apart - goes to ``_write_channels``."""
        if getattr(out, "ndim", 1) == 2:
            return self._write_channels(dst, out, src)
        probe = None
        if self.wav_out == "source":
            try:
                probe = wavio.probe(src)
            except ValueError as e:                  # a header the loader's reader took and ``probe`` does not
                logging.warning("%s: written at 16 kHz, 16-bit, mono: %s", dst, e)
        if probe is None:
            wavio.write_wav(dst, out.cpu().numpy() if torch.is_tensor(out) else out, 16000)
            return
        rate, ch, tag, width, n_src = probe
        tag, width = wavio.target_of((tag, width))
        fmt = wavio.WAV_FLOAT if tag == 3 else wavio.WAV_INT
        if ch > L.WAV_MAX_CH:
            logging.warning("%s: %d channels in the source, written as one", dst, ch)
            ch = 1
        out = torch.as_tensor(out, dtype=torch.float32).to(self.device).flatten()
        keep = min(n_src, wavio.out_len(out.numel(), 16000, rate))
        (payload,), (clipped,) = wavdev.encode(out[None], [out.numel()], self.device, rate, fmt, width, ch, n_keep=[keep])
        wavio.write_payload(dst, payload, rate, fmt, width, ch)
        if clipped:
            logging.warning("%s: %d of %d samples clipped at the %d-bit range", dst, clipped, keep, 8 * width)

    # ---- the validation epoch (:399-580) -------------------------------------
    @staticmethod
    def _pairs(noisy_wavs, clean_wavs):
        """-> (noisy, clean, lens): the utterance pairs of a batch as lists of 1-D fp32 tensors and their lengths; ValueError for
        a pair of unequal length and for an utterance no longer than the reflect padding."""
        noisy = [torch.as_tensor(w, dtype=torch.float32).flatten() for w in noisy_wavs]
        clean = [torch.as_tensor(w, dtype=torch.float32).flatten() for w in clean_wavs]
        lens = [int(w.numel()) for w in noisy]
        if len(clean) != len(noisy) or any(c.numel() != n for c, n in zip(clean, lens)):
            raise ValueError("every noisy utterance needs a clean partner of its own length")
        if min(lens) < 161:
            raise ValueError("utterances must be longer than the reflect padding (160 samples)")
        return noisy, clean, lens

    def _padded(self, wavs, lens):
        """The utterances zero-padded to the longest, [B, L] on the device (Collate.collate_fn, utils/dataset.py:45-58)."""
        batch = torch.zeros(len(wavs), max(lens), dtype=torch.float32, device=self.device)
        for b, w in enumerate(wavs):
            batch[b, :lens[b]] = w.to(self.device)
        return batch

    def validate_batch(self, noisy_wavs, clean_wavs, x_T=None, exact=False, prior=True, stoi=False, members=1):
        """One batch of the validation loop, scored on the device (:408-559).  noisy_wavs, clean_wavs: lists of 1-D
        waveforms, pair by pair of one length.  The pass is ``enhance_batch``'s - every noisy utterance RMS-normalised over its
        own samples, zero-padded to the longest, the padding takes part (exact=True: the exact ragged pass, every utterance as
        if enhanced alone; the label then reflects at the utterance's own end too) - on a plan with the label leg
        (``SamplerPipeline(label=True)``).  x_T: [B, 2, T, 161] of the padded batch; None: one draw of that shape.
        Scored: the final spectrogram and, with ``prior``, X_init against the label spectrogram (``ops.spec_losses`` over
        ``frame_num = len // 160 + 1`` frames), and their normalised-domain waveforms against the label's, all three the ISTFT of
        a decompressed spectrogram cut to ``(frame_num - 1) * 160`` samples, as compare_complex cuts them
        (``metrics.quality(..., stoi=stoi)``).
        Returns (enhanced, scores): enhanced is ``enhance_batch(..., trim_to_frames=True)``'s list; scores holds ``frames``
        (host list) and, under "x" and "init", device tensors: ``loss`` [3] (com_mse, mag_mse, com_mag_mse), ``per_utt`` [B, 2]
        float64 numerators and one [B] tensor per measure.  One synchronisation: the pass's own check (``_checked``).
        members: K > 1 runs a K-member ensemble of the padded batch (``enhance``; x_T [K, B, 2, T, 161] or [K B, 2, T, 161], None:
        K consecutive draws).  "x" then scores the ensemble mean - its spectrogram, and the waveforms the label leg makes of
        it - "init" is what it is for one member, and scores holds "ensemble": ``members``; ``loss_by_member`` [K], the com_mse of
        every member's own [B, 2, T, 161] block against the label (``ops.spec_losses``), with ``per_utt_by_member`` [K, B, 2], its
        numerators; ``loss_member_mean`` and ``loss_member_std`` (over the K members; the sample standard deviation) and
        ``relative_spread`` [B] (``enhance_members``).  With exact=True: ValueError."""
        self._no_window("validate_batch")
        from . import metrics, validation as V

        members = L.members_arg(members)
        if exact and members > 1:
            raise ValueError("validate_batch(exact=True, members=%d): an exact ragged plan runs one trajectory per utterance; ensembles "
                             "take the padded pass (exact=False)" % members)
        noisy, clean, lens = self._pairs(noisy_wavs, clean_wavs)
        frames, cut = [V.frame_num(n) for n in lens], [V.trim_len(n) for n in lens]
        if min(cut) < metrics.MIN_LEN:
            raise ValueError("utterances must keep at least %d samples after trimming to frames" % metrics.MIN_LEN)
        B, L_ = len(noisy), max(lens)
        if exact:
            ragged_args(self.prior_name, L_, masked=self.masked_prior)
        batch, cbatch = self._padded(noisy, lens), self._padded(clean, lens)
        x_T = self._x_T((B, 2, 1 + L_ // 160, 161), x_T, members)

        def run(pipe, graph):
            out, spec = pipe.enhance(batch, x_T, lens=lens, exact=exact, clean=cbatch)           # never replayed
            leg, scores = pipe.label, {"frames": frames}
            with torch.cuda.device(self.device):
                for name, sp, wav in (("x", spec, leg.est_wav), ("init", pipe.init_spec, leg.init_wav))[:2 if prior else 1]:
                    ls = ops.spec_losses(sp, leg.spec, frames)
                    q = metrics.quality(leg.wav, wav, lens=cut, stoi=stoi)
                    scores[name] = dict(q, loss=torch.stack([ls[k] for k in V.LOSSES]), per_utt=ls["per_utt"])
                if members > 1:
                    by = [ops.spec_losses(pipe.members_spec[k * B:(k + 1) * B], leg.spec, frames) for k in range(members)]
                    loss = torch.stack([r["com_mse"] for r in by])
                    scores["ensemble"] = {"members": members, "loss_by_member": loss, "per_utt_by_member": torch.stack([r["per_utt"] for r in by]),
                                          "loss_member_mean": loss.double().mean(), "loss_member_std": loss.double().std(),
                                          "relative_spread": ops.relative_spread(pipe.ensemble["per_utt"], members)}
            return [out[i, :cut[i]].clone() for i in range(B)], scores

        return self._checked(run, B=B, L_=L_, ragged=bool(exact), label=True, members=members)

    def validate(self, noisy_dir="data/noisy_testset_wav", clean_dir="data/clean_testset_wav", batch_size=None, order="sorted",
                 drop_last=False, exact=False, prior=True, stoi=False, rng_fidelity=True, x_T=None, members=1):
        """One validation epoch over the (noisy, clean) pairs of two directories: what ``train_ddpm`` runs after an epoch of
        training, and all it runs under ``--eval`` (:387, :399-580).  Returns the dictionary of ``validation.aggregate``.

        Pairs are matched by file name (VBCvDataset, utils/dataset.py:133-153), decoded on the device (``wavdev.load``, the
        trainer's ``wav_formats``); a noisy file without a partner and a pair of unequal length raise ValueError naming the
        file.  batch_size: None is ``config.train.batch_size``.  Batches are windows of the sorted names, the last one partial:
        every file is scored, in a reproducible order.  The reference shuffles and drops the last partial batch: order=
        "shuffled" takes one ``torch.randperm`` from the global generator, drop_last=True drops the tail.
        Per batch (``validate_batch``): x_T is one draw of the batch's shape, followed with ``rng_fidelity`` by the reverse loop's
        discarded draws (:448, :484); x_T: None, or a list with one [B, 2, T, 161] tensor per batch, in batch order (nothing is
        drawn then).  The scores stay on the device until the epoch ends and come back in one copy; a batch synchronises once,
        for its pass's own check.
        ``loss``: the mean of the batches' com_mse - the reference's cv_loss / test_com_mse_loss; ``loss_per_frame``: summed
        numerators over summed denominators; the same pair under ``mag_mse`` and ``com_mag_mse``; ``mean_ssnr``, ``mean_llr``,
        ``mean_wss``, ``mean_fwsnrseg`` (``mean_stoi``, ``mean_estoi`` with ``stoi``): means of batch means; with ``prior`` all of it
        again under "init", for X_init - what the diffusion adds over its prior; ``files``: per file its name, frames, loss
        numerators and measures.  PESQ and the composite figures that need it stay out, as in ``metrics``.
        members: K > 1 scores a K-member ensemble per batch (``validate_batch``): "x" is the ensemble mean's, "init" unchanged, and
        the dictionary gains "ensemble": ``members``, ``loss_by_member`` (K com_mse values, each the mean of the batches' as
        ``loss`` is), ``loss_member_mean`` and ``loss_member_std`` over those K (the sample standard deviation) and
        ``relative_spread``, the mean over files.  A batch's draws are member by member: member k's x_T, then with ``rng_fidelity``
        its discards - what K consecutive one-member passes of the batch draw.  x_T: per batch [K, B, 2, T, 161] or
        [K B, 2, T, 161].  With exact=True: ValueError."""
        members = L.members_arg(members)
        if exact and members > 1:
            raise ValueError("validate(exact=True, members=%d): an exact ragged plan runs one trajectory per utterance; ensembles take "
                             "the padded pass (exact=False)" % members)
        names, batches, load = self._pair_epoch(noisy_dir, clean_dir, batch_size, order, drop_last)
        if x_T is not None and len(x_T) != len(batches):
            raise ValueError("x_T: expected one tensor per batch (%d), got %d" % (len(batches), len(x_T)))
        ndiscard = len(self.inference_schedule(self.params.fast_sampling)[0]) - 1 if rng_fidelity else 0
        held = []
        with torch.no_grad():
            for k, idx in enumerate(batches):
                noisy, clean = load(idx)
                shape = (len(idx), 2, 1 + max(int(w.numel()) for w in noisy) // 160, 161)
                if x_T is None:
                    draws = []
                    for _ in range(members):
                        draws.append(self._x_T(shape, None))                       # :448 randn_like(init_audio)
                        for _ in range(ndiscard):
                            torch.randn(*shape, device=self.device, dtype=torch.float32)   # :484 randn_like(audio), scaled by 0
                    draw = draws[0] if members == 1 else torch.cat(draws)
                else:
                    draw = x_T[k]
                _, scores = self.validate_batch(noisy, clean, x_T=draw, exact=exact, prior=prior, stoi=stoi, members=members)
                held.append((idx, scores))
        res = self._collect_validation(held, names, prior, stoi)
        if members > 1:
            import numpy as np

            flat = torch.cat([torch.cat([sc["ensemble"]["loss_by_member"].double(), sc["ensemble"]["relative_spread"]]) for _, sc in held])
            host, by, spread, at = flat.cpu().numpy(), [], [], 0
            for idx, _ in held:
                by.append(host[at:at + members])
                spread += list(host[at + members:at + members + len(idx)])
                at += members + len(idx)
            loss = np.mean(by, axis=0)                                              # per member: the mean of the batches' com_mse
            res["ensemble"] = {"members": members, "loss_by_member": [float(v) for v in loss], "loss_member_mean": float(loss.mean()),
                               "loss_member_std": float(loss.std(ddof=1)), "relative_spread": float(np.mean(spread))}
        return res

    def _pair_epoch(self, noisy_dir, clean_dir, batch_size, order, drop_last):
        """The file loop of an epoch over the (noisy, clean) pairs of two directories, shared by ``validate`` and ``objective``:
        -> (names, batches, load).  names: the pairs' file names in name order (``validation.pair_names``); batches: the epoch's
        windows as lists of indices into them (``validation.windows``; batch_size None: ``config.train.batch_size``);
        load(idx) -> (noisy, clean): the pairs of one batch decoded on the device (``wavdev.load``, the trainer's
        ``wav_formats``) as lists of 1-D waveforms of their own lengths, a pair of unequal length raising ValueError."""
        from . import validation as V

        pairs = V.pair_names(noisy_dir, clean_dir)
        if batch_size is None:
            batch_size = self.config.train.batch_size
        batches = V.windows(len(pairs), batch_size, order=order, drop_last=drop_last)

        def load(idx):
            part = [pairs[i] for i in idx]
            nwav, nlens = wavdev.load([p for p, _ in part], self.device, 16000, formats=self.wav_formats)
            cwav, clens = wavdev.load([c for _, c in part], self.device, 16000, formats=self.wav_formats)
            V.check_lengths(part, nlens, clens)
            return [nwav[j, :nlens[j]] for j in range(len(idx))], [cwav[j, :clens[j]] for j in range(len(idx))]

        return [os.path.basename(p) for p, _ in pairs], batches, load

    def _collect_validation(self, held, names, prior, stoi):
        """The epoch's scores in one copy to the host, then ``validation.aggregate``."""
        from . import validation as V

        measures = V.MEASURES + (V.STOI_MEASURES if stoi else ())
        sections = ("x", "init") if prior else ("x",)
        flat = [t.double().flatten() for _, sc in held for s in sections
                for t in [sc[s]["loss"], sc[s]["per_utt"]] + [sc[s][m] for m in measures]]
        host = torch.cat(flat).cpu().numpy() if flat else None
        batches, at = [], 0
        for idx, sc in held:
            B = len(idx)
            row = {"names": idx, "frames": sc["frames"]}
            for s in sections:
                d = {"loss": host[at:at + 3], "per_utt": host[at + 3:at + 3 + 2 * B].reshape(B, 2)}
                at += 3 + 2 * B
                for m in measures:
                    d[m] = host[at:at + B]
                    at += B
                row[s] = d
            batches.append(row)
        return V.aggregate(batches, names, F=161, prior=prior, stoi=stoi)

    # ---- the denoising objective on a held-out set (train_step's figures, :633-760) ---------
    def objective_batch(self, noisy_wavs, clean_wavs, t=None, noise=None, tensors=False):
        """The quantity the eps-network is trained on, for one batch of (noisy, clean) pairs, on the device (:699-738): the
        front of a validation pass - every noisy utterance RMS-normalised over its own samples, zero-padded to the longest,
        the padding takes part; the label scaled by the noisy utterance's c; the prior - then X_init / 11 and label / 11, the
        forward noising at a per-utterance diffusion step (``ops.noising``), ONE eps-net step at those steps, and the loss of
        its prediction against the noise it was given (with ``--sigma``: against the masked noise, ``ops.sigma_loss``).  The
        parameterisation follows ``params.pirorgrad`` / ``params.deltamu`` as :720-733 reads them.  Both networks run in eval
        mode, as in validation: a held-out evaluation of the objective, not a replay of a training step
        (oracle/bn_train_mode_gap.py).  Padded batches only.

        t: [B] integer diffusion steps; None: ``torch.randint(0, len(noise_schedule), [B])``.  noise: [B, 2, T, 161]; None:
        ``torch.randn`` of that shape.  Both are drawn on the device from the global generator, t first (:707, :711), so a
        seeded run follows the reference's draws.
        Returns scores, device tensors but for ``frames`` (host list): ``t`` [B] int32; ``ddpm``: with ``--sigma``
        {"loss" [1], "per_utt" [B]} (``ops.sigma_loss``), else {"loss" [3] (com_mse, mag_mse, com_mag_mse), "per_utt" [B, 2]}
        (``ops.spec_losses``) over ``frame_num = len // 160 + 1`` frames; ``dis``: the latter for X_init against the label, both
        before the division by 11 (:668).  tensors=True: also clones of ``noisy``, ``target``, ``predicted``, ``init`` and
        ``label`` (the last two divided by 11), for tests and debugging.  One synchronisation: the pass's own check
        (``_checked``)."""
        self._no_window("objective_batch")
        from . import validation as V

        noisy, clean, lens = self._pairs(noisy_wavs, clean_wavs)
        frames = [V.frame_num(n) for n in lens]
        B, T = len(noisy), 1 + max(lens) // 160
        if t is None:
            t = torch.randint(0, len(self.params.noise_schedule), [B], device=self.device)               # :707
        if noise is None:
            noise = torch.randn(B, 2, T, 161, device=self.device, dtype=torch.float32)                    # :711 randn_like(batch_label)
        return self._objective_run(noisy, clean, lens, frames, t, noise, tensors)

    def _objective_run(self, noisy, clean, lens, frames, t, noise, tensors):
        """``objective_batch`` behind its draws: the verified pass on the objective plan of the geometry, and the losses."""
        from . import validation as V

        batch, cbatch = self._padded(noisy, lens), self._padded(clean, lens)
        noise = noise.to(self.device, torch.float32)
        sigma = bool(getattr(self.args, "sigma", False))

        def run(pipe, graph):
            predicted = pipe.objective_pass(batch, cbatch, t, noise, lens=lens)                             # never replayed
            leg = pipe.objective
            with torch.cuda.device(self.device):
                dis = ops.spec_losses(pipe.init_spec, pipe.label.spec, frames)
                if sigma:
                    ls = ops.sigma_loss(predicted, leg.target, pipe.init, leg.maxbuf, frames)
                    ddpm = {"loss": ls["com_mse_sigma"].reshape(1), "per_utt": ls["per_utt"]}
                else:
                    ls = ops.spec_losses(predicted, leg.target, frames)
                    ddpm = {"loss": torch.stack([ls[k] for k in V.LOSSES]), "per_utt": ls["per_utt"]}
            scores = {"frames": frames, "t": leg.t.clone(), "ddpm": ddpm,
                      "dis": {"loss": torch.stack([dis[k] for k in V.LOSSES]), "per_utt": dis["per_utt"]}}
            if tensors:
                scores.update(noisy=pipe.audio.clone(), target=leg.target.clone(), predicted=predicted.clone(),
                              init=pipe.init.clone(), label=leg.label.clone())
            return scores

        return self._checked(run, B=len(noisy), L_=max(lens), objective=True)

    def objective(self, noisy_dir="data/noisy_testset_wav", clean_dir="data/clean_testset_wav", batch_size=None, order="sorted",
                  drop_last=False, draws=1, t=None, noise=None, lam=None):
        """One epoch of the denoising objective over the (noisy, clean) pairs of two directories: ``train_step``'s three logged
        figures (:743-749) on a held-out set, and the eps-net's loss by diffusion step.  Returns the dictionary of
        ``objective.aggregate``.  The file loop is ``validate``'s (``_pair_epoch``): pairs by name, windows of the sorted names,
        ``order`` / ``drop_last`` as there.  draws: every batch is evaluated this many times with fresh (t, noise) - one draw per
        pair gives a noisy per-step curve on a small set.  t / noise: None, or lists with one entry per (batch, draw), batch by
        batch (nothing is drawn then).  lam: the weight of ddpm_loss in loss_sum; None: ``config.train.lam``, 1.0 where the
        config has none.  The loss is the one ``config.train.loss`` names (``objective.loss_name``), the --sigma loss for
        ddpm_loss with ``--sigma``.  The scores stay on the device until the epoch ends and come back in one copy; an
        evaluation synchronises once, for its pass's own check."""
        from . import objective as O

        loss = O.loss_name(self.config)
        draws = int(draws)
        if draws < 1:
            raise ValueError("draws must be at least 1, got %d" % draws)
        names, batches, load = self._pair_epoch(noisy_dir, clean_dir, batch_size, order, drop_last)
        for given, what in ((t, "t"), (noise, "noise")):
            if given is not None and len(given) != len(batches) * draws:
                raise ValueError("%s: expected one entry per (batch, draw) (%d), got %d" % (what, len(batches) * draws, len(given)))
        held = []
        with torch.no_grad():
            for k, idx in enumerate(batches):
                noisy, clean = load(idx)
                for j in range(draws):
                    at = k * draws + j
                    scores = self.objective_batch(noisy, clean, t=None if t is None else t[at], noise=None if noise is None else noise[at])
                    held.append((idx, scores))
        if lam is None:
            lam = getattr(self.config.train, "lam", 1.0)
        return self._collect_objective(held, names, loss, lam)

    def _collect_objective(self, held, names, loss, lam):
        """The epoch's scores in one copy to the host, then ``objective.aggregate``."""
        from . import objective as O

        sigma = bool(getattr(self.args, "sigma", False))
        flat = [x.double().flatten() for _, sc in held for x in (sc["t"], sc["ddpm"]["loss"], sc["ddpm"]["per_utt"], sc["dis"]["loss"],
                                                                  sc["dis"]["per_utt"])]
        host = torch.cat(flat).cpu().numpy() if flat else None
        batches, at = [], 0

        def take(n):
            nonlocal at
            at += n
            return host[at - n:at]

        for idx, sc in held:
            B = len(idx)
            row = {"names": idx, "frames": sc["frames"], "t": take(B).astype(int)}
            row["ddpm"] = {"loss": take(1), "per_utt": take(B)} if sigma else {"loss": take(3), "per_utt": take(2 * B).reshape(B, 2)}
            row["dis"] = {"loss": take(3), "per_utt": take(2 * B).reshape(B, 2)}
            batches.append(row)
        return O.aggregate(batches, names, len(self.params.noise_schedule), loss=loss, sigma=sigma, lam=lam,
                           joint=bool(getattr(self.args, "joint", False)), F=161)

    def train_ddpm(self):
        """With ``args.eval``: one validation epoch (``validate`` over ``args.data`` / ``args.clean``, ``--batch`` as the batch
        size where the CLI was given one), logged in one line, and its dictionary returned - the reference exits there
        (:579-580).  With ``args.objective`` as well: one epoch of the denoising objective instead (``objective``, ``args.draws``
        evaluations per batch).  Without ``args.eval``: training, which this package does not implement."""
        if not getattr(self.args, "eval", False):
            raise NotImplementedError("training is outside the sampling path this package implements (SURVEY.md §8)")
        from . import objective as O, validation as V

        kw = {}
        for arg, name in (("data", "noisy_dir"), ("clean", "clean_dir"), ("eval_batch", "batch_size")):
            if getattr(self.args, arg, None) is not None:
                kw[name] = getattr(self.args, arg)
        if getattr(self.args, "objective", False):
            res = self.objective(draws=getattr(self.args, "draws", 1), **kw)
            logging.info(O.log_line(res))
            return res
        res = self.validate(members=int(getattr(self.args, "members", 1) or 1), **kw)
        logging.info(V.log_line(res))
        return res

    def _no_training(self, *a, **kw):
        raise NotImplementedError("training is outside the sampling path this package implements (SURVEY.md §8)")

    train = train_step = draw_audio = _no_training
