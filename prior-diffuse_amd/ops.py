"""Operator-level boundary: callables with the reference's ``nn.Module.__call__``
signatures for the two networks on the path,

    self.model(feat) -> X_init                   trainer/complex_ddpm_trainer.py:941
    self.model_ddpm(audio, init, t) -> eps       trainer/complex_ddpm_trainer.py:968

on contiguous fp32 ``[B,2,T,161]`` tensors living on an MI355X.  Each (B, T) builds its
plan once (weights packed into HBM once per operator) and replays it afterwards.
"""
from collections import OrderedDict

import torch

from . import _lib as L
from . import nets


class _PlannedOp:
    MAX_PLANS = 3   # recorded (B, T) geometries kept (least recently used first out); packed weights are shared

    def __init__(self, state_dict, device="cuda:0", bank=None, exclusive=False):
        """exclusive: the caller runs nothing else on the GPU beside this operator (one batch in flight), which allows
        launches whose workgroups wait for each other - the persistent LSTM of the GCRN prior at B <= 4 (csrc/lstmp.hip).
        Off by default: with it a small batch takes another kernel than a large one, so an utterance's result is no longer
        bit-identical across batch compositions (it stays within 1e-5)."""
        self.exclusive = bool(exclusive)
        self.sd = state_dict
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.PdseError("operators run on the GPU only (no CPU fallback); got device %s" % device)
        L.load()
        self.bank = bank if bank is not None else nets.WeightBank()
        self._plans = OrderedDict()

    def _plan(self, key, build):
        """LRU of recorded plans; ``build(ctx)`` records a new one against the shared weight bank."""
        net = self._plans.get(key)
        if net is None:
            while len(self._plans) >= self.MAX_PLANS:
                self._plans.popitem(last=False)
            net = self._plans[key] = build(nets.Ctx(self.device, self.bank))
            net.finish()
        else:
            self._plans.move_to_end(key)
        return net

    def _check(self, x):
        if x.dim() != 4 or x.shape[1] != 2 or x.shape[3] != nets.F0:
            raise ValueError("expected [B,2,T,161], got %s" % (tuple(x.shape),))
        if x.dtype != torch.float32:
            raise TypeError("fp32 only (the reference is fp32-only)")

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def eval(self):  # parity contract: eval-mode statistics always
        return self

    @staticmethod
    def _steps(t):
        """Diffusion steps as float32 without a device->host round trip: a tensor that already lives on the GPU is
        range-checked by the kernel's clamp-free table walk only when ``PDSE_CHECK_STEPS`` asks for it (the check
        costs two synchronisations per call, i.e. per reverse step when the operator is driven from a Python loop);
        host tensors and python numbers are checked for free."""
        import os

        if not torch.is_tensor(t):
            t = torch.as_tensor(t)
        tf = t.to(torch.float32)
        if (not tf.is_cuda) or os.environ.get("PDSE_CHECK_STEPS", "0") == "1":
            if tf.numel() and (float(tf.min()) < 0 or float(tf.max()) > 49):
                raise IndexError("diffusion step outside the 50-entry embedding table")  # reference: IndexError
        return tf


class DiffUNet1Op(_PlannedOp):
    """ε-network ``DiffUNet1.forward(x, x_init, t)`` (model/diff3.py:37-57).
    ``t`` float32 -> lerp of the step embedding, int32/int64 -> table lookup."""

    def __call__(self, x, x_init, t):
        self._check(x)
        self._check(x_init)
        B, _, T, _ = x.shape
        if t.shape != (B,):
            raise ValueError("t must have shape [B]")
        tf = self._steps(t)

        def build(ctx):
            net = nets.EpsNetPlan(ctx, self.sd, B, T, time_cond=True, nsteps=1, exclusive=self.exclusive)
            net.build_time()
            net.build_step(0)
            return net

        net = self._plan((B, T), build)
        net.x.copy_(x)
        net.x_init.copy_(x_init)
        net.tsteps.copy_(tf.view(1, B))
        net.plan.run(self._stream())
        return net.out.clone()


class NoconOp(_PlannedOp):
    """Alt eps-net of the ``deltamu`` parameterisation: ``Nocon.forward(x, t)`` (model/piror_grad.py:28-40)."""

    def __call__(self, x, t):
        self._check(x)
        B, _, T, _ = x.shape
        if t.shape != (B,):
            raise ValueError("t must have shape [B]")
        tf = self._steps(t)

        def build(ctx):
            net = nets.EpsNetPlan(ctx, self.sd, B, T, time_cond=True, nsteps=1, with_pre=False, exclusive=self.exclusive)
            net.build_time()
            net.build_step(0)
            return net

        net = self._plan((B, T), build)
        net.x.copy_(x)
        net.tsteps.copy_(tf.view(1, B))
        net.plan.run(self._stream())
        return net.out.clone()


class DiffUNetOp(_PlannedOp):
    """Prior ``DiffUNet.forward(x)`` (model/diff.py:23-33)."""

    def __call__(self, x):
        self._check(x)
        B, _, T, _ = x.shape

        def build(ctx):
            net = nets.EpsNetPlan(ctx, self.sd, B, T, time_cond=False, exclusive=self.exclusive)
            net.build_step(0)
            return net

        net = self._plan((B, T), build)
        net.x.copy_(x)
        net.plan.run(self._stream())
        return net.out.clone()


class GCRNOp(_PlannedOp):
    """Prior ``GCRN.forward(x)`` (model/gcrn.py:136-166)."""

    def __call__(self, x):
        self._check(x)
        B, _, T, _ = x.shape

        def build(ctx):
            net = nets.GcrnPlan(ctx, self.sd, B, T, exclusive=self.exclusive)
            net.build()
            return net

        net = self._plan((B, T), build)
        net.x.copy_(x)
        net.plan.run(self._stream())
        return net.out.clone()


class AiaOp(_PlannedOp):
    """Prior ``aia_complex_trans_ri.forward(x)`` (model/dbaiat.py:461-478, conf/dbaiat.yml:13)."""

    PLAN = "AiaPlan"

    def __call__(self, x):
        self._check(x)
        B, _, T, _ = x.shape

        def build(ctx):
            net = getattr(nets, self.PLAN)(ctx, self.sd, B, T)
            net.build()
            return net

        net = self._plan((B, T), build)
        net.x.copy_(x)
        net.plan.run(self._stream())
        return net.out.clone()


class DualAiaOp(AiaOp):
    """Prior ``dual_aia_trans_merge_crm.forward(x)`` (model/dbaiat.py:386-413), the dual-branch DB-AIAT model."""

    PLAN = "DualAiaPlan"


PRIOR_OPS = {"GCRN": GCRNOp, "DiffUNet": DiffUNetOp, "aia_complex_trans_ri": AiaOp, "dual_aia_trans_merge_crm": DualAiaOp}


def q_sample(label, init, t, noise, noise_schedule=None, mode="pirorgrad", sigma=False):
    """Forward noising of the training step (trainer/complex_ddpm_trainer.py:42-44, :704-729),
    t int64 [B], alpha_bar the float32 cumprod the trainer keeps in ``noise_level``:

        mode "pirorgrad": noisy = sqrt(ab_t) * (label - init) + sqrt(1 - ab_t) * noise          (:718)
        mode "deltamu":   noisy = sqrt(ab_t) * label + sqrt(1 - ab_t) * (noise + init)          (:721)
        mode "plain":     noisy = sqrt(ab_t) * label + sqrt(1 - ab_t) * noise                   (:724)
        sigma: noise is first multiplied by sqrt(|init| / max|init| / 2 + 0.5) per (b, channel) (:709-715)

    ``label`` / ``init`` are already divided by 11 by the caller, like the reference.  Bit-exact with the
    reference's fp32 tensor arithmetic."""
    import numpy as np

    from .params import params as _p

    if label.device.type != "cuda":
        raise L.PdseError("q_sample runs on the GPU only (no CPU fallback)")
    modes = {"pirorgrad": 0, "deltamu": 1, "plain": 2}
    if mode not in modes:
        raise ValueError("mode must be one of %s" % sorted(modes))
    for x in (label, init, noise):
        if not x.is_contiguous() or x.dtype != torch.float32 or x.shape != label.shape:
            raise ValueError("label, init, noise must be contiguous fp32 tensors of one shape")
    stream = torch.cuda.current_stream(label.device).cuda_stream
    if sigma:
        if label.dim() != 4:
            raise ValueError("sigma mask needs [B,C,T,F] tensors")
        masked = torch.empty_like(noise)
        sd_ = L.SigmaDesc()
        sd_.init, sd_.a, sd_.out = init.data_ptr(), noise.data_ptr(), masked.data_ptr()
        maxbuf = torch.empty(label.shape[0] * label.shape[1], device=label.device, dtype=torch.float32)
        sd_.maxbuf, sd_.plane, sd_.nplanes = maxbuf.data_ptr(), label.shape[2] * label.shape[3], label.shape[0] * label.shape[1]
        L.launch(sd_, stream, device=label.device)
        noise = masked
    beta = np.array(_p.noise_schedule if noise_schedule is None else noise_schedule)
    noise_level = torch.tensor(np.cumprod(1 - beta).astype(np.float32), device=label.device)     # :42-44
    ns = noise_level[t.to(label.device).long()]
    a, s = ns ** 0.5, (1.0 - ns) ** 0.5
    out = torch.empty_like(label)
    d = L.QsampleDesc()
    d.label, d.init, d.noise, d.out = label.data_ptr(), init.data_ptr(), noise.data_ptr(), out.data_ptr()
    d.a, d.s, d.plane, d.B, d.mode = a.data_ptr(), s.data_ptr(), label[0].numel(), label.shape[0], modes[mode]
    L.launch(d, stream, device=label.device)
    return out


NOISING_MODES = {"pirorgrad": 0, "deltamu": 1, "plain": 2}     # the numbering of pdse_qsample_desc.mode
_NOISE_TABLES = OrderedDict()     # (device, schedule bytes) -> (a, s) of ``noise_tables``; a few schedules


def noise_tables(device, noise_schedule=None):
    """-> (a, s, steps): the fp32 device tables a[n] = sqrt(alpha_bar_n) and s[n] = sqrt(1 - alpha_bar_n) of a schedule of betas
    (None: ``params.noise_schedule``), with the reference's own arithmetic - the float32 cast of numpy's float64 cumprod the
    trainer keeps in ``noise_level`` (trainer/complex_ddpm_trainer.py:42-44), then ``** 0.5`` and ``(1.0 - x) ** 0.5`` in fp32
    (:710, :726) - computed once per (device, schedule).  The square roots are numpy's: correctly rounded, as ``q_sample``'s are
    on the device, which torch's vectorised CPU square root is not."""
    import numpy as np

    from .params import params as _p

    beta = np.ascontiguousarray(np.array(_p.noise_schedule if noise_schedule is None else noise_schedule, dtype=np.float64))
    key = (str(torch.device(device)), beta.tobytes())
    hit = _NOISE_TABLES.get(key)
    if hit is None:
        while len(_NOISE_TABLES) >= 4:
            _NOISE_TABLES.popitem(last=False)
        level = np.cumprod(1 - beta).astype(np.float32)
        hit = _NOISE_TABLES[key] = tuple(torch.from_numpy(x).to(device) for x in (np.sqrt(level), np.sqrt(np.float32(1.0) - level)))
    else:
        _NOISE_TABLES.move_to_end(key)
    return hit[0], hit[1], beta.size


def noising(label, init, t, noise, mode="pirorgrad", sigma=False, noise_schedule=None, out=None):
    """Forward noising of the denoising objective for a whole batch in one call of csrc/objective.hip (include/pdse.h:
    pdse_objective_noise; trainer/complex_ddpm_trainer.py:709-733): ``q_sample``'s formulas with the schedule indexed on the device
    by ``t`` and, with ``sigma``, the mask taken over every (b, channel) plane of ``init``, padding frames included.

    label, init, noise: contiguous fp32 [B,2,T,F] on the GPU, label and init already divided by 11.  t: [B] integers; a host
    tensor (or a list) is range-checked here (IndexError, as the reference's indexing raises), a device tensor is used as it is -
    the kernel walks the tables without a clamp, like the step embedding (``_PlannedOp._steps``; ``PDSE_CHECK_STEPS=1`` checks it
    at the price of a synchronisation).  mode: "pirorgrad", "deltamu" or "plain".
    Returns (noisy, target, maxbuf): target = noise * sqrt(mask) with ``sigma`` and a copy of noise without, maxbuf [B*2] the
    maxima of |init| (zeros without ``sigma``).  out: three tensors to write instead of new ones.  Bit-exact with the
    reference's fp32 tensor arithmetic; no host synchronisation."""
    import os

    if label.device.type != "cuda":
        raise L.PdseError("noising runs on the GPU only (no CPU fallback)")
    if mode not in NOISING_MODES:
        raise ValueError("mode must be one of %s" % sorted(NOISING_MODES))
    if label.dim() != 4 or label.shape[1] != 2:
        raise ValueError("label, init, noise: fp32 tensors of one [B,2,T,F] shape")
    for x in (label, init, noise):
        if not x.is_contiguous() or x.dtype != torch.float32 or x.shape != label.shape or x.device != label.device:
            raise ValueError("label, init, noise must be contiguous fp32 tensors of one shape and device")
    B, _, T, F_ = label.shape
    dev = label.device
    a, s, steps = noise_tables(dev, noise_schedule)
    t = torch.as_tensor(t)
    if t.shape != (B,) or t.dtype.is_floating_point:
        raise ValueError("t must be [B] integers")
    if (not t.is_cuda) or os.environ.get("PDSE_CHECK_STEPS", "0") == "1":
        if int(t.min()) < 0 or int(t.max()) >= steps:
            raise IndexError("diffusion step outside the %d-entry noise schedule" % steps)
    t = t.to(dev, torch.int32)
    if out is None:
        out = (torch.empty_like(label), torch.empty_like(label), torch.empty(2 * B, dtype=torch.float32, device=dev))
    noisy, target, maxbuf = out
    L.objective_noise(label.data_ptr(), init.data_ptr(), noise.data_ptr(), t.data_ptr(), a.data_ptr(), s.data_ptr(), noisy.data_ptr(),
                      target.data_ptr(), maxbuf.data_ptr(), B, T, F_, NOISING_MODES[mode], 1 if sigma else 0,
                      torch.cuda.current_stream(dev).cuda_stream, device=dev)
    return noisy, target, maxbuf


def sigma_loss(predicted, target, init, maxbuf, frame_list):
    """``com_mse_sigma_loss`` (utils/loss.py:46-56; trainer/complex_ddpm_trainer.py:736) of ``predicted`` against ``target`` over the
    first ``frame_list[b]`` frames of every utterance, in one call of csrc/objective.hip (include/pdse.h: pdse_sigma_loss):

        com_mse_sigma    ((predicted - target) * m / mask * (predicted - target) * m).sum() / (2 F sum frames)

    with mask = |init| / max / 2 + 0.5 recomputed from ``init`` and ``noising``'s ``maxbuf``.  Returns a dict: ``com_mse_sigma``, a
    0-dim fp32 device tensor, and ``per_utt``, float64 [B]: every utterance's numerator, which depends on the utterance alone.
    The element terms are the reference's fp32 terms, added in double in a fixed order.  frame_list: host integers in [0, T], not
    all zero (ValueError).  No host synchronisation."""
    import numpy as np

    if predicted.device.type != "cuda":
        raise L.PdseError("sigma_loss runs on the GPU only (no CPU fallback)")
    if predicted.dim() != 4 or predicted.shape[1] != 2:
        raise ValueError("predicted, target, init: fp32 tensors of one [B,2,T,F] shape")
    for x in (predicted, target, init):
        if not x.is_contiguous() or x.dtype != torch.float32 or x.shape != predicted.shape or x.device != predicted.device:
            raise ValueError("predicted, target, init must be contiguous fp32 tensors of one shape and device")
    B, _, T, F_ = predicted.shape
    dev = predicted.device
    if maxbuf.dtype != torch.float32 or maxbuf.numel() != 2 * B or not maxbuf.is_contiguous() or maxbuf.device != dev:
        raise ValueError("maxbuf: the contiguous fp32 [B*2] tensor of noising()")
    frames_h = np.ascontiguousarray(np.asarray(list(frame_list), dtype=np.int64).reshape(-1))
    if frames_h.size != B or frames_h.min() < 0 or frames_h.max() > T:
        raise ValueError("frame_list: one frame count in [0, T] per utterance")
    if frames_h.sum() == 0:
        raise ValueError("frame_list: no frame in the batch, the loss has no denominator")
    frames_h = frames_h.astype(np.int32)
    frames = torch.from_numpy(frames_h).to(dev)
    partial = torch.empty(B * L.SPECLOSS_BLOCKS, dtype=torch.float64, device=dev)
    per_utt = torch.empty(B, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    L.sigma_loss(predicted.data_ptr(), target.data_ptr(), init.data_ptr(), maxbuf.data_ptr(), frames_h.ctypes.data, frames.data_ptr(),
                 partial.data_ptr(), per_utt.data_ptr(), loss.data_ptr(), B, T, F_, torch.cuda.current_stream(dev).cuda_stream, device=dev)
    return {"com_mse_sigma": loss[0], "per_utt": per_utt}


def com_mse_loss(esti, label, frame_list):
    """Masked complex MSE of the validation loop (utils/loss.py:34-44; trainer/complex_ddpm_trainer.py:490):
    ``((esti - label) * mask) ** 2).sum() / mask.sum()`` over [B,2,T,F] with mask = 1 on the first ``frame_list[b]``
    frames of utterance b.  Returns a 0-dim fp32 tensor on the device (no host synchronisation)."""
    if esti.device.type != "cuda":
        raise L.PdseError("com_mse_loss runs on the GPU only (no CPU fallback)")
    if esti.dim() != 4 or esti.shape != label.shape or esti.dtype != torch.float32 or label.dtype != torch.float32:
        raise ValueError("esti, label: fp32 tensors of one [B,C,T,F] shape")
    if not (esti.is_contiguous() and label.is_contiguous()):
        raise ValueError("esti, label must be contiguous")
    B, C_, T, F_ = esti.shape
    frames = torch.as_tensor(list(frame_list), dtype=torch.int32)
    if frames.numel() != B or int(frames.min()) < 0 or int(frames.max()) > T:
        raise ValueError("frame_list: one frame count in [0, T] per utterance")
    frames = frames.to(esti.device)
    partial = torch.empty(B * L.MASKLOSS_BLOCKS, dtype=torch.float64, device=esti.device)
    out = torch.empty(1, dtype=torch.float32, device=esti.device)
    d = L.MasklossDesc()
    d.esti, d.label, d.frames, d.partial, d.out = (esti.data_ptr(), label.data_ptr(), frames.data_ptr(), partial.data_ptr(),
                                                    out.data_ptr())
    d.B, d.C, d.T, d.F = B, C_, T, F_
    L.launch(d, torch.cuda.current_stream(esti.device).cuda_stream, device=esti.device)
    return out[0]


def spec_losses(esti, label, frame_list):
    """The three masked losses of utils/loss.py over the first ``frame_list[b]`` frames of every utterance of two fp32
    [B,2,T,F] tensors (trainer/complex_ddpm_trainer.py:537; conf/gcrn.yml and conf/dbaiat.yml name ``com_mag_mse_loss``), in one
    call of csrc/valid.hip (include/pdse.h: pdse_spec_losses):

        com_mse      ((esti - label) * mask) ** 2).sum() / (2 F sum frames)                              :34-44
        mag_mse      ((|esti| - |label|) * mask) ** 2).sum() / (F sum frames), |x| = torch.norm(x, dim=1)  :10-19
        com_mag_mse  0.5 * (com_mse + mag_mse)                                                            :59-71

    Returns a dict of 0-dim fp32 device tensors under those names plus ``per_utt``, float64 [B,2]: every utterance's two
    numerators, which depend on the utterance alone (an epoch's per-frame loss is their sum over the summed denominators).
    The element terms are the reference's fp32 terms, added in double in a fixed order.  frame_list: host integers in [0, T], not
    all zero (ValueError).  No host synchronisation."""
    import numpy as np

    if esti.device.type != "cuda":
        raise L.PdseError("spec_losses runs on the GPU only (no CPU fallback)")
    if esti.dim() != 4 or esti.shape[1] != 2 or esti.shape != label.shape or esti.dtype != torch.float32 or label.dtype != torch.float32:
        raise ValueError("esti, label: fp32 tensors of one [B,2,T,F] shape")
    if not (esti.is_contiguous() and label.is_contiguous()) or label.device != esti.device:
        raise ValueError("esti, label must be contiguous tensors of one device")
    B, _, T, F_ = esti.shape
    frames_h = np.ascontiguousarray(np.asarray(list(frame_list), dtype=np.int64).reshape(-1))
    if frames_h.size != B or frames_h.min() < 0 or frames_h.max() > T:
        raise ValueError("frame_list: one frame count in [0, T] per utterance")
    if frames_h.sum() == 0:
        raise ValueError("frame_list: no frame in the batch, the losses have no denominator")
    frames_h = frames_h.astype(np.int32)
    dev = esti.device
    frames = torch.from_numpy(frames_h).to(dev)
    partial = torch.empty(B * L.SPECLOSS_BLOCKS * 2, dtype=torch.float64, device=dev)
    per_utt = torch.empty(B, 2, dtype=torch.float64, device=dev)
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    L.spec_losses(esti.data_ptr(), label.data_ptr(), frames_h.ctypes.data, frames.data_ptr(), partial.data_ptr(), per_utt.data_ptr(),
                  loss.data_ptr(), B, T, F_, torch.cuda.current_stream(dev).cuda_stream, device=dev)
    return {"com_mse": loss[0], "mag_mse": loss[1], "com_mag_mse": loss[2], "per_utt": per_utt}


def ensemble_stats(members, K, frames, out=None):
    """The statistics of a posterior ensemble in one call of csrc/ensemble.hip (include/pdse.h: pdse_ensemble_stats).  members: the
    K members of B utterances, member-major - a contiguous fp32 [K*B,2,T,F] (row k B + b is member k of utterance b) or
    [K,B,2,T,F] tensor; frames: every utterance's own frames, host integers in [0, T].  Returns a dict of device tensors:

        mean        fp32 [B,2,T,F]   the members added in double in member order, divided by K, rounded once
        spread      fp32 [B,T,F]     sqrt(sum_k |x_k - mean|^2 / (K - 1)) per complex bin, from the double mean; zeros for K = 1
        per_utt     float64 [B,2]    over an utterance's own frames: sum_bins sum_k |x_k - mean|^2, and sum_bins |mean|^2
        per_member  float64 [K,B]    over an utterance's own frames: sum_bins |x_k - mean|^2

    ``mean`` and ``spread`` cover every frame, the sums an utterance's own.  The sums are added in a fixed order: two calls give the
    same bits.  out: (mean, spread) to write into - contiguous fp32 tensors of those shapes on the members' device.  No host
    synchronisation."""
    import numpy as np

    K = L.members_arg(K)
    if members.device.type != "cuda":
        raise L.PdseError("ensemble_stats runs on the GPU only (no CPU fallback)")
    if members.dim() == 5:
        if members.shape[0] != K:
            raise ValueError("members: expected [K,B,2,T,F] with K = %d, got %s" % (K, tuple(members.shape)))
        members = members.reshape((-1,) + tuple(members.shape[2:])) if members.is_contiguous() else members
    if members.dim() != 4 or members.shape[1] != 2 or members.dtype != torch.float32 or not members.is_contiguous() or members.shape[0] % K \
            or members.numel() == 0:
        raise ValueError("members: a contiguous fp32 [K*B,2,T,F] or [K,B,2,T,F] tensor")
    B, T, F_ = members.shape[0] // K, members.shape[2], members.shape[3]
    dev = members.device
    frames_h = np.ascontiguousarray(np.asarray(list(frames), dtype=np.int64).reshape(-1))
    if frames_h.size != B or frames_h.min() < 0 or frames_h.max() > T:
        raise ValueError("frames: one frame count in [0, T] per utterance")
    frames_h = frames_h.astype(np.int32)
    if out is None:
        mean, spread = torch.empty(B, 2, T, F_, dtype=torch.float32, device=dev), torch.empty(B, T, F_, dtype=torch.float32, device=dev)
    else:
        mean, spread = out
        for t, shape in ((mean, (B, 2, T, F_)), (spread, (B, T, F_))):
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError("out: contiguous fp32 tensors [B,2,T,F] and [B,T,F] on the members' device")
    frames_d = torch.from_numpy(frames_h).to(dev)
    partial = torch.empty(B * L.ENSEMBLE_BLOCKS * (K + 2), dtype=torch.float64, device=dev)
    per_utt = torch.empty(B, 2, dtype=torch.float64, device=dev)
    per_member = torch.empty(K, B, dtype=torch.float64, device=dev)
    L.ensemble_stats(members.data_ptr(), mean.data_ptr(), spread.data_ptr(), frames_h.ctypes.data, frames_d.data_ptr(), partial.data_ptr(),
                     per_utt.data_ptr(), per_member.data_ptr(), K, B, T, F_, torch.cuda.current_stream(dev).cuda_stream, device=dev)
    return {"mean": mean, "spread": spread, "per_utt": per_utt, "per_member": per_member}


def relative_spread(per_utt, K):
    """``sqrt(per_utt[b][0] / (K - 1) / per_utt[b][1])`` of ``ensemble_stats``' sums: the ensemble's standard deviation over the
    norm of its mean, per utterance, float64 [B] (K = 1: zeros)."""
    if K == 1:
        return torch.zeros_like(per_utt[:, 0])
    return torch.sqrt(per_utt[:, 0] / (K - 1) / per_utt[:, 1])


def _compand(spec, mode, what):
    if spec.device.type != "cuda":
        raise L.PdseError("%s runs on the GPU only (no CPU fallback)" % what)
    if spec.dim() != 4 or spec.shape[1] != 2 or spec.dtype != torch.float32 or spec.numel() == 0:
        raise ValueError("spec: an fp32 [B,2,T,F] tensor")
    spec = spec.contiguous()
    out = torch.empty_like(spec)
    d = L.CompandDesc()
    d.in_, d.out, d.plane, d.B, d.mode = spec.data_ptr(), out.data_ptr(), spec.shape[2] * spec.shape[3], spec.shape[0], mode
    L.launch(d, torch.cuda.current_stream(spec.device).cuda_stream, device=spec.device)
    return out


def compress(spec, feat_type="sqrt"):
    """The front end's compression of a complex spectrogram, fp32 [B,2,T,161] -> a new tensor of that shape: the magnitude m = |X|
    through ``feat_type`` with the phase kept (trainer/complex_ddpm_trainer.py:414-435) - "sqrt" m ** 0.5, "normal" m (re-stacked
    through the phase), "cubic" m ** 0.3, "log_1x" log(m + 1), "none" the spectrogram as it is; any other string: ValueError.
    cos / sin of the phase are re / m, im / m with (1, 0) at m == 0.  One launch of the compand operator (csrc/misc.hip,
    include/pdse.h: pdse_compand_desc), the copy mode for "none".  GPU only, no host synchronisation."""
    mode = L.COMPRESS_MODE[L.feat_type_of(feat_type)]
    return _compand(spec, L.COMPAND_COPY if mode is None else mode, "compress")


def decompress(spec, feat_type="sqrt"):
    """The back end's decompression, the inverse of ``compress`` (utils/metrics.py:531-551): "sqrt" m ** 2, "cubic" m ** (10 / 3),
    "log_1x" exp(m) - 1 (beyond the fp32 range: non-finite, nothing is clamped), "normal" and "none" the spectrogram as it is.
    fp32 [B,2,T,161] -> a new tensor of that shape.  GPU only, no host synchronisation."""
    return _compand(spec, L.DECOMPRESS_MODE[L.feat_type_of(feat_type)], "decompress")


_LABEL_PLANS = OrderedDict()     # (device, B, L, reflect_own, feat_type) -> (context, plan, front end) of label_spec; a few geometries


def label_spec(noisy, clean, lens=None, reflect_own=False, feat_type="sqrt"):
    """The label of a validation batch, on the device: noisy, clean fp32 [B,L] (zero-padded utterance pairs), lens the
    utterances' own lengths (host integers; None: every utterance spans L) -> (label [B,2,T,161], c [B]).  Collate.collate_fn
    (utils/dataset.py:45-74) scales the clean utterance by the NOISY utterance's c and takes the STFT of the padded batch; the
    validation loop compresses it as ``feat_type`` says (trainer/complex_ddpm_trainer.py:414-435; ``compress``).  Here: pdse_pair_prep (csrc/valid.hip), then
    the framing GEMM and the compression of the sampling path's front end on the clean rows.  c is this package's
    sqrt(sum x^2 / len), the divisor (the reference multiplies by its reciprocal).  reflect_own: reflect at every utterance's
    own end, the convention of exact ragged batches.  No host synchronisation; a (B, L) records its small plan once."""
    if noisy.device.type != "cuda":
        raise L.PdseError("label_spec runs on the GPU only (no CPU fallback)")
    if noisy.dim() != 2 or noisy.shape != clean.shape or noisy.dtype != torch.float32 or clean.dtype != torch.float32:
        raise ValueError("noisy, clean: fp32 tensors of one [B,L] shape")
    B, L_ = noisy.shape
    dev = noisy.device
    key = _label_key(dev, B, L_, reflect_own, feat_type)
    hit = _LABEL_PLANS.get(key)
    if hit is None:
        while len(_LABEL_PLANS) >= 3:
            _LABEL_PLANS.popitem(last=False)
        ctx = nets.Ctx(dev)
        st = nets.StftPlan(ctx, B, L_, reflect_own=reflect_own, feat_type=feat_type)
        st.build(prep=False)
        st.finish()
        hit = _LABEL_PLANS[key] = (ctx, st, ctx.alloc(B, L_ + 320))
    else:
        _LABEL_PLANS.move_to_end(key)
    _, st, noisy_pad = hit
    if lens is None:
        st.lens.fill_(L_)
    else:
        lens_t = torch.as_tensor(lens, dtype=torch.int32).reshape(-1)
        if lens_t.numel() != B or int(lens_t.min()) < 161 or int(lens_t.max()) > L_:
            raise ValueError("lens: one length in 161 .. L per utterance")
        st.lens.copy_(lens_t)
    noisy, clean = noisy.contiguous(), clean.contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.pair_prep(noisy.data_ptr(), clean.data_ptr(), st.lens.data_ptr(), noisy_pad.data_ptr(), st.xpad.data_ptr(), st.c.data_ptr(),
                B, L_, 160, 1 if reflect_own else 0, stream, device=dev)
    st.plan.run(stream)
    return st.feat.clone(), st.c.clone()


def _label_key(dev, B, L_, reflect_own, feat_type):
    """The key of a label_spec plan in _LABEL_PLANS: two compressions never share a recorded plan."""
    return (str(dev), B, L_, bool(reflect_own), L.feat_type_of(feat_type))


_FRAME_TABLES = {}      # device -> (basis [322, 320] float64, win2 [320] fp32) of spec_to_wav and the label leg


def frame_tables(device):
    """The constant tables of the scored waveforms, uploaded once per device: the double inverse-DFT basis of pdse_spec_frames
    (row k = ri * 161 + f, window and 1 / n_fft folded in) and the squared window the overlap-add divides by."""
    import numpy as np

    from . import packing as P

    key = str(torch.device(device))
    if key not in _FRAME_TABLES:
        k = P.istft_kmat(320)
        basis = torch.from_numpy(np.ascontiguousarray(np.concatenate([k[0::2], k[1::2]]), dtype=np.float64)).to(device)
        win2 = torch.from_numpy((P.hann_periodic(320) ** 2).astype(np.float32)).to(device)
        _FRAME_TABLES[key] = (basis, win2)
    return _FRAME_TABLES[key]


def spec_to_wav(spec, feat_type="sqrt"):
    """Compressed spectrogram fp32 [B,2,T,161] -> waveforms [B, (T - 1) * 160] in the normalised domain, as the quality measures
    compare them (utils/metrics.py:531-561: magnitude squared with the phase kept, torch.istft): pdse_spec_frames - decompression
    and windowed inverse DFT in double, frames rounded to fp32 once (csrc/valid.hip) - then the path's overlap-add operator without
    the rescale by c.  feat_type: the decompression, as in ``decompress`` (utils/metrics.py:534-551; pdse_spec_frames_mode for a
    value other than "sqrt").  The waveforms of a validation pass (``SamplerPipeline(label=True)``) are made the same way.  No host
    synchronisation."""
    mode = L.DECOMPRESS_MODE[L.feat_type_of(feat_type)]
    if spec.device.type != "cuda":
        raise L.PdseError("spec_to_wav runs on the GPU only (no CPU fallback)")
    if spec.dim() != 4 or spec.shape[1] != 2 or spec.shape[3] != nets.F0 or spec.dtype != torch.float32 or spec.shape[2] < 2:
        raise ValueError("spec: an fp32 [B,2,T,161] tensor with T >= 2")
    spec = spec.contiguous()
    B, _, T, _ = spec.shape
    dev, L_ = spec.device, (T - 1) * 160
    basis, win2 = frame_tables(dev)
    frames = torch.empty(B, 320, T, dtype=torch.float32, device=dev)
    wav = torch.empty(B, L_, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if mode == L.COMPAND_SQUARE:
        L.spec_frames(spec.data_ptr(), basis.data_ptr(), frames.data_ptr(), B, T, nets.F0, stream, device=dev)
    else:
        L.spec_frames_mode(spec.data_ptr(), basis.data_ptr(), frames.data_ptr(), B, T, nets.F0, mode, stream, device=dev)
    o = L.OlaDesc()
    o.frames, o.win2, o.c, o.out = frames.data_ptr(), win2.data_ptr(), 0, wav.data_ptr()
    o.B, o.T, o.L, o.n_fft, o.hop = B, T, L_, 320, 160
    L.launch(o, stream, device=dev)
    return wav
