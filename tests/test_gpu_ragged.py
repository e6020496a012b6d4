"""GPU: exact ragged batches - every utterance of a zero-padded batch must come out as if it had been enhanced alone
(``SamplerPipeline(ragged=True)``, ``ComplexDDPMTrainer.enhance_batch(exact=True)``, ``generate_wav(batch=N)``).

Lengths (16000, 10080, 10240, 7300, 3333): no padding; T_b = 64 on a 32-frame tile edge; 65 one past it; 46 mid-tile; 21 with 80
padding frames - more than the 64-frame margin of the TCM bottleneck tensor and than 2 x 32, the reach of the widest dilation.
Trainers are built with ``exclusive=False``: the small-batch persistent LSTM is another kernel, 1e-5 from the one batches take.
Bit equality is asked wherever the same kernels run on both sides; the oracle comparisons (oracle/restate.py on each utterance
alone, independent of this code) use the suite's 1e-4 rel-L2 - without the masks the oracle puts these cases at 7e-2 .. 1.5e-1."""
import argparse
import os
import wave

import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS = (16000, 10080, 10240, 7300, 3333)
TOL = 1e-4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _trainer(weights, prior="GCRN", sigma=False, out="y", **kw):
    ns = argparse.Namespace
    kw.setdefault("exclusive", False)
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=sigma, checkpoint="x", generated_wav=out),
        ns(model=ns(name=prior), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=weights(prior), ddpm_state_dict=weights("DiffUNet1"), **kw)


@pytest.fixture(scope="module")
def inputs():
    """Per-utterance waveforms (speech-like, different scales) and x_T at each utterance's own shape; never modified."""
    synth = pkg("synth")
    wavs = [torch.from_numpy(np.ascontiguousarray(synth.speechlike(1, n, 300 + i)[0])) * (0.5 + i) for i, n in enumerate(LENS)]
    g = torch.Generator().manual_seed(77)
    x_Ts = [torch.randn(2, 1 + n // 160, 161, generator=g, dtype=torch.float32) for n in LENS]
    return wavs, x_Ts


def _alone(tr, wavs, x_Ts):
    """Every utterance through the B = 1 path: [(wav [len], spec [2, T_b, 161])]."""
    out = []
    for w, x in zip(wavs, x_Ts):
        y = tr.enhance(w[None].to(DEV), x_T=x[None].to(DEV))[0].clone()
        out.append((y, tr._pipes[next(reversed(tr._pipes))].spec[0].clone()))
    return out


def _ragged_spec(tr):
    """The spectrogram of the last ragged pass as ``SamplerPipeline.enhance`` hands it out (frames behind T_b zeroed)."""
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert pipe.ragged
    spec = pipe.spec.clone()
    dead = torch.arange(pipe.T, device=DEV)[None, :] >= pipe.frames_tab[:, None]
    return spec.masked_fill_(dead[:, None, :, None], 0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# whole path, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", ("f16x2", "bf16x3", "fp32"))
def test_whole_path_bit_identical_to_each_utterance_alone(L, weights, inputs, arith, monkeypatch):
    wavs, x_Ts = inputs
    if arith == "fp32":     # the exact fp32 MFMA kernels (csrc/tcm.hip's block among them) on the 6-step schedule
        pl = pkg("pipeline")
        real = pl.SamplerPipeline

        def fp32_pipeline(*a, **kw):
            kw["split_bf16"] = False
            return real(*a, **kw)

        monkeypatch.setattr(pkg("trainer"), "SamplerPipeline", fp32_pipeline)
        tr = _trainer(weights)
    else:
        tr = _trainer(weights, split=arith)
    alone = _alone(tr, wavs, x_Ts)
    got = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert pipe.ragged and pipe.split_bf16 == (arith != "fp32") and (arith == "fp32" or pipe.split == arith)
    spec = _ragged_spec(tr)
    for b, n in enumerate(LENS):
        Tb = 1 + n // 160
        assert got[b].shape == (n,)
        print(arith, n, "max |d wav|", float((got[b] - alone[b][0]).abs().max()), "max |d spec|", float((spec[b, :, :Tb] - alone[b][1]).abs().max()))
    for b, n in enumerate(LENS):
        Tb = 1 + n // 160
        assert torch.equal(got[b], alone[b][0]), (arith, n)
        assert torch.equal(spec[b, :, :Tb], alone[b][1]), (arith, n)
        assert not spec[b, :, Tb:].any()
    # the returned tensors of the pipeline itself: zeros behind an utterance's own samples and frames
    batch = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True).to(DEV)
    xp = torch.zeros(len(LENS), 2, pipe.T, 161, device=DEV)
    for b, x in enumerate(x_Ts):
        xp[b, :, :x.shape[1]] = x.to(DEV)
    w2, s2 = pipe.enhance(batch, xp, lens=list(LENS), exact=True)
    pipe.check()
    for b, n in enumerate(LENS):
        assert torch.equal(w2[b, :n], alone[b][0]) and not w2[b, n:].any() and not s2[b, :, 1 + n // 160:].any()
    assert torch.isfinite(pipe.eps.tcm_a).all() and torch.isfinite(pipe.eps.out).all()


# ---------------------------------------------------------------------------------------------------------------------------
# against the oracle, independent of this code
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prior,sigma", (("GCRN", False), ("DiffUNet", False), ("GCRN", True)))
def test_each_utterance_against_the_oracle_alone(L, weights, inputs, prior, sigma):
    from oracle import restate as R

    params = pkg("params").params
    wavs, x_Ts = inputs
    tr = _trainer(weights, prior=prior, sigma=sigma)
    got = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)
    spec = _ragged_spec(tr)
    errs = []
    for b, n in enumerate(LENS):
        with torch.no_grad():
            ref_wav, ref_spec = R.enhance(prior, weights(prior), weights("DiffUNet1"), wavs[b][None], x_Ts[b][None],
                                          params.noise_schedule, params.inference_noise_schedule, True, sigma)
        Tb = 1 + n // 160
        errs.append((rel_l2(got[b].cpu().numpy(), ref_wav[0].numpy()), rel_l2(spec[b, :, :Tb].cpu().numpy(), ref_spec[0].numpy())))
        print(prior, sigma, n, "rel-L2 wav %.3e spec %.3e" % errs[-1])
    for (ew, es), n in zip(errs, LENS):
        assert ew < TOL and es < TOL, (prior, sigma, n, ew, es)


# ---------------------------------------------------------------------------------------------------------------------------
# stale state: the plan's buffers outlive a pass
# ---------------------------------------------------------------------------------------------------------------------------
def test_second_pass_with_permuted_lengths_and_graph_replay(L, weights, inputs):
    wavs, x_Ts = inputs
    tr = _trainer(weights)
    alone = _alone(tr, wavs, x_Ts)
    perm = [4, 3, 2, 1, 0]            # the shortest utterance sits where the longest was
    first = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert not pipe.plan.has_graph
    second = tr.enhance_batch([wavs[i] for i in perm], x_T=[x_Ts[i] for i in perm], exact=True)
    assert tr._pipes[next(reversed(tr._pipes))] is pipe and pipe.plan.has_graph          # same plan, now captured
    third = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)                                  # a replay, lengths changed again
    for b in range(len(LENS)):
        assert torch.equal(first[b], alone[b][0]), b
        assert torch.equal(second[b], alone[perm[b]][0]), b
        assert torch.equal(third[b], alone[b][0]), b


# ---------------------------------------------------------------------------------------------------------------------------
# kernel level: the TCM forms
# ---------------------------------------------------------------------------------------------------------------------------
KB, KT, KFR = 2, 96, (96, 40)
P1, P2, P3 = "TCMs.0.residual1", "TCMs.0.residual2", "TCMs.0.residual3"


def _net(weights, B, T, frames=None, **kw):
    nets = pkg("nets")
    ctx = nets.Ctx(DEV)
    tab = None if frames is None else torch.tensor(frames, dtype=torch.int32, device=DEV)
    net = nets.EpsNetPlan(ctx, weights("DiffUNet1"), B, T, frames=tab, **kw)
    net._keep_tab = tab
    return net


def _hs(net, fill):
    P = pkg("packing")
    hs = torch.zeros(*P.tcm2_hs_shape(net.B, net.T, net.tcm_planes), dtype=torch.int16, device=DEV)
    hs[..., 64:64 + net.T, :] = fill            # the margins stay zero, every frame starts out non-zero
    return hs


def _hs_frames(hs, b, lo, hi):
    return hs[b][..., 64 + lo:64 + hi, :]


def _launch(L, net, n0):
    for d, _ in net.descs[n0:]:
        L.launch(d)
    torch.cuda.synchronize()


def _tcm2_run(L, net, x, dil, mode, stack=False):
    """mode 1: hs_out of the first block's conv1; mode 0: conv1, then one residual block (or, ``stack``, two as one launch).
    Returns (x_out or None, the hs buffer the last launch wrote, the other one)."""
    hs0, hs1 = _hs(net, 0x1234), _hs(net, 0x1234)
    n0 = len(net.descs)
    net._tcm_stack = None
    net._residual_split(None, 1, x, None, None, hs0, P1, mode=1)
    if mode == 1:
        _launch(L, net, n0)
        return None, hs0, hs1
    xa, xb = torch.empty_like(x), torch.empty_like(x)
    if not stack:
        net._residual_split(P1, dil, x, xa, hs0, hs1, P2)
        _launch(L, net, n0)
        return xa, hs1, hs0
    net._tcm_stack = []
    net._residual_split(P1, 1, x, xa, hs0, hs1, P2)
    net._residual_split(P2, 32, xa, xb, hs1, hs0, P3)
    sd_ = L.Tcm2sDesc()
    for n, blk in enumerate(net._tcm_stack):
        sd_.blk[n] = blk
    sd_.n = 2
    sd_.flags, sd_.status = net.tcm_flags.data_ptr(), net.tcm_status.data_ptr()
    net._tcm_stack = None
    net.add(sd_)
    _launch(L, net, n0)
    assert int(net.tcm_status[0].item()) == 0
    return xb, hs0, hs1


@pytest.fixture(scope="module")
def tcm_x():
    g = torch.Generator().manual_seed(5)
    return torch.randn(KB, 256, KT, generator=g, dtype=torch.float32).to(DEV)


@pytest.mark.parametrize("np_", (1, 2, 3))
@pytest.mark.parametrize("form", ("mode1", "dil1", "dil32", "stack"))
def test_tcm2_zeroes_hs_behind_the_own_frames_and_matches_the_truncated_launch(L, weights, tcm_x, np_, form):
    mode = 1 if form == "mode1" else 0
    dil = 32 if form == "dil32" else 1
    run = lambda net, x: _tcm2_run(L, net, x, dil, mode, stack=form == "stack")   # noqa: E731
    x_out, hs_w, _ = run(_net(weights, KB, KT, frames=KFR, planes=np_), tcm_x)
    for b, Tb in enumerate(KFR):
        assert not _hs_frames(hs_w, b, Tb, KT).any(), (b, "hs_out behind the own frames must be stored as zeros")
        assert not hs_w[b][..., :64, :].any() and not hs_w[b][..., 64 + KT:, :].any()       # margins untouched
        if Tb:
            assert _hs_frames(hs_w, b, 0, Tb).any()
        xt = tcm_x[b:b + 1, :, :Tb].contiguous()
        x_ref, hs_ref, _ = run(_net(weights, 1, Tb, planes=np_), xt)                        # the dense launch on the utterance alone
        assert torch.equal(_hs_frames(hs_w, b, 0, Tb), _hs_frames(hs_ref, 0, 0, Tb)), (form, np_, b)
        if x_out is not None:
            assert torch.equal(x_out[b, :, :Tb], x_ref[0]), (form, np_, b)


@pytest.mark.parametrize("dil", (1, 32))
def test_tcm_f32_reads_zero_padding_at_the_own_end(L, weights, tcm_x, dil):
    def run(net, x):
        n0 = len(net.descs)
        h, h2, xo = torch.empty(net.B, 64, net.T, device=DEV), torch.empty(net.B, 64, net.T, device=DEV), torch.empty_like(x)
        net._tcm_conv1(P1, x, h)
        net._residual_fused(P1, dil, x, xo, h, h2, P2)
        _launch(L, net, n0)
        return xo, h2

    xo, h2 = run(_net(weights, KB, KT, frames=KFR, split_bf16=False), tcm_x)
    for b, Tb in enumerate(KFR):
        x_ref, h_ref = run(_net(weights, 1, Tb, split_bf16=False), tcm_x[b:b + 1, :, :Tb].contiguous())
        assert torch.equal(xo[b, :, :Tb], x_ref[0]) and torch.equal(h2[b, :, :Tb], h_ref[0]), (dil, b)
    # and the table is what makes the difference: the dense launch lets frames 40.. of utterance 1 reach its own
    xd, _ = run(_net(weights, KB, KT, split_bf16=False), tcm_x)
    assert torch.equal(xd[0], xo[0]) and not torch.equal(xd[1, :, :KFR[1]], xo[1, :, :KFR[1]])


# ---------------------------------------------------------------------------------------------------------------------------
# wavprep, overlap-add, sigma: each against its own dense launch per utterance
# ---------------------------------------------------------------------------------------------------------------------------
def test_wavprep_ola_sigma_equal_their_dense_launch_per_utterance(L, inputs):
    wavs, _ = inputs
    B, Lm = len(LENS), max(LENS)
    T = 1 + Lm // 160
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    frames = 1 + lens // 160
    g = torch.Generator().manual_seed(9)
    # ---- wavprep
    wav = torch.nn.utils.rnn.pad_sequence(wavs, batch_first=True).to(DEV)
    xpad, c = torch.full((B, Lm + 320), 7.0, device=DEV), torch.zeros(B, device=DEV)
    d = L.WavprepDesc()
    d.wav, d.xpad, d.c, d.lens = wav.data_ptr(), xpad.data_ptr(), c.data_ptr(), lens.data_ptr()
    d.B, d.L, d.pad, d.normalize, d.reflect_own = B, Lm, 160, 1, 1
    L.launch(d)
    # ---- overlap-add
    fr = torch.randn(B, 320, T, generator=g).to(DEV)
    win2 = torch.from_numpy(pkg("packing").hann_periodic(320).astype(np.float32) ** 2).to(DEV)
    out = torch.full((B, Lm), 7.0, device=DEV)
    o = L.OlaDesc()
    o.frames, o.win2, o.c, o.out = fr.data_ptr(), win2.data_ptr(), c.data_ptr(), out.data_ptr()
    o.B, o.T, o.L, o.n_fft, o.hop = B, T, Lm, 320, 160
    o.nframes, o.lens = frames.data_ptr(), lens.data_ptr()
    L.launch(o)
    # ---- sigma
    init, a = torch.randn(B, 2, T, 161, generator=g).to(DEV), torch.randn(B, 2, T, 161, generator=g).to(DEV)
    init[:, :, -1, 3] = 50.0          # the largest magnitude of every padded plane lies in its padding (none for the full-length one)
    sg, mx = torch.zeros_like(a), torch.zeros(2 * B, device=DEV)
    valid = torch.repeat_interleave(frames * 161, 2).to(torch.int32)
    s = L.SigmaDesc()
    s.init, s.a, s.out, s.maxbuf, s.plane, s.nplanes, s.valid = init.data_ptr(), a.data_ptr(), sg.data_ptr(), mx.data_ptr(), T * 161, 2 * B, valid.data_ptr()
    L.launch(s)
    torch.cuda.synchronize()
    for b, n in enumerate(LENS):
        Tb = 1 + n // 160
        w1 = wavs[b][None].to(DEV).contiguous()
        xp1, c1 = torch.zeros(1, n + 320, device=DEV), torch.zeros(1, device=DEV)
        d1 = L.WavprepDesc()
        d1.wav, d1.xpad, d1.c = w1.data_ptr(), xp1.data_ptr(), c1.data_ptr()
        d1.B, d1.L, d1.pad, d1.normalize = 1, n, 160, 1
        L.launch(d1)
        f1 = fr[b:b + 1, :, :Tb].contiguous()
        o1t = torch.zeros(1, n, device=DEV)
        o1 = L.OlaDesc()
        o1.frames, o1.win2, o1.c, o1.out = f1.data_ptr(), win2.data_ptr(), c1.data_ptr(), o1t.data_ptr()
        o1.B, o1.T, o1.L, o1.n_fft, o1.hop = 1, Tb, n, 320, 160
        L.launch(o1)
        i1, a1 = init[b:b + 1, :, :Tb].contiguous(), a[b:b + 1, :, :Tb].contiguous()
        s1t, m1 = torch.zeros_like(a1), torch.zeros(2, device=DEV)
        s1 = L.SigmaDesc()
        s1.init, s1.a, s1.out, s1.maxbuf, s1.plane, s1.nplanes = i1.data_ptr(), a1.data_ptr(), s1t.data_ptr(), m1.data_ptr(), Tb * 161, 2
        L.launch(s1)
        torch.cuda.synchronize()
        assert torch.equal(c[b:b + 1], c1)
        assert torch.equal(xpad[b, :n + 320], xp1[0]) and not xpad[b, n + 320:].any(), n
        assert torch.equal(out[b, :n], o1t[0]) and not out[b, n:].any(), n
        assert torch.equal(sg[b, :, :Tb], s1t[0]) and torch.equal(sg[b, :, Tb:], a[b, :, Tb:]), n
        assert torch.equal(mx[2 * b:2 * b + 2], m1)


# ---------------------------------------------------------------------------------------------------------------------------
# the file loop
# ---------------------------------------------------------------------------------------------------------------------------
def _write_wav(path, x, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_generate_wav_batched_writes_the_same_bytes(L, weights, tmp_path, caplog):
    synth = pkg("synth")
    src = tmp_path / "in"
    src.mkdir()
    for i, (n, rate) in enumerate(((4000, 16000), (2900, 16000), (9000, 48000), (4000, 16000), (1777, 16000), (5300, 16000))):
        _write_wav(src / ("f%d.wav" % i), 0.5 * synth.speechlike(1, n, 60 + i)[0], rate)
    (src / "f2b.wav").write_bytes(b"RIFF\x04\x00\x00\x00WAVE")                # unreadable: skipped by both loops
    outs = []
    for batch in (1, 4):
        tr = _trainer(weights, out=str(tmp_path / ("out%d" % batch)))
        torch.manual_seed(4321)
        with caplog.at_level("WARNING"):
            caplog.clear()
            written = tr.generate_wav(load_pre_train=False, data_path=str(src), batch=batch)
            assert sum("skipping" in r.getMessage() and "f2b.wav" in r.getMessage() for r in caplog.records) == 1
        assert [os.path.basename(w) for w in written] == ["f%d.wav" % i for i in range(6)]
        outs.append(written)
    for one, four in zip(*outs):
        with open(one, "rb") as f1, open(four, "rb") as f4:
            assert f1.read() == f4.read(), os.path.basename(one)


# ---------------------------------------------------------------------------------------------------------------------------
# refusals, and the convention that did not change
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_unchanged_validation_convention(L, weights, inputs):
    wavs, x_Ts = inputs
    tr = _trainer(weights, prior="aia_complex_trans_ri")
    with pytest.raises(ValueError, match="bidirectional GRU"):
        tr.enhance_batch([w[:3000] for w in wavs[:2]], exact=True)
    with pytest.raises(ValueError, match="bidirectional GRU"):
        tr.generate_wav(load_pre_train=False, data_path="nowhere", batch=2)
    tr = _trainer(weights)
    short = [w[:n] for w, n in zip(wavs[:3], (4000, 2500, 3300))]
    x_T = torch.randn(3, 2, 26, 161, generator=torch.Generator().manual_seed(3))
    # exact=False is the default and still the padded pass: the dense pipeline with the lengths as RMS lengths only
    a = tr.enhance_batch(short, x_T=x_T)
    b = tr.enhance_batch(short, x_T=x_T, exact=False)
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert not pipe.ragged and len(tr._pipes) == 1
    batch = torch.nn.utils.rnn.pad_sequence(short, batch_first=True).to(DEV)
    want = pipe.enhance(batch, x_T.to(DEV), lens=[4000, 2500, 3300])[0]
    for i, n in enumerate((4000, 2500, 3300)):
        assert torch.equal(a[i], b[i]) and torch.equal(a[i], want[i, :n])
    e = tr.enhance_batch(short, x_T=x_T, exact=True)
    assert not torch.equal(e[1], a[1])                   # a padded utterance differs between the two conventions
    with pytest.raises(ValueError, match="ragged=True"):
        pipe.enhance(batch, x_T.to(DEV), lens=[4000, 2500, 3300], exact=True)
    with pytest.raises(ValueError):
        tr.enhance_batch(short, x_T=[x_T[0]] * 3, exact=True)          # per-utterance x_T of the wrong frame count
