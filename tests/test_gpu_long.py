"""GPU: recordings of any length through one window plan - the windowed pass against the whole-file pass of an
``exclusive=False`` trainer, the LSTM's carried state, and the gather / scatter kernels of csrc/window.hip."""
import argparse
import ctypes as C_

import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H_LEFT, H_RIGHT = 388, 378                 # tests/test_long_host.py holds the builders' own figure against the oracle
W = -(-(H_LEFT + H_RIGHT + 64) // 32) * 32  # 832


def _trainer(weights, tmp_path_factory, prior="GCRN", sigma=False, **kw):
    tmp = tmp_path_factory.mktemp("long")
    args = argparse.Namespace(retrain=False, joint=True, draw=False, sigma=sigma, checkpoint=str(tmp / "ck"), generated_wav=str(tmp / "out"))
    config = argparse.Namespace(model=argparse.Namespace(name=prior),
                                train=argparse.Namespace(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt", batch_size=2))
    return pkg("trainer").ComplexDDPMTrainer(args, config, device=DEV, prior_state_dict=weights(prior),
                                             ddpm_state_dict=weights("DiffUNet1"), exclusive=False, **kw)


_TRAINERS = {}


@pytest.fixture(scope="module")
def trainers(weights, tmp_path_factory):
    def get(prior, sigma=False):
        if (prior, sigma) not in _TRAINERS:
            _TRAINERS[(prior, sigma)] = _trainer(weights, tmp_path_factory, prior, sigma)
        return _TRAINERS[(prior, sigma)]

    yield get
    _TRAINERS.clear()


def _pair(tr, B, T, seed):
    """(whole-file (wav, spec), windowed (wav, spec)) of one seeded batch of T frames, on the same trainer and weights."""
    L_ = (T - 1) * 160
    wav, x_T = pkg("synth").synthetic_waveforms(B, L_, seed=seed)
    wav, x_T = wav.to(DEV), x_T.to(DEV)
    assert tr._long_sampler(B, W)[0].eps_field == (H_LEFT, H_RIGHT)
    with torch.no_grad():
        pipe = tr._plan(B=B, L_=L_)[0]
        whole = pipe.enhance(wav, x_T)
        pipe.check()
        xinit = pipe.prior.out.clone()
        long = tr._long_sampler(B, W)[0]
        windowed = long.enhance(wav, x_T)
        long.check()
    del tr._pipes[tr._key(B=B, L_=L_)]       # the whole-file activation set of this length is not needed again
    return whole, windowed, long, xinit


@pytest.mark.parametrize("prior,B,T,sigma", [("GCRN", 1, 2 * W + 37, False), ("GCRN", 1, W + 1, False), ("GCRN", 2, W + 1, True),
                                             ("DiffUNet", 1, 2 * W + 37, False)],
                         ids=["gcrn_B1_2W37", "gcrn_B1_W1", "gcrn_B2_W1_sigma", "diffunet_B1_2W37"])
def test_windowed_pass_is_the_whole_file_pass(trainers, prior, B, T, sigma):
    """Six fast steps; W = H_left + H_right + 64 rounded up to the frame tile; T = 2 W + 37: a first window, middle windows and a
    clamped, overlapping last one.  Every kept frame sees its full receptive field (or the file's own edge).

    The GCRN prior's X_init is held to ``torch.equal``: its convolutions are per frame and the LSTM's state is carried bit for bit.
    The eps-net (and a DiffUNet prior) is held to the project's parity tolerance, rel-L2 1e-4, not to equal bits: ``tcm2_kernel``
    (csrc/tcm2.hip) walks the five K blocks of its dilated branches in an order rotated by the frame tile index
    (``js = blockIdx.x % 5``), so a frame's summation order depends on which tile of its plan it falls in, and a window that does
    not start at frame 0 shifts the tiles (the encoder in front of it, en5, is bit-identical in every kept frame at every window
    start; the TCM stream behind it differs in the last bits whether or not the start is a multiple of 32).  Measured on an
    MI355X, windowed against whole-file, spectrogram / waveform: GCRN B=1 T=1701 8.9e-07 / 1.1e-06, T=833 7.0e-07 / 8.6e-07,
    B=2 T=833 --sigma 2.4e-07 / 3.7e-07; DiffUNet prior B=1 T=1701 7.1e-06 / 8.4e-06 (``PDSE_MARGINS`` records each run's)."""
    tr = trainers(prior, sigma)
    (wav_a, spec_a), (wav_b, spec_b), long, xinit_a = _pair(tr, B, T, seed=11 + T + B)
    assert len(long.eps_windows) == (2 if T == W + 1 else 2 + -(-(T - 2 * W + H_LEFT + H_RIGHT) // (W - H_LEFT - H_RIGHT)))   # 2 / 15
    assert long.eps_windows[-1][0] == T - W and long.eps_windows[0][0] == 0
    if prior == "GCRN":
        assert len(long.prior_windows) == -(-T // W) and long.prior_windows[-1][0] + W > T      # the last one hangs over the end
        assert torch.equal(long.xinit, xinit_a)
    else:
        assert rel_l2(long.xinit.cpu(), xinit_a.cpu()) < 1e-4
    e_spec, e_wav = rel_l2(spec_b.cpu(), spec_a.cpu()), rel_l2(wav_b.cpu(), wav_a.cpu())
    print("windowed against whole-file: rel-L2 spectrogram %.3e waveform %.3e" % (e_spec, e_wav))
    assert torch.isfinite(spec_b).all() and torch.isfinite(wav_b).all()
    assert e_spec < 1e-4 and e_wav < 1e-4


def test_trainer_enhance_window_and_short_files(trainers):
    """``enhance(window=W)``: a recording that fits the window takes the whole-file plan (no windowed sampler is built); a longer
    one the windowed pass, with one window plan for two different lengths."""
    tr = trainers("GCRN")
    wav, x_T = pkg("synth").synthetic_waveforms(1, 16 * 160, seed=3)
    n = len(tr._long)
    short = tr.enhance(wav.to(DEV), x_T.to(DEV), window=W)
    assert len(tr._long) == n and torch.equal(short, tr.enhance(wav.to(DEV), x_T.to(DEV)))
    outs = []
    for T in (W + 1, W + 3):
        wav, x_T = pkg("synth").synthetic_waveforms(1, (T - 1) * 160, seed=4)
        outs.append(tr.enhance(wav.to(DEV), x_T.to(DEV), window=W))
        assert outs[-1].shape == (1, (T - 1) * 160) and torch.isfinite(outs[-1]).all()
    assert len([k for k in tr._long if k[1] == 1 and k[2] == W]) == 1
    win, whole = tr._long_sampler(1, W)[0].activation_bytes()
    assert win > 4 * whole > 0


def test_rejected_combinations_raise(trainers, weights, tmp_path_factory):
    tr = trainers("GCRN")
    wav = torch.randn(1, 2560, generator=torch.Generator().manual_seed(1)).to(DEV)
    with pytest.raises(ValueError, match="members=2"):
        tr.enhance(wav, members=2, window=W)
    for kw, word in ((dict(batch=2), "ragged"), (dict(inflight=2), "inflight=2"), (dict(members=2), "members=2")):
        with pytest.raises(ValueError, match=word):
            tr.generate_wav(load_pre_train=False, data_path="/nonexistent", window=W, **kw)
    with pytest.raises(ValueError, match="multiple of 32"):
        tr.enhance(wav, window=100)
    with pytest.raises(ValueError, match="per_channel"):
        _trainer(weights, tmp_path_factory, channels="each", window=W)
    with pytest.raises(ValueError, match="audit"):
        _trainer(weights, tmp_path_factory, audit=True, window=W)
    with pytest.raises(ValueError, match="attends"):
        _trainer(weights, tmp_path_factory, prior="aia_complex_trans_ri", window=W)
    with pytest.raises(ValueError, match="receptive field"):
        pkg("pipeline").LongSampler(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), 1, 736)
    # a trainer built with window=W: the entry points that record whole-file plans refuse instead of ignoring the option
    trw = _trainer(weights, tmp_path_factory, window=W)
    for call in (lambda: trw.sample(torch.zeros(1, 2, 17, 161)), lambda: trw.enhance_members(wav), lambda: trw.enhance_batch([wav[0]]),
                 lambda: trw.validate_batch([wav[0]], [wav[0]]), lambda: trw.objective_batch([wav[0]], [wav[0]]),
                 lambda: trw.enhance_stream([wav])):
        with pytest.raises(ValueError, match="built with window=%d" % W):
            call()
    assert torch.isfinite(trw.enhance(wav)).all()                      # a recording that fits the window: today's path
    # a pipeline built for more frames than its window holds no whole-file plan: its other entry points say so
    T = W + 1
    lp = pkg("pipeline").SamplerPipeline(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), 1, L_=(T - 1) * 160, window=W, bank=tr.bank)
    assert lp.long is not None
    for call in (lambda: lp.run(), lambda: lp.sample(None, None), lambda: lp.range_report()):
        with pytest.raises(ValueError, match="no whole-file plan"):
            call()
    wl, xl = pkg("synth").synthetic_waveforms(1, (T - 1) * 160, seed=2)
    out, spec = lp.enhance(wl.to(DEV), xl.to(DEV))
    lp.check()
    assert out.shape == (1, (T - 1) * 160) and spec.shape == (1, 2, T, 161)
    pipe = pkg("pipeline").SamplerPipeline("cpu", "GCRN", weights("GCRN"), weights("DiffUNet1"), 1, L_=2560, window=32)
    with pytest.raises(ValueError, match="window=32"):
        pkg("planfile").save_pipeline("/nonexistent/plan.bin", pipe)


# ---- csrc/window.hip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0, "end", 7, -5, "over"], ids=["a0", "aT-W", "a7", "before", "over"])
def test_gather_scatter_round_trip(a):
    L = pkg("_lib")
    B, Cn, T, F, Wn = 2, 2, 97, 161, 32
    a = {"end": T - Wn, "over": T - 9}.get(a, a)
    g = torch.Generator().manual_seed(9)
    whole = torch.randn(B, Cn, T, F, generator=g).to(DEV)
    win = torch.full((B, Cn, Wn, F), float("nan"), device=DEV)
    L.window_gather(whole.data_ptr(), win.data_ptr(), B, Cn, T, F, Wn, a, device=DEV)
    want = torch.zeros(B, Cn, Wn, F, device=DEV)
    lo, hi = max(a, 0), min(a + Wn, T)
    want[:, :, lo - a:hi - a] = whole[:, :, lo:hi]
    assert torch.equal(win, want)
    SENT = -12345.0
    dst = torch.full((B, Cn, T, F), SENT, device=DEV)
    klo, khi = lo + 3, hi - 2
    L.window_scatter(win.data_ptr(), dst.data_ptr(), B, Cn, T, F, Wn, a, klo, khi, device=DEV)
    want = torch.full((B, Cn, T, F), SENT, device=DEV)
    want[:, :, klo:khi] = whole[:, :, klo:khi]
    assert torch.equal(dst, want)
    L.window_scatter(win.data_ptr(), dst.data_ptr(), B, Cn, T, F, Wn, a, klo, klo, device=DEV)     # nothing kept: nothing written
    assert torch.equal(dst, want)
    for bad in ((lo - 1, khi), (klo, hi + 1), (khi, klo)):
        with pytest.raises(L.PdseError, match="kept frames"):
            L.window_scatter(win.data_ptr(), dst.data_ptr(), B, Cn, T, F, Wn, a, bad[0], bad[1], device=DEV)
    with pytest.raises(L.PdseError, match="no frame"):
        L.window_gather(whole.data_ptr(), win.data_ptr(), B, Cn, T, F, Wn, T, device=DEV)
    torch.cuda.synchronize()
    assert torch.equal(dst, want)


# ---- the grouped LSTM's carried state ----------------------------------------------------------------------------------------
def _glstm_run(L, base, gx_full, frames, state_in, state_out, tc=0):
    """One launch of the case's descriptor over ``frames`` of gx_full [G, T, Bp, 4H]; returns y [B, n, 1024] (cat layout)."""
    t0, t1 = frames
    n = t1 - t0
    d = L.GlstmDesc.from_buffer_copy(base.desc)
    gx = gx_full[:, t0:t1].contiguous()
    y = torch.full((d.B, n, 1024), float("nan"), device=DEV)
    R = 2 * tc if tc else 2
    scr = {k: torch.full((sz,), float("nan"), device=DEV) for k, sz in (("hT1", R * 2 * 512 * d.Bp), ("gx2", R * 2 * 2048 * d.Bp),
                                                                       ("part", R * 2 * 64 * d.Bp * 2))}
    d.hT1, d.gx2, d.part = (scr[k].data_ptr() for k in ("hT1", "gx2", "part"))
    d.gx1, d.y, d.T = gx.data_ptr(), y.data_ptr(), n
    d.y_sb, d.y_st, d.y_su, d.y_sg = n * 1024, 1024, 1, 512
    d.tc, d.lag = (tc, tc + 1) if tc else (0, 0)
    d.state_in = None if state_in is None else state_in.data_ptr()
    d.state_out = None if state_out is None else state_out.data_ptr()
    L.launch(d, device=DEV)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("name,slices,tc", [("glstm_s2_B33_T7_n01_cat", 2, 0), ("glstm_s2_B33_T7_n01_cat", 1, 0),
                                            ("glstm_s2_B1_T7_offset_il", 1, 2)], ids=["B33_s2", "B33_s1", "B1_chunked"])
def test_lstm_state_split_equals_one_call(name, slices, tc):
    """T = 7 split 3 + 4: two calls with state_out -> state_in equal one call, bit for bit; a NULL state_in equals the kernel
    without the fields, and so does a state of zeros."""
    from helpers import lstm_cases as Cs

    L = pkg("_lib")
    case = Cs.variant(Cs.find(name), slices=slices)
    base = Cs.build(case, DEV)
    assert base.desc.state_in is None and base.desc.state_out is None
    d = base.desc
    gx_full = torch.zeros(2, 7, d.Bp, 2048)
    gx_full[:, :, :d.B] = Cs.projections(case).permute(0, 2, 1, 3)
    gx_full = gx_full.to(DEV)
    one = _glstm_run(L, base, gx_full, (0, 7), None, None, tc)
    ref = Cs.ref(case, torch.float64)                                                 # [G, B, T, H]
    assert rel_l2(one.cpu().reshape(d.B, 7, 2, 512).permute(2, 0, 1, 3), ref) < 1e-4  # the launch is the operator the suite knows
    mk = lambda fill: torch.full((4, 2, 512, d.Bp), fill, device=DEV)                 # noqa: E731
    s0, s1, s2 = mk(0.0), mk(float("nan")), mk(float("nan"))
    assert torch.equal(_glstm_run(L, base, gx_full, (0, 7), s0, s1, tc), one)         # zeros in: the NULL launch's bits
    assert torch.isfinite(s1).all()
    first = _glstm_run(L, base, gx_full, (0, 3), None, s2, tc)
    assert torch.isfinite(s2).all()
    s3 = mk(float("nan"))
    second = _glstm_run(L, base, gx_full, (3, 7), s2, s3, tc)
    assert torch.equal(torch.cat([first, second], 1), one)
    assert torch.equal(s3, s1)                                                        # the state after frame 6, either way
    with pytest.raises(L.PdseError, match="state_in and state_out"):
        _glstm_run(L, base, gx_full, (0, 3), s2, s2, tc)
