"""GPU: the spectral compression modes (``feat_type``: sqrt, normal, cubic, log_1x, none) - the compand operator's modes
(csrc/misc.hip), pdse_spec_frames_mode (csrc/valid.hip), ops.compress / ops.decompress / ops.spec_to_wav / ops.label_spec and a
ComplexDDPMTrainer whose configuration names another mode than "sqrt".

Tolerance of the operators.  tests/golden/feat_type.npz holds what the reference's own fp32 statements give on the CPU;
tools/make_golden_feattype.py measured their distance from the float64 restatement of tests/helpers/feat_refs.py and wrote it
to profiles/feat_type_parity.txt:

    transform                rel-L2      max-abs bound rel-L2 bound max-abs
    compress normal       6.200e-08    2.623e-06    1.240e-07    5.245e-06
    decompress normal     0.000e+00    0.000e+00    0.000e+00    0.000e+00
    compress cubic        6.440e-08    2.425e-07    1.288e-07    4.851e-07
    decompress cubic      2.261e-07    1.985e-02    4.522e-07    3.970e-02
    compress log_1x       6.831e-08    3.002e-07    1.366e-07    6.004e-07
    decompress log_1x     6.479e-08    9.342e+05    1.296e-07    1.868e+06
    compress none         0.000e+00    0.000e+00    0.000e+00    0.000e+00
    decompress none       0.000e+00    0.000e+00    0.000e+00    0.000e+00

The device gets twice the measured distance against float64 (its powf / logf / expf need not round like torch's CPU ones); the
test computes the distance again from the fixture, so the bound is the table's.  Against the fixture itself the triangle
inequality gives three times the distance.  (max-abs of "decompress log_1x" is 0.9 ulp of exp(30) = 1.07e13, a planted bin.)"""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, pkg, rel_l2, seeded

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import feat_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEW = (("compress", "normal"), ("compress", "cubic"), ("compress", "log_1x"), ("compress", "none"),
       ("decompress", "normal"), ("decompress", "cubic"), ("decompress", "log_1x"), ("decompress", "none"))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


@pytest.fixture(scope="module")
def fixture():
    g = golden("feat_type")
    return {k: g[k] for k in g.files}


def _trainer(weights, feat_type, prior="GCRN", **kw):
    ns = argparse.Namespace
    kw.setdefault("exclusive", False)
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav="y"),
        ns(model=ns(name=prior), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type=feat_type, batch_size=2)),
        device=DEV, prior_state_dict=weights(prior), ddpm_state_dict=weights("DiffUNet1"), **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. operator parity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corner", (False, True), ids=("B2_T9", "B1_T2"))
@pytest.mark.parametrize("kind,mode", NEW)
def test_operator_parity(L, fixture, kind, mode, corner):
    """The eight new transforms on the fixture's input (B = 2, T = 9) and on its [0:1, :, 0:2] corner (B = 1, T = 2), which holds
    every planted bin; bounds: the module docstring, for each shape from the fixture's own distance on that shape."""
    ops = pkg("ops")
    cut = (slice(0, 1), slice(None), slice(0, 2)) if corner else (slice(None),) * 3
    x = np.ascontiguousarray(fixture["input"][cut])
    ref = np.ascontiguousarray(fixture[("comp_" if kind == "compress" else "dec_") + mode][cut])
    want = getattr(R, kind)(x, mode)
    xd = torch.from_numpy(x).to(DEV)
    keep = xd.clone()
    got_t = getattr(ops, kind)(xd, mode)
    assert got_t.shape == xd.shape and got_t.dtype == torch.float32 and got_t.data_ptr() != xd.data_ptr() and torch.equal(xd, keep)
    got = got_t.cpu().numpy()
    rel0, max0 = R.errors(ref, want)
    rel, mx = R.errors(got, want)
    relf, mxf = R.errors(got, ref)
    print(kind, mode, x.shape, "fixture vs f64", rel0, max0, "device vs f64", rel, mx, "device vs fixture", relf, mxf)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    zero = (x[:, 0] == 0) & (x[:, 1] == 0)
    assert zero.sum() >= 4
    assert np.all(got[:, 0][zero] == 0) and np.all(got[:, 1][zero] == 0)          # (f(0), 0), and f(0) = 0 in every mode
    assert rel <= 2 * rel0 and mx <= 2 * max0, (kind, mode, rel, rel0, mx, max0)
    assert relf <= 3 * rel0 and mxf <= 3 * max0, (kind, mode, relf, rel0, mxf, max0)
    if rel0 == 0:                                                              # the copies
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_compress_argument_errors(L):
    ops = pkg("ops")
    with pytest.raises(ValueError, match="fp32"):
        ops.compress(torch.zeros(1, 3, 2, 161, device=DEV), "cubic")
    with pytest.raises(ValueError, match="fp32"):
        ops.decompress(torch.zeros(1, 2, 2, 161, device=DEV, dtype=torch.float64), "cubic")
    with pytest.raises(L.PdseError, match="GPU only"):
        ops.compress(torch.zeros(1, 2, 2, 161), "cubic")
    big = torch.full((1, 2, 1, 161), 80.0, device=DEV)                         # |X| = 113: exp() leaves the fp32 range, nothing is clamped
    assert torch.isinf(ops.decompress(big, "log_1x")).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the scattered layout of the ISTFT GEMM
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.FEAT_TYPES)
def test_istft_plan_scattered_layout(L, fixture, mode):
    """Every decompress mode through an IstftPlan at B = 2, T = 5: its frame-major rows hold ops.decompress bit for bit, the 7 pad
    entries per row stay zero, and the waveform equals ops.decompress followed by the copy-mode plan (GEMM and overlap-add)."""
    nets, ops = pkg("nets"), pkg("ops")
    B, T, L_ = 2, 5, 640
    x = torch.from_numpy(np.ascontiguousarray(fixture["input"][:, :, :T])).to(DEV)
    ctx = nets.Ctx(DEV)
    a = nets.IstftPlan(ctx, B, T, L_, feat_type=mode)
    a.build()
    a.finish()
    b = nets.IstftPlan(ctx, B, T, L_, feat_type="none")
    b.build()
    b.finish()
    dec = ops.decompress(x, mode)
    a.spec.copy_(x)
    b.spec.copy_(dec)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    a.plan.run(stream)
    b.plan.run(stream)
    torch.cuda.synchronize()
    rows = a.dec.view(B, T, 2, 168)
    assert torch.equal(rows[:, :, :, :161], dec.permute(0, 2, 1, 3))
    assert not rows[:, :, :, 161:].any()
    assert torch.equal(a.dec, b.dec) and torch.equal(a.wav, b.wav) and torch.isfinite(a.wav).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the scored waveforms
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("cubic", "log_1x", "normal", "none"))
def test_spec_to_wav_vs_fixture(L, fixture, mode):
    """ops.spec_to_wav(feat_type=...) against the waveforms compare_complex made of the fixture's input (the reference's fp32
    decompression and torch.istft) and against the float64 helper: 3.6e-7 rel-L2, the bound of
    tests/test_gpu_valid.py::test_spec_to_wav_vs_float64_istft for the same comparison in the sqrt mode."""
    ops = pkg("ops")
    x = torch.from_numpy(fixture["input"]).to(DEV)
    got = ops.spec_to_wav(x, feat_type=mode).cpu().numpy()
    ref, want = fixture["wav_" + mode], R.wav_of(fixture["input"], mode)
    assert got.shape == ref.shape == want.shape
    d_ref, d_64 = rel_l2(got, ref), rel_l2(got, want)
    print(mode, "device vs fixture", d_ref, "device vs float64", d_64, "fixture vs float64", rel_l2(ref, want))
    assert d_64 < 3.6e-7
    assert d_ref < 3.6e-7
    if mode == "none":
        assert np.array_equal(got, ops.spec_to_wav(x, feat_type="normal").cpu().numpy())
    one = ops.spec_to_wav(x[1:2, :, :6].contiguous(), feat_type=mode)                  # rows do not depend on B or T
    assert torch.equal(one[0, :640].cpu(), torch.from_numpy(got[1, :640]))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. round trip and a pass assembled by hand
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("none", "normal", "cubic", "log_1x"))
def test_round_trip_and_hand_assembled_pass(L, weights, mode):
    nets, ops, P = pkg("nets"), pkg("ops"), pkg("pipeline").SamplerPipeline
    B, L_ = 2, 3200
    T = 1 + L_ // 160
    wav = torch.from_numpy(np.ascontiguousarray(pkg("synth").speechlike(B, L_, 500))).float() * torch.tensor([[0.3], [2.0]])
    x_T = seeded((B, 2, T, 161), 501).to(DEV)
    wav_d = wav.to(DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    ctx = nets.Ctx(DEV)
    front = nets.StftPlan(ctx, B, L_, split_bf16=True, feat_type="none")        # the raw STFT of wav / c
    front.build()
    front.finish()
    back = nets.IstftPlan(ctx, B, T, L_, split_bf16=True, feat_type="none")     # GEMM + overlap-add + rescale by c
    back.build(c=front.c)
    back.finish()
    front.wav.copy_(wav_d)
    front.plan.run(stream)
    feat = ops.compress(front.feat, mode)
    # ---- first stage: decompress(compress(stft(x))) -> istft gives x back
    back.spec.copy_(ops.decompress(feat, mode))
    back.plan.run(stream)
    torch.cuda.synchronize()
    d = rel_l2(back.wav.cpu(), wav)
    print(mode, "round trip rel-L2", d)
    assert d < 1e-4
    # ---- the trainer's pass against the same pass assembled from the operators
    tr = _trainer(weights, mode)
    got = tr.enhance(wav_d, x_T=x_T).clone()
    pipe = tr._pipe(B, L_=L_)
    assert pipe.feat_type == mode and torch.isfinite(got).all() and torch.isfinite(pipe.spec).all()
    assert torch.equal(pipe.feat, feat)
    hand = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, T=T, fast_sampling=tr.params.fast_sampling, params=tr.params,
             deltamu=tr.deltamu, cond=tr.cond, xT_plus_init=tr.xT_plus_init, dtype=tr.dtype, split=pipe.split, exclusive=False)
    spec, _ = hand.sample(feat, x_T)
    hand.check()
    assert torch.equal(spec, pipe.spec)
    back.spec.copy_(ops.decompress(spec, mode))
    back.plan.run(stream)
    torch.cuda.synchronize()
    assert torch.equal(back.wav, got)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a validation batch in another mode than sqrt
# ---------------------------------------------------------------------------------------------------------------------------
def test_validation_batch_cubic(L, weights):
    """validate_batch on a "cubic" trainer, the comparison of tests/test_gpu_valid.py with its bounds: the label against the
    float64 STFT of clean / c compressed by the helper (2e-6, the front end's bound), com_mse against the float64 sum over the
    device's own spectrograms (2e-6 relative), and SSNR / LLR / WSS / fwSNRseg of the final spectrogram and of X_init against
    tests/emu_metrics.py on the helper's float64 decompression and inverse STFT of those spectrograms (emu_metrics.TOL)."""
    import emu_metrics as E

    lens = (1600, 1121)
    noisy = [seeded((n,), 600 + b) * (0.05 * (b + 1)) for b, n in enumerate(lens)]
    clean = [seeded((n,), 610 + b) * 0.04 for b, n in enumerate(lens)]
    x_T = seeded((2, 2, 11, 161), 620).to(DEV)
    tr = _trainer(weights, "cubic")
    _, scores = tr.validate_batch(noisy, clean, x_T=x_T)
    pipe = tr._pipe(2, L_=1600, label=True)
    frames = [n // 160 + 1 for n in lens]
    assert scores["frames"] == frames and pipe.feat_type == "cubic"
    label, spec, init = pipe.label.spec.cpu().numpy(), pipe.spec.cpu().numpy(), pipe.init_spec.cpu().numpy()
    # label: float64 STFT of clean / c, zero-padded as the batch is
    cpad = torch.zeros(2, 1600, dtype=torch.float64)
    for b, n in enumerate(lens):
        cpad[b, :n] = clean[b].double() / noisy[b].double().pow(2).mean().sqrt()
    st = torch.stft(cpad, 320, 160, 320, torch.hann_window(320, dtype=torch.float64), return_complex=True).permute(0, 2, 1)
    want_label = R.compress(torch.stack((st.real, st.imag), 1).numpy(), "cubic")
    assert rel_l2(label, want_label) < 2e-6
    cut = [(f - 1) * 160 for f in frames]
    ref_wav = R.wav_of(label, "cubic")
    bad = []
    for name, sp in (("x", spec), ("init", init)):
        num = sum(((sp[b, :, :fr].astype(np.float32) - label[b, :, :fr]) ** 2).astype(np.float64).sum() for b, fr in enumerate(frames))
        want = num / (2.0 * sum(frames) * 161)
        got = float(scores[name]["loss"][0])
        print(name, "com_mse", got, want)
        assert abs(got - want) <= 2e-6 * want
        wav = R.wav_of(sp, "cubic")
        for b in range(2):
            emu = E.emulate(ref_wav[b, :cut[b]], wav[b, :cut[b]])
            for k in E.KEYS:
                g_, w_ = float(scores[name][k][b]), emu[k]
                print(name, b, k, g_, w_, abs(g_ - w_), E.TOL[k])
                if not E.same(g_, w_, E.TOL[k]).all():
                    bad.append((name, b, k, g_, w_))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------------
# 6. exact ragged batches inherit the mode
# ---------------------------------------------------------------------------------------------------------------------------
def test_exact_ragged_log_1x(L, weights):
    lens = (1700, 3200)
    synth = pkg("synth")
    wavs = [torch.from_numpy(np.ascontiguousarray(synth.speechlike(1, n, 700 + i)[0])).float() * (0.5 + i) for i, n in enumerate(lens)]
    x_Ts = [seeded((2, 1 + n // 160, 161), 710 + i) for i, n in enumerate(lens)]
    tr = _trainer(weights, "log_1x")
    alone = [tr.enhance(w[None].to(DEV), x_T=x[None].to(DEV))[0].clone() for w, x in zip(wavs, x_Ts)]
    got = tr.enhance_batch(wavs, x_T=x_Ts, exact=True)
    pipe = tr._pipes[next(reversed(tr._pipes))]
    assert pipe.ragged and pipe.feat_type == "log_1x"
    for b, n in enumerate(lens):
        assert got[b].shape == (n,) and torch.isfinite(got[b]).all()
        assert torch.equal(got[b], alone[b]), n


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the default
# ---------------------------------------------------------------------------------------------------------------------------
def test_sqrt_is_untouched(L, weights):
    """A pipeline with feat_type="sqrt" passed explicitly and one without the argument give the same bits, and ops.compress /
    ops.decompress in the sqrt mode are the front and back end's own launches."""
    ops, P = pkg("ops"), pkg("pipeline").SamplerPipeline
    B, L_ = 2, 1600
    wav = (seeded((B, L_), 800) * 0.1).to(DEV)
    x_T = seeded((B, 2, 11, 161), 801).to(DEV)
    out = []
    for kw in (dict(), dict(feat_type="sqrt")):
        p = P(DEV, "GCRN", weights("GCRN"), weights("DiffUNet1"), B, L_=L_, **kw)
        w, s = p.enhance(wav, x_T)
        p.check()
        out.append((w, s, p.feat.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    tr = _trainer(weights, "sqrt")
    assert torch.equal(tr.enhance(wav, x_T=x_T), tr.enhance(wav, x_T=x_T)) and tr.feat_type == "sqrt"
    x = seeded((1, 2, 3, 161), 802).to(DEV)
    m = torch.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2)
    assert rel_l2(ops.decompress(ops.compress(x)).cpu(), x.cpu()) < 1e-6
    assert rel_l2(ops.compress(x).cpu(), (x / m[:, None].sqrt()).cpu()) < 1e-6
