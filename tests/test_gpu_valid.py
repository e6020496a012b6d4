"""GPU: the validation epoch - csrc/valid.hip behind pdse_pair_prep / pdse_spec_losses, the label leg of SamplerPipeline,
ComplexDDPMTrainer.validate and ``main.py --eval``.

Tolerances.  spec_losses against numpy: the fp32 element terms are evaluated by numpy in fp32 exactly as the kernel states them
and added in float64; only the order of the double additions differs, N <= 2 * 33 * 161 terms of one sign, so the relative
distance is bounded by N * 2^-53 ~ 1.2e-12 in the worst case and by sqrt(N) * 2^-53 ~ 1e-14 typically: 1e-12.  com_mse against
ops.com_mse_loss (which squares in double): 2e-6 relative, the margin tests/test_gpu_round2.py applies to that kernel."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2, seeded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS5 = (1600, 1121, 801, 2400, 961)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def _wavprep(L, wav, lens, reflect_own):
    B, L_ = wav.shape
    xpad = torch.empty(B, L_ + 320, device=DEV)
    c = torch.empty(B, device=DEV)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    d = L.WavprepDesc()
    d.wav, d.xpad, d.c, d.lens = wav.data_ptr(), xpad.data_ptr(), c.data_ptr(), lens_t.data_ptr()
    d.B, d.L, d.pad, d.normalize, d.reflect_own = B, L_, 160, 1, reflect_own
    L.launch(d)
    torch.cuda.synchronize()
    return xpad, c


@pytest.mark.parametrize("reflect_own", (0, 1))
@pytest.mark.parametrize("B,L_,lens", ((3, 1600, (1600, 1121, 801)), (1, 161, (161,))))
def test_pair_prep_equals_wavprep(L, B, L_, lens, reflect_own):
    noisy = torch.zeros(B, L_)
    clean = torch.zeros(B, L_)
    for b, n in enumerate(lens):
        noisy[b, :n] = seeded((n,), 10 + b) * (0.03 * (b + 1))
        clean[b, :n] = seeded((n,), 20 + b) * 0.02
    noisy, clean = noisy.to(DEV), clean.to(DEV)
    want_pad, want_c = _wavprep(L, noisy, lens, reflect_own)
    lens_t = torch.tensor(lens, dtype=torch.int32, device=DEV)
    npad = torch.full((B, L_ + 320), float("nan"), device=DEV)
    cpad = torch.full((B, L_ + 320), float("nan"), device=DEV)
    c = torch.empty(B, device=DEV)
    L.pair_prep(noisy.data_ptr(), clean.data_ptr(), lens_t.data_ptr(), npad.data_ptr(), cpad.data_ptr(), c.data_ptr(), B, L_, 160, reflect_own)
    torch.cuda.synchronize()
    assert torch.equal(c, want_c) and torch.equal(npad, want_pad)
    # the clean row: the same formula with the noisy row's c (fp32 division, reflect padding at L or at the utterance's own end)
    cc, ch = c.cpu(), clean.cpu()
    for b, n in enumerate(lens):
        end = n if reflect_own else L_
        k = torch.arange(-160, L_ + 160).abs()
        tail = k >= end + 160
        k = torch.where(k >= end, 2 * (end - 1) - k, k).clamp(min=0)
        want = torch.where(tail, torch.zeros(()), ch[b][k] / cc[b])
        assert torch.equal(cpad[b].cpu(), want), (b, reflect_own)


def _np_losses(esti, label, frames):
    """float64 sums of the kernel's fp32 element terms (include/pdse.h: pdse_spec_losses)."""
    e, l = esti.astype(np.float32), label.astype(np.float32)
    B, _, T, F = e.shape
    per = np.zeros((B, 2))
    for b in range(B):
        fr = frames[b]
        d = e[b, :, :fr] - l[b, :, :fr]
        per[b, 0] = (d * d).astype(np.float64).sum()
        me = np.sqrt(e[b, 0, :fr] * e[b, 0, :fr] + e[b, 1, :fr] * e[b, 1, :fr])
        ml = np.sqrt(l[b, 0, :fr] * l[b, 0, :fr] + l[b, 1, :fr] * l[b, 1, :fr])
        dm = me - ml
        per[b, 1] = (dm * dm).astype(np.float64).sum()
    n = float(sum(frames)) * F
    com, mag = per[:, 0].sum() / (2 * n), per[:, 1].sum() / n
    return per, (com, mag, 0.5 * (com + mag))


@pytest.mark.parametrize("B,T,frames", ((1, 1, (1,)), (3, 5, (5, 1, 0)), (2, 33, (33, 17))))
def test_spec_losses_vs_float64(L, B, T, frames):
    ops = pkg("ops")
    esti, label = seeded((B, 2, T, 161), 100 + T), seeded((B, 2, T, 161), 200 + T) * 0.7
    got = ops.spec_losses(esti.to(DEV), label.to(DEV), frames)
    again = ops.spec_losses(esti.to(DEV), label.to(DEV), frames)
    per, losses = _np_losses(esti.numpy(), label.numpy(), frames)
    gp = got["per_utt"].cpu().numpy()
    print("per_utt", gp, per, "losses", [float(got[k]) for k in ("com_mse", "mag_mse", "com_mag_mse")], losses)
    assert gp.shape == (B, 2) and got["per_utt"].dtype == torch.float64
    assert np.all(np.abs(gp - per) <= 1e-12 * np.abs(per))
    for k, want in zip(("com_mse", "mag_mse", "com_mag_mse"), losses):
        assert got[k].dim() == 0 and got[k].dtype == torch.float32
        assert abs(float(got[k]) - want) <= 1.2e-7 * want          # one rounding to fp32 (2^-24) of a double within 1e-12
        assert torch.equal(got[k], again[k])
    assert torch.equal(got["per_utt"], again["per_utt"])               # two runs: bit-identical
    old = float(ops.com_mse_loss(esti.to(DEV), label.to(DEV), frames))
    assert abs(float(got["com_mse"]) - old) <= 2e-6 * old


def test_spec_losses_rejects_empty_batch(L):
    ops = pkg("ops")
    z = torch.zeros(2, 2, 4, 161, device=DEV)
    with pytest.raises(ValueError, match="no frame"):
        ops.spec_losses(z, z, [0, 0])
    fr = np.zeros(2, dtype=np.int32)
    with pytest.raises(L.PdseError, match="sum of frames is 0"):
        L.spec_losses(z.data_ptr(), z.data_ptr(), fr.ctypes.data, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), 2, 4, 161)
    with pytest.raises(ValueError):
        ops.spec_losses(z, z, [5, 1])


def test_label_spec_and_per_utterance_independence(L):
    """ops.label_spec against torch's STFT of clean / c (the front end's 2e-6 of tests/test_gpu_parity.py), and the numerators
    of an utterance do not depend on the batch it sits in."""
    ops = pkg("ops")
    lens = (1600, 1121, 801)
    noisy, clean = torch.zeros(3, 1600), torch.zeros(3, 1600)
    for b, n in enumerate(lens):
        noisy[b, :n], clean[b, :n] = seeded((n,), 30 + b) * 0.05, seeded((n,), 40 + b) * 0.03
    label, c = ops.label_spec(noisy.to(DEV), clean.to(DEV), lens)
    want_c = torch.stack([noisy[b, :n].double().pow(2).mean().sqrt() for b, n in enumerate(lens)])
    assert rel_l2(c.cpu(), want_c) < 2e-6
    st = torch.stft(clean.double() / want_c[:, None], 320, 160, 320, torch.hann_window(320, dtype=torch.float64), return_complex=True)
    mag = st.abs().sqrt()
    want = torch.stack((mag * torch.cos(st.angle()), mag * torch.sin(st.angle())), 1).permute(0, 1, 3, 2)
    assert rel_l2(label.cpu(), want) < 2e-6
    esti = seeded(tuple(label.shape), 5).to(DEV)
    frames = [n // 160 + 1 for n in lens]
    per = ops.spec_losses(esti, label, frames)["per_utt"]
    for b in range(3):
        one = ops.spec_losses(esti[b:b + 1, :, :frames[b]].contiguous(), label[b:b + 1, :, :frames[b]].contiguous(), frames[b:b + 1])["per_utt"]
        assert torch.equal(one[0], per[b]), b


# ---------------------------------------------------------------- against the reference's own functions
def _fixture():
    from conftest import golden

    g = golden("validation_epoch")
    lens = [int(n) for n in g["lens"]]
    noisy, clean = torch.zeros(3, max(lens)), torch.zeros(3, max(lens))
    for b, n in enumerate(lens):
        noisy[b, :n] = seeded((n,), int(g["seed"]) + b) * float(g["noisy_scale"][b])
        clean[b, :n] = seeded((n,), int(g["seed"]) + 10 + b) * float(g["clean_scale"][b])
    return g, lens, [n // 160 + 1 for n in lens], noisy, clean


def test_validation_fixture_label_and_losses_vs_reference(L):
    """tests/golden/validation_epoch.npz (tools/make_golden_validation.py: Collate.collate_fn, the validation loop's compression
    and utils/loss.py, executed from the reference's text).  The label: the front end's 2e-6 of tests/test_gpu_parity.py.
    mag_mse / com_mag_mse: the reference sums in fp32; the float64 evaluation of the formula on the fixture's own tensors lies
    at most 4.5e-8 (mag_mse) and 4.7e-8 (com_mag_mse) relative from the fixture's values (measured by the tool on the CPU, kept
    in the fixture as ``f64_distance``); four times that, 1.9e-7, is below 2e-6, so 2e-6 relative holds for all three."""
    ops = pkg("ops")
    g, lens, frames, noisy, clean = _fixture()
    label, c = ops.label_spec(noisy.to(DEV), clean.to(DEV), lens)
    assert rel_l2(1.0 / c.cpu().numpy(), g["c"]) < 2e-6                 # the reference multiplies by its c, this package divides
    assert rel_l2(label.cpu(), g["label"]) < 2e-6
    ref_label = torch.from_numpy(g["label"]).to(DEV)
    for name in ("audio", "init"):
        got = ops.spec_losses(torch.from_numpy(g[name]).to(DEV), ref_label, frames)
        for k in ("com_mse", "mag_mse", "com_mag_mse"):
            want = float(g[name + "_" + k])
            print(name, k, float(got[k]), want, abs(float(got[k]) - want) / want)
            assert abs(float(got[k]) - want) <= 2e-6 * want, (name, k)


def test_validation_fixture_metrics_vs_reference(L):
    """compare_complex on the fixture: the decompressed spectrograms inverted as the label leg inverts them (ops.spec_to_wav:
    pdse_spec_frames in double, then the overlap-add operator), cut to (frame_num - 1) * 160, then the four measures, against
    utils/metrics.py's own functions on the reference's torch.istft waveforms.  Tolerances: those tests/test_gpu_metrics.py
    holds the measures to (emu_metrics.TOL: 2.0e-5, 2.2e-5, 3.7e-5, 2.0e-5 absolute).
    (With the sampling path's own fp32 decompression and ISTFT GEMM in front, fwSNRseg lay 2.1e-5 and 3.4e-5 from the fixture:
    those waveforms are 2e-6 from torch.istft, and a score of 20 - 27 dB over the few frames of a 0.1 s signal shows that.)"""
    import emu_metrics as E

    M, ops = pkg("metrics"), pkg("ops")
    g, lens, frames, _, _ = _fixture()
    ref_wav = ops.spec_to_wav(torch.from_numpy(g["label"]).to(DEV))
    cut = [(f - 1) * 160 for f in frames]
    bad = []
    for name in ("audio", "init"):
        q = M.quality(ref_wav, ops.spec_to_wav(torch.from_numpy(g[name]).to(DEV)), lens=cut)
        for k in E.KEYS:
            got_m, want_m = q[k].cpu().numpy(), g[name + "_" + k]
            print(name, k, got_m, want_m, "distance", np.abs(got_m - want_m).max(), "bound", E.TOL[k])
            if not E.same(got_m, want_m, E.TOL[k]).all():
                bad.append((name, k, got_m, want_m))
    assert not bad, bad


def test_spec_to_wav_vs_float64_istft(L):
    """ops.spec_to_wav against torch.istft of the decompressed spectrogram in float64.  T = 11 (three row groups of the kernel,
    the last partial), B = 3.  Bound: the frames are exact double sums rounded to fp32 once, and a sample is (f1 + f2) / env in
    fp32 - three roundings of at most 2^-24 each, relative to |f1| + |f2| <= about 2 |y| in the mean: 3 * 2 * 6e-8 = 3.6e-7
    rel-L2 (a numpy emulation of these roundings sits at 5.4e-8)."""
    ops = pkg("ops")
    g, _, _, _, _ = _fixture()
    for name in ("label", "audio"):
        s = torch.from_numpy(g[name]).double()
        mag = torch.sqrt(s[:, 0] ** 2 + s[:, 1] ** 2)
        want = torch.istft(torch.complex(mag * s[:, 0], mag * s[:, 1]).permute(0, 2, 1), 320, 160, 320,
                           torch.hann_window(320, dtype=torch.float64))
        got = ops.spec_to_wav(torch.from_numpy(g[name]).to(DEV))
        assert got.shape == want.shape
        d = rel_l2(got.cpu(), want)
        print(name, "rel-L2", d)
        assert d < 3.6e-7
    one = ops.spec_to_wav(torch.from_numpy(g["audio"][1:2, :, :7]).contiguous().to(DEV))      # rows do not depend on B or T
    assert torch.equal(one[0, :800], ops.spec_to_wav(torch.from_numpy(g["audio"]).to(DEV))[1, :800])


# ---------------------------------------------------------------- the epoch
def _trainer(weights, tmp_path, prior="GCRN", sigma=False, exclusive=False, **kw):
    args = argparse.Namespace(retrain=False, joint=True, draw=False, sigma=sigma, checkpoint=str(tmp_path / "ck"),
                              generated_wav=str(tmp_path / "out"))
    config = argparse.Namespace(model=argparse.Namespace(name=prior),
                                train=argparse.Namespace(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt", batch_size=2))
    return pkg("trainer").ComplexDDPMTrainer(args, config, device=DEV, prior_state_dict=weights(prior),
                                             ddpm_state_dict=weights("DiffUNet1"), exclusive=exclusive, **kw)


@pytest.fixture(scope="module")
def pairs_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("valid_pairs")
    wavio = pkg("wavio")
    for sub in ("noisy", "clean"):
        os.makedirs(str(root / sub))
    for i, n in enumerate(LENS5):
        clean = 0.05 * seeded((n,), 300 + i).numpy()
        wavio.write_wav(str(root / "clean" / ("p%d.wav" % i)), clean)
        wavio.write_wav(str(root / "noisy" / ("p%d.wav" % i)), clean + 0.02 * seeded((n,), 400 + i).numpy())
    return root


def _read(root, sub, i):
    return torch.from_numpy(pkg("wavio").read_wav(str(root / sub / ("p%d.wav" % i))).astype(np.float32))


def _draws(lens, batch, seed):
    out = []
    for k in range(0, len(lens), batch):
        part = lens[k:k + batch]
        out.append(seeded((len(part), 2, 1 + max(part) // 160, 161), seed + k))
    return out


def test_validate_epoch(L, weights, tmp_path, pairs_dir, monkeypatch):
    ops = pkg("ops")
    t = _trainer(weights, tmp_path)
    x_T = _draws(LENS5, 2, 50)
    kept = []
    orig = t.validate_batch

    def spy(noisy, clean, **kw):
        out = orig(noisy, clean, **kw)
        pipe = t._pipe(len(noisy), L_=max(int(w.numel()) for w in noisy), label=True)      # the plan the batch just ran on
        kept.append(out + (pipe.spec.clone(), pipe.init_spec.clone(), pipe.label.spec.clone()))
        return out

    monkeypatch.setattr(t, "validate_batch", spy)
    res = t.validate(str(pairs_dir / "noisy"), str(pairs_dir / "clean"), x_T=x_T)
    assert [f["name"] for f in res["files"]] == ["p%d.wav" % i for i in range(5)] and res["batches"] == 3
    assert [f["frames"] for f in res["files"]] == [n // 160 + 1 for n in LENS5]
    losses, init_losses = [], []
    for k, (enhanced, scores, spec, init_spec, label) in enumerate(kept):
        idx = list(range(2 * k, min(2 * k + 2, 5)))
        noisy = [_read(pairs_dir, "noisy", i) for i in idx]
        frames = [LENS5[i] // 160 + 1 for i in idx]
        want = t.enhance_batch(noisy, x_T=x_T[k], trim_to_frames=True)
        assert all(torch.equal(a, b) for a, b in zip(enhanced, want)), k
        losses.append(float(ops.com_mse_loss(spec, label, frames)))
        init = ops.spec_losses(init_spec, label, frames)                 # the "init" scores: spec_losses on the pipeline's X_init
        init_losses.append(float(init["com_mse"]))
        assert torch.equal(init["per_utt"], scores["init"]["per_utt"]) and torch.equal(init["com_mse"], scores["init"]["loss"][0])
    assert abs(res["loss"] - np.mean(losses)) <= 2e-6 * np.mean(losses)
    assert abs(res["init"]["loss"] - np.mean(init_losses)) <= 1e-7 * np.mean(init_losses)
    for key in ("loss_per_frame", "mag_mse", "mag_mse_per_frame", "com_mag_mse", "mean_ssnr", "mean_llr", "mean_wss", "mean_fwsnrseg"):
        assert np.isfinite(res[key]) and np.isfinite(res["init"][key]), key
    assert "mean_stoi" not in res
    # drop_last scores 4 files; prior=False leaves no "init"
    short = t.validate(str(pairs_dir / "noisy"), str(pairs_dir / "clean"), x_T=x_T[:2], drop_last=True, prior=False)
    assert len(short["files"]) == 4 and "init" not in short and "init" not in short["files"][0]
    assert [f["com_num"] for f in short["files"]] == [f["com_num"] for f in res["files"][:4]]


def _exact_alone(t, root, tmp_path, files, batch, seed):
    """validate(exact=True) over the pairs ``files`` against a B = 1 validate of every file alone: per-file numerators, bit for bit."""
    import shutil

    def subset(name, idx):
        d = tmp_path / name
        for sub in ("noisy", "clean"):
            os.makedirs(str(d / sub))
            for i in idx:
                shutil.copy(str(root / sub / ("p%d.wav" % i)), str(d / sub))
        return str(d / "noisy"), str(d / "clean")

    lens = [LENS5[i] for i in files]
    x_T = _draws(lens, batch, seed)
    res = t.validate(*subset("all", files), x_T=x_T, exact=True, batch_size=batch)
    assert len(res["files"]) == len(files)
    for j, i in enumerate(files):
        x1 = x_T[j // batch][j % batch:j % batch + 1, :, :1 + lens[j] // 160].contiguous()
        alone = t.validate(*subset("one%d" % i, [i]), x_T=[x1], exact=True, batch_size=1)
        a, b = alone["files"][0], res["files"][j]
        assert a["name"] == b["name"] and a["frames"] == b["frames"]
        assert (a["com_num"], a["mag_num"]) == (b["com_num"], b["mag_num"]), i
        assert (a["init"]["com_num"], a["init"]["mag_num"]) == (b["init"]["com_num"], b["init"]["mag_num"]), i


def test_validate_exact_equals_files_alone(L, weights, tmp_path, pairs_dir):
    _exact_alone(_trainer(weights, tmp_path, exclusive=False), pairs_dir, tmp_path, [0, 1, 2, 3, 4], 2, 60)


def test_validate_exact_masked_dbaiat_prior(L, weights, tmp_path, pairs_dir):
    t = _trainer(weights, tmp_path, prior="aia_complex_trans_ri", exclusive=False, masked_prior=True)
    _exact_alone(t, pairs_dir, tmp_path, [0, 1], 2, 70)


def test_validate_sigma_is_finite(L, weights, tmp_path, pairs_dir):
    t = _trainer(weights, tmp_path, sigma=True)
    torch.manual_seed(3)
    res = t.validate(str(pairs_dir / "noisy"), str(pairs_dir / "clean"))
    flat = [res[k] for k in res if k not in ("init", "files", "batches")] + [res["init"][k] for k in res["init"]]
    assert len(res["files"]) == 5 and np.isfinite(flat).all()


def test_cli_eval_writes_json(L, weights, tmp_path, pairs_dir, monkeypatch):
    main = pkg("main")
    os.makedirs(str(tmp_path / "conf"))
    with open(str(tmp_path / "conf" / "diff.yml"), "w") as f:
        f.write("model:\n  name: GCRN\ntrain:\n  fft_num: 320\n  win_size: 320\n  win_shift: 160\n  feat_type: sqrt\n  batch_size: 2\n")
    monkeypatch.chdir(tmp_path)
    tr = pkg("trainer")
    made = []

    class Synthetic(tr.ComplexDDPMTrainer):
        def __init__(self, args, config):
            super().__init__(args, config, device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights("DiffUNet1"))
            made.append(self)

    monkeypatch.setattr(tr, "ComplexDDPMTrainer", Synthetic)
    argv = ["--assets", str(tmp_path / "assets"), "--eval", "--data", str(pairs_dir / "noisy"), "--clean", str(pairs_dir / "clean"),
            "--seed", "77"]
    res = main.main(argv)
    with open(str(tmp_path / "assets" / "log" / "diff" / "eval.json")) as f:
        disk = json.load(f)
    assert disk["loss"] == res["loss"] and len(disk["files"]) == 5 and "init" in disk
    torch.manual_seed(77)
    torch.cuda.manual_seed_all(77)
    again = made[0].validate(str(pairs_dir / "noisy"), str(pairs_dir / "clean"))
    assert again["loss"] == res["loss"]
