"""GPU: csrc/metrics.hip behind metrics.quality against the reference's float64 results (tests/golden/metrics_*.npz), its
independence of the batch an utterance sits in, and ComplexDDPMTrainer.evaluate_batch.

Tolerances (tests/emu_metrics.py: TOL, absolute, in each measure's unit): 10 x the largest distance of the numpy restatement
of the kernel arithmetic from the reference over the fixtures - measured 1.90e-6 (SSNR), 2.13e-6 (LLR), 3.69e-6 (WSS),
1.90e-6 (fwSNRseg), committed as 2.0e-6, 2.2e-6, 3.7e-6, 2.0e-6, so 2.0e-5, 2.2e-5, 3.7e-5, 2.0e-5 (profiles/metrics_parity.txt holds both, and the GPU's own distances)."""
import argparse
import os

import numpy as np
import pytest

import emu_metrics as E
from conftest import pkg

pytestmark = pytest.mark.gpu


def _quality(pairs, per_frame=True):
    """Score a list of (clean, proc) numpy pairs as one (ragged) batch; returns (scores [B,4] float32, list of [4, m] frames)."""
    import torch

    M = pkg("metrics")
    lens = [len(c) for c, _ in pairs]
    pad = lambda xs: torch.nn.utils.rnn.pad_sequence([torch.from_numpy(x) for x in xs], batch_first=True).cuda()   # noqa: E731
    q = M.quality(pad([c for c, _ in pairs]), pad([p for _, p in pairs]), lens=lens, per_frame=per_frame)
    out = torch.stack([q[k] for k in E.KEYS], dim=1).cpu().numpy()
    fr = q["frames"].cpu().numpy()
    return out, [fr[:, b, :m] for b, m in enumerate(q["frame_counts"])]


@pytest.mark.parametrize("name", E.CASES)
def test_golden_metrics_vs_reference(name):
    g = E.load_case(name)
    out, frames = _quality([E.case_inputs(g)])
    log = os.environ.get("PDSE_METRICS_PARITY_GPU")
    for i, k in enumerate(E.KEYS):
        ref_fr = g[k + "_frames"]
        assert frames[0][i].shape == ref_fr.shape
        ds, df = E.distance(out[0, i], g[k]), E.distance(frames[0][i], ref_fr)
        bad = float(np.mean(~E.same(frames[0][i], ref_fr, E.TOL[k])))
        print("%s %s: score %.9g reference %.9g distance %.2e; frames distance %.2e, outside tolerance %.4f"
              % (name, k, out[0, i], float(g[k]), ds, df, bad))
        if log:
            with open(log, "a") as f:
                f.write("%-16s %-9s score distance %.2e  per-frame distance %.2e  frames outside tolerance %.4f  (tolerance %.1e)\n"
                        % (name, k, ds, df, bad, E.TOL[k]))
    for i, k in enumerate(E.KEYS):
        # the score: within TOL of the reference, and non-finite exactly where the reference is
        assert E.same(out[0, i], g[k], E.TOL[k]).all(), (name, k, out[0, i], float(g[k]))
        # per-frame values: the restatement has no frame outside TOL on any fixture (profiles/metrics_parity.txt), so the cap
        # on the fraction of frames outside tolerance - what the restatement itself shows, at most 1 % - is zero, WSS included
        bad = float(np.mean(~E.same(frames[0][i], g[k + "_frames"], E.TOL[k])))
        assert bad <= E.FRAME_OUTLIERS, (name, k, bad)


def test_golden_identity_and_silence():
    g = E.load_case("same_L4000")
    out, _ = _quality([E.case_inputs(g)])
    assert abs(out[0, 0] - 35.0) <= E.TOL["ssnr"] and abs(out[0, 1]) <= E.TOL["llr"]
    g = E.load_case("silence_L32000")
    out, frames = _quality([E.case_inputs(g)])
    for i, k in enumerate(E.KEYS):
        assert np.isfinite(out[0, i]) == np.isfinite(float(g[k])), k
        assert np.array_equal(np.isfinite(frames[0][i]), np.isfinite(g[k + "_frames"])), k
        assert np.isnan(out[0, i]) == np.isnan(float(g[k])), k


def test_golden_ragged_batch_equals_single_utterances_bit_for_bit():
    names = ["snr0_L64000", "snr10_L600", "snr5_L47321", "same_L4000", "silence_L32000", "snr10_L4000", "snr40_L64000",
             "snr5_L47321"]
    pairs = [E.case_inputs(E.load_case(n)) for n in names]
    out, frames = _quality(pairs)
    for b, pair in enumerate(pairs):
        one, fr1 = _quality([pair])
        assert one[0].tobytes() == out[b].tobytes(), (names[b], one[0], out[b])
        assert fr1[0].tobytes() == frames[b].tobytes(), names[b]


def test_b32_twice_is_bit_identical():
    import torch

    synth, M = pkg("synth"), pkg("metrics")
    clean = synth.speechlike(32, 64000, 5)
    noise = np.random.RandomState(6).standard_normal(clean.shape).astype(np.float32)
    c, p = torch.from_numpy(clean).cuda(), torch.from_numpy(clean + 0.05 * noise).cuda()
    runs = []
    for _ in range(2):
        q = M.quality(c, p, per_frame=True)
        runs.append((torch.stack([q[k] for k in E.KEYS]).cpu().numpy().tobytes(), q["frames"].cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    assert np.isfinite(np.frombuffer(runs[0][0], dtype=np.float32)).all()


def test_evaluate_batch_scores_are_quality_of_what_it_returns(weights):
    import torch

    synth, M = pkg("synth"), pkg("metrics")
    ns = argparse.Namespace
    args = ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav="y")
    config = ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt"))
    tr = pkg("trainer").ComplexDDPMTrainer(args, config, device="cuda:0", prior_state_dict=weights("GCRN"),
                                           ddpm_state_dict=weights("DiffUNet1"))
    lens = [2560, 2000, 1777]
    clean = [synth.speechlike(1, n, 40 + i)[0] for i, n in enumerate(lens)]
    noisy = [c + 0.05 * np.random.RandomState(50 + i).standard_normal(len(c)).astype(np.float32) for i, c in enumerate(clean)]
    enhanced, scores = tr.evaluate_batch(noisy, clean)
    cut = [(n // 160) * 160 for n in lens]
    assert [int(e.numel()) for e in enhanced] == cut and all(e.is_cuda for e in enhanced)
    pad = torch.nn.utils.rnn.pad_sequence
    q = M.quality(pad([torch.from_numpy(c[:n]) for c, n in zip(clean, cut)], batch_first=True).cuda(),
                  pad(enhanced, batch_first=True), lens=cut)
    for k in E.KEYS:
        assert scores[k].shape == (3,) and scores[k].is_cuda
        assert scores[k].cpu().numpy().tobytes() == q[k].cpu().numpy().tobytes(), k
        assert torch.equal(scores["mean_" + k].cpu(), q[k].mean().cpu()), k
    with pytest.raises(ValueError):
        tr.evaluate_batch(noisy, clean[:2])


def test_cli_prints_the_means_of_quality(tmp_path, capsys):
    import torch

    M, wavio, synth = pkg("metrics"), pkg("wavio"), pkg("synth")
    ref, deg = tmp_path / "ref", tmp_path / "deg"
    ref.mkdir(), deg.mkdir()
    for i, n in enumerate((4000, 3000, 4000)):
        c, p = synth.noisy_pair(n, 60 + i, 10.0)
        wavio.write_wav(str(ref / ("%d.wav" % i)), c)
        wavio.write_wav(str(deg / ("%d.wav" % i)), p)
    assert M.main([str(ref), str(deg)]) == 0
    text = capsys.readouterr().out
    assert "PESQ and STOI are not computed" in text
    rows = []
    for i in range(3):
        c, p = wavio.read_wav(str(ref / ("%d.wav" % i))), wavio.read_wav(str(deg / ("%d.wav" % i)))
        q = M.quality(torch.from_numpy(c)[None].cuda(), torch.from_numpy(p)[None].cuda())
        rows.append([float(q[k][0]) for k in E.KEYS])
    want = "ssnr:%6.4f llr:%6.4f wss:%6.4f fwsnrseg:%6.4f" % tuple(np.mean(np.array(rows, dtype=np.float64), axis=0))
    assert want in text, (want, text)
