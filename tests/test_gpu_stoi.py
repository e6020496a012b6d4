"""GPU: csrc/stoi.hip behind metrics.quality(stoi=True) against the float64 oracle (tests/helpers/stoi_refs.py), its independence
of the batch an utterance sits in, the unchanged default, ComplexDDPMTrainer.evaluate_batch(stoi=True) and the command line.

Tolerance (tests/emu_stoi.py: TOL, absolute): 10 x the largest distance of the numpy restatement of the kernel arithmetic from
the oracle over the same inputs - measured 2.63e-8, committed as 3.0e-8 (half an fp32 ulp below 1), so 3.0e-7 (profiles/stoi_parity.txt holds both, and the
GPU's own distances)."""
import argparse
import os

import numpy as np
import pytest

import emu_stoi as E
from conftest import pkg
from helpers import stoi_refs as R

pytestmark = pytest.mark.gpu

FOUR = ["ssnr", "llr", "wss", "fwsnrseg"]


def _batch(pairs):
    import torch

    pad = lambda xs: torch.nn.utils.rnn.pad_sequence([torch.from_numpy(x) for x in xs], batch_first=True).cuda()   # noqa: E731
    return pad([c for c, _ in pairs]), pad([p for _, p in pairs]), [len(c) for c, _ in pairs]


def _scores(pairs):
    """quality(stoi=True) of a list of (clean, proc) numpy pairs as one ragged batch -> ([B, 2] fp32 {stoi, estoi}, [B, 4] fp32)."""
    import torch

    c, p, lens = _batch(pairs)
    q = pkg("metrics").quality(c, p, lens=lens, stoi=True)
    return (torch.stack([q[k] for k in E.KEYS], dim=1).cpu().numpy(), torch.stack([q[k] for k in FOUR], dim=1).cpu().numpy())


@pytest.fixture(scope="module")
def batch():
    """The ragged batch of the parity test, its oracle values (the keep-mask condition asserted on the CPU first) and the
    device's scores, computed once."""
    pairs = [R.case(n) for n in R.CASES]
    for n in R.CASES:
        assert R.oracle(n)["margin_db"] >= R.MARGIN_DB, (n, R.oracle(n)["margin_db"])    # no frame within rounding of the 40 dB line
    o = R.oracle("min_L6400")
    assert o["frames"] == o["kept"] == 30
    assert [len(c) for c, _ in pairs] == [16000, 8000, 6400, 3000]
    got, four = _scores(pairs)
    return pairs, got, four


def test_vs_reference_oracle_ragged_batch(batch):
    pairs, got, _ = batch
    log = os.environ.get("PDSE_METRICS_PARITY_GPU")
    for b, name in enumerate(R.CASES):
        o = R.oracle(name)
        for i, k in enumerate(E.KEYS):
            d = abs(float(got[b, i]) - o[k])
            print("%s %s: device %.9g oracle %.9g distance %.2e (tolerance %.1e)" % (name, k, got[b, i], o[k], d, E.TOL))
            if log:
                with open(log, "a") as f:
                    f.write("%-12s %-5s device %.9f oracle %.9f distance %.2e  (tolerance %.1e)\n" % (name, k, got[b, i], o[k], d, E.TOL))
    for b, name in enumerate(R.CASES):
        o = R.oracle(name)
        for i, k in enumerate(E.KEYS):
            assert np.isfinite(got[b, i]) and abs(float(got[b, i]) - o[k]) <= E.TOL, (name, k, got[b, i], o[k])
    assert got[3].tobytes() == np.array([1e-5, 1e-5], dtype=np.float32).tobytes()        # short_L3000: exactly 1e-5
    assert 0.0 < got[2, 0] < 1.0                                                          # min_L6400 rests on one segment


def test_scores_do_not_depend_on_the_batch(batch):
    pairs, got, four = batch
    perm = [2, 0, 3, 1]
    got_p, four_p = _scores([pairs[i] for i in perm])
    for at, i in enumerate(perm):
        assert got_p[at].tobytes() == got[i].tobytes(), (R.CASES[i], got_p[at], got[i])
        assert four_p[at].tobytes() == four[i].tobytes(), R.CASES[i]
    for i, pair in enumerate(pairs):
        one, one4 = _scores([pair])
        assert one[0].tobytes() == got[i].tobytes(), (R.CASES[i], one[0], got[i])
        assert one4[0].tobytes() == four[i].tobytes(), R.CASES[i]


def test_default_is_unchanged(batch, monkeypatch):
    import torch

    pairs, _, four = batch
    M, L = pkg("metrics"), pkg("_lib")
    seen = []
    launch = L.launch
    monkeypatch.setattr(L, "launch", lambda d, *a, **k: (seen.append((d.measures, d.stoi_tables, d.stoi_work, d.stoi_out)), launch(d, *a, **k))[1])
    c, p, lens = _batch(pairs)
    q = M.quality(c, p, lens=lens)
    assert sorted(q) == sorted(FOUR) and seen == [(0, None, None, None)]
    assert torch.stack([q[k] for k in FOUR], dim=1).cpu().numpy().tobytes() == four.tobytes()     # the selector changes none of the four
    q = M.quality(c, p, lens=lens, per_frame=True)
    assert sorted(q) == sorted(FOUR + ["frames", "frame_counts"])


def test_evaluate_batch_passes_stoi_through(weights):
    import torch

    synth = pkg("synth")
    ns = argparse.Namespace
    args = ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav="y")
    config = ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt"))
    tr = pkg("trainer").ComplexDDPMTrainer(args, config, device="cuda:0", prior_state_dict=weights("GCRN"),
                                           ddpm_state_dict=weights("DiffUNet1"))
    lens = [6400, 2560]
    clean = [synth.speechlike(1, n, 70 + i)[0] for i, n in enumerate(lens)]
    noisy = [R.add_noise(c, 80 + i, 10.0) for i, c in enumerate(clean)]
    enhanced, scores = tr.evaluate_batch(noisy, clean, stoi=True)
    assert sorted(scores) == sorted(FOUR + E.KEYS + ["mean_" + k for k in FOUR + E.KEYS])
    for k in E.KEYS:
        assert scores[k].shape == (2,) and scores[k].is_cuda and torch.isfinite(scores[k]).all()
        assert torch.equal(scores["mean_" + k].cpu(), scores[k].mean().cpu()), k
    assert float(scores["stoi"][1]) == float(np.float32(1e-5)) and float(scores["stoi"][0]) != float(np.float32(1e-5))
    _, plain = tr.evaluate_batch(noisy, clean)
    assert sorted(plain) == sorted(FOUR + ["mean_" + k for k in FOUR])


def test_cli_prints_the_stoi_means(tmp_path, capsys):
    import torch

    M, wavio = pkg("metrics"), pkg("wavio")
    ref, deg = tmp_path / "ref", tmp_path / "deg"
    ref.mkdir(), deg.mkdir()
    for i, name in enumerate(("min_L6400", "snr10_L8000")):
        c, p = R.case(name)
        wavio.write_wav(str(ref / ("%d.wav" % i)), c)
        wavio.write_wav(str(deg / ("%d.wav" % i)), p)
    assert M.main(["--stoi", str(ref), str(deg)]) == 0
    text = capsys.readouterr().out
    assert "PESQ is not computed" in text and "STOI are not" not in text
    rows = []
    for i in range(2):
        c, p = wavio.read_wav(str(ref / ("%d.wav" % i))), wavio.read_wav(str(deg / ("%d.wav" % i)))
        q = M.quality(torch.from_numpy(c)[None].cuda(), torch.from_numpy(p)[None].cuda(), stoi=True)
        rows.append([float(q[k][0]) for k in FOUR + E.KEYS])
    want = "ssnr:%6.4f llr:%6.4f wss:%6.4f fwsnrseg:%6.4f stoi:%6.4f estoi:%6.4f" % tuple(np.mean(np.array(rows, dtype=np.float64), axis=0))
    assert want in text, (want, text)
    assert M.main([str(ref), str(deg)]) == 0
    assert "stoi:" not in capsys.readouterr().out
