"""GPU: posterior ensembles - csrc/ensemble.hip behind pdse_ensemble_stats, ``SamplerPipeline(members=K)``, and the trainer's
``enhance_members``, ``validate_batch(members=K)`` and ``main.py --generate --members K``.

Yardsticks: the float64 numpy statement of tests/helpers/ensemble_refs.py (held to a naive formulation in
tests/test_ensemble_host.py) and this package's own one-member passes on an ``exclusive=False`` trainer, whose kernels do not
depend on the batch size.

Tolerances.  ``mean``: the double mean is a sum of K <= 16 fp32 values, which is exact in double (24 + 4 bits), and one IEEE
division, rounded to fp32 once - bit for bit.  ``spread``: the kernel adds the K squared deviations of re and then of im, numpy
adds |d_k|^2 member by member; the doubles differ by a few 2^-53, so the fp32 roundings agree or are neighbours: 1 fp32 ulp.
``per_utt`` / ``per_member``: double sums of non-negative terms that differ from numpy's in order alone; the largest case has
16 * 2 * 33 * 161 < 2e5 terms in per_utt[0] and fewer than 2e4 in every other sum, N 2^-53 < 2e-11 in the worst case and
sqrt(N) 2^-53 ~ 5e-14 typically: 1e-12 relative, as the issue states it."""
import argparse
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, pkg, seeded

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ensemble_refs as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def _trainer(weights, tmp_path, prior="GCRN", sigma=False, exclusive=False, **kw):
    args = argparse.Namespace(retrain=False, joint=True, draw=False, sigma=sigma, checkpoint=str(tmp_path / "ck"),
                              generated_wav=str(tmp_path / "out"))
    config = argparse.Namespace(model=argparse.Namespace(name=prior),
                                train=argparse.Namespace(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt", batch_size=2))
    return pkg("trainer").ComplexDDPMTrainer(args, config, device=DEV, prior_state_dict=weights(prior),
                                             ddpm_state_dict=weights("DiffUNet1"), exclusive=exclusive, **kw)


def _ulps(a, b):
    """Distance of two fp32 arrays in units in the last place (of the larger magnitude)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


# the issue's four, then two whose planes are a multiple of 4 and of 2 floats long: the 16- and 8-byte paths of the kernel
SHAPES = ((2, 1, 1, (1,)), (3, 3, 5, (5, 1, 0)), (16, 2, 33, (33, 17)), (5, 1, 21, (21,)), (4, 2, 4, (4, 3)), (9, 2, 2, (2, 1)))


@pytest.mark.parametrize("K,B,T,frames", SHAPES)
def test_ensemble_stats_vs_float64(L, K, B, T, frames):
    ops = pkg("ops")
    same = seeded((1, 1, 2, T, 161), 7).expand(K, 1, 2, T, 161)            # plus one utterance with all members equal, all T frames its own
    x = torch.cat([seeded((K, B, 2, T, 161), 1000 + 10 * K + T), same], dim=1).contiguous()
    B, frames = B + 1, tuple(frames) + (T,)
    want = E.ensemble_stats(x.numpy(), K, frames)
    xd = x.reshape(K * B, 2, T, 161).to(DEV)
    got = ops.ensemble_stats(xd, K, frames)
    again = ops.ensemble_stats(x.to(DEV), K, frames)                       # the [K,B,2,T,F] form, a second call
    torch.cuda.synchronize()
    mean, spread = got["mean"].cpu().numpy(), got["spread"].cpu().numpy()
    pu, pm = got["per_utt"].cpu().numpy(), got["per_member"].cpu().numpy()
    u = _ulps(spread, want["spread"])
    print("K", K, "B", B, "T", T, "spread ulps max", u.max(), "per_utt", pu.tolist(), want["per_utt"].tolist())
    assert mean.dtype == np.float32 and mean.shape == (B, 2, T, 161) and spread.shape == (B, T, 161)
    assert got["per_utt"].dtype == torch.float64 and pu.shape == (B, 2) and pm.shape == (K, B)
    assert np.array_equal(mean, want["mean"])                              # bit for bit
    assert u.max() <= 1
    assert np.all(spread[B - 1] == 0) and pu[B - 1, 0] == 0 and np.all(pm[:, B - 1] == 0)     # all members equal: exactly zero
    assert np.all(np.abs(pu - want["per_utt"]) <= 1e-12 * np.abs(want["per_utt"]))
    assert np.all(np.abs(pm - want["per_member"]) <= 1e-12 * np.abs(want["per_member"]))
    for k in ("mean", "spread", "per_utt", "per_member"):
        assert torch.equal(got[k], again[k]), k                            # two calls: the same bits
    if K > 1 and frames[0] > 0:
        rs = ops.relative_spread(got["per_utt"], K).cpu().numpy()
        assert abs(rs[0] - E.relative_spread(want["per_utt"], K)[0]) <= 1e-12 * rs[0]


def test_ensemble_stats_one_member_and_out(L):
    ops = pkg("ops")
    x = seeded((3, 2, 5, 161), 5).to(DEV)
    mean, spread = torch.full((3, 2, 5, 161), float("nan"), device=DEV), torch.full((3, 5, 161), float("nan"), device=DEV)
    got = ops.ensemble_stats(x, 1, [5, 2, 0], out=(mean, spread))
    assert got["mean"] is mean and torch.equal(mean, x) and not spread.any()
    assert not got["per_member"].any() and not got["per_utt"][:, 0].any()
    want = (x.double() ** 2).sum(dim=(1, 3))                               # [B,T]
    for b, fr in enumerate((5, 2, 0)):
        w = float(want[b, :fr].sum())
        assert abs(float(got["per_utt"][b, 1]) - w) <= 1e-12 * w
    with pytest.raises(ValueError, match="out:"):
        ops.ensemble_stats(x, 1, [5, 2, 0], out=(mean, spread[:2]))
    with pytest.raises(ValueError, match="frames"):
        ops.ensemble_stats(x, 1, [6, 2, 0])


def _wavs(B, L_, seed):
    return torch.stack([0.05 * (b + 1) * seeded((L_,), seed + b) for b in range(B)]).to(DEV)


@pytest.mark.parametrize("prior,sigma", (("GCRN", False), ("GCRN", True), ("DiffUNet", False)))
def test_members_are_passes(L, weights, tmp_path, prior, sigma):
    """Member k of an ensemble pass is, bit for bit, the one-member pass given x_T[k]: the reverse loop's kernels do not depend
    on the batch size (``exclusive=False``).  Mean, spread and sums are the float64 reference applied to those members, and the
    waveform is what the one-member plan's back end makes of the mean."""
    t = _trainer(weights, tmp_path, prior=prior, sigma=sigma)
    B, L_, K, T = 2, 1600, 3, 11
    wav, x_T = _wavs(B, L_, 40), seeded((K, B, 2, T, 161), 41).to(DEV)
    res = t.enhance_members(wav, x_T, members=K)
    torch.cuda.synchronize()
    assert sorted(res) == ["members_spec", "per_member", "per_utt", "relative_spread", "spec", "spread", "wav"]
    assert tuple(res["members_spec"].shape) == (K * B, 2, T, 161) and tuple(res["spread"].shape) == (B, T, 161)
    one = t._pipe(B, L_=L_)
    for k in range(K):
        t.enhance(wav, x_T[k])
        assert torch.equal(res["members_spec"][k * B:(k + 1) * B], one.spec), (prior, sigma, k)
    want = E.ensemble_stats(res["members_spec"].cpu().numpy(), K, [T] * B)
    assert np.array_equal(res["spec"].cpu().numpy(), want["mean"])
    assert _ulps(res["spread"].cpu().numpy(), want["spread"]).max() <= 1
    pu, pm = res["per_utt"].cpu().numpy(), res["per_member"].cpu().numpy()
    assert np.all(np.abs(pu - want["per_utt"]) <= 1e-12 * want["per_utt"]) and np.all(np.abs(pm - want["per_member"]) <= 1e-12 * want["per_member"])
    rs = res["relative_spread"].cpu().numpy()
    print(prior, sigma, "relative_spread", rs)
    assert np.all(np.abs(rs - E.relative_spread(want["per_utt"], K)) <= 1e-12 * rs) and np.all(rs > 0) and np.isfinite(rs).all()
    # the back end of the one-member plan (its c is this wav's, left by the passes above) fed the mean
    one.spec.copy_(res["spec"])
    one.run("istft", "istft")
    assert torch.equal(res["wav"], one.istft.wav)
    # enhance(members=K) is that waveform; [K B, ...] is the same x_T
    assert torch.equal(t.enhance(wav, x_T.reshape(K * B, 2, T, 161), members=K), res["wav"])
    if prior == "GCRN" and not sigma:
        mean_batch = t.enhance_batch([w for w in wav], x_T=x_T, members=K)
        assert all(torch.equal(m, res["wav"][b]) for b, m in enumerate(mean_batch))
        feat = t._pipe(B, L_=L_).feat.clone()
        assert torch.equal(t.sample(feat, x_T, members=K), res["spec"])


def test_one_member_is_todays_pass(L, weights, tmp_path):
    t = _trainer(weights, tmp_path)
    B, L_, T = 2, 1600, 11
    wav, x_T = _wavs(B, L_, 50), seeded((B, 2, T, 161), 51).to(DEV)
    base = t.enhance(wav, x_T)
    spec = t._pipe(B, L_=L_).spec.clone()
    assert torch.equal(t.enhance(wav, x_T, members=1), base) and torch.equal(t.enhance(wav, x_T[None], members=1), base)
    res = t.enhance_members(wav, x_T, members=1)
    assert torch.equal(res["wav"], base) and torch.equal(res["spec"], spec) and torch.equal(res["members_spec"], spec)
    assert not res["spread"].any() and not res["relative_spread"].any() and len(t._pipes) == 1      # the same cached plan


def test_validate_batch_members(L, weights, tmp_path):
    t = _trainer(weights, tmp_path)
    lens, K = (1600, 1121, 801), 4
    clean = [0.05 * seeded((n,), 300 + i) for i, n in enumerate(lens)]
    noisy = [c + 0.02 * seeded((n,), 400 + i) for i, (c, n) in enumerate(zip(clean, lens))]
    x_T = seeded((K, 3, 2, 11, 161), 60).to(DEV)
    _, sc = t.validate_batch(noisy, clean, x_T=x_T, members=K)
    ens = sc["ensemble"]
    assert sorted(ens) == ["loss_by_member", "loss_member_mean", "loss_member_std", "members", "per_utt_by_member", "relative_spread"]
    assert ens["members"] == K and tuple(ens["loss_by_member"].shape) == (K,) and tuple(ens["relative_spread"].shape) == (3,)
    nums = []
    for k in range(K):
        _, one = t.validate_batch(noisy, clean, x_T=x_T[k])
        assert torch.equal(ens["loss_by_member"][k], one["x"]["loss"][0]), k
        assert torch.equal(ens["per_utt_by_member"][k], one["x"]["per_utt"]), k
        nums.append(one["x"]["per_utt"][:, 0].cpu().numpy())
        assert "ensemble" not in one
        for key in one["init"]:
            assert torch.equal(sc["init"][key], one["init"][key]), key           # the prior ran once, at B: unchanged
    lbm = ens["loss_by_member"].double().cpu().numpy()
    assert abs(float(ens["loss_member_mean"]) - lbm.mean()) <= 1e-12 and abs(float(ens["loss_member_std"]) - lbm.std(ddof=1)) <= 1e-12
    # |mean - y|^2 <= mean_k |x_k - y|^2 in exact arithmetic (convexity), per utterance; the mean is rounded to fp32 once, which moves
    # its numerator by at most ~2^-24 relative to the terms it is made of: 1e-6 relative is allowed for that rounding
    got, bound = sc["x"]["per_utt"][:, 0].cpu().numpy(), np.mean(nums, axis=0)
    print("numerators: mean", got, "mean of members", bound, "loss_by_member", lbm, "relative_spread", ens["relative_spread"].tolist())
    assert np.all(got <= bound * (1 + 1e-6))
    assert np.isfinite(ens["relative_spread"].cpu().numpy()).all() and (ens["relative_spread"] > 0).all()
    with pytest.raises(ValueError, match="exact=True, members=4"):
        t.validate_batch(noisy, clean, exact=True, members=K)


def test_cli_generate_members(L, weights, tmp_path, monkeypatch):
    main, wavio, tr = pkg("main"), pkg("wavio"), pkg("trainer")
    os.makedirs(str(tmp_path / "conf"))
    os.makedirs(str(tmp_path / "noisy"))
    with open(str(tmp_path / "conf" / "diff.yml"), "w") as f:
        f.write("model:\n  name: GCRN\ntrain:\n  fft_num: 320\n  win_size: 320\n  win_shift: 160\n  feat_type: sqrt\n  batch_size: 2\n")
    for i, n in enumerate((1600, 1121)):
        wavio.write_wav(str(tmp_path / "noisy" / ("f%d.wav" % i)), 0.05 * seeded((n,), 500 + i).numpy())
    monkeypatch.chdir(tmp_path)

    class Synthetic(tr.ComplexDDPMTrainer):
        def __init__(self, args, config):
            super().__init__(args, config, device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights("DiffUNet1"))

    monkeypatch.setattr(tr, "ComplexDDPMTrainer", Synthetic)
    runs = []
    for tag in ("a", "b"):
        assets = tmp_path / ("assets_" + tag)
        written = main.main(["--assets", str(assets), "--generate", "--members", "2", "--data", str(tmp_path / "noisy"), "--seed", "9"])
        assert [os.path.basename(w) for w in written] == ["f0.wav", "f1.wav"] and all(os.path.isfile(w) for w in written)
        with open(str(assets / "log" / "diff" / "ensemble.json")) as f:
            report = json.load(f)
        assert report["members"] == 2 and sorted(report["files"]) == ["f0.wav", "f1.wav"]
        for row in report["files"].values():
            assert np.isfinite(row["relative_spread"]) and row["relative_spread"] > 0 and row["medoid"] in (0, 1)
        runs.append(([open(w, "rb").read() for w in written], report))
    assert runs[0] == runs[1]                                                 # a seeded rerun: identical bytes
