"""GPU: the denoising objective - csrc/objective.hip behind ops.noising / ops.sigma_loss, the objective plan of SamplerPipeline,
ComplexDDPMTrainer.objective_batch / objective and ``main.py --eval --objective``.

Tolerances.  noisy / target: bit for bit against the reference's statements (tests/golden/objective_step.npz) and against the
numpy restatement (tests/helpers/objective_refs.py).  Numerators against numpy: the fp32 element terms are evaluated by numpy
exactly as the kernels state them and added in float64; only the order of the double additions differs, N <= 1e4 terms of one
sign, so the relative distance is bounded by N * 2^-53 ~ 1.1e-12: 1e-12, as tests/test_gpu_valid.py derives it.  The fp32 loss
is that double rounded once: 2^-24 = 6e-8, 1.2e-7 with the numerator's share.  Against the reference's fp32 sums: four times the
distance the fixture's tool measured between them and the float64 sums (``f64_distance``)."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from conftest import golden, pkg, rel_l2, seeded
from helpers import objective_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS3 = (1600, 1121, 801)
LENS5 = (1600, 1121, 801, 1440, 961)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


@pytest.fixture(scope="module")
def g():
    return golden("objective_step")


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays)


def _distance(g, key):
    return float(g["f64_distance"][[str(k) for k in g["f64_distance_keys"]].index(key)])


# ---------------------------------------------------------------- ops.noising
@pytest.mark.parametrize("sigma", (False, True))
@pytest.mark.parametrize("mode", R.MODES)
def test_noising_vs_reference_fixture_bit_exact(L, g, mode, sigma):
    ops = pkg("ops")
    label, init, noise, _ = R.inputs()
    dl, di, dn = _dev(label, init, noise)
    noisy, target, maxbuf = ops.noising(dl, di, torch.tensor(R.STEPS), dn, mode=mode, sigma=sigma)
    assert np.array_equal(noisy.cpu().numpy(), g[R.case_key(mode, sigma) + "_noisy"])
    assert np.array_equal(target.cpu().numpy(), g["target_sigma"] if sigma else noise)
    want_max = np.abs(init).reshape(6, -1).max(axis=1) if sigma else np.zeros(6, dtype=np.float32)
    assert np.array_equal(maxbuf.cpu().numpy(), want_max)            # utterance 1: the maximum of a padding frame
    old = ops.q_sample(dl, di, torch.tensor(R.STEPS), dn, mode=mode, sigma=sigma)
    assert torch.equal(noisy, old)
    again = ops.noising(dl, di, torch.tensor(R.STEPS, device=DEV), dn, mode=mode, sigma=sigma)      # t on the device: the same bits
    assert all(torch.equal(a, b) for a, b in zip(again, (noisy, target, maxbuf)))


@pytest.mark.parametrize("sigma", (False, True))
@pytest.mark.parametrize("mode", R.MODES)
def test_noising_small_planes_vs_helper(L, mode, sigma):
    """B = 2, T = 3, F = 7: planes of 21 elements - the vector path's tail, a quad across the channel boundary, planes that are
    not 16-byte aligned and the reduction of a plane smaller than a workgroup."""
    ops = pkg("ops")
    shape = (2, 2, 3, 7)
    label, init, noise = (seeded(shape, 60 + k).numpy() for k in range(3))
    t = [31, 2]
    noisy, target, maxbuf = ops.noising(*_dev(label, init), torch.tensor(t), *_dev(noise), mode=mode, sigma=sigma)
    want = R.noising(label, init, t, noise, mode, sigma)
    for got, ref in zip((noisy, target, maxbuf), want):
        assert np.array_equal(got.cpu().numpy(), ref)


def test_noising_argument_checks(L):
    ops = pkg("ops")
    z = torch.zeros(2, 2, 3, 7, device=DEV)
    for bad in ([0, 50], [-1, 0]):
        with pytest.raises(IndexError):
            ops.noising(z, z, torch.tensor(bad), z)
    with pytest.raises(ValueError):
        ops.noising(z, z, torch.tensor([0, 1, 2]), z)
    with pytest.raises(ValueError):
        ops.noising(z, z, torch.tensor([0, 1]), z, mode="ours")
    with pytest.raises(ValueError):
        ops.noising(z, z[:, :, :2], torch.tensor([0, 1]), z)


# ---------------------------------------------------------------- ops.sigma_loss
@pytest.mark.parametrize("frames", (R.FRAMES, (5, 0, 2)))
def test_sigma_loss_vs_float64_and_reference(L, g, frames):
    ops = pkg("ops")
    label, init, noise, predicted = R.inputs()
    _, target, maxbuf = R.noising(label, init, R.STEPS, noise, "pirorgrad", True)
    args = _dev(predicted, target, init, maxbuf)
    got, again = ops.sigma_loss(*args, frames), ops.sigma_loss(*args, frames)
    per, loss = R.sigma_loss(predicted, target, init, maxbuf, frames)
    gp = got["per_utt"].cpu().numpy()
    print("per_utt", gp, per, "loss", float(got["com_mse_sigma"]), loss)
    assert gp.shape == (3,) and got["per_utt"].dtype == torch.float64
    assert np.all(np.abs(gp - per) <= 1e-12 * np.abs(per)) and (frames[1] or gp[1] == 0.0)
    assert got["com_mse_sigma"].dim() == 0 and got["com_mse_sigma"].dtype == torch.float32
    assert abs(float(got["com_mse_sigma"]) - loss) <= 1.2e-7 * loss
    assert torch.equal(got["per_utt"], again["per_utt"]) and torch.equal(got["com_mse_sigma"], again["com_mse_sigma"])
    if frames == R.FRAMES:
        key = "pirorgrad_sigma_com_mse_sigma"
        want, allow = float(g[key]), 4 * _distance(g, key)
        print("reference", want, "distance", abs(float(got["com_mse_sigma"]) - want) / want, "allowed", allow)
        assert abs(float(got["com_mse_sigma"]) - want) <= allow * want


def test_sigma_loss_small_planes_and_empty_batch(L):
    ops = pkg("ops")
    shape = (2, 2, 3, 7)
    predicted, target, init = (seeded(shape, 70 + k).numpy() for k in range(3))
    _, maxbuf = R.mask_of(init)
    got = ops.sigma_loss(*_dev(predicted, target, init, maxbuf), [3, 2])
    per, loss = R.sigma_loss(predicted, target, init, maxbuf, [3, 2])
    assert np.all(np.abs(got["per_utt"].cpu().numpy() - per) <= 1e-12 * np.abs(per))
    assert abs(float(got["com_mse_sigma"]) - loss) <= 1.2e-7 * loss
    z = torch.zeros(2, 2, 4, 161, device=DEV)
    with pytest.raises(ValueError, match="no frame"):
        ops.sigma_loss(z, z, z, torch.ones(4, device=DEV), [0, 0])
    with pytest.raises(ValueError):
        ops.sigma_loss(z, z, z, torch.ones(4, device=DEV), [5, 1])
    with pytest.raises(ValueError, match="maxbuf"):
        ops.sigma_loss(z, z, z, torch.ones(3, device=DEV), [1, 1])


def test_fixture_plain_losses_through_spec_losses(L, g):
    """The losses without --sigma need no new kernel: ops.spec_losses on (predicted, noise) against the reference's values."""
    ops = pkg("ops")
    _, _, noise, predicted = R.inputs()
    got = ops.spec_losses(*_dev(predicted, noise), list(R.FRAMES))
    for name in ("com_mse", "com_mag_mse"):
        key = "pirorgrad_plain_" + name
        want, allow = float(g[key]), 4 * _distance(g, key)
        print(name, float(got[name]), want, abs(float(got[name]) - want) / want, "allowed", allow)
        assert abs(float(got[name]) - want) <= allow * want


# ---------------------------------------------------------------- objective_batch
def _trainer(weights, tmp_path, sigma=False, exclusive=False, params=None, ddpm="DiffUNet1", loss=None, **kw):
    args = argparse.Namespace(retrain=False, joint=True, draw=False, sigma=sigma, checkpoint=str(tmp_path / "ck"),
                              generated_wav=str(tmp_path / "out"))
    train = argparse.Namespace(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt", batch_size=2)
    if loss:
        train.loss = loss
    config = argparse.Namespace(model=argparse.Namespace(name="GCRN"), train=train)
    return pkg("trainer").ComplexDDPMTrainer(args, config, device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights(ddpm),
                                             exclusive=exclusive, params=params, **kw)


def _pairs3():
    clean = [0.05 * seeded((n,), 500 + i) for i, n in enumerate(LENS3)]
    return [c + 0.02 * seeded((c.numel(),), 510 + i) for i, c in enumerate(clean)], clean


T3 = 1 + max(LENS3) // 160
STEPS = torch.tensor(R.STEPS)


def _check_losses(sc, sigma, frames):
    """The scores of a pass against the helper's evaluation on the pass's own predicted and target."""
    p, tg, init = (sc[k].cpu().numpy() for k in ("predicted", "target", "init"))
    if sigma:
        per, loss = R.sigma_loss(p, tg, init, R.mask_of(init)[1], frames)
        losses = (loss,)
    else:
        per, losses = R.spec_losses(p, tg, frames)
    gp = sc["ddpm"]["per_utt"].cpu().numpy()
    print("per_utt", gp, per, "loss", sc["ddpm"]["loss"].cpu().numpy(), losses)
    assert np.all(np.abs(gp - per) <= 1e-12 * np.abs(per))
    for got, want in zip(sc["ddpm"]["loss"].cpu().numpy(), losses):
        assert abs(float(got) - want) <= 1.2e-7 * want


def test_objective_batch_pirorgrad(L, weights, tmp_path):
    t = _trainer(weights, tmp_path)
    noisy, clean = _pairs3()
    noise = seeded((3, 2, T3, 161), 520)
    sc = t.objective_batch(noisy, clean, t=STEPS, noise=noise, tensors=True)
    frames = [n // 160 + 1 for n in LENS3]
    assert sc["frames"] == frames and sc["t"].cpu().tolist() == list(R.STEPS) and sc["t"].dtype == torch.int32
    # the noising of the pass: the helper on the pass's own label and init
    want = R.noising(sc["label"].cpu().numpy(), sc["init"].cpu().numpy(), R.STEPS, noise.numpy(), "pirorgrad", False)
    assert np.array_equal(sc["noisy"].cpu().numpy(), want[0]) and torch.equal(sc["target"].cpu(), noise)
    # one recorded step of the plan = the operator, built by the same plan builder
    eps = t.model_ddpm(sc["noisy"], sc["init"], STEPS.to(DEV))
    assert torch.equal(sc["predicted"], eps)
    _check_losses(sc, False, frames)
    # dis: the prior against the label before the division by 11 - validate_batch's "init" losses
    _, val = t.validate_batch(noisy, clean, x_T=seeded((3, 2, T3, 161), 521))
    assert torch.equal(sc["dis"]["loss"], val["init"]["loss"]) and torch.equal(sc["dis"]["per_utt"], val["init"]["per_utt"])
    # a default (exclusive) trainer: the project's 1e-4
    d = _trainer(weights, tmp_path, exclusive=None).objective_batch(noisy, clean, t=STEPS, noise=noise, tensors=True)
    assert rel_l2(d["predicted"].cpu(), sc["predicted"].cpu()) < 1e-4
    with pytest.raises(IndexError):
        t.objective_batch(noisy, clean, t=torch.tensor([0, 50, 1]), noise=noise)
    with pytest.raises(NotImplementedError):
        t.train_step(None)


def test_objective_batch_sigma_and_other_parameterisations(L, weights, tmp_path):
    noisy, clean = _pairs3()
    noise = seeded((3, 2, T3, 161), 520)
    frames = [n // 160 + 1 for n in LENS3]
    base = _trainer(weights, tmp_path).objective_batch(noisy, clean, t=STEPS, noise=noise, tensors=True)
    sig = _trainer(weights, tmp_path, sigma=True).objective_batch(noisy, clean, t=STEPS, noise=noise, tensors=True)
    assert not torch.equal(sig["target"].cpu(), noise) and sig["ddpm"]["loss"].shape == (1,) and sig["ddpm"]["per_utt"].shape == (3,)
    want = R.noising(sig["label"].cpu().numpy(), sig["init"].cpu().numpy(), R.STEPS, noise.numpy(), "pirorgrad", True)
    assert np.array_equal(sig["noisy"].cpu().numpy(), want[0]) and np.array_equal(sig["target"].cpu().numpy(), want[1])
    _check_losses(sig, True, frames)
    prm = pkg("params").params
    delta_p = dict(prm, pirorgrad=False, deltamu=True)
    feat_p = dict(prm, pirorgrad=False, deltamu=False)
    AttrDict = type(prm)
    for name, p, ddpm, mode in (("deltamu", AttrDict(delta_p), "Nocon", "deltamu"), ("feat", AttrDict(feat_p), "DiffUNet1", "plain")):
        tr = _trainer(weights, tmp_path, params=p, ddpm=ddpm)
        sc = tr.objective_batch(noisy, clean, t=STEPS, noise=noise, tensors=True)
        want = R.noising(sc["label"].cpu().numpy(), sc["init"].cpu().numpy(), R.STEPS, noise.numpy(), mode, False)
        assert np.array_equal(sc["noisy"].cpu().numpy(), want[0]), name
        assert torch.equal(sc["init"], base["init"]) and torch.equal(sc["label"], base["label"])          # the shared front
        assert not torch.equal(sc["noisy"], base["noisy"]) and not torch.equal(sc["predicted"], base["predicted"]), name
        assert bool(torch.isfinite(sc["predicted"]).all())
        _check_losses(sc, False, frames)


# ---------------------------------------------------------------- the epoch and the CLI
@pytest.fixture(scope="module")
def pairs_dir(tmp_path_factory):
    root = tmp_path_factory.mktemp("objective_pairs")
    wavio = pkg("wavio")
    for sub in ("noisy", "clean"):
        os.makedirs(str(root / sub))
    for i, n in enumerate(LENS5):
        clean = 0.05 * seeded((n,), 600 + i).numpy()
        wavio.write_wav(str(root / "clean" / ("p%d.wav" % i)), clean)
        wavio.write_wav(str(root / "noisy" / ("p%d.wav" % i)), clean + 0.02 * seeded((n,), 610 + i).numpy())
    return root


def test_objective_epoch_seeded_equals_explicit(L, weights, tmp_path, pairs_dir):
    t = _trainer(weights, tmp_path, loss="com_mse_loss")
    dirs = (str(pairs_dir / "noisy"), str(pairs_dir / "clean"))
    torch.manual_seed(11)
    torch.cuda.manual_seed_all(11)
    res = t.objective(*dirs, draws=2)
    torch.manual_seed(11)
    torch.cuda.manual_seed_all(11)
    ts, ns = [], []
    for k in range(0, 5, 2):
        part = LENS5[k:k + 2]
        for _ in range(2):
            ts.append(torch.randint(0, 50, [len(part)], device=DEV))
            ns.append(torch.randn(len(part), 2, 1 + max(part) // 160, 161, device=DEV))
    given = t.objective(*dirs, draws=2, t=ts, noise=ns)
    assert given == res
    assert res["batches"] == 6 and sum(r["count"] for r in res["by_step"]) == 10 and len(res["by_step"]) == 50
    assert [f["name"] for f in res["files"]] == ["p%d.wav" % i for i in range(5)] and all(len(f["draws"]) == 2 for f in res["files"])
    assert [d["t"] for f in res["files"][:2] for d in f["draws"]] == [int(ts[0][0]), int(ts[1][0]), int(ts[0][1]), int(ts[1][1])]
    # ddpm_loss: the mean of the six evaluations' com_mse
    losses = []
    at = 0
    for k in range(0, 5, 2):
        idx = list(range(k, min(k + 2, 5)))
        wavio = pkg("wavio")
        noisy = [torch.from_numpy(wavio.read_wav(str(pairs_dir / "noisy" / ("p%d.wav" % i))).astype(np.float32)) for i in idx]
        clean = [torch.from_numpy(wavio.read_wav(str(pairs_dir / "clean" / ("p%d.wav" % i))).astype(np.float32)) for i in idx]
        for _ in range(2):
            losses.append(float(t.objective_batch(noisy, clean, t=ts[at], noise=ns[at])["ddpm"]["loss"][0]))
            at += 1
    assert res["ddpm_loss"] == float(np.mean(losses)) and res["loss"] == "com_mse_loss"
    assert res["loss_sum"] == res["ddpm_loss"] + res["dis_loss"] and np.isfinite(res["ddpm_loss_per_frame"])


def test_cli_eval_objective_writes_json(L, weights, tmp_path, pairs_dir, monkeypatch):
    main = pkg("main")
    os.makedirs(str(tmp_path / "conf"))
    with open(str(tmp_path / "conf" / "diff.yml"), "w") as f:
        f.write("model:\n  name: GCRN\ntrain:\n  fft_num: 320\n  win_size: 320\n  win_shift: 160\n  feat_type: sqrt\n  batch_size: 2\n"
                "  lam: 0.5\n")
    monkeypatch.chdir(tmp_path)
    tr = pkg("trainer")
    made = []

    class Synthetic(tr.ComplexDDPMTrainer):
        def __init__(self, args, config):
            super().__init__(args, config, device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights("DiffUNet1"))
            made.append(self)

    monkeypatch.setattr(tr, "ComplexDDPMTrainer", Synthetic)
    argv = ["--assets", str(tmp_path / "assets"), "--eval", "--objective", "--draws", "2", "--sigma", "--data", str(pairs_dir / "noisy"),
            "--clean", str(pairs_dir / "clean"), "--seed", "77"]
    res = main.main(argv)
    with open(str(tmp_path / "assets" / "log" / "diff" / "objective.json")) as f:
        disk = json.load(f)
    assert disk == res and not os.path.exists(str(tmp_path / "assets" / "log" / "diff" / "eval.json"))
    assert disk["loss"] == "com_mse_sigma_loss" and disk["dis_loss_name"] == "com_mag_mse_loss" and disk["batches"] == 6
    assert disk["loss_sum"] == 0.5 * disk["ddpm_loss"] and disk["joint"] is False and len(disk["files"]) == 5       # no --joint: dis_loss reported only
    assert sum(r["count"] for r in disk["by_step"]) == 10 and np.isfinite(disk["ddpm_loss"]) and np.isfinite(disk["dis_loss"])
    torch.manual_seed(77)
    torch.cuda.manual_seed_all(77)
    again = made[0].objective(str(pairs_dir / "noisy"), str(pairs_dir / "clean"), draws=2)
    assert again["ddpm_loss"] == res["ddpm_loss"] and again["by_step"] == res["by_step"]
