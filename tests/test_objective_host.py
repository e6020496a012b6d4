"""CPU: the host side of the denoising-objective epoch - aggregation (objective.py), the draw order of
``ComplexDDPMTrainer.objective`` on a stubbed trainer, the CLI's ``--eval --objective --draws``, the two new exports and the
argument checks of pdse_objective_noise / pdse_sigma_loss, which need no device."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import pkg

F = 161


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def _eval(names, frames, t, seed, sigma=False):
    """One hand-made (batch, draw) evaluation in the layout ``_collect_objective`` hands to ``aggregate``."""
    rng = np.random.default_rng(seed)
    n = float(sum(frames)) * F

    def spec():
        per = rng.uniform(1.0, 50.0, (len(names), 2))
        com, mag = per[:, 0].sum() / (2 * n), per[:, 1].sum() / n
        return {"loss": np.array([com, mag, 0.5 * (com + mag)]), "per_utt": per}

    ddpm = spec()
    if sigma:
        per = rng.uniform(1.0, 50.0, len(names))
        ddpm = {"loss": np.array([per.sum() / (2 * n)]), "per_utt": per}
    return {"names": names, "frames": frames, "t": t, "ddpm": ddpm, "dis": spec()}


NAMES = ["a", "b", "c", "d", "e"]


def _epoch(sigma=False):
    return [_eval([0, 1], [11, 8], [3, 49], 1, sigma), _eval([0, 1], [11, 8], [3, 0], 2, sigma),
            _eval([2, 3], [6, 16], [17, 3], 3, sigma), _eval([2, 3], [6, 16], [0, 0], 4, sigma),
            _eval([4], [7], [49], 5, sigma), _eval([4], [7], [20], 6, sigma)]


@pytest.mark.parametrize("loss,k", (("com_mse_loss", 0), ("mag_mse_loss", 1), ("com_mag_mse_loss", 2)))
def test_aggregation_batch_means_against_per_frame(loss, k):
    O = pkg("objective")
    ev = _epoch()
    res = O.aggregate(ev, NAMES, 50, loss=loss, joint=True)
    assert res["ddpm_loss"] == pytest.approx(np.mean([b["ddpm"]["loss"][k] for b in ev]), rel=1e-15)
    assert res["dis_loss"] == pytest.approx(np.mean([b["dis"]["loss"][k] for b in ev]), rel=1e-15)
    frames = sum(sum(b["frames"]) for b in ev)
    for sec, key in (("ddpm", "ddpm_loss_per_frame"), ("dis", "dis_loss_per_frame")):
        num = np.sum([b[sec]["per_utt"].sum(0) for b in ev], axis=0)
        per_frame = (num[0] / (2 * F * frames), num[1] / (F * frames))
        per_frame += (0.5 * (per_frame[0] + per_frame[1]),)
        assert res[key] == pytest.approx(per_frame[k], rel=1e-14)
    assert res["ddpm_loss"] != pytest.approx(res["ddpm_loss_per_frame"], rel=1e-6)          # unequal batches: the two differ
    assert res["batches"] == 6 and res["loss"] == loss


def test_by_step_counts_sums_and_empty_steps():
    O = pkg("objective")
    ev = _epoch()
    res = O.aggregate(ev, NAMES, 50, loss="com_mse_loss")
    rows = res["by_step"]
    assert [r["t"] for r in rows] == list(range(50)) and sum(r["count"] for r in rows) == 10
    assert {r["t"]: r["count"] for r in rows if r["count"]} == {0: 3, 3: 3, 17: 1, 20: 1, 49: 2}
    assert all(r["per_frame"] is None and r["num"] == 0.0 and r["frames"] == 0 for r in rows if not r["count"])
    # t = 3: utterance a in both draws of batch 0, utterance d in the first draw of batch 1
    num = ev[0]["ddpm"]["per_utt"][0, 0] + ev[1]["ddpm"]["per_utt"][0, 0] + ev[2]["ddpm"]["per_utt"][1, 0]
    assert rows[3]["num"] == pytest.approx(num, rel=1e-15) and rows[3]["frames"] == 11 + 11 + 16
    assert rows[3]["per_frame"] == pytest.approx(num / (2 * F * 38), rel=1e-15)
    assert sum(r["num"] for r in rows) / (2 * F * sum(r["frames"] for r in rows)) == pytest.approx(res["ddpm_loss_per_frame"], rel=1e-14)
    files = res["files"]
    assert [f["name"] for f in files] == NAMES and [f["frames"] for f in files] == [11, 8, 6, 16, 7]
    assert all(len(f["draws"]) == 2 for f in files)
    assert files[3]["draws"] == [{"t": 3, "num": ev[2]["ddpm"]["per_utt"][1, 0]}, {"t": 0, "num": ev[3]["ddpm"]["per_utt"][1, 0]}]
    with pytest.raises(ValueError, match="outside"):
        O.aggregate([_eval([0], [5], [50], 1)], NAMES, 50)
    with pytest.raises(ValueError):
        O.aggregate([], NAMES, 50)


def test_sigma_joint_lam_and_loss_names():
    O = pkg("objective")
    ev = _epoch(sigma=True)
    res = O.aggregate(ev, NAMES, 50, loss="com_mag_mse_loss", sigma=True, lam=0.25, joint=True)
    ddpm = np.mean([b["ddpm"]["loss"][0] for b in ev])
    dis = np.mean([b["dis"]["loss"][2] for b in ev])
    assert res["ddpm_loss"] == pytest.approx(ddpm, rel=1e-15) and res["dis_loss"] == pytest.approx(dis, rel=1e-15)
    assert res["loss_sum"] == pytest.approx(0.25 * ddpm + dis, rel=1e-15) and res["loss"] == "com_mse_sigma_loss"
    num = sum(b["ddpm"]["per_utt"].sum() for b in ev)
    assert res["ddpm_loss_per_frame"] == pytest.approx(num / (2 * F * sum(sum(b["frames"]) for b in ev)), rel=1e-14)
    off = O.aggregate(ev, NAMES, 50, loss="com_mag_mse_loss", sigma=True, lam=0.25, joint=False)
    assert off["dis_loss"] == res["dis_loss"] and off["loss_sum"] == pytest.approx(0.25 * ddpm, rel=1e-15)     # reported, not summed
    assert O.aggregate(ev, NAMES, 50, sigma=True)["loss_sum"] == pytest.approx(ddpm, rel=1e-15)                # lam 1.0, no joint
    with pytest.raises(ValueError, match="pesq_loss"):
        O.aggregate(ev, NAMES, 50, loss="pesq_loss")
    train = argparse.Namespace
    assert O.loss_name(train(train=train(loss="mag_mse_loss"))) == "mag_mse_loss"
    assert O.loss_name(train(train=train())) == "com_mag_mse_loss" == O.loss_name(train())
    with pytest.raises(ValueError, match="mag_mae_loss"):
        O.loss_name(train(train=train(loss="mag_mae_loss")))
    line = O.log_line(res)
    assert "\n" not in line and line.startswith("dis_loss ") and " ddpm_loss " in line and " loss_sum " in line and "5/50" in line


def test_draw_order_randint_before_randn_per_batch_and_draw(monkeypatch):
    """``objective`` on a stubbed trainer: per batch, per draw, one ``torch.randint`` of [B] and then one ``torch.randn`` of the
    batch's label shape (trainer/complex_ddpm_trainer.py:707, :711); with t and noise handed in nothing is drawn."""
    tr_mod = pkg("trainer")
    lens = [1600, 1121, 801, 2400, 961]
    calls, runs = [], []

    class Stub(tr_mod.ComplexDDPMTrainer):
        def __init__(self, lam=None):
            self.device, self.params = torch.device("cpu"), pkg("params").params
            self.args = argparse.Namespace(sigma=False, joint=False)
            self.config = argparse.Namespace(train=argparse.Namespace(batch_size=2, loss="com_mse_loss", **({} if lam is None else {"lam": lam})))

        def _pair_epoch(self, noisy_dir, clean_dir, batch_size, order, drop_last):
            assert (noisy_dir, clean_dir, batch_size, order, drop_last) == ("n", "c", None, "sorted", False)
            return (["p%d.wav" % i for i in range(5)], [[0, 1], [2, 3], [4]],
                    lambda idx: ([torch.ones(lens[i]) for i in idx], [torch.ones(lens[i]) for i in idx]))

        def _objective_run(self, noisy, clean, lens_, frames, t, noise, tensors):
            B = len(noisy)
            runs.append((lens_, frames, t, noise))
            calls.append(("run", B))
            spec = {"loss": torch.tensor([2.0, 4.0, 3.0]), "per_utt": torch.ones(B, 2, dtype=torch.float64)}
            return {"frames": frames, "t": torch.as_tensor(t).to(torch.int32), "ddpm": spec, "dis": spec}

    monkeypatch.setattr(torch, "randint", lambda lo, hi, shape, **kw: calls.append(("randint", lo, hi, tuple(shape))) or torch.full(shape, 7))
    monkeypatch.setattr(torch, "randn", lambda *shape, **kw: calls.append(("randn", tuple(shape))) or torch.zeros(1))
    res = Stub().objective("n", "c", draws=2)
    want = []
    for idx in ([0, 1], [2, 3], [4]):
        T = 1 + max(lens[i] for i in idx) // 160
        want += [("randint", 0, 50, (len(idx),)), ("randn", (len(idx), 2, T, 161)), ("run", len(idx))] * 2
    assert calls == want
    assert [r[1] for r in runs[::2]] == [[11, 8], [6, 16], [7]]
    assert res["ddpm_loss"] == 2.0 and res["by_step"][7]["count"] == 10 and res["loss_sum"] == 2.0 and all(len(f["draws"]) == 2 for f in res["files"])
    assert Stub(lam=0.5).objective("n", "c")["loss_sum"] == 1.0 and Stub().objective("n", "c", lam=3.0)["loss_sum"] == 6.0
    del calls[:], runs[:]
    ts = [torch.tensor([k] * n) for k, n in enumerate((2, 2, 1))]
    ns = [torch.zeros(1)] * 3
    given = Stub().objective("n", "c", t=ts, noise=ns)
    assert calls == [("run", 2), ("run", 2), ("run", 1)] and all(r[2] is ts[k] and r[3] is ns[k] for k, r in enumerate(runs))
    assert [given["by_step"][k]["count"] for k in range(3)] == [2, 2, 1]
    with pytest.raises(ValueError, match="one entry per"):
        Stub().objective("n", "c", draws=2, t=ts)
    with pytest.raises(ValueError, match="draws"):
        Stub().objective("n", "c", draws=0)


def test_cli_parses_objective_and_draws(tmp_path, monkeypatch, capsys):
    os.makedirs(str(tmp_path / "conf"))
    with open(str(tmp_path / "conf" / "diff.yml"), "w") as f:
        f.write("model:\n  name: GCRN\ntrain:\n  batch_size: 8\n")
    monkeypatch.chdir(tmp_path)
    main = pkg("main")
    base = ["--assets", str(tmp_path / "a")]
    args, _ = main.parse_args_and_config(base + ["--eval", "--objective", "--draws", "3", "--batch", "4"])
    assert args.eval and args.objective and args.draws == 3 and args.eval_batch == 4
    args, _ = main.parse_args_and_config(base + ["--eval"])
    assert args.eval and not args.objective and args.draws == 1                  # --eval alone is unchanged
    for bad in (["--objective"], ["--objective", "--generate"], ["--eval", "--objective", "--draws", "0"]):
        with pytest.raises(SystemExit):
            main.parse_args_and_config(base + bad)
    assert "--objective" in capsys.readouterr().err


def test_train_ddpm_routes_objective_and_still_refuses_training():
    tr = pkg("trainer").ComplexDDPMTrainer
    t = tr.__new__(tr)
    seen = {}
    row = {"t": 0, "count": 1, "num": 1.0, "frames": 5, "per_frame": 1.0}
    res = {"dis_loss": 1.0, "ddpm_loss": 2.0, "loss_sum": 3.0, "ddpm_loss_per_frame": 2.0, "by_step": [row], "loss": "com_mse_loss"}
    t.objective = lambda **kw: seen.update(kw) or res
    t.args = argparse.Namespace(eval=True, objective=True, draws=4, data="n", clean="c", eval_batch=2)
    assert t.train_ddpm() is res and seen == {"draws": 4, "noisy_dir": "n", "clean_dir": "c", "batch_size": 2}
    t.args = argparse.Namespace(eval=False, objective=True)
    with pytest.raises(NotImplementedError):
        t.train_ddpm()


def test_exports_and_abi_version(lib):
    assert "pdse_objective_noise" in lib.EXPORTS and "pdse_sigma_loss" in lib.EXPORTS and lib.ABI_VERSION == 9
    handle = lib.load()
    assert handle.pdse_abi_version() == 9 and hasattr(handle, "pdse_objective_noise") and hasattr(handle, "pdse_sigma_loss")


def test_entry_points_validate_without_a_device(lib):
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    good = dict(label=p, init=p, noise=p, t=p, a_tab=p, s_tab=p, noisy=p, target=p, maxbuf=p, B=2, T=4, F=161, mode=0, sigma=1)
    for name in ("label", "init", "noise", "t", "a_tab", "s_tab", "noisy", "target", "maxbuf"):
        with pytest.raises(lib.PdseError, match="objective_noise: null"):
            lib.objective_noise(**dict(good, **{name: 0}))
    for bad in (dict(B=0), dict(B=-1), dict(T=0), dict(F=0), dict(B=32768)):
        with pytest.raises(lib.PdseError, match="objective_noise: bad sizes"):
            lib.objective_noise(**dict(good, **bad))
    for bad in (dict(mode=-1), dict(mode=3)):
        with pytest.raises(lib.PdseError, match="objective_noise: mode"):
            lib.objective_noise(**dict(good, **bad))
    with pytest.raises(lib.PdseError, match="objective_noise: sigma"):
        lib.objective_noise(**dict(good, sigma=2))

    frames = (C.c_int32 * 2)(3, 4)
    good = dict(predicted=p, target=p, init=p, maxbuf=p, frames_host=C.addressof(frames), frames=p, partial=p, per_utt=p, loss=p,
                B=2, T=4, F=161)
    for name in ("predicted", "target", "init", "maxbuf", "frames_host", "frames", "partial", "per_utt", "loss"):
        with pytest.raises(lib.PdseError, match="sigma_loss: null"):
            lib.sigma_loss(**dict(good, **{name: 0}))
    for bad in (dict(B=0), dict(B=-3), dict(T=0), dict(F=0), dict(B=32768)):
        with pytest.raises(lib.PdseError, match="sigma_loss: bad sizes"):
            lib.sigma_loss(**dict(good, **bad))
    for values in ((5, 1), (-1, 2)):
        fr = (C.c_int32 * 2)(*values)
        with pytest.raises(lib.PdseError, match=r"frames outside \[0, T\]"):
            lib.sigma_loss(**dict(good, frames_host=C.addressof(fr)))
    fr = (C.c_int32 * 2)(0, 0)
    with pytest.raises(lib.PdseError, match="sum of frames is 0"):
        lib.sigma_loss(**dict(good, frames_host=C.addressof(fr)))


def test_ops_argument_checks_without_a_device():
    ops = pkg("ops")
    z = torch.zeros(2, 2, 4, 161)
    with pytest.raises(pkg("_lib").PdseError, match="GPU only"):
        ops.noising(z, z, torch.tensor([0, 1]), z)
    with pytest.raises(pkg("_lib").PdseError, match="GPU only"):
        ops.sigma_loss(z, z, z, torch.ones(4), [1, 1])
    a, s, steps = ops.noise_tables("cpu")
    assert steps == 50 and a.dtype == torch.float32 and a.shape == s.shape == (50,)
    with pytest.raises(ValueError, match="objective=True"):
        pkg("pipeline").SamplerPipeline.objective_pass(argparse.Namespace(objective=None), z, z, [0, 1], z)
    with pytest.raises(ValueError, match="objective plan"):
        pkg("pipeline").SamplerPipeline("cpu", "GCRN", None, None, 1, T=3, objective=True)
