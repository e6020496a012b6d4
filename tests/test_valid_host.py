"""CPU: the host side of the validation epoch - pairing, batching, frame arithmetic and aggregation (validation.py), the CLI's
``--eval --clean``, ``train_ddpm`` without ``args.eval``, and the argument checks of pdse_pair_prep / pdse_spec_losses, which need
no device."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import pkg


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def _touch(path):
    with open(str(path), "wb") as f:
        f.write(b"")


def test_pairing_by_name_and_missing_partner(tmp_path):
    V = pkg("validation")
    noisy, clean = tmp_path / "noisy", tmp_path / "clean"
    noisy.mkdir()
    clean.mkdir()
    for name in ("b.wav", "a.wav", "c.wav"):
        _touch(noisy / name)
        _touch(clean / name)
    _touch(clean / "extra.wav")                    # a clean file nobody asks for is not an error
    _touch(noisy / "notes.txt")
    pairs = V.pair_names(str(noisy), str(clean))
    assert [os.path.basename(p) for p, _ in pairs] == ["a.wav", "b.wav", "c.wav"]
    assert all(os.path.basename(p) == os.path.basename(c) and os.path.dirname(c) == str(clean) for p, c in pairs)
    _touch(noisy / "d.wav")
    with pytest.raises(ValueError, match="d.wav"):
        V.pair_names(str(noisy), str(clean))


def test_unequal_pair_names_the_file():
    V = pkg("validation")
    pairs = [("n/a.wav", "c/a.wav"), ("n/b.wav", "c/b.wav")]
    V.check_lengths(pairs, [1600, 801], [1600, 801])
    with pytest.raises(ValueError, match="n/b.wav holds 801 samples"):
        V.check_lengths(pairs, [1600, 801], [1600, 800])


def test_windows_sorted_drop_last_and_shuffled():
    V = pkg("validation")
    assert V.windows(5, 2) == [[0, 1], [2, 3], [4]]
    assert V.windows(5, 2, drop_last=True) == [[0, 1], [2, 3]]
    assert V.windows(4, 2, drop_last=True) == [[0, 1], [2, 3]]
    assert V.windows(1, 8, drop_last=True) == [] and V.windows(0, 3) == []
    torch.manual_seed(5)
    perm = torch.randperm(7).tolist()
    after = torch.rand(1)
    torch.manual_seed(5)
    got = V.windows(7, 3, order="shuffled")
    assert got == [perm[0:3], perm[3:6], perm[6:]] and torch.equal(torch.rand(1), after)      # exactly one randperm was consumed
    torch.manual_seed(5)
    V.windows(7, 3)
    assert torch.equal(torch.randperm(7), torch.tensor(perm))                                  # "sorted" draws nothing
    with pytest.raises(ValueError):
        V.windows(5, 0)
    with pytest.raises(ValueError):
        V.windows(5, 2, order="random")


def test_frame_num_and_trim():
    V = pkg("validation")
    for n, frames, cut in ((1600, 11, 1600), (1121, 8, 1120), (801, 6, 800), (961, 7, 960), (161, 2, 160), (159, 1, 0)):
        assert V.frame_num(n) == frames == (n - 320 + 320) // 160 + 1 and V.trim_len(n) == cut == (frames - 1) * 160


def _batch(names, frames, seed, prior=True):
    rng = np.random.default_rng(seed)
    F = 161

    def section():
        per = rng.uniform(1.0, 50.0, (len(names), 2))
        n = float(sum(frames)) * F
        com, mag = per[:, 0].sum() / (2 * n), per[:, 1].sum() / n
        d = {"loss": (com, mag, 0.5 * (com + mag)), "per_utt": per}
        for m in ("ssnr", "llr", "wss", "fwsnrseg", "stoi", "estoi"):
            d[m] = rng.uniform(0.0, 10.0, len(names))
        return d

    b = {"names": names, "frames": frames, "x": section()}
    if prior:
        b["init"] = section()
    return b


def test_aggregation_batch_means_against_per_frame():
    V = pkg("validation")
    names = ["a", "b", "c", "d", "e"]
    batches = [_batch([0, 1], [11, 8], 1), _batch([2, 3], [6, 16], 2), _batch([4], [7], 3)]
    res = V.aggregate(batches, names, F=161, prior=True, stoi=True)
    for sec, out in (("x", res), ("init", res["init"])):
        assert out["loss"] == pytest.approx(np.mean([b[sec]["loss"][0] for b in batches]), rel=1e-15)
        assert out["mag_mse"] == pytest.approx(np.mean([b[sec]["loss"][1] for b in batches]), rel=1e-15)
        assert out["com_mag_mse"] == pytest.approx(np.mean([b[sec]["loss"][2] for b in batches]), rel=1e-15)
        num = np.sum([b[sec]["per_utt"].sum(0) for b in batches], axis=0)
        fr = sum(sum(b["frames"]) for b in batches)
        assert out["loss_per_frame"] == pytest.approx(num[0] / (2 * 161 * fr), rel=1e-14)
        assert out["mag_mse_per_frame"] == pytest.approx(num[1] / (161 * fr), rel=1e-14)
        assert out["com_mag_mse_per_frame"] == pytest.approx(0.5 * (num[0] / (2 * 161 * fr) + num[1] / (161 * fr)), rel=1e-14)
        assert out["loss"] != pytest.approx(out["loss_per_frame"], rel=1e-6)            # unequal batches: the two differ
        for m in ("ssnr", "llr", "wss", "fwsnrseg", "stoi", "estoi"):
            assert out["mean_" + m] == pytest.approx(np.mean([b[sec][m].mean() for b in batches]), rel=1e-15)
            flat = np.concatenate([b[sec][m] for b in batches]).mean()
            assert out["mean_" + m] != pytest.approx(flat, rel=1e-9)                      # means of batch means, not of files
    assert [f["name"] for f in res["files"]] == names and res["batches"] == 3
    assert res["files"][3]["frames"] == 16 and res["files"][3]["com_num"] == batches[1]["x"]["per_utt"][1][0]
    assert res["files"][4]["init"]["wss"] == batches[2]["init"]["wss"][0]
    plain = V.aggregate([_batch([0, 1], [11, 8], 1, prior=False)], names, prior=False)
    assert "init" not in plain and "mean_stoi" not in plain and "init" not in plain["files"][0]
    with pytest.raises(ValueError):
        V.aggregate([], names)
    line = V.log_line(res)
    assert line.startswith("test_com_mse_loss ") and " test_mean_ssnr " in line and " test_com_mse_loss_init " in line
    assert line.index("test_mean_ssnr ") < line.index("test_com_mse_loss_init")


def test_cli_parses_eval_and_clean(tmp_path, monkeypatch):
    os.makedirs(str(tmp_path / "conf"))
    with open(str(tmp_path / "conf" / "diff.yml"), "w") as f:
        f.write("model:\n  name: GCRN\ntrain:\n  batch_size: 8\n")
    monkeypatch.chdir(tmp_path)
    main = pkg("main")
    args, config = main.parse_args_and_config(["--assets", str(tmp_path / "a"), "--eval", "--clean", "some/clean", "--data", "some/noisy"])
    assert args.eval is True and args.clean == "some/clean" and args.data == "some/noisy" and args.eval_batch is None
    assert args.generate is False and config.train.batch_size == 8
    args, _ = main.parse_args_and_config(["--assets", str(tmp_path / "a"), "--eval", "--batch", "4", "--masked-prior", "--all-wav",
                                          "--sigma", "--bf16", "--split", "bf16x3"])
    assert args.clean == "data/clean_testset_wav" and args.eval_batch == 4 and args.batch == 4
    assert args.masked_prior and args.all_wav and args.sigma and args.bf16 and args.split == "bf16x3"
    args, _ = main.parse_args_and_config(["--assets", str(tmp_path / "a"), "--eval", "--batch=1"])
    assert args.eval_batch == 1


def test_train_ddpm_without_eval_still_raises():
    tr = pkg("trainer").ComplexDDPMTrainer
    t = tr.__new__(tr)                                   # no device here: the methods under test read ``args`` only
    t.args = argparse.Namespace(eval=False)
    with pytest.raises(NotImplementedError):
        t.train_ddpm()
    t.args = argparse.Namespace()
    with pytest.raises(NotImplementedError):
        t.train_ddpm()
    for name in ("train", "train_step", "draw_audio"):
        t.args = argparse.Namespace(eval=True)
        with pytest.raises(NotImplementedError):
            getattr(t, name)()


def test_entry_points_validate_without_a_device(lib):
    buf = (C.c_float * 4096)()
    p = C.addressof(buf)
    lens = (C.c_int32 * 2)(400, 300)
    lp = C.addressof(lens)
    good = dict(noisy=p, clean=p, lens=lp, noisy_pad=p, clean_pad=p, c=p, B=2, L=400, pad=160, reflect_own=0)
    for name in ("noisy", "clean", "lens", "noisy_pad", "clean_pad", "c"):
        with pytest.raises(lib.PdseError, match="pair_prep: null"):
            lib.pair_prep(**dict(good, **{name: 0}))
    for bad in (dict(B=0), dict(B=-1), dict(L=0), dict(pad=-1)):
        with pytest.raises(lib.PdseError, match="pair_prep: bad sizes"):
            lib.pair_prep(**dict(good, **bad))
    with pytest.raises(lib.PdseError, match="pad < L"):
        lib.pair_prep(**dict(good, L=160))
    with pytest.raises(lib.PdseError, match="reflect_own"):
        lib.pair_prep(**dict(good, reflect_own=2))

    frames = (C.c_int32 * 2)(3, 4)
    fp = C.addressof(frames)
    good = dict(esti=p, label=p, frames_host=fp, frames=p, partial=p, per_utt=p, loss=p, B=2, T=4, F=161)
    for name in ("esti", "label", "frames_host", "frames", "partial", "per_utt", "loss"):
        with pytest.raises(lib.PdseError, match="spec_losses: null"):
            lib.spec_losses(**dict(good, **{name: 0}))
    for bad in (dict(B=0), dict(B=-3), dict(T=0), dict(F=0), dict(B=65536)):
        with pytest.raises(lib.PdseError, match="spec_losses: bad sizes"):
            lib.spec_losses(**dict(good, **bad))
    for values in ((5, 1), (-1, 2)):
        fr = (C.c_int32 * 2)(*values)
        with pytest.raises(lib.PdseError, match=r"frames outside \[0, T\]"):
            lib.spec_losses(**dict(good, frames_host=C.addressof(fr)))
    fr = (C.c_int32 * 2)(0, 0)
    with pytest.raises(lib.PdseError, match="sum of frames is 0"):
        lib.spec_losses(**dict(good, frames_host=C.addressof(fr)))


def test_spec_frames_validates_without_a_device(lib):
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    good = dict(spec=p, basis=p, frames=p, B=1, T=2, F=161)
    for name in ("spec", "basis", "frames"):
        with pytest.raises(lib.PdseError, match="spec_frames: null"):
            lib.spec_frames(**dict(good, **{name: 0}))
    for bad in (dict(B=0), dict(T=0), dict(B=65536)):
        with pytest.raises(lib.PdseError, match="spec_frames: bad sizes"):
            lib.spec_frames(**dict(good, **bad))
    with pytest.raises(lib.PdseError, match="F must be 161"):
        lib.spec_frames(**dict(good, F=129))
    with pytest.raises(lib.PdseError, match="GPU only"):
        pkg("ops").spec_to_wav(torch.zeros(1, 2, 3, 161))


def test_ops_argument_checks_without_a_device():
    ops = pkg("ops")
    z = torch.zeros(2, 2, 4, 161)
    with pytest.raises(pkg("_lib").PdseError, match="GPU only"):
        ops.spec_losses(z, z, [1, 1])
    with pytest.raises(pkg("_lib").PdseError, match="GPU only"):
        ops.label_spec(torch.zeros(2, 400), torch.zeros(2, 400), [400, 300])
    with pytest.raises(ValueError, match="label=True"):
        pkg("pipeline").SamplerPipeline.enhance(argparse.Namespace(stft=argparse.Namespace(wav=torch.zeros(1, 400)),
                                                                   xT_in=torch.zeros(1, 2, 3, 161), label=None),
                                                torch.zeros(1, 400), torch.zeros(1, 2, 3, 161), clean=torch.zeros(1, 400))
