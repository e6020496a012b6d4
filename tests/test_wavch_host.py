"""CPU: the host side of per-channel enhancement - the oracles ``wavio.read_channels`` and ``wavio.encode_channels``, the argument
checks of ``pdse_wav_encode_channels`` and of the split mode of ``pdse_resample_desc`` (no device), and the trainer's plumbing
(``channels="each"``) with the enhancer stubbed: which noise is drawn for which channel, and what the loops are handed."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from helpers.wavch_cases import ALAW, FLOAT, FORMATS, INT, NAMES, ULAW, payload, rows_signal, same_bits, split_files, wav_bytes

RATES = (16000, 48000, 44100, 8000)
TARGETS = ((INT, 2), (INT, 3), (INT, 4), (FLOAT, 4))


# ---- wavio.read_channels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,width", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_read_channels_rows_are_read_any_of_the_split_files(tmp_path, fmt, width):
    wavio = pkg("wavio")
    rs = np.random.RandomState(10 * fmt + width)
    for ch in (2, 3, 8):
        for rate in RATES:
            for ext in (False, True):
                n = 150 + 7 * ch + (rate // 1000) % 5
                path, monos = split_files(tmp_path, "x%d_%d_%d" % (ch, rate, ext), fmt, width, rate, payload(rs, fmt, width, n, ch), ext)
                got = wavio.read_channels(path)
                assert got.dtype == np.float32 and got.shape == (ch, wavio.out_len(n, rate, 16000))
                for c in range(ch):
                    assert same_bits(got[c], wavio.read_any(monos[c])), (ch, rate, ext, c)
                if ch == 2 and not ext and rate != 16000:          # and at another target rate
                    assert same_bits(wavio.read_channels(path, sr=8000)[1], wavio.read_any(monos[1], sr=8000))


def test_read_channels_of_a_mono_file_is_read_any(tmp_path):
    wavio = pkg("wavio")
    rs = np.random.RandomState(3)
    for fmt, width in FORMATS:
        for rate in (16000, 44100):
            p = tmp_path / ("m_%s_%d.wav" % (NAMES[fmt, width], rate))
            p.write_bytes(wav_bytes(fmt, width, 1, rate, payload(rs, fmt, width, 211, 1).tobytes()))
            got = wavio.read_channels(str(p))
            assert got.shape[0] == 1 and same_bits(got[0], wavio.read_any(str(p)))
    empty = tmp_path / "empty.wav"
    empty.write_bytes(wav_bytes(INT, 2, 2, 16000, b""))
    assert wavio.read_channels(str(empty)).shape == (2, 0)


def test_a_nan_payload_survives_in_its_channel_alone(tmp_path):
    """binary32 stereo at 16 kHz: channel 0 holds NaNs with payloads (a signalling one among them), infinities, a subnormal and -0;
    its bits come back as they are, and channel 1 - which the mix's sum would have turned into NaN - is untouched."""
    wavio = pkg("wavio")
    special = np.array([0x7FC00001, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x80000000, 0x3F800000], dtype="<u4")
    other = (0.3 * np.random.RandomState(5).standard_normal(special.size)).astype("<f4")
    frames = np.stack([special.view(np.uint8).reshape(-1, 4), other.view(np.uint8).reshape(-1, 4)], axis=1)
    p = tmp_path / "nan.wav"
    p.write_bytes(wav_bytes(FLOAT, 4, 2, 16000, frames.tobytes()))
    got = wavio.read_channels(str(p))
    assert np.array_equal(got[0].view(np.uint32), special) and np.array_equal(got[1].view(np.uint32), other.view(np.uint32))
    assert np.isnan(wavio.read_any(str(p))[:3]).all()                  # the mix is what loses it


# ---- wavio.encode_channels -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,width", TARGETS)
def test_encode_channels_interleaves_the_rows_own_payloads(fmt, width):
    wavio = pkg("wavio")
    for ch in (1, 2, 3, 8):
        x = rows_signal(ch, 301, 40 + ch, clip_channel=ch - 1, width=width)
        got, clipped = wavio.encode_channels(x, fmt, width)
        image = np.frombuffer(got, dtype=np.uint8).reshape(301, ch, width)
        for c in range(ch):
            want, k = wavio.encode(x[c], fmt, width, 1)
            assert image[:, c].tobytes() == want and clipped[c] == k, (ch, c)
        if fmt == INT:                                                 # +1.0, -1.5, NaN, +-inf, 2.5 in the last channel only
            assert clipped == [0] * (ch - 1) + [6]
        else:
            assert clipped == [0] * ch
        same = np.repeat(x[:1], ch, axis=0)
        assert wavio.encode_channels(same, fmt, width)[0] == wavio.encode(x[0], fmt, width, ch)[0]
    assert wavio.encode_channels(np.zeros((2, 0), dtype=np.float32), fmt, width) == (b"", [0, 0])


def test_encode_channels_refuses_what_encode_refuses():
    wavio = pkg("wavio")
    x = np.zeros((2, 4), dtype=np.float32)
    for fmt, width in ((INT, 1), (INT, 5), (FLOAT, 8), (ALAW, 1), (ULAW, 1), (0, 2)):
        with pytest.raises(ValueError, match="no encoder"):
            wavio.encode_channels(x, fmt, width)
    with pytest.raises(ValueError, match="channels"):
        wavio.encode_channels(np.zeros((9, 4), dtype=np.float32), INT, 2)
    with pytest.raises(ValueError, match=r"\[ch, n\]"):
        wavio.encode_channels(np.zeros(4, dtype=np.float32), INT, 2)


# ---- the library's argument checks: before the launch, without a device ------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def _call(lib, n_in=(100,), n_keep=None, stride=None, Lmax=128, up=3, down=1, half=48, fmt=INT, width=2, ch=2, taps=True):
    B = len(n_in)
    n_keep = [-(-n * up // down) for n in n_in] if n_keep is None else list(n_keep)
    meta = np.array(list(n_in) + n_keep, dtype=np.int32)
    dummy = (C.c_double * 8)()                           # stands in for every device pointer: nothing is launched
    ptr = C.addressof(dummy)
    stride = max(max(n_keep) * ch * width, 1) if stride is None else stride
    lib.wav_encode_channels(ptr, meta.ctypes.data, meta.ctypes.data + 4 * B, ptr, ptr, ptr if taps else None, ptr, ptr, stride, B, Lmax,
                            up, down, half, fmt, width, ch)


@pytest.mark.parametrize("kw,text", (
    (dict(width=1), "width of 2, 3 or 4"), (dict(fmt=FLOAT, width=8), "width of 4"), (dict(fmt=3, width=1), "fmt must be"),
    (dict(ch=0), "ch must be 1 .. 8"), (dict(ch=9), "ch must be 1 .. 8"),
    (dict(n_in=(100, 0), n_keep=(300, 0)), "n_in < 1"), (dict(n_in=(129,)), "n_in > Lmax"), (dict(n_keep=(301,)), "n_keep"),
    (dict(stride=1199), "stride"), (dict(ch=3, width=3, stride=2699), "stride"),         # 300 frames of 4 and of 9 bytes
    (dict(taps=False), "null taps"), (dict(up=0), "up < 1"),
    (dict(n_in=(1,) * 8192, n_keep=(1,) * 8192, up=1, half=16, ch=8), "65535"),          # B ch = 65536 rows
    (dict(up=1, down=8, half=128, ch=8), "LDS"),         # 16 -> 2 kHz: a window of 2300 samples fits once (mono encoder) and not 8 times
))
def test_wav_encode_channels_refuses_bad_arguments_without_a_device(lib, kw, text):
    with pytest.raises(lib.PdseError, match="wav_encode_channels: .*" + text):
        _call(lib, **kw)


def test_the_lds_budget_takes_the_factor_ch(lib):
    """16 -> 2 kHz (up 1, down 8, half 128): one window is 4 * 2300 bytes; with the 8 KB image the mono encoder and up to 6 channels
    fit in 64 KB, 7 and 8 do not - the library and ``wavdev.encoder_covers`` agree, and both reach the check without a device."""
    wavdev = pkg("wavdev")
    win = (lib.RESAMPLE_BLOCK - 1) * 8 + 2 * 129 + 2
    assert win == 2300 and wavdev.encoder_covers(2000)
    for ch in range(1, 9):
        fits = 4 * win * ch + lib.WAVCH_STATIC_BYTES <= 64 * 1024
        assert wavdev.encoder_covers(2000, ch=ch) == fits == (ch <= 6)
        if not fits:
            with pytest.raises(lib.PdseError, match="LDS"):
                _call(lib, up=1, down=8, half=128, ch=ch)
    assert all(wavdev.encoder_covers(r, ch=8) for r in (16000, 48000, 44100, 8000, 22050, 96000))


def test_the_new_symbol_is_declared_and_exported_and_the_descriptor_keeps_its_size(lib):
    assert "pdse_wav_encode_channels" in lib.EXPORTS and hasattr(lib.load(), "pdse_wav_encode_channels")
    with pytest.raises(lib.PdseError, match="wav_encode_channels: null pointer"):
        lib.wav_encode_channels(None, None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 0, INT, 2, 2)
    assert C.sizeof(lib.ResampleDesc) == 88 == lib.load().pdse_desc_size(lib.OP_RESAMPLE) and lib.ABI_VERSION == 9
    assert [n for n, _ in lib.ResampleDesc._fields_][-2:] == ["ch", "fmt"] and lib.ResampleDesc.fmt.offset == 84
    assert lib.WAV_SPLIT == 256 and all(lib.WAV_SPLIT & f == 0 for f in (lib.WAV_INT, lib.WAV_FLOAT, lib.WAV_ALAW, lib.WAV_ULAW))


def test_split_mode_argument_errors_need_no_device(lib):
    buf = (C.c_double * 8)()
    ptr = C.addressof(buf)
    keep = []

    def desc(fmt, width, ch, B=1):
        n_in = (C.c_int32 * B)(*([3] * B))
        keep.append(n_in)
        d = lib.ResampleDesc()
        d.pcm, d.offs, d.n_in, d.out, d.taps, d.n_in_host = ptr, ptr, ptr, ptr, ptr, C.addressof(n_in)
        d.pcm_bytes, d.B, d.Lmax = 64, B, 4
        d.up, d.down, d.half, d.width, d.ch, d.fmt = 1, 3, 48, width, ch, fmt
        return d

    S = lib.WAV_SPLIT
    with pytest.raises(lib.PdseError, match="65535 rows"):
        lib.launch(desc(INT | S, 2, 8, B=8192))                        # B ch = 65536
    with pytest.raises(lib.PdseError, match="65535 rows"):
        lib.launch(desc(ULAW | S, 1, 2, B=40000))
    for fmt in (S, 5 | S, 99 | S, -1):                                 # the flag alone, and unknown encodings under it
        with pytest.raises(lib.PdseError, match="resample: unknown fmt"):
            lib.launch(desc(fmt, 2, 2))
    with pytest.raises(lib.PdseError, match="PDSE_WAV_INT takes a width of 1, 2, 3 or 4"):
        lib.launch(desc(INT | S, 8, 2))
    with pytest.raises(lib.PdseError, match="PDSE_WAV_FLOAT takes a width of 4 or 8"):
        lib.launch(desc(FLOAT | S, 2, 2))
    with pytest.raises(lib.PdseError, match=r"ch must be 1 \.\. 8"):
        lib.launch(desc(ALAW | S, 1, 9))
    d = desc(FLOAT | S, 8, 8)
    long = (C.c_int32 * 1)(100)                                       # 34 outputs in a row of 4
    d.n_in_host = C.addressof(long)
    with pytest.raises(lib.PdseError, match="n_out > Lmax"):
        lib.launch(d)


# ---- the trainer's plumbing, the enhancer stubbed ------------------------------------------------------------------------------
def _stub(monkeypatch, files, channels, prior="GCRN", masked=False):
    """A trainer without a device: ``_load_window`` hands out zeros of the shapes in ``files`` (name -> length, or (C, length));
    draws, enhancer calls and written files are recorded."""
    import torch

    tr_mod = pkg("trainer")
    log = {"calls": [], "enh": [], "written": []}

    class Stub(tr_mod.ComplexDDPMTrainer):
        def __init__(self):
            self.prior_name, self.device, self.masked_prior = prior, torch.device("cpu"), masked
            self.params = pkg("params").params
            self.args = type("A", (), {"generated_wav": "out"})()
            self.channels = channels

        def _load_window(self, paths):
            shape = lambda v: (v,) if isinstance(v, int) else v       # noqa: E731
            return [(p, torch.zeros(*shape(files[p.split("/")[-1]]))) for p in paths]

        def _x_T(self, shape, x_T):
            log["calls"].append(("x_T", tuple(shape)))
            return torch.zeros(*shape)

        def _checked(self, run, **geom):                              # behind ``_enhance_ragged``'s argument checks
            log["enh"].append(("ragged", geom["B"], geom["L_"]))
            return torch.zeros(geom["B"], geom["L_"])

        def enhance(self, wav, x_T=None, verify=True):
            log["enh"].append(("enhance", tuple(wav.shape), tuple(x_T.shape)))
            return wav

        def enhance_stream(self, items, inflight=3):
            for wav, x_T in items:
                log["enh"].append(("item", tuple(wav.shape), tuple(x_T.shape)))
                yield wav, None

        def _write_wav(self, dst, out, src):
            log["written"].append((dst, tuple(out.shape)))

    monkeypatch.setattr(tr_mod.glob, "glob", lambda pat: ["d/" + k for k in reversed(sorted(files))])
    monkeypatch.setattr(torch, "randn", lambda *shape, **kw: log["calls"].append(("discard", tuple(shape))) or torch.zeros(1))
    return Stub(), log


MODES = ((1, 1), (1, 2), (4, 1))                                       # (batch, inflight)


@pytest.mark.parametrize("fidelity", (True, False))
def test_a_stereo_file_draws_what_its_two_mono_files_draw(monkeypatch, fidelity):
    """b.wav with 2 channels and d.wav with 3 against the directory of their split files, named to sort in the same place: the
    generator is asked for the same shapes in the same order, discards included, in every mode - and the multichannel files come
    out as [C, len] under their own names."""
    multi = {"a.wav": 4000, "b.wav": (2, 3000), "c.wav": 1700, "d.wav": (3, 5000)}
    split = {"a.wav": 4000, "b_c0.wav": 3000, "b_c1.wav": 3000, "c.wav": 1700, "d_c0.wav": 5000, "d_c1.wav": 5000, "d_c2.wav": 5000}
    for batch, inflight in MODES:
        tr, log = _stub(monkeypatch, multi, "each")
        out = tr.generate_wav(load_pre_train=False, data_path="d", rng_fidelity=fidelity, batch=batch, inflight=inflight)
        ref, want = _stub(monkeypatch, split, "mix")
        ref.generate_wav(load_pre_train=False, data_path="d", rng_fidelity=fidelity, batch=batch, inflight=inflight)
        assert log["calls"] == want["calls"] and len(log["calls"]) >= 7
        assert fidelity == any(c[0] == "discard" for c in log["calls"])
        assert out == ["out/" + n for n in sorted(multi)]
        assert [w[1] for w in log["written"]] == [(4000,), (2, 3000), (1700,), (3, 5000)]
        if (batch, inflight) == (1, 1):                                # one exact ragged pass of B = C per file, nothing padded
            assert log["enh"] == [("enhance", (1, 4000), (1, 2, 26, 161)), ("ragged", 2, 3000), ("enhance", (1, 1700), (1, 2, 11, 161)),
                                  ("ragged", 3, 5000)]
        elif inflight > 1:                                             # one item [C, L] with x_T [C, 2, T, 161]
            assert log["enh"] == [("item", (1, 4000), (1, 2, 26, 161)), ("item", (2, 3000), (2, 2, 19, 161)),
                                  ("item", (1, 1700), (1, 2, 11, 161)), ("item", (3, 5000), (3, 2, 32, 161))]
        else:                                                          # every channel a row of the window: 7 rows in buckets of 4
            assert sorted(e[1] for e in log["enh"]) == [3, 4] and log["enh"] == want["enh"]


def test_a_mono_directory_is_the_same_under_each_and_mix(monkeypatch):
    files = {"a.wav": 4000, "b.wav": 161 + 160 * 7, "c.wav": 9000}
    for batch, inflight in MODES:
        seen = []
        for channels in ("mix", "each"):
            tr, log = _stub(monkeypatch, files, channels)
            out = tr.generate_wav(load_pre_train=False, data_path="d", batch=batch, inflight=inflight)
            seen.append((out, log))
        assert seen[0] == seen[1] and len(seen[0][1]["enh"]) >= 1 and len(seen[0][1]["written"]) == 3


def test_the_db_aiat_priors_need_masked_prior_for_a_multichannel_file(monkeypatch):
    files = {"a.wav": 4000, "b.wav": (2, 3000)}
    tr, log = _stub(monkeypatch, files, "each", prior="aia_complex_trans_ri")
    with pytest.raises(ValueError, match="bidirectional GRU"):
        tr.generate_wav(load_pre_train=False, data_path="d")
    assert log["enh"] == [("enhance", (1, 4000), (1, 2, 26, 161))]    # raised when the first multichannel file was met
    tr, log = _stub(monkeypatch, files, "each", prior="aia_complex_trans_ri", masked=True)
    tr.generate_wav(load_pre_train=False, data_path="d")
    assert log["enh"][1] == ("ragged", 2, 3000)
    tr, log = _stub(monkeypatch, files, "each", prior="aia_complex_trans_ri", masked=True)
    with pytest.raises(ValueError, match="inflight"):                  # in flight the channels would share a dense pass
        tr.generate_wav(load_pre_train=False, data_path="d", inflight=2)


def test_more_than_eight_channels_take_the_mix(monkeypatch, tmp_path, caplog):
    """``_load_channels`` on real headers with ``wavdev.load`` stubbed: the 9-channel file goes to the mix's loader and comes back
    1-D (with a warning), stereo comes back [2, len], mono 1-D; the files reach the two loaders in path order."""
    import logging

    import torch

    tr_mod = pkg("trainer")
    rs = np.random.RandomState(9)
    paths = []
    for name, ch in (("a.wav", 1), ("b.wav", 9), ("c.wav", 2)):
        (tmp_path / name).write_bytes(wav_bytes(INT, 2, ch, 16000, payload(rs, INT, 2, 400, ch).tobytes()))
        paths.append(str(tmp_path / name))
    asked = []

    def load(ps, device, sr, formats="pcm", channels="mix"):
        asked.append((list(ps), formats, channels))
        chans = [pkg("wavio").probe(p)[1] for p in ps]
        if channels == "each":
            return torch.ones(sum(chans), 400), [400] * sum(chans), chans
        return torch.zeros(len(ps), 400), [400] * len(ps)

    monkeypatch.setattr(tr_mod.wavdev, "load", load)
    tr = tr_mod.ComplexDDPMTrainer.__new__(tr_mod.ComplexDDPMTrainer)
    tr.device, tr.channels, tr.wav_formats = torch.device("cpu"), "each", "all"
    with caplog.at_level(logging.WARNING):
        got = tr._load_window(paths)
    assert asked == [([paths[0], paths[2]], "all", "each"), ([paths[1]], "all", "mix")]
    assert [p for p, _ in got] == paths and [tuple(w.shape) for _, w in got] == [(400,), (400,), (2, 400)]
    assert float(got[1][1].sum()) == 0.0 and float(got[2][1].sum()) == 800.0
    assert [r.getMessage() for r in caplog.records] == ["%s: more than 8 channels, enhanced as the mix" % paths[1]]


def test_constructor_and_cli_options():
    tr_mod = pkg("trainer")
    assert tr_mod.ComplexDDPMTrainer.channels == "mix"
    import argparse
    import inspect

    assert inspect.signature(tr_mod.ComplexDDPMTrainer.__init__).parameters["channels"].default is None
    ns = argparse.Namespace
    args = ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav="y")
    config = ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt"))
    with pytest.raises(ValueError, match="channels must be"):
        tr_mod.ComplexDDPMTrainer(args, config, device="cpu", prior_state_dict={}, ddpm_state_dict={}, channels="all")
    import os

    from conftest import ROOT

    assert '"--per-channel"' in open(os.path.join(ROOT, "prior-diffuse_amd", "main.py")).read()
