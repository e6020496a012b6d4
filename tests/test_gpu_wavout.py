"""GPU: the wav back end (csrc/wavout.hip, ``wavdev.encode``) against its host oracle (``wavio.resample`` + ``wavio.encode``), and
``generate_wav(wav_out="source")`` on a directory of files of four formats.  The contract is bit identity with the host path: no
tolerance anywhere."""
import argparse
import logging
import struct

import numpy as np
import pytest
import torch

from conftest import pkg
from helpers.wavout_cases import special_values

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT, FLOAT = 1, 2                                        # include/pdse.h: PDSE_WAV_INT, PDSE_WAV_FLOAT
TARGETS = ((INT, 2), (INT, 3), (INT, 4), (FLOAT, 4))
CHANNELS = (1, 2, 8)
RATES = (16000, 48000, 44100, 8000, 22050)               # ratio 1 (no taps), 3:1, 441:160, 1:2, 441:320
COUNTS = (1, 2, 85, 86, 255, 256, 257, 700)              # 16 kHz samples: 85 / 86 -> 255 / 258 frames at 48 kHz, 255 .. 257 at ratio 1,
#                                                          700 -> 350 at 8 kHz, 965 at 22.05 kHz, 1930 at 44.1 kHz, 2100 at 48 kHz (9 workgroups)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _signal(n, seed, nonfinite, width=2):
    """Seeded randn * 0.5 with the special values of the host test spliced in where they fit: all of them (NaN and the infinities
    included) when ``nonfinite``, else the finite ones.  A rate conversion spreads a NaN over the filter's length, and which NaN a
    sum of infinities makes is the processor's business: binary32 targets behind a conversion get finite samples only, integer
    targets write every NaN as 0."""
    x = (0.5 * np.random.RandomState(seed).standard_normal(n)).astype(np.float32)
    sp = special_values(width)[0]
    if not nonfinite:
        sp = sp[np.isfinite(sp)]
    if n >= 85:
        at = np.linspace(3, n - 4, sp.size).astype(np.int64)
        x[at] = sp
    elif n == 2:
        x[1] = 1.5
    return x


def _host(wavio, x, rate, fmt, width, ch, keep=None):
    with np.errstate(over="ignore", invalid="ignore"):
        y = wavio.resample(x, 16000, rate)
    return wavio.encode(y if keep is None else y[:keep], fmt, width, ch)


@pytest.mark.parametrize("rate", RATES)
def test_rows_are_resample_and_encode_byte_for_byte(L, rate):
    """A sparse product: every rate meets every length, and over the five rates every target meets every channel count."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    r = RATES.index(rate)
    seen = 0
    for i, n in enumerate(COUNTS):
        k = 8 * r + i
        fmt, width = TARGETS[k % 4]
        ch = CHANNELS[(k // 4 + k) % 3]
        x = _signal(n, 1000 + k, nonfinite=fmt == INT or rate == 16000, width=width)
        want, clipped = _host(wavio, x, rate, fmt, width, ch)
        got, counts = wavdev.encode(torch.from_numpy(x)[None].to(DEV), [n], DEV, rate, fmt, width, ch)
        assert len(got) == 1 and len(got[0]) == wavio.out_len(n, 16000, rate) * ch * width
        assert got[0] == want, (rate, n, fmt, width, ch)
        assert counts == [clipped], (rate, n, fmt, width, ch)
        seen += clipped
    assert seen > 0                                      # the clamp was at work in this rate's cases


def test_the_sparse_product_meets_every_target_with_every_channel_count():
    pairs = {(TARGETS[k % 4], CHANNELS[(k // 4 + k) % 3]) for k in range(8 * len(RATES))}
    assert len(pairs) == len(TARGETS) * len(CHANNELS)


@pytest.mark.parametrize("rate,fmt,width,ch", ((48000, INT, 3, 2), (44100, FLOAT, 4, 1), (8000, INT, 3, 1), (16000, INT, 2, 1), (22050, INT, 4, 8)))
def test_ragged_rows_equal_their_own_launch_and_end_in_zeros(L, rate, fmt, width, ch):
    """B = 3 with 1, 257 and 700 samples, the longer two cut short of what they convert to: row b is its own B = 1 result and the
    host's bytes, and everything behind n_keep * ch * width bytes is zero up to the stride (odd for one channel of 24 bits: rows
    that start at every alignment)."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    lens = [1, 257, 700]
    xs = [_signal(n, 2000 + n, nonfinite=fmt == INT, width=width) for n in lens]
    keep = [wavio.out_len(1, 16000, rate), wavio.out_len(257, 16000, rate) - 3, wavio.out_len(700, 16000, rate) - 5]
    rows = torch.zeros(3, 700)
    for b, x in enumerate(xs):
        rows[b, :lens[b]] = torch.from_numpy(x)
    rows[0, 1:] = 7.0                                    # behind a row's length: never read
    rows[1, 257:] = float("nan")
    out, kept, counts = wavdev.encode_rows(rows.to(DEV), lens, DEV, rate, fmt, width, ch, n_keep=keep)
    fb = ch * width
    assert kept == keep and out.shape == (3, keep[2] * fb)
    for b in range(3):
        want, clipped = _host(wavio, xs[b], rate, fmt, width, ch, keep=keep[b])
        assert out[b, :keep[b] * fb].tobytes() == want and counts[b] == clipped, b
        assert not out[b, keep[b] * fb:].any(), b
        alone, c1 = wavdev.encode(torch.from_numpy(xs[b])[None].to(DEV), [lens[b]], DEV, rate, fmt, width, ch, n_keep=[keep[b]])
        assert alone[0] == want and c1 == [clipped], b


def test_a_rate_beyond_the_kernels_window_takes_the_host_functions(L):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    assert wavdev.encoder_covers(8000) and not wavdev.encoder_covers(160)
    x = _signal(700, 9, nonfinite=True)
    got, counts = wavdev.encode(torch.from_numpy(x)[None].to(DEV), [700], DEV, 160, INT, 2, 2)
    want, clipped = _host(wavio, x, 160, INT, 2, 2)
    assert got == [want] and counts == [clipped]
    with pytest.raises(L.PdseError, match="LDS"):        # the library itself refuses such a pair: no kernel runs on a clipped window
        buf = torch.zeros(64, dtype=torch.float64, device=DEV)
        meta = np.array([700, 7], dtype=np.int32)
        L.wav_encode(buf.data_ptr(), meta.ctypes.data, meta.ctypes.data + 4, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                     buf.data_ptr(), 64, 1, 700, 1, 100, 1600, INT, 2, 1)


# ---- the whole path -----------------------------------------------------------------------------------------------------------
def _trainer(weights, out, **kw):
    ns = argparse.Namespace
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=str(out)),
        ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights("DiffUNet1"), exclusive=False, **kw)


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed_all(s)


def _wav_file(path, tag, width, ch, rate, data):
    head = struct.pack("<HHIIHH", tag, ch, rate, rate * ch * width, ch * width, 8 * width)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(head)) + head + b"data" + struct.pack("<I", len(data)) + data
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body + (b"\0" if len(data) & 1 else b""))
    return str(path)


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    """16 kHz 16-bit mono, 48 kHz 24-bit stereo, 44.1 kHz float32 mono, 8 kHz mu-law and a 16-bit file at full scale: 0.2 s each,
    3200 samples at 16 kHz (T = 21)."""
    rs = np.random.RandomState(81)
    data = tmp_path_factory.mktemp("wavout") / "noisy"
    data.mkdir()
    s16 = (0.1 * 32768 * rs.standard_normal(3200)).clip(-32768, 32767).astype("<i2")
    s24 = (0.1 * 2 ** 23 * rs.standard_normal(2 * 9600)).clip(-2 ** 23, 2 ** 23 - 1).astype("<i4")
    s24 = s24.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    f32 = (0.1 * rs.standard_normal(8820)).astype("<f4")
    loud = rs.randint(-32768, 32768, 3200).astype("<i2")
    return [_wav_file(data / "a_s16.wav", 1, 2, 1, 16000, s16.tobytes()),
            _wav_file(data / "b_s24.wav", 1, 3, 2, 48000, s24),
            _wav_file(data / "c_f32.wav", 3, 4, 1, 44100, f32.tobytes()),
            _wav_file(data / "d_ulaw.wav", 7, 1, 1, 8000, rs.randint(0, 256, 1600).astype(np.uint8).tobytes()),
            _wav_file(data / "e_loud.wav", 1, 2, 1, 16000, loud.tobytes())]


SOURCES = {"a_s16.wav": (16000, 1, 1, 2, 3200), "b_s24.wav": (48000, 2, 1, 3, 9600), "c_f32.wav": (44100, 1, 3, 4, 8820),
           "d_ulaw.wav": (8000, 1, 7, 1, 1600), "e_loud.wav": (16000, 1, 1, 2, 3200)}


@pytest.fixture(scope="module")
def reference(L, directory, weights, tmp_path_factory):
    """The waveform ``enhance`` returns for every file and the x_T of the file loop (seed 56, the ``rng_fidelity`` discards behind
    every file), and from it both files a loop may write: ``write_wav``'s, and the source's format around
    ``wavio.encode(wavio.restore(...))`` with its clip count."""
    wavio = pkg("wavio")
    tmp = tmp_path_factory.mktemp("wavout_ref")
    t = _trainer(weights, tmp / "unused")
    _seed(56)
    out = {}
    for p in directory:
        name = p.split("/")[-1]
        wav = torch.from_numpy(wavio.read_any(p))[None]
        assert wav.shape[1] == 3200
        shape = (1, 2, 21, 161)
        x_T = torch.randn(*shape, device=DEV, dtype=torch.float32)
        y = t.enhance(wav, x_T=x_T)[0].cpu().numpy()
        for _ in range(len(t._pipes[next(reversed(t._pipes))].schedule[0]) - 1):
            torch.randn(*shape, device=DEV, dtype=torch.float32)
        ref = str(tmp / name)
        wavio.write_wav(ref, y, 16000)
        rate, ch, tag, width, n_src = SOURCES[name]
        assert wavio.probe(p) == SOURCES[name]
        tag, width = wavio.target_of((tag, width))
        fmt = {1: INT, 3: FLOAT}[tag]
        payload, clipped = wavio.encode(wavio.restore(y, rate, n_src), fmt, width, ch)
        out[name] = (open(ref, "rb").read(), (rate, ch, tag, width, n_src), payload, clipped)
    assert out["e_loud.wav"][3] > 0, "the full-scale file does not clip: the clip warning has nothing to show"
    return out


def _clip_warnings(caplog):
    return [r.getMessage() for r in caplog.records if "clipped" in r.getMessage()]


@pytest.mark.parametrize("form", ({}, {"inflight": 2}, {"batch": 2}), ids=("one", "inflight", "batch"))
def test_generate_wav_source_writes_the_sources_format(L, weights, directory, reference, tmp_path, caplog, form):
    wavio = pkg("wavio")
    tr = _trainer(weights, tmp_path / "out", wav_formats="all", wav_out="source")
    _seed(56)
    with caplog.at_level(logging.WARNING):
        written = tr.generate_wav(load_pre_train=False, data_path=directory[0].rsplit("/", 1)[0], **form)
    assert [w.split("/")[-1] for w in written] == sorted(SOURCES)
    warned = _clip_warnings(caplog)
    for w in written:
        name = w.split("/")[-1]
        pcm16, probe, payload, clipped = reference[name]
        assert wavio.probe(w) == probe, name
        got = open(w, "rb").read()
        head = len(wavio.wav_header(len(payload), probe[0], {1: INT, 3: FLOAT}[probe[2]], probe[3], probe[1]))
        assert got[head:head + len(payload)] == payload and len(got) == head + len(payload) + (len(payload) & 1), name
        frames = wavio.read_frames(w)[0]
        assert frames.tobytes() == payload, name
        mine = [m for m in warned if name in m]
        assert len(mine) == (1 if clipped else 0), (name, clipped, warned)
        if clipped:
            assert ("%d of %d samples" % (clipped, probe[4])) in mine[0]
        if name == "a_s16.wav":
            assert got == pcm16                          # 16 kHz 16-bit mono: the file the default trainer writes
    assert len(warned) == sum(1 for v in reference.values() if v[3])


def test_the_default_trainer_writes_write_wavs_files(L, weights, directory, reference, tmp_path, caplog):
    tr = _trainer(weights, tmp_path / "out", wav_formats="all")
    assert tr.wav_out == "pcm16"
    _seed(56)
    with caplog.at_level(logging.WARNING):
        written = tr.generate_wav(load_pre_train=False, data_path=directory[0].rsplit("/", 1)[0])
    assert [w.split("/")[-1] for w in written] == sorted(SOURCES)
    for w in written:
        assert open(w, "rb").read() == reference[w.split("/")[-1]][0], w
    assert _clip_warnings(caplog) == []                  # the 16-bit clamp of the default path stays silent, as it was


def test_one_clip_warning_with_the_count(L, weights, directory, tmp_path, caplog):
    """The writer alone, on a waveform whose clipped samples are known: 7 beyond +-1 (one of them NaN) at 16 kHz."""
    wavio = pkg("wavio")
    tr = _trainer(weights, tmp_path / "out", wav_formats="all", wav_out="source")
    (tmp_path / "out").mkdir()
    y = (0.25 * np.random.RandomState(6).standard_normal(3200)).clip(-0.9, 0.9).astype(np.float32)
    y[[5, 600, 601, 1999, 2500, 3100, 3199]] = [1.0, -1.25, 3.0, np.nan, np.inf, -7.0, 1.0000001]
    dst = str(tmp_path / "out" / "a_s16.wav")
    with caplog.at_level(logging.WARNING):
        tr._write_wav(dst, torch.from_numpy(y).to(DEV), directory[0])
    warned = _clip_warnings(caplog)
    assert len(warned) == 1 and "a_s16.wav" in warned[0] and "7 of 3200 samples" in warned[0]
    ref = str(tmp_path / "ref.wav")
    wavio.write_wav(ref, np.nan_to_num(y, nan=0.0, posinf=1.0, neginf=-1.0), 16000)
    assert open(dst, "rb").read() == open(ref, "rb").read()
