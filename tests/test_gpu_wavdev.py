"""GPU: the device wav front end (prior-diffuse_amd/wavdev.py, csrc/resample.hip) against its oracle, ``wavio.read_wav``: the
fp32 16 kHz waveform must be the same bits, for every rate pair, sample format and length class, in a ragged batch as alone, and
through the two callers - ``ComplexDDPMTrainer.generate_wav`` (written files byte-identical to the host path's) and the metrics
command line.  No tolerance anywhere: the kernel repeats the host's arithmetic operation for operation."""
import argparse
import logging
import struct
import wave

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BLOCK = 256      # outputs per workgroup (include/pdse.h: PDSE_RESAMPLE_BLOCK)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert lib.RESAMPLE_BLOCK == BLOCK
    return lib


def _trainer(weights, out):
    ns = argparse.Namespace
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=out),
        ns(model=ns(name="GCRN"), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=weights("GCRN"), ddpm_state_dict=weights("DiffUNet1"))


def _write(path, samples, ch, rate):
    """samples: integer array, uint8 / <i2 / <i4, interleaved."""
    with wave.open(str(path), "wb") as f:
        f.setnchannels(ch)
        f.setsampwidth(samples.dtype.itemsize)
        f.setframerate(rate)
        f.writeframes(samples.tobytes())
    return str(path)


def _i16(rs, n, ch=1):
    x = rs.randint(-32768, 32768, n * ch).astype("<i2")
    x[0] = -32768                       # both ends of the range are in every file that has room for them
    x[-1] = 32767 if x.size > 1 else x[-1]
    return x


def _same_bits(got, want):
    got = got.detach().cpu().numpy()
    return got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape and \
        np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _counts(rate):
    """1, 2; 47: at 48 kHz shorter than the filter's half length of 48 input samples, so both edges reach every output; 1001:
    no multiple of any ``down`` here (3, 441, 2); and the shortest file whose output fills three workgroups and at least 17
    outputs of a fourth (exactly 17 wherever the rate pair can produce that count)."""
    wavio = pkg("wavio")
    n = 1
    while wavio.out_len(n, rate, 16000) < 3 * BLOCK + 17:
        n += 1
    return (1, 2, 47, 1001, n)


@pytest.mark.parametrize("rate", (48000, 44100, 22050, 32000, 8000, 11025, 16000))
def test_bit_identical_to_read_wav_16bit_mono(L, tmp_path, rate):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(rate % 997)
    down = wavio.taps(rate, 16000)[2]
    assert down == 1 or 1001 % down
    for n in _counts(rate):
        path = _write(tmp_path / ("m_%d_%d.wav" % (rate, n)), _i16(rs, n), 1, rate)
        want = wavio.read_wav(path)
        wav, lens = wavdev.load([path], DEV)
        assert lens == [want.size] and tuple(wav.shape) == (1, want.size)
        assert _same_bits(wav[0], want), (rate, n)


def test_bit_identical_16bit_stereo_48k(L, tmp_path):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(2)
    for n in _counts(48000):
        path = _write(tmp_path / ("s_%d.wav" % n), _i16(rs, n, 2), 2, 48000)
        want = wavio.read_wav(path)
        wav, lens = wavdev.load([path], DEV)
        assert lens == [want.size] and _same_bits(wav[0], want), n


def test_bit_identical_8bit_mono_44k1(L, tmp_path):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(3)
    for n in _counts(44100):
        x = rs.randint(0, 256, n).astype(np.uint8)
        x[0], x[-1] = 0, 255
        path = _write(tmp_path / ("b_%d.wav" % n), x, 1, 44100)
        want = wavio.read_wav(path)
        wav, lens = wavdev.load([path], DEV)
        assert lens == [want.size] and _same_bits(wav[0], want), n


@pytest.mark.parametrize("ch", (1, 2))
def test_bit_identical_32bit_48k_with_both_extremes(L, tmp_path, ch):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(4 + ch)
    for n in _counts(48000):
        x = rs.randint(-2 ** 31, 2 ** 31, n * ch, dtype=np.int64).astype("<i4")
        x[0] = -2 ** 31
        x[-1] = 2 ** 31 - 1 if x.size > 1 else x[-1]
        path = _write(tmp_path / ("w_%d_%d.wav" % (ch, n)), x, ch, 48000)
        want = wavio.read_wav(path)
        wav, lens = wavdev.load([path], DEV)
        assert lens == [want.size] and _same_bits(wav[0], want), n
    # 2^31 - 1 is no fp32 number: the conversion rounds it to 2^31, the decoded sample is 1.0
    x = np.array([2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1], dtype="<i4")
    path = _write(tmp_path / "edge.wav", x, 1, 16000)
    wav, _ = wavdev.load([path], DEV)
    assert wav[0].tolist() == [1.0, -1.0, 1.0] and _same_bits(wav[0], wavio.read_wav(path))


def test_ragged_batch_rows_equal_single_calls_and_end_in_zeros(L, tmp_path):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(6)
    counts = (_counts(48000)[-1], 1, 47, 1001, 5000)
    paths = [_write(tmp_path / ("r%d.wav" % i), _i16(rs, n), 1, 48000) for i, n in enumerate(counts)]
    wav, lens = wavdev.load(paths, DEV)
    assert lens == [wavio.out_len(n, 48000, 16000) for n in counts] and tuple(wav.shape) == (5, max(lens))
    for b, path in enumerate(paths):
        one, n1 = wavdev.load([path], DEV)
        assert n1 == [lens[b]] and torch.equal(one[0].view(torch.int32), wav[b, :lens[b]].view(torch.int32)), b
        assert _same_bits(wav[b, :lens[b]], wavio.read_wav(path)), b
        assert not wav[b, lens[b]:].view(torch.int32).any(), b        # +0.0 up to Lmax
    # the same utterances in another order and batch size: a row depends on its own utterance alone
    back, blens = wavdev.load(paths[::-1][:3], DEV)
    for b in range(3):
        assert torch.equal(back[b, :blens[b]].view(torch.int32), wav[4 - b, :lens[4 - b]].view(torch.int32))
    # pre-read frames, the ``decode`` entry point
    frames = [wavio.read_pcm(p)[0] for p in paths]
    dec, dlens = wavdev.decode(frames, 1, 2, 48000, DEV)
    assert dlens == lens and torch.equal(dec.view(torch.int32), wav.view(torch.int32))


def test_mixed_formats_in_one_call_take_separate_launches(L, tmp_path):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(7)
    paths = [_write(tmp_path / "a.wav", _i16(rs, 3000), 1, 48000),
             _write(tmp_path / "b.wav", _i16(rs, 2000, 2), 2, 44100),
             _write(tmp_path / "c.wav", _i16(rs, 700), 1, 16000),
             _write(tmp_path / "d.wav", _i16(rs, 1500), 1, 48000),
             _write(tmp_path / "e.wav", _i16(rs, 400, 3), 3, 48000),      # three channels: the host path
             _write(tmp_path / "f.wav", np.zeros(0, "<i2"), 1, 48000)]    # no frames: the host path
    wav, lens = wavdev.load(paths, DEV)
    want = [wavio.read_wav(p) for p in paths]
    assert lens == [w.size for w in want] and lens[5] == 0 and tuple(wav.shape) == (6, max(lens))
    for b, w in enumerate(want):
        assert _same_bits(wav[b, :lens[b]], w) and not wav[b, lens[b]:].view(torch.int32).any(), b
    before = torch.cuda.memory_allocated()
    for n in (811, 1223, 1999, 2503):                                     # new lengths leave nothing behind
        wavdev.load([_write(tmp_path / "g.wav", _i16(rs, n), 1, 48000)], DEV)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


def test_a_rate_pair_beyond_the_kernels_window_takes_the_host_path(L, tmp_path):
    """960 kHz -> 16 kHz (down / up = 60) needs more LDS than the kernel stages: such a file is converted on the host and uploaded,
    as on the parent, instead of raising; generate_wav and the metrics command therefore still read it."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    assert not wavdev.kernel_covers(1, 6001, 960000)
    path = _write(tmp_path / "fast.wav", _i16(np.random.RandomState(11), 6001), 1, 960000)
    wav, lens = wavdev.load([path, path], DEV)
    want = wavio.read_wav(path)
    assert lens == [want.size, want.size] == [101, 101] and _same_bits(wav[0], want) and _same_bits(wav[1], want)


def _recurrence_at(x, h, up, down, half, ns):
    """The kernel's per-output recurrence (include/pdse.h: pdse_resample_desc) for the outputs ``ns`` of a long signal, in
    Python integers and floats (float64, never fused)."""
    jmax, out = half // up + 1, []
    for n in ns:
        q = int(n) * down
        k_c, r = q // up, q % up
        acc = 0.0
        for j in range(-jmax, jmax + 1):
            off, k = r + j * up, k_c - j
            if abs(off) > half or k < 0 or k >= x.size:
                continue
            acc = acc + float(h[off + half]) * float(x[k])
        out.append(acc)
    return np.array(out, dtype=np.float64).astype(np.float32)


def test_ten_minute_44k1_file_positions_pass_2_31(L):
    """n * down passes 2^31 at output 4869577 of a ten-minute 44.1 kHz file: the outputs around that position, the first and
    the last ones against the recurrence evaluated on the host (tests/test_wavdev_host.py shows it equal to
    ``wavio.resample``, whose 91 passes over ten minutes of float64 would take this test beyond its seconds)."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    n_in = 600 * 44100 + 1
    rs = np.random.RandomState(8)
    pcm = rs.randint(-32768, 32768, n_in).astype("<i2")
    h, up, down, half = wavio.taps(44100, 16000)
    wav, lens = wavdev.decode([pcm.view(np.uint8)], 1, 2, 44100, DEV)
    n_out = lens[0]
    assert n_out == wavio.out_len(n_in, 44100, 16000) == -(-n_in * up // down) and (n_out - 1) * down > 2 ** 31
    cross = 2 ** 31 // down
    ns = np.concatenate([np.arange(0, 60), np.arange(cross - 40, cross + 40), np.arange(n_out - 60, n_out)])
    x = pcm.astype(np.float32) / np.float32(32768.0)
    want = _recurrence_at(x, h, up, down, half, ns)
    got = wav[0, torch.from_numpy(ns).to(DEV)].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(want).max() > 0.1


def _reference_files(t, paths, tmp_path, rng_fidelity, seed):
    """The loop body of generate_wav on the host path, on a trainer of its own: read_wav, the file's x_T draw, enhance, the
    discarded per-step draws."""
    wavio = pkg("wavio")
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    out = []
    for i, p in enumerate(paths):
        wav = torch.from_numpy(wavio.read_wav(p))[None]
        shape = (1, 2, 1 + wav.shape[1] // 160, 161)
        x_T = torch.randn(*shape, device=DEV, dtype=torch.float32)
        y = t.enhance(wav, x_T=x_T)[0].cpu().numpy()
        if rng_fidelity:
            for _ in range(len(t._pipes[next(reversed(t._pipes))].schedule[0]) - 1):
                torch.randn(*shape, device=DEV, dtype=torch.float32)
        ref = str(tmp_path / ("ref_%d_%d.wav" % (int(rng_fidelity), i)))
        wavio.write_wav(ref, y, 16000)
        out.append(open(ref, "rb").read())
    return out


@pytest.mark.parametrize("rng_fidelity", (True, False))
def test_generate_wav_on_48k_and_44k1_files_writes_the_host_paths_bytes(L, weights, tmp_path, rng_fidelity):
    rs = np.random.RandomState(9)
    data = tmp_path / "noisy"
    data.mkdir()
    paths = [_write(data / ("a%d.wav" % i), (0.1 * 32768 * rs.standard_normal(n)).clip(-32768, 32767).astype("<i2"), 1, 48000)
             for i, n in enumerate((9600, 12001, 14400))]                                   # 0.2 .. 0.3 s
    paths.append(_write(data / "b.wav", (0.1 * 32768 * rs.standard_normal(2 * 11025)).clip(-32768, 32767).astype("<i2"), 2, 44100))
    t = _trainer(weights, out=str(tmp_path / "out"))
    torch.manual_seed(31)
    torch.cuda.manual_seed_all(31)
    written = t.generate_wav(load_pre_train=False, data_path=str(data), rng_fidelity=rng_fidelity)
    assert [w.split("/")[-1] for w in written] == ["a0.wav", "a1.wav", "a2.wav", "b.wav"]
    got = [open(w, "rb").read() for w in written]
    want = _reference_files(_trainer(weights, out=str(tmp_path / "unused")), sorted(paths), tmp_path, rng_fidelity, 31)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) > 44 + 2 * 3000 and g == w, (i, rng_fidelity)


def test_generate_wav_fallbacks_three_channels_and_a_rejected_file(L, weights, tmp_path, caplog):
    rs = np.random.RandomState(10)
    data = tmp_path / "noisy"
    data.mkdir()
    three = _write(data / "a3.wav", (0.1 * 32768 * rs.standard_normal(3 * 9600)).clip(-32768, 32767).astype("<i2"), 3, 48000)
    raw = open(three, "rb").read()
    (data / "b_float.wav").write_bytes(raw[:20] + struct.pack("<H", 3) + raw[22:])          # WAVE_FORMAT_IEEE_FLOAT: wave rejects it
    t = _trainer(weights, out=str(tmp_path / "out"))
    torch.manual_seed(32)
    torch.cuda.manual_seed_all(32)
    with caplog.at_level(logging.WARNING):
        written = t.generate_wav(load_pre_train=False, data_path=str(data))
    assert [w.split("/")[-1] for w in written] == ["a3.wav"]
    assert any("skipping" in r.getMessage() and "b_float.wav" in r.getMessage() for r in caplog.records)
    want = _reference_files(_trainer(weights, out=str(tmp_path / "unused")), [three], tmp_path, True, 32)
    assert open(written[0], "rb").read() == want[0]


def test_metrics_cli_on_48k_pairs_prints_the_read_wav_line(L, tmp_path, capsys):
    M, wavio, synth = pkg("metrics"), pkg("wavio"), pkg("synth")
    ref, deg = tmp_path / "ref", tmp_path / "deg"
    ref.mkdir(), deg.mkdir()
    for i, n in enumerate((12000, 9000, 12000, 9001)):
        c, p = synth.noisy_pair(n, 70 + i, 10.0)
        for d, x in ((ref, c), (deg, p)):
            _write(d / ("%d.wav" % i), np.round(np.clip(np.asarray(x, dtype=np.float64), -1, 1 - 2.0 ** -15) * 32768).astype("<i2"), 1, 48000)
    assert M.main([str(ref), str(deg)]) == 0
    text = capsys.readouterr().out
    rows = {}
    for i in range(4):
        c, p = wavio.read_wav(str(ref / ("%d.wav" % i))), wavio.read_wav(str(deg / ("%d.wav" % i)))
        assert c.size == p.size and c.size in (4000, 3000, 3001)
        q = M.quality(torch.from_numpy(c)[None].cuda(), torch.from_numpy(p)[None].cuda())
        rows.setdefault(c.size, []).append([float(q[k][0]) for k in ("ssnr", "llr", "wss", "fwsnrseg")])
    rows = [r for n in sorted(rows) for r in rows[n]]                    # the order main() averages in
    want = "ssnr:%6.4f llr:%6.4f wss:%6.4f fwsnrseg:%6.4f" % tuple(np.mean(np.array(rows, dtype=np.float64), axis=0))
    assert want in text, (want, text)
