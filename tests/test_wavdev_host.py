"""CPU: the host side of the device wav front end (prior-diffuse_amd/wavdev.py, csrc/resample.hip).  The per-output recurrence
the kernel computes, restated as a plain Python loop on ``wavio.taps`` / ``wavio.out_len``, reproduces ``wavio.resample`` bit for
bit; ``wavio.read_pcm`` hands out the frames ``wavio.read_wav`` decodes and raises what it raises; the new descriptor's layout and
its argument checks, without a device."""
import ctypes as C
import struct
import wave

import numpy as np
import pytest

from conftest import pkg

RATES = (48000, 44100, 8000, 22050, 32000, 11025, 96000)
LENGTHS = (1, 2, 3, 47, 50, 443, 1000, 3001)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def recurrence(x, h, up, down, half, n_out):
    """include/pdse.h, pdse_resample_desc: one output at a time, j ascending, product rounded before the add (Python floats are
    float64 and Python never fuses), accumulator started at +0.0, one cast to fp32."""
    x = [float(v) for v in x]
    h = [float(v) for v in h]
    n_in, jmax = len(x), half // up + 1
    out = np.zeros(n_out, dtype=np.float32)
    for n in range(n_out):
        q = n * down
        k_c, r = q // up, q % up
        acc = 0.0
        for j in range(-jmax, jmax + 1):
            off, k = r + j * up, k_c - j
            if abs(off) > half or k < 0 or k >= n_in:
                continue
            acc = acc + h[off + half] * x[k]
        out[n] = np.float32(acc)
    return out


@pytest.mark.parametrize("rate", RATES)
def test_taps_and_recurrence_reproduce_resample(rate):
    wavio = pkg("wavio")
    h, up, down, half = wavio.taps(rate, 16000)
    assert h.dtype == np.float64 and h.size == 2 * half + 1 and up * rate == down * 16000
    rs = np.random.RandomState(rate % 1000)
    for n_in in LENGTHS:
        x = (rs.randint(-32768, 32768, n_in).astype(np.float32) / 32768.0)
        want = wavio.resample(x, rate, 16000)
        n_out = wavio.out_len(n_in, rate, 16000)
        assert n_out == want.size == -(-n_in * up // down)
        got = recurrence(x, h, up, down, half, n_out)
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rate, n_in)


def test_equal_rates_need_no_table():
    wavio = pkg("wavio")
    h, up, down, half = wavio.taps(16000, 16000)
    assert h is None and up == down == 1
    assert wavio.out_len(777, 16000, 16000) == 777 and wavio.out_len(0, 48000, 16000) == 0
    assert [wavio.taps(r, 16000)[1:3] for r in (48000, 44100, 22050, 32000, 8000, 11025)] == [
        (1, 3), (160, 441), (320, 441), (1, 2), (2, 1), (640, 441)]
    assert wavio.taps(48000, 16000)[0].size == 97 and wavio.taps(44100, 16000)[0].size == 14113


def _write(path, data, ch, width, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(ch)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(data)


@pytest.mark.parametrize("width", (1, 2, 4))
@pytest.mark.parametrize("ch", (1, 2))
def test_read_pcm_hands_out_what_read_wav_decodes(tmp_path, width, ch):
    wavio = pkg("wavio")
    rs = np.random.RandomState(10 * width + ch)
    for rate in (16000, 44100, 48000):
        n = 301 + rate % 7
        raw = rs.randint(0, 256, n * ch * width).astype(np.uint8).tobytes()
        path = tmp_path / ("w%d_c%d_%d.wav" % (width, ch, rate))
        _write(path, raw, ch, width, rate)
        frames, n_frames, c, w, r = wavio.read_pcm(str(path))
        assert frames.dtype == np.uint8 and frames.tobytes() == raw
        assert (n_frames, c, w, r) == (n, ch, width, rate)
        # the frames are the ones read_wav decodes: decode them by the rules of include/pdse.h and compare at the file's own rate
        if width == 1:
            x = (frames.astype(np.float32) - 128.0) / 128.0
        else:
            x = frames.view("<i2" if width == 2 else "<i4").astype(np.float32) / np.float32(2.0 ** (8 * width - 1))
        if ch == 2:
            x = (x[0::2] + x[1::2]) / np.float32(2.0)
        want = wavio.read_wav(str(path), sr=rate)
        assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), want.view(np.uint32))
        assert wavio.out_len(n_frames, rate, 16000) == wavio.read_wav(str(path)).size


def test_read_pcm_raises_what_read_wav_raises(tmp_path):
    wavio = pkg("wavio")
    good = tmp_path / "good.wav"
    _write(good, np.arange(400, dtype="<i2").tobytes(), 2, 2, 48000)
    raw = good.read_bytes()
    cases = {
        "cut_header.wav": raw[:20],                                        # ends inside the fmt chunk
        "cut_in_frame.wav": raw[:-3],                                      # the data chunk ends inside a frame
        "float.wav": raw[:20] + struct.pack("<H", 3) + raw[22:],           # WAVE_FORMAT_IEEE_FLOAT
        "extensible.wav": raw[:20] + struct.pack("<H", 0xFFFE) + raw[22:],
        "not_riff.wav": b"RIFX" + raw[4:],
        "empty.wav": b"",
    }
    w24 = tmp_path / "w24.wav"
    _write(w24, bytes(range(240)), 1, 3, 16000)
    cases["w24.wav"] = w24.read_bytes()
    for name, data in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        with pytest.raises((ValueError, EOFError, wave.Error)) as want:
            wavio.read_wav(str(path))
        with pytest.raises(want.type):
            wavio.read_pcm(str(path))
    # a data chunk cut at a frame boundary is a shorter file for both
    path = tmp_path / "short.wav"
    path.write_bytes(raw[:-8])
    assert wavio.read_pcm(str(path))[1] == 198 and wavio.read_wav(str(path), sr=48000).size == 198


def test_descriptor_layout_and_abi(lib):
    pf = pkg("planfile")
    assert lib.OP_RESAMPLE == 30 and lib.DESC_TYPES[lib.OP_RESAMPLE] is lib.ResampleDesc
    assert lib.load().pdse_desc_size(lib.OP_RESAMPLE) == C.sizeof(lib.ResampleDesc) and lib.ABI_VERSION == 9
    assert lib.load().pdse_abi_version() == 9
    offs = pf.pointer_offsets(lib.ResampleDesc)
    assert offs == [0, 8, 16, 24, 32, 40] and lib.ResampleDesc.pcm_bytes.offset == 48
    assert "pdse_pcm_resample_f32" in lib.EXPORTS and lib.RESAMPLE_BLOCK == 256


def test_argument_errors_need_no_device(lib):
    with pytest.raises(lib.PdseError, match="resample: null"):
        lib.launch(lib.ResampleDesc())
    buf = (C.c_double * 8)()
    ptr = C.addressof(buf)

    def desc(counts=(100,), Lmax=34, up=1, down=3, half=48, width=2, ch=1, B=None, **null):
        d = lib.ResampleDesc()
        host = (C.c_int32 * max(len(counts), 1))(*counts)
        d.pcm = d.offs = d.n_in = d.taps = d.out = ptr
        d.n_in_host = C.addressof(host)
        d.pcm_bytes, d.B, d.Lmax = 64, (len(counts) if B is None else B), Lmax
        d.up, d.down, d.half, d.width, d.ch = up, down, half, width, ch
        for k in null:
            setattr(d, k, None)
        d._keep = host
        return d

    for field in ("pcm", "offs", "n_in_host", "n_in", "out"):
        with pytest.raises(lib.PdseError, match="resample: null pointer"):
            lib.launch(desc(**{field: None}))
    with pytest.raises(lib.PdseError, match="resample: B < 1"):
        lib.launch(desc(counts=(), B=0))
    for bad in (dict(up=0), dict(down=0), dict(half=-1)):
        with pytest.raises(lib.PdseError, match="resample: up < 1, down < 1 or half < 0"):
            lib.launch(desc(**bad))
    for w in (0, 3, 8):
        with pytest.raises(lib.PdseError, match="resample: width"):
            lib.launch(desc(width=w))
    for c in (0, 3):
        with pytest.raises(lib.PdseError, match="resample: ch"):
            lib.launch(desc(ch=c))
    with pytest.raises(lib.PdseError, match="resample: n_in < 1"):
        lib.launch(desc(counts=(100, 0)))
    with pytest.raises(lib.PdseError, match="resample: n_out > Lmax"):
        lib.launch(desc(counts=(100, 103), Lmax=34))             # ceil(103 / 3) = 35
    with pytest.raises(lib.PdseError, match="resample: null taps"):
        lib.launch(desc(taps=None))
    with pytest.raises(lib.PdseError, match="resample: .*LDS"):
        lib.launch(desc(counts=(100,), Lmax=2, up=1, down=100, half=1600))
    p = lib.Plan()
    d = desc(counts=(100, 0))                                    # its host array must live as long as the plan
    p.add(d)
    with pytest.raises(lib.PdseError, match="resample: n_in < 1"):
        p.run()                                                # the plan dispatch reaches the same checks


def test_kernel_covers_is_the_librarys_own_window_limit(lib):
    """``wavdev.load`` sends a file to the host path when the library would refuse its rate pair (the input window of one
    workgroup's outputs beyond 64 KB of LDS), so no readable file reaches that refusal.  Only refused descriptors are handed to
    the library here: validation stops them before any launch."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    buf = (C.c_double * 8)()
    host = (C.c_int32 * 1)(1)
    for rate in (8000, 15999, 16000, 44100, 48000, 96000, 192000, 800000, 912000, 928000, 960000, 1600000):
        _, up, down, half = wavio.taps(rate, 16000)
        fits = up == down or 4 * ((lib.RESAMPLE_BLOCK - 1) * down // up + 2 * (half // up + 1) + 2) <= 64 * 1024
        assert wavdev.kernel_covers(1, 1, rate) == fits, rate
        if not fits:
            d = lib.ResampleDesc()
            d.pcm = d.offs = d.n_in = d.taps = d.out = C.addressof(buf)
            d.n_in_host = C.addressof(host)
            d.pcm_bytes, d.B, d.Lmax, d.width, d.ch = 2, 1, 1, 2, 1
            d.up, d.down, d.half = up, down, half
            with pytest.raises(lib.PdseError, match="resample: .*LDS"):
                lib.launch(d)
    assert wavdev.kernel_covers(1, 1, 912000) and not wavdev.kernel_covers(1, 1, 960000)        # down / up = 57 and 60
    assert wavdev.kernel_covers(2, 1, 48000) and not wavdev.kernel_covers(3, 1, 48000) and not wavdev.kernel_covers(1, 0, 48000)


def test_decode_rejects_bad_arguments_before_touching_a_device():
    wavdev = pkg("wavdev")
    with pytest.raises(pkg("_lib").PdseError, match="no CPU fallback"):
        wavdev.decode([np.zeros(4, np.uint8)], 1, 2, 48000, "cpu")
