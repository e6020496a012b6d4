"""CPU: the host oracle of the wav back end (prior-diffuse_amd/wavio.py: encode, write_any, target_of, probe, restore) and the
argument checks of ``pdse_wav_encode``, which need no device."""
import ctypes as C
import struct

import numpy as np
import pytest

from conftest import pkg
from helpers.wavout_cases import special_values

INT, FLOAT = 1, 2                                        # include/pdse.h: PDSE_WAV_INT, PDSE_WAV_FLOAT
TARGETS = ((INT, 2), (INT, 3), (INT, 4), (FLOAT, 4))


@pytest.fixture(scope="module")
def wavio():
    w = pkg("wavio")
    assert (w.WAV_INT, w.WAV_FLOAT) == (INT, FLOAT)
    return w


def _ints(payload, width, ch=1):
    raw = np.frombuffer(payload, dtype=np.uint8).reshape(-1, width).astype(np.int64)
    v = sum(raw[:, k] << (8 * k) for k in range(width))
    v = v - ((v >> (8 * width - 1)) << (8 * width))
    frames = v.reshape(-1, ch)
    assert (frames == frames[:, :1]).all()               # every channel carries the same sample
    return frames[:, 0]


@pytest.mark.parametrize("width", (2, 3, 4))
def test_encode_rounds_half_to_even_clamps_and_counts(wavio, width):
    x, want, clipped = special_values(width)
    payload, n = wavio.encode(x, INT, width, 1)
    assert len(payload) == width * x.size and n == clipped
    assert _ints(payload, width).tolist() == want
    for ch in (2, 8):
        p, n = wavio.encode(x, INT, width, ch)
        assert n == clipped and _ints(p, width, ch).tolist() == want


def test_encode_float_keeps_the_bits(wavio):
    x = special_values(2)[0]
    x = np.concatenate([x, np.array([0x7FC12345, 0x00000001, 0x80000000], dtype=np.uint32).view(np.float32)])
    payload, n = wavio.encode(x, FLOAT, 4, 1)
    assert n == 0 and payload == x.tobytes()
    p, n = wavio.encode(x, FLOAT, 4, 2)
    assert n == 0 and p == np.repeat(x.view(np.uint32), 2).tobytes()


def test_encode_16_bit_mono_is_write_wavs_payload(wavio, tmp_path):
    rs = np.random.RandomState(3)
    x = np.concatenate([(0.5 * rs.standard_normal(1000)).astype(np.float32), special_values(2)[0][:10], special_values(2)[0][11:]])
    wavio.write_wav(str(tmp_path / "a.wav"), x, 16000)
    ref = (tmp_path / "a.wav").read_bytes()
    payload, _ = wavio.encode(x, INT, 2, 1)
    assert ref[44:] == payload
    wavio.write_any(str(tmp_path / "b.wav"), x, 16000, INT, 2, 1)
    assert (tmp_path / "b.wav").read_bytes() == ref     # header included


@pytest.mark.parametrize("bad", ((INT, 1, 1), (INT, 5, 1), (FLOAT, 8, 1), (FLOAT, 2, 1), (3, 1, 1), (INT, 2, 0), (INT, 2, 9)))
def test_encode_refuses_other_targets(wavio, bad):
    with pytest.raises(ValueError):
        wavio.encode(np.zeros(4, dtype=np.float32), *bad)


@pytest.mark.parametrize("ch", (1, 2, 8))
@pytest.mark.parametrize("fmt,width", TARGETS)
def test_write_any_read_any_round_trip(wavio, tmp_path, fmt, width, ch):
    rs = np.random.RandomState(10 * width + ch)
    x = (0.2 * rs.standard_normal(333)).clip(-0.9, 0.9).astype(np.float32)      # odd count: a 24-bit mono data chunk gets its pad byte
    path = str(tmp_path / "t.wav")
    assert wavio.write_any(path, x, 22050, fmt, width, ch) == 0
    frames, n, c, w, rate, f = wavio.read_frames(path)
    assert (n, c, w, rate, f) == (333, ch, width, 22050, fmt) and frames.size == 333 * ch * width
    assert len(open(path, "rb").read()) % 2 == 0
    # channel by channel (the mono mix of ``read_any`` rounds a sum of three equal samples), and the mix itself where it is exact
    backs = [wavio.decode_frames(frames.reshape(n, ch, width)[:, k], 1, width, fmt) for k in range(ch)]
    if ch <= 2:
        backs.append(wavio.read_any(path, 22050))
    for back in backs:
        if fmt == FLOAT:
            assert np.array_equal(back.view(np.uint32), x.view(np.uint32))
        else:
            assert np.abs(back.astype(np.float64) - x.astype(np.float64)).max() <= 2.0 ** -(8 * width - 1)      # one LSB


def test_target_of(wavio):
    table = {(1, 1): (1, 2), (1, 2): (1, 2), (1, 3): (1, 3), (1, 4): (1, 4), (3, 4): (3, 4), (3, 8): (3, 4), (6, 1): (1, 2), (7, 1): (1, 2)}
    for src, want in table.items():
        assert wavio.target_of(src) == want, src
    for bad in ((1, 8), (3, 2), (6, 2), (2, 2), (0xFFFE, 2)):
        with pytest.raises(ValueError):
            wavio.target_of(bad)


def _raw_file(path, tag, width, ch, rate, data, extensible=False, extra=b"", size=None):
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, ch, rate, rate * ch * width, ch * width, 8 * width)
    if extensible:
        head += struct.pack("<HHIH", 22, 8 * width, 0, tag) + bytes([0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])
    body = b"WAVE" + extra + b"fmt " + struct.pack("<I", len(head)) + head + b"data" + struct.pack("<I", len(data) if size is None else size) + data
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body + (b"\0" if len(data) & 1 else b""))
    return str(path)


def test_probe_reads_what_read_frames_reads(wavio, tmp_path):
    rs = np.random.RandomState(4)
    for i, (fmt, width) in enumerate(TARGETS):
        for ch in (1, 2, 8):
            p = str(tmp_path / ("w%d_%d.wav" % (i, ch)))
            wavio.write_any(p, rs.standard_normal(77).astype(np.float32), 44100 + i, fmt, width, ch)
            assert wavio.probe(p) == (44100 + i, ch, {INT: 1, FLOAT: 3}[fmt], width, 77)
    junk = b"LIST" + struct.pack("<I", 3) + b"abc\0"                      # an odd chunk and its pad byte in front of fmt
    cases = [(_raw_file(tmp_path / "ulaw.wav", 7, 1, 1, 8000, bytes(range(201))), (8000, 1, 7, 1, 201)),
             (_raw_file(tmp_path / "alaw.wav", 6, 1, 2, 8000, bytes(200), extra=junk), (8000, 2, 6, 1, 100)),
             (_raw_file(tmp_path / "f64.wav", 3, 8, 1, 96000, bytes(80)), (96000, 1, 3, 8, 10)),
             (_raw_file(tmp_path / "u8.wav", 1, 1, 1, 11025, bytes(9)), (11025, 1, 1, 1, 9)),
             (_raw_file(tmp_path / "ext.wav", 1, 2, 6, 44100, bytes(12 * 50), extensible=True), (44100, 6, 1, 2, 50)),
             (_raw_file(tmp_path / "pipe.wav", 1, 2, 1, 16000, bytes(64), size=0xFFFFFFFF), (16000, 1, 1, 2, 32))]
    for path, want in cases:
        assert wavio.probe(path) == want, path
        frames, n, ch, width, rate, fmt = wavio.read_frames(path)
        assert (rate, ch, width, n) == (want[0], want[1], want[3], want[4]) and wavio._TAG_FMT[want[2]] == fmt
    for path in (_raw_file(tmp_path / "tag.wav", 2, 2, 1, 16000, bytes(8)), _raw_file(tmp_path / "cut.wav", 1, 2, 2, 16000, bytes(6))):
        with pytest.raises(ValueError):
            wavio.read_frames(path)
        with pytest.raises(ValueError):
            wavio.probe(path)


def test_there_and_back_is_never_shorter_than_the_source(wavio):
    for r in (8000, 11025, 22050, 32000, 44100, 48000, 96000):
        n = np.arange(1, 3001)
        back = np.array([wavio.out_len(wavio.out_len(int(k), r, 16000), 16000, r) for k in n])
        assert (back - n).min() >= 0 and (back - n).max() <= 5, r
    x = np.random.RandomState(5).standard_normal(wavio.out_len(1001, 44100, 16000)).astype(np.float32)
    y = wavio.restore(x, 44100, 1001)
    assert y.dtype == np.float32 and np.array_equal(y, wavio.resample(x, 16000, 44100)[:1001])
    with pytest.raises(ValueError):
        wavio.restore(x, 44100, 1100)


# ---- the library's argument checks: before the launch, without a device ------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def _call(lib, n_in=(100,), n_keep=None, stride=None, Lmax=128, up=3, down=1, half=48, fmt=INT, width=2, ch=1, taps=True):
    B = len(n_in)
    n_keep = [-(-n * up // down) for n in n_in] if n_keep is None else list(n_keep)
    meta = np.array(list(n_in) + n_keep, dtype=np.int32)
    dummy = (C.c_double * 8)()                           # stands in for every device pointer: nothing is launched
    ptr = C.addressof(dummy)
    stride = max(max(n_keep) * ch * width, 1) if stride is None else stride
    lib.wav_encode(ptr, meta.ctypes.data, meta.ctypes.data + 4 * B, ptr, ptr, ptr if taps else None, ptr, ptr, stride, B, Lmax, up, down,
                   half, fmt, width, ch)


@pytest.mark.parametrize("kw,text", (
    (dict(width=1), "width of 2, 3 or 4"), (dict(width=5), "width of 2, 3 or 4"), (dict(fmt=FLOAT, width=8), "width of 4"),
    (dict(fmt=FLOAT, width=2), "width of 4"), (dict(fmt=3, width=1), "fmt must be"), (dict(fmt=0), "fmt must be"),
    (dict(ch=0), "ch must be 1 .. 8"), (dict(ch=9), "ch must be 1 .. 8"),
    (dict(n_in=(100, 0), n_keep=(300, 0)), "n_in < 1"), (dict(n_in=(129,)), "n_in > Lmax"),
    (dict(n_keep=(301,)), "n_keep"), (dict(n_keep=(-1,)), "n_keep"),
    (dict(stride=599), "stride"), (dict(ch=2, width=3, stride=1799), "stride"), (dict(n_in=(100, 50), stride=299), "stride"),
    (dict(taps=False), "null taps"), (dict(up=0), "up < 1"),
    (dict(up=1, down=100, half=1600), "LDS"),             # 16 kHz -> 160 Hz: a window of 255 * 100 + 3204 samples
))
def test_wav_encode_refuses_bad_arguments_without_a_device(lib, kw, text):
    with pytest.raises(lib.PdseError, match=text):
        _call(lib, **kw)


def test_wav_encode_is_declared_and_exported(lib):
    assert "pdse_wav_encode" in lib.EXPORTS and hasattr(lib.load(), "pdse_wav_encode")
    with pytest.raises(lib.PdseError, match="null pointer"):
        lib.wav_encode(None, None, None, None, None, None, None, None, 1, 1, 1, 1, 1, 0, INT, 2, 1)
