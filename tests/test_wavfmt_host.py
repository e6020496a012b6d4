"""CPU: the host side of the wav encodings beyond integer PCM (``wavio.read_frames`` / ``wavio.read_any``, the ``fmt`` word of
``pdse_resample_desc``).  Files are written here with ``struct`` - plain and WAVE_FORMAT_EXTENSIBLE headers - for every (format,
width) and 1, 2, 3 and 6 channels; ``read_frames`` must hand out the written bytes and fields, ``read_any`` must equal a decode
written independently in this file (``np.frombuffer`` views, s24 by byte arithmetic, both G.711 tables spelled out) and, where
``read_wav`` opens the file, ``read_wav`` bit for bit.  No tolerance anywhere."""
import ctypes as C
import os
import struct
import wave

import numpy as np
import pytest

from conftest import pkg

INT, FLOAT, ALAW, ULAW = 1, 2, 3, 4                      # include/pdse.h: PDSE_WAV_*
TAG = {INT: 1, FLOAT: 3, ALAW: 6, ULAW: 7}
FORMATS = ((INT, 1), (INT, 2), (INT, 3), (INT, 4), (FLOAT, 4), (FLOAT, 8), (ALAW, 1), (ULAW, 1))
GUID_TAIL = bytes([0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])

# ITU-T G.711: the 16-bit linear value of each of the 256 codes
ALAW_TABLE = (
    -5504, -5248, -6016, -5760, -4480, -4224, -4992, -4736, -7552, -7296, -8064, -7808, -6528, -6272, -7040, -6784,
    -2752, -2624, -3008, -2880, -2240, -2112, -2496, -2368, -3776, -3648, -4032, -3904, -3264, -3136, -3520, -3392,
    -22016, -20992, -24064, -23040, -17920, -16896, -19968, -18944, -30208, -29184, -32256, -31232, -26112, -25088, -28160, -27136,
    -11008, -10496, -12032, -11520, -8960, -8448, -9984, -9472, -15104, -14592, -16128, -15616, -13056, -12544, -14080, -13568,
    -344, -328, -376, -360, -280, -264, -312, -296, -472, -456, -504, -488, -408, -392, -440, -424,
    -88, -72, -120, -104, -24, -8, -56, -40, -216, -200, -248, -232, -152, -136, -184, -168,
    -1376, -1312, -1504, -1440, -1120, -1056, -1248, -1184, -1888, -1824, -2016, -1952, -1632, -1568, -1760, -1696,
    -688, -656, -752, -720, -560, -528, -624, -592, -944, -912, -1008, -976, -816, -784, -880, -848,
    5504, 5248, 6016, 5760, 4480, 4224, 4992, 4736, 7552, 7296, 8064, 7808, 6528, 6272, 7040, 6784,
    2752, 2624, 3008, 2880, 2240, 2112, 2496, 2368, 3776, 3648, 4032, 3904, 3264, 3136, 3520, 3392,
    22016, 20992, 24064, 23040, 17920, 16896, 19968, 18944, 30208, 29184, 32256, 31232, 26112, 25088, 28160, 27136,
    11008, 10496, 12032, 11520, 8960, 8448, 9984, 9472, 15104, 14592, 16128, 15616, 13056, 12544, 14080, 13568,
    344, 328, 376, 360, 280, 264, 312, 296, 472, 456, 504, 488, 408, 392, 440, 424,
    88, 72, 120, 104, 24, 8, 56, 40, 216, 200, 248, 232, 152, 136, 184, 168,
    1376, 1312, 1504, 1440, 1120, 1056, 1248, 1184, 1888, 1824, 2016, 1952, 1632, 1568, 1760, 1696,
    688, 656, 752, 720, 560, 528, 624, 592, 944, 912, 1008, 976, 816, 784, 880, 848)
ULAW_TABLE = (
    -32124, -31100, -30076, -29052, -28028, -27004, -25980, -24956, -23932, -22908, -21884, -20860, -19836, -18812, -17788, -16764,
    -15996, -15484, -14972, -14460, -13948, -13436, -12924, -12412, -11900, -11388, -10876, -10364, -9852, -9340, -8828, -8316,
    -7932, -7676, -7420, -7164, -6908, -6652, -6396, -6140, -5884, -5628, -5372, -5116, -4860, -4604, -4348, -4092,
    -3900, -3772, -3644, -3516, -3388, -3260, -3132, -3004, -2876, -2748, -2620, -2492, -2364, -2236, -2108, -1980,
    -1884, -1820, -1756, -1692, -1628, -1564, -1500, -1436, -1372, -1308, -1244, -1180, -1116, -1052, -988, -924,
    -876, -844, -812, -780, -748, -716, -684, -652, -620, -588, -556, -524, -492, -460, -428, -396,
    -372, -356, -340, -324, -308, -292, -276, -260, -244, -228, -212, -196, -180, -164, -148, -132,
    -120, -112, -104, -96, -88, -80, -72, -64, -56, -48, -40, -32, -24, -16, -8, 0,
    32124, 31100, 30076, 29052, 28028, 27004, 25980, 24956, 23932, 22908, 21884, 20860, 19836, 18812, 17788, 16764,
    15996, 15484, 14972, 14460, 13948, 13436, 12924, 12412, 11900, 11388, 10876, 10364, 9852, 9340, 8828, 8316,
    7932, 7676, 7420, 7164, 6908, 6652, 6396, 6140, 5884, 5628, 5372, 5116, 4860, 4604, 4348, 4092,
    3900, 3772, 3644, 3516, 3388, 3260, 3132, 3004, 2876, 2748, 2620, 2492, 2364, 2236, 2108, 1980,
    1884, 1820, 1756, 1692, 1628, 1564, 1500, 1436, 1372, 1308, 1244, 1180, 1116, 1052, 988, 924,
    876, 844, 812, 780, 748, 716, 684, 652, 620, 588, 556, 524, 492, 460, 428, 396,
    372, 356, 340, 324, 308, 292, 276, 260, 244, 228, 212, 196, 180, 164, 148, 132,
    120, 112, 104, 96, 88, 80, 72, 64, 56, 48, 40, 32, 24, 16, 8, 0)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return pkg("_lib")


def fmt_chunk(fmt, width, ch, rate, extensible, align=None, guid_tail=GUID_TAIL):
    align = ch * width if align is None else align
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else TAG[fmt], ch, rate, rate * align, align, 8 * width)
    if extensible:          # cbSize 22, valid bits, channel mask, SubFormat {tag, 0000-0010-8000-00AA00389B71}
        head += struct.pack("<HHIH", 22, 8 * width, 0, TAG[fmt]) + guid_tail
    return head


def riff(chunks):
    body = b"WAVE"
    for cid, data in chunks:
        body += cid + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def wav_bytes(fmt, width, ch, rate, data, extensible=False, **kw):
    return riff([(b"fmt ", fmt_chunk(fmt, width, ch, rate, extensible, **kw)), (b"data", data)])


def payload(rs, fmt, width, n):
    """n samples of random bytes - every code, every bit pattern of the integers - or, for floats, finite values around +-1."""
    if fmt == FLOAT:
        return rs.uniform(-1.5, 1.5, n).astype("<f4" if width == 4 else "<f8").tobytes()
    return rs.randint(0, 256, n * width).astype(np.uint8).tobytes()


def independent_decode(raw, fmt, width, ch):
    """Not the code under test: ``np.frombuffer`` views, s24 by byte arithmetic, the G.711 tables above; the mix is the fp32
    sum in channel order and one division."""
    f32 = np.float32
    if fmt == INT and width == 1:
        x = (np.frombuffer(raw, np.uint8).astype(f32) - f32(128)) / f32(128)
    elif fmt == INT and width == 2:
        x = np.frombuffer(raw, "<i2").astype(f32) / f32(32768)
    elif fmt == INT and width == 4:
        x = np.frombuffer(raw, "<i4").astype(f32) / f32(2147483648)
    elif fmt == INT:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int64)
        v = b[:, 0] + 256 * b[:, 1] + 65536 * b[:, 2]
        v = np.where(v >= 2 ** 23, v - 2 ** 24, v)
        x = v.astype(f32) / f32(8388608)
    elif fmt == FLOAT and width == 4:
        x = np.frombuffer(raw, "<f4").copy()
    elif fmt == FLOAT:
        with np.errstate(over="ignore", invalid="ignore"):
            x = np.frombuffer(raw, "<f8").astype(f32)
    else:
        table = np.array(ALAW_TABLE if fmt == ALAW else ULAW_TABLE, dtype=np.int32)
        x = table[np.frombuffer(raw, np.uint8)].astype(f32) / f32(32768)
    if ch == 1:
        return x
    acc = x[0::ch].copy()
    for c in range(1, ch):
        acc = acc + x[c::ch]
    return acc / f32(ch)


def same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_g711_expansions_reproduce_the_tables():
    wavio = pkg("wavio")
    alaw, ulaw = wavio._g711_tables()
    assert alaw.tolist() == list(ALAW_TABLE) and ulaw.tolist() == list(ULAW_TABLE)
    assert len(set(ALAW_TABLE)) == 256 and len(set(ULAW_TABLE)) == 255          # mu-law has two zeros


def test_g711_tables_against_audioop():
    audioop = pytest.importorskip("audioop")
    codes = bytes(range(256))
    assert np.frombuffer(audioop.alaw2lin(codes, 2), "<i2").tolist() == list(ALAW_TABLE)
    assert np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2").tolist() == list(ULAW_TABLE)


@pytest.mark.parametrize("extensible", (False, True))
@pytest.mark.parametrize("fmt,width", FORMATS)
def test_read_frames_and_read_any_for_every_format(tmp_path, fmt, width, extensible):
    wavio = pkg("wavio")
    assert (wavio.WAV_INT, wavio.WAV_FLOAT, wavio.WAV_ALAW, wavio.WAV_ULAW) == (INT, FLOAT, ALAW, ULAW)
    rs = np.random.RandomState(100 * fmt + 10 * width + extensible)
    for ch in (1, 2, 3, 6):
        n = 257 + ch
        rate = (8000, 16000, 44100, 48000)[ch % 4]
        raw = payload(rs, fmt, width, n * ch)
        path = tmp_path / ("f%d_w%d_c%d.wav" % (fmt, width, ch))
        path.write_bytes(wav_bytes(fmt, width, ch, rate, raw, extensible))
        frames, n_frames, c, w, r, f = wavio.read_frames(str(path))
        assert frames.dtype == np.uint8 and frames.tobytes() == raw
        assert (n_frames, c, w, r, f) == (n, ch, width, rate, fmt)
        want = independent_decode(raw, fmt, width, ch)
        got = wavio.read_any(str(path), sr=rate)
        assert same_bits(got, want), (fmt, width, ch)
        assert same_bits(wavio.decode_frames(frames, ch, width, fmt), want)
        # at 16 kHz: the existing converter on those samples
        assert same_bits(wavio.read_any(str(path)), want if rate == 16000 else wavio.resample(want, rate, 16000))


def test_float_specials_decode_as_the_formats_say(tmp_path):
    wavio = pkg("wavio")
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00001, 0x7FA00000, 0x3F800000],
                    dtype="<u4")
    path = tmp_path / "f32.wav"
    path.write_bytes(wav_bytes(FLOAT, 4, 1, 16000, bits.tobytes()))
    assert wavio.read_any(str(path)).view(np.uint32).tolist() == bits.tolist()          # NaN payloads included
    d = np.array([0.0, -0.0, 1e-40, -1e-46, 2.0 ** -150, 3.5e38, -1e300, float(np.finfo(np.float32).max), 0.1], dtype="<f8")
    path = tmp_path / "f64.wav"
    path.write_bytes(wav_bytes(FLOAT, 8, 1, 16000, d.tobytes()))
    got = wavio.read_any(str(path))
    with np.errstate(over="ignore"):
        assert same_bits(got, d.astype(np.float32))
    assert got[2] > 0 and got[2] < np.finfo(np.float32).tiny and got[3] == 0 and np.signbit(got[3]) and got[4] == 0
    assert got[5] == np.inf and got[6] == -np.inf and got[7] == np.finfo(np.float32).max


@pytest.mark.parametrize("width", (1, 2, 4))
@pytest.mark.parametrize("ch", (1, 2))
def test_read_any_is_read_wav_where_read_wav_reads(tmp_path, width, ch):
    wavio = pkg("wavio")
    rs = np.random.RandomState(7 * width + ch)
    for rate in (16000, 44100, 48000):
        raw = payload(rs, INT, width, (300 + rate % 11) * ch)
        path = tmp_path / ("w%d_c%d_%d.wav" % (width, ch, rate))
        with wave.open(str(path), "wb") as f:                 # the writer the existing tests use
            f.setnchannels(ch)
            f.setsampwidth(width)
            f.setframerate(rate)
            f.writeframes(raw)
        for sr in (16000, rate):
            assert same_bits(wavio.read_any(str(path), sr), wavio.read_wav(str(path), sr)), (width, ch, rate, sr)
        assert wavio.read_frames(str(path))[0].tobytes() == wavio.read_pcm(str(path))[0].tobytes() == raw


def test_refusals_name_the_file(tmp_path):
    wavio = pkg("wavio")
    good = wav_bytes(INT, 2, 2, 48000, np.arange(400, dtype="<i2").tobytes())
    ext = wav_bytes(INT, 2, 2, 48000, bytes(400), extensible=True)
    cases = {
        "tag3_16bit.wav": good[:20] + struct.pack("<H", 3) + good[22:],            # as tests/test_wavdev_host.py fabricates it
        "ext_short_fmt.wav": good[:20] + struct.pack("<H", 0xFFFE) + good[22:],    # tag 0xFFFE in a 16-byte fmt chunk
        "ext_cbsize.wav": ext[:36] + struct.pack("<H", 0) + ext[38:],              # cbSize < 22
        "wrong_guid.wav": wav_bytes(INT, 2, 2, 48000, bytes(400), extensible=True, guid_tail=GUID_TAIL[:-1] + b"\x72"),
        "wrong_align.wav": wav_bytes(INT, 2, 2, 48000, bytes(400), align=2),
        "cut_in_frame.wav": good[:-3],
        "rifx.wav": b"RIFX" + good[4:],
        "rf64.wav": b"RF64" + good[4:],
        "adpcm.wav": good[:20] + struct.pack("<H", 2) + good[22:],
        "float16.wav": wav_bytes(FLOAT, 2, 1, 16000, bytes(64)),
        "float24.wav": wav_bytes(FLOAT, 3, 1, 16000, bytes(66)),
        "ulaw16.wav": wav_bytes(ULAW, 2, 1, 8000, bytes(64)),
        "alaw16.wav": wav_bytes(ALAW, 2, 1, 8000, bytes(64)),
        "pcm40.wav": wav_bytes(INT, 5, 1, 16000, bytes(65)),
        "short_fmt.wav": riff([(b"fmt ", fmt_chunk(INT, 2, 1, 16000, False)[:14]), (b"data", bytes(8))]),
        "no_data.wav": riff([(b"fmt ", fmt_chunk(INT, 2, 1, 16000, False))]),
        "empty.wav": b"",
    }
    for name, data in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        for read in (wavio.read_frames, wavio.read_any):
            with pytest.raises(ValueError, match=name.replace(".", r"\.")):
                read(str(path))
    # cut at a frame boundary: a shorter file
    path = tmp_path / "short.wav"
    path.write_bytes(good[:-8])
    assert wavio.read_frames(str(path))[1] == 198


def test_chunk_walk_pad_bytes_and_data_sizes_beyond_the_file(tmp_path):
    wavio = pkg("wavio")
    raw = np.arange(-150, 150, dtype="<i2").tobytes()
    fmt = fmt_chunk(INT, 2, 1, 16000, False)
    path = tmp_path / "list.wav"                  # an odd-sized LIST chunk (7 bytes + pad) and an odd-sized unknown one before data
    path.write_bytes(riff([(b"fmt ", fmt), (b"LIST", b"INFOabc"), (b"junk", b"\xff"), (b"data", raw), (b"tail", b"xyz")]))
    frames, n, ch, width, rate, f = wavio.read_frames(str(path))
    assert frames.tobytes() == raw and (n, ch, width, rate, f) == (300, 1, 2, 16000, INT)
    plain = wavio.read_any(str(path))
    assert same_bits(plain, np.arange(-150, 150).astype(np.float32) / np.float32(32768))
    # without honouring the pad byte the walk would land one byte early and find no data chunk: show that the pad is there
    blob = path.read_bytes()
    assert blob[12 + 8 + 16 + 8 + 7:][:1] == b"\0" and blob[12 + 8 + 16 + 8 + 8:][:4] == b"junk"
    # a fmt chunk of 18 bytes (cbSize 0), as many writers emit for float and G.711
    path = tmp_path / "fmt18.wav"
    path.write_bytes(riff([(b"fmt ", fmt_chunk(ULAW, 1, 1, 8000, False) + b"\0\0"), (b"fact", struct.pack("<I", 300)), (b"data", raw[:300])]))
    assert wavio.read_frames(str(path))[1:] == (300, 1, 1, 8000, ULAW)
    # a writer on a pipe: data size 0xFFFFFFFF (and a RIFF size of the same kind); the chunk is clamped to the end of the file
    head = b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", 0xFFFFFFFF)
    path = tmp_path / "pipe.wav"
    path.write_bytes(head + raw)
    assert wavio.read_frames(str(path))[0].tobytes() == raw
    path.write_bytes(head + raw + b"\x01")        # ... and then ends inside a frame
    with pytest.raises(ValueError, match="inside a frame"):
        wavio.read_frames(str(path))


def test_more_channels_than_two_follow_the_channel_order_sum(tmp_path):
    """``read_wav`` takes numpy's mean over the channel axis; ``read_any`` sums in channel order, and the docstring says that the
    two may differ.  Either sum of six samples of magnitude <= 1 makes five roundings of at most 2^-22 (half an ulp below 8) before
    the division by 6 and one of at most 2^-25 after it: the two results lie within 2 (5 * 2^-22 / 6 + 2^-25) < 2^-20."""
    wavio = pkg("wavio")
    rs = np.random.RandomState(5)
    raw = rs.randint(-32768, 32768, 6 * 500).astype("<i2")
    path = tmp_path / "six.wav"
    path.write_bytes(wav_bytes(INT, 2, 6, 16000, raw.tobytes()))
    got, mean = wavio.read_any(str(path)), wavio.read_wav(str(path))
    assert same_bits(got, independent_decode(raw.tobytes(), INT, 2, 6))
    assert np.abs(got.astype(np.float64) - mean).max() < 2.0 ** -20
    assert "last bit" in wavio.read_any.__doc__


def test_descriptor_keeps_its_layout_with_fmt_where_the_pad_was(lib):
    names = [n for n, _ in lib.ResampleDesc._fields_]
    assert names[-1] == "fmt" and "pad_" not in names
    assert lib.ResampleDesc.fmt.offset == 84 and lib.ResampleDesc.fmt.size == 4 and lib.ResampleDesc.ch.offset == 80
    assert C.sizeof(lib.ResampleDesc) == 88 == lib.load().pdse_desc_size(lib.OP_RESAMPLE)
    assert lib.ResampleDesc.pcm_bytes.offset == 48 and lib.ABI_VERSION == 9
    assert (lib.WAV_INT, lib.WAV_FLOAT, lib.WAV_ALAW, lib.WAV_ULAW, lib.WAV_MAX_CH) == (1, 2, 3, 4, 8)
    root = os.path.dirname(os.path.dirname(os.path.abspath(lib.__file__)))
    header = open(os.path.join(root, "include", "pdse.h")).read()
    for name, value in (("INT", 1), ("FLOAT", 2), ("ALAW", 3), ("ULAW", 4), ("MAX_CH", 8)):
        assert "#define PDSE_WAV_%s %d\n" % (name, value) in header


def test_fmt_argument_errors_need_no_device(lib):
    buf = (C.c_double * 8)()
    host = (C.c_int32 * 1)(100)

    def desc(fmt, width, ch):
        d = lib.ResampleDesc()
        d.pcm = d.offs = d.n_in = d.taps = d.out = C.addressof(buf)
        d.n_in_host = C.addressof(host)
        d.pcm_bytes, d.B, d.Lmax = 64, 1, 34
        d.up, d.down, d.half, d.width, d.ch, d.fmt = 1, 3, 48, width, ch, fmt
        return d

    for fmt in (-1, 5, 99):
        with pytest.raises(lib.PdseError, match="resample: unknown fmt"):
            lib.launch(desc(fmt, 2, 1))
    for fmt, widths, text in ((INT, (0, 5, 8), "PDSE_WAV_INT takes a width of 1, 2, 3 or 4"),
                              (FLOAT, (1, 2, 3, 16), "PDSE_WAV_FLOAT takes a width of 4 or 8"),
                              (ALAW, (0, 2), "PDSE_WAV_ALAW / _ULAW takes a width of 1"),
                              (ULAW, (2, 4), "PDSE_WAV_ALAW / _ULAW takes a width of 1")):
        for w in widths:
            with pytest.raises(lib.PdseError, match="resample: fmt " + text):
                lib.launch(desc(fmt, w, 1))
    for ch in (0, 9, -1):
        with pytest.raises(lib.PdseError, match=r"resample: with fmt != 0 ch must be 1 \.\. 8"):
            lib.launch(desc(INT, 3, ch))
    # fmt 0 is the operator as it was: the old texts
    with pytest.raises(lib.PdseError, match="resample: width must be 1, 2 or 4 bytes"):
        lib.launch(desc(0, 3, 1))
    with pytest.raises(lib.PdseError, match="resample: ch must be 1 or 2"):
        lib.launch(desc(0, 2, 3))
    # the checks behind width and ch are shared: a valid fmt still reaches them
    d = desc(INT, 3, 8)
    d.Lmax = 33
    with pytest.raises(lib.PdseError, match="resample: n_out > Lmax"):
        lib.launch(d)


def test_load_and_trainer_arguments():
    wavdev, trainer = pkg("wavdev"), pkg("trainer")
    with pytest.raises(ValueError, match="formats must be"):
        wavdev.load([], "cpu", formats="flac")
    assert trainer.ComplexDDPMTrainer.wav_formats == "pcm"
    assert wavdev.kernel_covers(8, 1, 48000, max_channels=8) and not wavdev.kernel_covers(9, 1, 48000, max_channels=8)
    assert not wavdev.kernel_covers(3, 1, 48000)
