"""GPU: the wav encodings beyond integer PCM on the device (csrc/resample.hip: wav_kernel, ``pdse_resample_desc.fmt``) against their
oracle, ``wavio.read_any``: 24-bit PCM, binary32 / binary64, G.711 A-law and mu-law and the integer widths again, 1 to 8 channels,
ragged batches whose utterances start at odd byte offsets, the float special values, a buffer that ends inside a frame, and the
three ``generate_wav`` loops on a directory of such files.  The contract is bit identity with the host path: no tolerance."""
import argparse
import logging
import struct

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INT, FLOAT, ALAW, ULAW = 1, 2, 3, 4                      # include/pdse.h: PDSE_WAV_*
TAG = {INT: 1, FLOAT: 3, ALAW: 6, ULAW: 7}
FORMATS = ((INT, 1), (INT, 2), (INT, 3), (INT, 4), (FLOAT, 4), (FLOAT, 8), (ALAW, 1), (ULAW, 1))
RATES = (16000, 48000, 44100, 8000)                      # ratio 1, 1:3, 160:441, 2:1
COUNTS = ((1, 47, 3001), (3, 2, 443), (2, 3001, 1), (443, 3, 47))     # B = 3 frame counts per channel count; 1- and 3-frame heads
GUID_TAIL = bytes([0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert (lib.WAV_INT, lib.WAV_FLOAT, lib.WAV_ALAW, lib.WAV_ULAW) == (INT, FLOAT, ALAW, ULAW)
    return lib


def _wav_file(path, fmt, width, ch, rate, data, extensible=False):
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else TAG[fmt], ch, rate, rate * ch * width, ch * width, 8 * width)
    if extensible:
        head += struct.pack("<HHIH", 22, 8 * width, 0, TAG[fmt]) + GUID_TAIL
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(head)) + head + b"data" + struct.pack("<I", len(data)) + data
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body + (b"\0" if len(data) & 1 else b""))
    return str(path)


def _payload(rs, fmt, width, n):
    if fmt == FLOAT:
        return rs.uniform(-1.5, 1.5, n).astype("<f4" if width == 4 else "<f8").tobytes()
    return rs.randint(0, 256, n * width).astype(np.uint8).tobytes()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _host(tmp_path, name, fmt, width, ch, rate, raw):
    """``wavio.read_any`` of these frames, through a file: the reference of every row."""
    return torch.from_numpy(pkg("wavio").read_any(_wav_file(tmp_path / name, fmt, width, ch, rate, raw)))


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("fmt,width", FORMATS)
def test_decode_rows_are_read_anys_bits(L, tmp_path, fmt, width, rate):
    wavdev = pkg("wavdev")
    rs = np.random.RandomState(1000 * fmt + 100 * width + rate % 97)
    for ch, counts in zip((1, 2, 3, 8), COUNTS):
        raws = [_payload(rs, fmt, width, n * ch) for n in counts]
        starts = np.cumsum([0] + [len(r) for r in raws[:-1]])
        assert not (width * ch) % 2 or any(int(o) % 2 for o in starts)       # odd frame sizes: an utterance starts at an odd byte
        want = [_host(tmp_path, "c%d_%d.wav" % (ch, i), fmt, width, ch, rate, raw) for i, raw in enumerate(raws)]
        wav, lens = wavdev.decode(raws, ch, width, rate, DEV, fmt=fmt)
        assert lens == [w.numel() for w in want] and tuple(wav.shape) == (3, max(lens))
        got = wav.cpu()
        for b in range(3):
            assert torch.equal(_bits(got[b, :lens[b]]), _bits(want[b])), (ch, b)
            assert not _bits(got[b, lens[b]:]).any(), (ch, b)             # +0.0 up to Lmax
        perm = (2, 0, 1)
        again, plens = wavdev.decode([raws[p] for p in perm], ch, width, rate, DEV, fmt=fmt)
        again = again.cpu()
        for b, p in enumerate(perm):
            assert plens[b] == lens[p] and torch.equal(_bits(again[b, :plens[b]]), _bits(got[p, :lens[p]])), (ch, p)


F32_SPECIALS = (0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000,
                0x7FC00000, 0xFFC12345, 0x7FA00000, 0x7F800001)                              # the last four: NaN, quiet and signalling
F64_SPECIALS = (0.0, -0.0, 1e-40, -1e-40, 2.0 ** -149, 1.5 * 2.0 ** -150, 2.0 ** -150, -1e-46, 1e-320, 3.4028234663852886e38,
                3.4028235e38, 3.4028235677973366e38, 3.5e38, -1e300, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, float("nan"))


def _special_frames(width, ch, n=400):
    """An utterance of n frames of finite samples with the special values at its head (channel 0 of the first frames)."""
    rs = np.random.RandomState(width)
    if width == 4:
        x = rs.uniform(-1, 1, n * ch).astype("<f4")
        x.view("<u4")[0:len(F32_SPECIALS) * ch:ch] = F32_SPECIALS
    else:
        x = rs.uniform(-1, 1, n * ch).astype("<f8")
        x[0:len(F64_SPECIALS) * ch:ch] = F64_SPECIALS
    return x.tobytes()


@pytest.mark.parametrize("width", (4, 8))
def test_float_special_values(L, tmp_path, width):
    """+-0, fp32 subnormals, +-max, binary64 values that round to fp32 subnormals, to zero and beyond the fp32 maximum, NaN: the NaN
    positions agree with ``read_any`` and every other sample is its bits; a mono binary32 file at its own rate keeps every bit,
    NaN payloads included (nothing but moves touches a sample there)."""
    wavdev = pkg("wavdev")
    for ch, rate in ((1, 16000), (2, 16000), (1, 48000), (3, 44100)):
        raw = _special_frames(width, ch)
        with np.errstate(all="ignore"):
            want = _host(tmp_path, "s%d_%d_%d.wav" % (width, ch, rate), FLOAT, width, ch, rate, raw)
        wav, lens = wavdev.decode([raw], ch, width, rate, DEV, fmt=FLOAT)
        got = wav[0].cpu()
        assert lens == [want.numel()]
        nan = torch.isnan(want)
        assert 0 < int(nan.sum()) < want.numel() and torch.equal(torch.isnan(got), nan), (ch, rate)
        assert torch.equal(_bits(got)[~nan], _bits(want)[~nan]), (ch, rate)
        if ch == 1 and rate == 16000:
            if width == 4:
                assert _bits(got)[:len(F32_SPECIALS)].tolist() == [v - (1 << 32) if v >> 31 else v for v in F32_SPECIALS]
            else:
                tiny = float(np.finfo(np.float32).tiny)
                g = got[:len(F64_SPECIALS)].double().tolist()
                assert 0 < g[2] < tiny and -tiny < g[3] < 0 and g[4] == g[5] == 2.0 ** -149 and g[6] == 0     # 2^-150: a tie, to even
                assert g[7] == 0 and np.signbit(got[7].item()) and g[8] == 0
                assert g[9] == g[10] == float(np.finfo(np.float32).max)
                assert g[11] == g[12] == float("inf") and g[13] == -float("inf")       # max + half an ulp: a tie, to 2^128
                assert g[14] == 1.0 and g[15] == 1.0 + 2.0 ** -22                      # ties go to the even neighbour


def test_a_buffer_that_ends_inside_the_last_frame_reads_it_as_zero(L):
    """s24 stereo, 10 frames announced, ``pcm_bytes`` one byte short of them (the allocation itself holds all 60 bytes): the last
    frame decodes to 0.0, the others as ever - at ratio 1 and through the converter."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(77)
    raw = rs.randint(1, 256, 60).astype(np.uint8)
    zeroed = raw.copy()
    zeroed[54:] = 0
    pcm = torch.from_numpy(raw).to(DEV)
    for rate in (16000, 48000):
        want = wavio.decode_frames(zeroed, 2, 3, INT)
        assert want[9] == 0 and want[8] != 0
        want = torch.from_numpy(want if rate == 16000 else wavio.resample(want, rate, 16000))
        taps, up, down, half = wavdev._device_taps(torch.device(DEV), rate, 16000)
        n_out = wavio.out_len(10, rate, 16000)
        meta = torch.zeros(1, dtype=torch.int64, device=DEV)
        host = np.array([10], dtype=np.int32)
        n_in = torch.from_numpy(host).to(DEV)
        out = torch.full((1, n_out + 3), 7.0, device=DEV)
        d = L.ResampleDesc()
        d.pcm, d.offs, d.n_in, d.n_in_host, d.out = pcm.data_ptr(), meta.data_ptr(), n_in.data_ptr(), host.ctypes.data, out.data_ptr()
        d.taps = taps.data_ptr() if taps is not None else None
        d.pcm_bytes, d.B, d.Lmax, d.up, d.down, d.half, d.width, d.ch, d.fmt = 59, 1, n_out + 3, up, down, half, 3, 2, INT
        L.launch(d, torch.cuda.current_stream().cuda_stream, device=torch.device(DEV))
        got = out[0].cpu()
        assert torch.equal(_bits(got[:n_out]), _bits(want)) and not _bits(got[n_out:]).any(), rate
        d.pcm_bytes = 60                                    # the whole buffer: the last frame is there
        L.launch(d, torch.cuda.current_stream().cuda_stream, device=torch.device(DEV))
        full = wavio.decode_frames(raw, 2, 3, INT)
        full = torch.from_numpy(full if rate == 16000 else wavio.resample(full, rate, 16000))
        assert torch.equal(_bits(out[0, :n_out].cpu()), _bits(full)) and not torch.equal(full, want)


def test_fmt_0_and_wav_int_agree_on_16_bit_stereo_48k(L):
    wavdev = pkg("wavdev")
    rs = np.random.RandomState(78)
    raws = [rs.randint(-32768, 32768, 2 * n).astype("<i2").tobytes() for n in (3001, 47, 443)]
    old, lens = wavdev.decode(raws, 2, 2, 48000, DEV)
    new, nlens = wavdev.decode(raws, 2, 2, 48000, DEV, fmt=INT)
    assert lens == nlens == [1001, 16, 148] and torch.equal(_bits(old), _bits(new)) and old.abs().max() > 0.5


def test_load_all_groups_formats_and_takes_the_host_path_for_nine_channels(L, tmp_path):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(79)
    paths = [_wav_file(tmp_path / "a.wav", INT, 3, 2, 48000, _payload(rs, INT, 3, 2 * 901)),
             _wav_file(tmp_path / "b.wav", FLOAT, 4, 1, 16000, _payload(rs, FLOAT, 4, 700)),
             _wav_file(tmp_path / "c.wav", INT, 3, 2, 48000, _payload(rs, INT, 3, 2 * 333)),
             _wav_file(tmp_path / "d.wav", INT, 2, 9, 44100, _payload(rs, INT, 2, 9 * 500)),         # nine channels: read_any on the host
             _wav_file(tmp_path / "e.wav", ULAW, 1, 1, 8000, _payload(rs, ULAW, 1, 801), extensible=True),
             _wav_file(tmp_path / "f.wav", FLOAT, 8, 2, 16000, b"")]                                 # no frames
    wav, lens = wavdev.load(paths, DEV, formats="all")
    want = [torch.from_numpy(wavio.read_any(p)) for p in paths]
    assert lens == [w.numel() for w in want] and lens[5] == 0 and tuple(wav.shape) == (6, max(lens))
    for b, w in enumerate(want):
        assert torch.equal(_bits(wav[b, :lens[b]].cpu()), _bits(w)) and not _bits(wav[b, lens[b]:]).any(), b
    one, n1 = wavdev.load(paths[:1], DEV, formats="all")
    assert n1 == lens[:1] and torch.equal(_bits(one[0]), _bits(wav[0, :lens[0]]))
    bad = _wav_file(tmp_path / "nan.wav", FLOAT, 4, 1, 16000, np.array([0.5, np.nan, 0.25], "<f4").tobytes())
    with pytest.raises(ValueError, match=r"nan\.wav.*not finite"):
        wavdev.load([paths[1], bad], DEV, formats="all")
    for p in paths[:3] + [bad]:                                 # the default reads none of them
        with pytest.raises((ValueError, EOFError, wavio.wave.Error)):
            wavdev.load([p], DEV)


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


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    """s24 48 kHz stereo, f32 16 kHz mono, mu-law 8 kHz, extensible 16-bit 5.1 at 44.1 kHz and an f32 file with one NaN; 0.2 s
    each (0.18 s the last)."""
    rs = np.random.RandomState(80)
    data = tmp_path_factory.mktemp("wavfmt") / "noisy"
    data.mkdir()
    s24 = (0.1 * 2 ** 23 * rs.standard_normal(2 * 9600)).clip(-2 ** 23, 2 ** 23 - 1).astype("<i4")
    s24 = s24.view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    f32 = (0.1 * rs.standard_normal(3200)).astype("<f4")
    nan = (0.1 * rs.standard_normal(2880)).astype("<f4")
    nan[1234] = np.nan
    s16 = (0.1 * 32768 * rs.standard_normal(6 * 8820)).clip(-32768, 32767).astype("<i2")
    return [_wav_file(data / "a_s24.wav", INT, 3, 2, 48000, s24),
            _wav_file(data / "b_f32.wav", FLOAT, 4, 1, 16000, f32.tobytes()),
            _wav_file(data / "c_nan.wav", FLOAT, 4, 1, 16000, nan.tobytes()),
            _wav_file(data / "d_ulaw.wav", ULAW, 1, 1, 8000, rs.randint(0, 256, 1600).astype(np.uint8).tobytes()),
            _wav_file(data / "e_51.wav", INT, 2, 6, 44100, s16.tobytes(), extensible=True)]


@pytest.fixture(scope="module")
def reference(directory, weights, tmp_path_factory):
    """``read_any``'s waveforms through ``enhance`` with the x_T draws of the file loop (seed 55, the discards of ``rng_fidelity``
    behind every file, none for the NaN file): the bytes every loop form has to write, and the generator state it has to leave."""
    wavio = pkg("wavio")
    tmp = tmp_path_factory.mktemp("wavfmt_ref")
    t = _trainer(weights, tmp / "unused")
    _seed(55)
    out = {}
    for p in directory:
        if p.endswith("c_nan.wav"):
            continue
        wav = torch.from_numpy(wavio.read_any(p))[None]
        assert wav.shape[1] == 3200
        shape = (1, 2, 1 + wav.shape[1] // 160, 161)
        x_T = torch.randn(*shape, device=DEV, dtype=torch.float32)
        y = t.enhance(wav, x_T=x_T)[0].cpu().numpy()
        for _ in range(len(t._pipes[next(reversed(t._pipes))].schedule[0]) - 1):
            torch.randn(*shape, device=DEV, dtype=torch.float32)
        ref = str(tmp / p.split("/")[-1])
        wavio.write_wav(ref, y, 16000)
        out[p.split("/")[-1]] = open(ref, "rb").read()
    return out, torch.cuda.get_rng_state(DEV)


@pytest.mark.parametrize("form", ({}, {"inflight": 2}, {"batch": 2}), ids=("one", "inflight", "batch"))
def test_generate_wav_all_formats_writes_the_read_any_bytes(L, weights, directory, reference, tmp_path, caplog, form):
    want, rng = reference
    tr = _trainer(weights, tmp_path / "out", wav_formats="all")
    _seed(55)
    with caplog.at_level(logging.WARNING):
        written = tr.generate_wav(load_pre_train=False, data_path=directory[0].rsplit("/", 1)[0], **form)
    assert [w.split("/")[-1] for w in written] == ["a_s24.wav", "b_f32.wav", "d_ulaw.wav", "e_51.wav"]
    skipped = [r.getMessage() for r in caplog.records if "skipping" in r.getMessage()]
    assert len(skipped) == 1 and "c_nan.wav" in skipped[0]
    for w in written:
        got = open(w, "rb").read()
        assert len(got) >= 44 + 2 * 3200 and got == want[w.split("/")[-1]], w
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng)        # the NaN file drew nothing


def test_the_default_trainer_skips_all_five(L, weights, directory, tmp_path, caplog):
    tr = _trainer(weights, tmp_path / "out")
    assert tr.wav_formats == "pcm"
    with caplog.at_level(logging.WARNING):
        written = tr.generate_wav(load_pre_train=False, data_path=directory[0].rsplit("/", 1)[0])
    skipped = [r.getMessage() for r in caplog.records if "skipping" in r.getMessage()]
    assert written == [] and len(skipped) == 5 and all(p in " ".join(skipped) for p in directory)
