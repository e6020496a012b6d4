"""GPU: per-channel enhancement on the device - the split mode of the wav front end (csrc/resample.hip: wav_split_kernel,
``wavdev.decode(split=True)``, ``wavdev.load(channels="each")``) against ``wavio.read_channels``, the channel encoder (csrc/wavout.hip:
wavch_kernel, ``wavdev.encode_channels``) against ``wavio.resample`` + ``wavio.encode_channels``, both bit for bit, and the file loop
of a trainer built with ``channels="each"`` against the same trainer on the directory of the split mono files."""
import argparse
import logging

import numpy as np
import pytest
import torch

from conftest import pkg, rel_l2
from helpers.wavch_cases import FLOAT, FORMATS, INT, NAMES, payload, rows_signal, split_files, wav_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATES = (16000, 48000, 44100, 8000)                      # ratio 1 (no LDS), 1:3, 160:441 (the 14113-tap table), 2:1 (upsampling)
OUT_LENS = (255, 256, 257, 513)                          # around the workgroup's 256 outputs, and a third workgroup
TARGETS = ((INT, 2), (INT, 3), (INT, 4), (FLOAT, 4))
TOL = 1e-4                                               # the suite's rel-L2 (tests/test_gpu_ragged.py); the persistent LSTM is 1e-5 away


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge

    ge.build()
    lib = pkg("_lib")
    lib.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return lib


def _frames_for(wavio, n_out, rate):
    """The fewest input frames at ``rate`` that convert to ``n_out`` samples at 16 kHz - or, where no count does (8 kHz doubles:
    every length is even), to ``n_out`` + 1."""
    for want in (n_out, n_out + 1):
        for n in range(1, 4 * n_out + 8):
            if wavio.out_len(n, rate, 16000) == want:
                return n
    raise AssertionError((n_out, rate))


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,width", FORMATS, ids=[NAMES[f] for f in FORMATS])
def test_split_rows_are_read_channels_bits(L, tmp_path, fmt, width):
    """Every wav_kernel instantiation's split twin, 2, 3 and 8 channels (3 channels of 3 bytes: frames of 9 bytes, every byte
    offset), four rates, rows that end just before, at and just behind a workgroup's 256 outputs: the four lengths of a (channels,
    rate) are one ragged launch, and row b ch + c is ``read_channels``'s row c of file b with zeros behind it."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(100 * fmt + width)
    for ch in (2, 3, 8):
        for rate in RATES:
            counts = [_frames_for(wavio, n, rate) for n in OUT_LENS]
            frames = [payload(rs, fmt, width, n, ch) for n in counts]
            wav, lens = wavdev.decode([f.reshape(-1) for f in frames], ch, width, rate, DEV, fmt=fmt, split=True)
            assert wav.shape == (4 * ch, max(lens)) and len(lens) == 4 * ch
            wav = wav.cpu()
            for b, f in enumerate(frames):
                path, _ = split_files(tmp_path, "f%d_%d_%d" % (ch, rate, b), fmt, width, rate, f)
                want = torch.from_numpy(wavio.read_channels(path))
                assert lens[b * ch:(b + 1) * ch] == [want.shape[1]] * ch and want.shape[1] in (OUT_LENS[b], OUT_LENS[b] + 1)
                got = wav[b * ch:(b + 1) * ch]
                assert torch.equal(_bits(got[:, :want.shape[1]]), _bits(want)), (ch, rate, b)
                assert not got[:, want.shape[1]:].any(), (ch, rate, b)


def test_rows_do_not_depend_on_the_place_in_the_batch_and_the_dense_call_is_untouched(L, tmp_path):
    """Three 24-bit files of 3 channels and different lengths at 44.1 kHz in one launch, then permuted in a second one: every
    file's rows are the same bits, and ``read_channels``'s.  ``split=False`` on the same frames is still ``read_any`` (the mix),
    fmt 0 with ``split=True`` decodes 16-bit PCM as ``L.WAV_INT`` does, and a mono file's single row is the dense row."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(71)
    frames = [payload(rs, INT, 3, n, 3) for n in (1000, 333, 1414)]
    flat = [f.reshape(-1) for f in frames]
    paths = [split_files(tmp_path, "p%d" % i, INT, 3, 44100, f)[0] for i, f in enumerate(frames)]
    first, lens = wavdev.decode(flat, 3, 3, 44100, DEV, fmt=INT, split=True)
    order = [2, 0, 1]
    second, lens2 = wavdev.decode([flat[i] for i in order], 3, 3, 44100, DEV, fmt=INT, split=True)
    for k, i in enumerate(order):
        n = lens[3 * i]
        assert lens2[3 * k] == n
        want = torch.from_numpy(wavio.read_channels(paths[i]))
        assert torch.equal(_bits(first[3 * i:3 * i + 3, :n].cpu()), _bits(want))
        assert torch.equal(_bits(second[3 * k:3 * k + 3, :n].cpu()), _bits(want))
    dense, dlens = wavdev.decode(flat, 3, 3, 44100, DEV, fmt=INT)
    assert dense.shape[0] == 3 and dlens == lens[::3]
    for i, p in enumerate(paths):
        assert torch.equal(_bits(dense[i, :dlens[i]].cpu()), _bits(torch.from_numpy(wavio.read_any(p))))
    s16 = payload(rs, INT, 2, 700, 2)
    a, la = wavdev.decode([s16.reshape(-1)], 2, 2, 48000, DEV, fmt=0, split=True)
    b, lb = wavdev.decode([s16.reshape(-1)], 2, 2, 48000, DEV, fmt=INT, split=True)
    assert la == lb and torch.equal(_bits(a), _bits(b)) and a.shape[0] == 2 and not torch.equal(a[0], a[1])
    mono = payload(rs, FLOAT, 8, 500, 1)
    a, _ = wavdev.decode([mono.reshape(-1)], 1, 8, 44100, DEV, fmt=FLOAT, split=True)
    b, _ = wavdev.decode([mono.reshape(-1)], 1, 8, 44100, DEV, fmt=FLOAT)
    assert torch.equal(_bits(a), _bits(b))


def test_load_each_groups_files_and_keeps_nan_payloads(L, tmp_path):
    """``load(channels="each")``: mono s16, stereo f32 with a NaN-free payload, 3-channel s24 at another rate and a 9-channel file
    (the host's ``read_channels``) in one call - rows in file order, then channel order.  A binary32 NaN payload in one channel
    passes the decode bit for bit (``decode``), and ``load`` names the file and the channel."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    rs = np.random.RandomState(17)
    specs = (("a", INT, 2, 1, 16000, 900), ("b", FLOAT, 4, 2, 16000, 400), ("c", INT, 3, 3, 44100, 1200), ("d", INT, 2, 9, 48000, 600))
    paths = [split_files(tmp_path, name, fmt, width, rate, payload(rs, fmt, width, n, ch))[0] for name, fmt, width, ch, rate, n in specs]
    for formats in ("all", "pcm"):
        use = paths if formats == "all" else [paths[0], paths[3]]
        wav, lens, chans = wavdev.load(use, DEV, formats=formats, channels="each")
        assert chans == [wavio.probe(p)[1] for p in use] and wav.shape[0] == len(lens) == sum(chans)
        r = 0
        for p, ch in zip(use, chans):
            want = torch.from_numpy(wavio.read_channels(p))
            assert lens[r:r + ch] == [want.shape[1]] * ch
            assert torch.equal(_bits(wav[r:r + ch, :want.shape[1]].cpu()), _bits(want)), p
            assert not wav[r:r + ch, want.shape[1]:].any()
            r += ch
    with pytest.raises(wavio.wave.Error):                              # formats="pcm" still refuses what read_wav refuses
        wavdev.load([paths[1]], DEV, formats="pcm", channels="each")
    one, lens, chans = wavdev.load([paths[2]], DEV, formats="all", channels="each")      # one group: the launch's own tensor
    assert chans == [3] and one.shape == (3, lens[0])
    special = np.array([0x7FC00001, 0x7F800001, 0xFFC12345, 0x00000001, 0x80000000], dtype="<u4")
    other = (0.3 * rs.standard_normal(special.size)).astype("<f4")
    frames = np.stack([special.view(np.uint8).reshape(-1, 4), other.view(np.uint8).reshape(-1, 4)], axis=1)
    got, _ = wavdev.decode([frames.reshape(-1)], 2, 4, 16000, DEV, fmt=FLOAT, split=True)
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), special) and np.array_equal(got[1].cpu().numpy().view(np.uint32), other.view(np.uint32))
    nan = tmp_path / "nan.wav"
    nan.write_bytes(wav_bytes(FLOAT, 4, 2, 16000, frames.tobytes()))
    with pytest.raises(ValueError, match=r"nan\.wav \(channel 0\): float samples that are not finite"):
        wavdev.load([str(nan)], DEV, formats="all", channels="each")


# ---- encode -----------------------------------------------------------------------------------------------------------------------
def _host(wavio, x, rate, fmt, width, keep):
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.stack([wavio.resample(row, 16000, rate)[:keep] for row in x])
    return wavio.encode_channels(y, fmt, width)


@pytest.mark.parametrize("fmt,width", TARGETS)
def test_files_are_resample_and_encode_channels_byte_for_byte(L, fmt, width):
    """2, 3 and 8 channels (3 x 3 bytes: frames of 9 bytes, a stride that is no multiple of 4) at four rates: two files of
    different lengths and different ``n_keep`` in one launch, frames crossing 256 in both, values the clamp changes - NaN and the
    infinities among them for the integer targets - in one channel only; bytes and per-channel clip counts are the host's."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    seen = 0
    for ch in (2, 3, 8):
        for rate in RATES:
            lens = [700, 257]
            hot = (ch + rate // 1000) % ch                             # the channel that clips
            nonfinite = fmt == INT or rate == 16000                    # binary32 behind a conversion: finite samples (which NaN a sum makes is the processor's business)
            xs = [rows_signal(ch, n, 7 * ch + n + rate % 97, clip_channel=hot if nonfinite else None, width=width) for n in lens]
            if not nonfinite:
                xs[0][hot, 5] = 1.5
            keep = [wavio.out_len(700, 16000, rate) - 3, wavio.out_len(257, 16000, rate)]
            rows = torch.zeros(2 * ch, 700)
            rows[:ch] = torch.from_numpy(xs[0])
            rows[ch:, :257] = torch.from_numpy(xs[1])
            rows[ch:, 257:] = float("nan")                             # behind a row's length: never read
            got, counts = wavdev.encode_channels(rows.to(DEV), [700] * ch + [257] * ch, [ch, ch], DEV, rate, fmt, width, n_keep=keep)
            for b in range(2):
                want, clipped = _host(wavio, xs[b], rate, fmt, width, keep[b])
                assert len(got[b]) == keep[b] * ch * width and got[b] == want, (ch, rate, b)
                assert counts[b] == clipped, (ch, rate, b)
                assert fmt == FLOAT or all(k == 0 for c, k in enumerate(clipped) if c != hot)
                seen += sum(clipped)
    assert (seen > 0) == (fmt == INT)


def test_the_raw_call_writes_zeros_behind_the_kept_frames(L):
    """``pdse_wav_encode_channels`` itself, 3 channels of 24 bits to 48 kHz with a stride beyond both files: every byte of out is
    written - the kept frames, then zeros - and clipped is [B][blocks][ch], zero in the blocks behind the kept frames."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    ch, width, lens = 3, 3, [300, 100]
    keep = [850, 300]                                                  # of 900 and 300 frames
    stride = 903 * ch * width + 2                                      # not a multiple of 4: file 1 starts at an odd alignment
    xs = [rows_signal(ch, n, 90 + n, clip_channel=1, width=width) for n in lens]
    rows = torch.zeros(2 * ch, 300)
    rows[:ch] = torch.from_numpy(xs[0])
    rows[ch:, :100] = torch.from_numpy(xs[1])
    rows = rows.to(DEV)
    taps, up, down, half = wavdev._device_taps(torch.device(DEV), 16000, 48000)
    blocks = -(-stride // (L.RESAMPLE_BLOCK * ch * width))
    meta = np.array(lens + keep, dtype=np.int32)
    meta_dev = torch.from_numpy(meta).to(DEV)
    out = torch.full((2 * stride,), 0xAB, dtype=torch.uint8, device=DEV)
    clipped = torch.full((2, blocks, ch), -1, dtype=torch.int32, device=DEV)
    L.wav_encode_channels(rows.data_ptr(), meta.ctypes.data, meta.ctypes.data + 8, meta_dev.data_ptr(), meta_dev.data_ptr() + 8, taps.data_ptr(),
                          out.data_ptr(), clipped.data_ptr(), stride, 2, 300, up, down, half, INT, width, ch,
                          stream=torch.cuda.current_stream().cuda_stream)
    out, clipped = out.cpu().numpy().reshape(2, stride), clipped.cpu().numpy()
    for b in range(2):
        want, counts = _host(wavio, xs[b], 48000, INT, width, keep[b])
        assert out[b, :len(want)].tobytes() == want and not out[b, len(want):].any(), b
        assert clipped[b].sum(axis=0).tolist() == counts and counts[1] > 0 and counts[0] == counts[2] == 0
        assert not clipped[b, -(-keep[b] // L.RESAMPLE_BLOCK):].any() and (clipped[b] >= 0).all()


def test_equal_rows_give_the_mono_encoders_bytes_and_mixed_channel_counts_are_regrouped(L):
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    x = rows_signal(1, 600, 3, clip_channel=0)[0]
    row = torch.from_numpy(x).to(DEV)
    for (fmt, width), rate, C in zip(TARGETS, (44100, 48000, 8000, 16000), (2, 3, 8, 2)):
        want, clipped = wavdev.encode(row[None], [600], DEV, rate, fmt, width, C)
        got, counts = wavdev.encode_channels(row[None].repeat(C, 1), [600] * C, [C], DEV, rate, fmt, width)
        assert got == want and counts == [[clipped[0]] * C], (fmt, width, rate)
    # files of 2, 1 and 2 channels in one call: one launch per distinct count, results in file order
    xs = [rows_signal(2, 400, 11), rows_signal(1, 300, 12), rows_signal(2, 500, 13)]
    rows = torch.zeros(5, 500)
    r = 0
    for xf in xs:
        rows[r:r + xf.shape[0], :xf.shape[1]] = torch.from_numpy(xf)
        r += xf.shape[0]
    got, counts = wavdev.encode_channels(rows.to(DEV), [400, 400, 300, 500, 500], [2, 1, 2], DEV, 48000, INT, 3)
    for b, xf in enumerate(xs):
        assert (got[b], counts[b]) == _host(wavio, xf, 48000, INT, 3, 3 * xf.shape[1]), b
    with pytest.raises(ValueError, match="one length"):
        wavdev.encode_channels(rows.to(DEV), [400, 399, 300, 500, 500], [2, 1, 2], DEV, 48000, INT, 3)


# ---- the whole path -----------------------------------------------------------------------------------------------------------
def _trainer(weights, out, prior="GCRN", **kw):
    ns = argparse.Namespace
    kw.setdefault("exclusive", False)
    return pkg("trainer").ComplexDDPMTrainer(
        ns(retrain=False, joint=True, draw=False, sigma=False, checkpoint="x", generated_wav=str(out)),
        ns(model=ns(name=prior), train=ns(fft_num=320, win_size=320, win_shift=160, feat_type="sqrt")),
        device=DEV, prior_state_dict=weights(prior), ddpm_state_dict=weights("DiffUNet1"), wav_formats="all", **kw)


def _seed(s):
    torch.manual_seed(s)
    torch.cuda.manual_seed_all(s)


def _speech(rs, n, ch, scale):
    """[n, ch] float64: every channel its own speech-like signal (16-bit headroom kept)."""
    synth = pkg("synth")
    return np.stack([scale * np.asarray(synth.speechlike(1, n, int(rs.randint(1, 10000)))[0], dtype=np.float64) for _ in range(ch)], axis=1)


@pytest.fixture(scope="module")
def directories(tmp_path_factory):
    """``multi``: a.wav mono s16 at 16 kHz (3200 samples), b.wav stereo s16 at 48 kHz (7200 frames: 2400 samples), c.wav 3 channels
    of s24 at 44.1 kHz (5000 frames: 1815 samples) - T <= 21.  ``split``: a.wav and the mono files b_c0 .. c_c2 of the channels, which
    sort where their files stood.  Returns (multi dir, split dir, {name: (rate, ch, tag, width, frames)})."""
    rs = np.random.RandomState(23)
    root = tmp_path_factory.mktemp("wavch")
    multi, split = root / "multi", root / "split"
    multi.mkdir()
    split.mkdir()
    sources = {}
    for name, fmt, width, ch, rate, n in (("a", INT, 2, 1, 16000, 3200), ("b", INT, 2, 2, 48000, 7200), ("c", INT, 3, 3, 44100, 5000)):
        v = np.round(_speech(rs, n, ch, 0.3).clip(-1, 1 - 2.0 ** -15) * 2.0 ** (8 * width - 1)).astype("<i4")
        frames = np.ascontiguousarray(v.view(np.uint8).reshape(n, ch, 4)[:, :, :width])
        split_files(multi, name, fmt, width, rate, frames)
        for c in range(ch):
            (multi / ("%s_c%d.wav" % (name, c))).rename(split / ("%s_c%d.wav" % (name, c)))
        sources[name + ".wav"] = (rate, ch, 1, width, n)
    (split / "a_c0.wav").rename(split / "a.wav")
    return str(multi), str(split), sources


@pytest.fixture(scope="module")
def reference(L, weights, directories, tmp_path_factory):
    """What an ``exclusive=False`` trainer writes for the split mono files, seed 91, with ``wav_out`` "source" and "pcm16"."""
    _, split, _ = directories
    out = {}
    for wav_out in ("source", "pcm16"):
        tr = _trainer(weights, tmp_path_factory.mktemp("wavch_ref_" + wav_out), wav_out=wav_out)
        _seed(91)
        written = tr.generate_wav(load_pre_train=False, data_path=split)
        assert len(written) == 6
        out[wav_out] = {w.split("/")[-1]: w for w in written}
    return out


def _channels_of(wavio, path):
    frames, n, ch, width, rate, fmt = wavio.read_frames(path)
    return frames.reshape(n, ch, width), (rate, ch, width, n, fmt)


def _check_against_split(wavio, written, sources, ref, source_format):
    assert [w.split("/")[-1] for w in written] == sorted(sources)
    for w in written:
        name = w.split("/")[-1]
        rate, ch, tag, width, n = sources[name]
        got, head = _channels_of(wavio, w)
        assert head == ((rate, ch, width, n, INT) if source_format else (16000, ch, 2, wavio.out_len(n, rate, 16000), INT)), name
        for c in range(ch):
            mono, mhead = _channels_of(wavio, ref[name if ch == 1 else "%s_c%d.wav" % (name[:-4], c)])
            assert mhead == head[:1] + (1,) + head[2:]
            assert got[:, c].tobytes() == mono[:, 0].tobytes(), (name, c)
        if ch == 1:
            assert open(w, "rb").read() == open(ref[name], "rb").read()        # a mono file: the very file, header included
        else:
            assert got[:, 0].tobytes() != got[:, 1].tobytes(), name            # different content in, different content out


@pytest.mark.parametrize("form", ({}, {"batch": 4}, {"inflight": 2}), ids=("one", "batch", "inflight"))
@pytest.mark.parametrize("wav_out", ("source", "pcm16"))
def test_every_channel_is_what_the_split_file_gives(L, weights, directories, reference, tmp_path, caplog, wav_out, form):
    wavio = pkg("wavio")
    multi, _, sources = directories
    tr = _trainer(weights, tmp_path / "out", wav_out=wav_out, channels="each")
    _seed(91)
    with caplog.at_level(logging.WARNING):
        written = tr.generate_wav(load_pre_train=False, data_path=multi, **form)
    _check_against_split(wavio, written, sources, reference[wav_out], wav_out == "source")
    # synthetic weights: the enhancer's output leaves +-1, so a file may log its clip warning - one per file, per channel for b and c
    warned = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert all("clipped" in m for m in warned) and len({m.split(":")[0] for m in warned}) == len(warned) <= 3
    assert all(("samples per channel" in m) == (not m.split(":")[0].endswith("a.wav")) for m in warned)


def test_the_mix_is_todays_output(L, weights, directories, tmp_path):
    """``channels="mix"`` (the default) on the same directory: b.wav is ``wavdev.encode(..., ch=2)`` of the mix's result - both
    channels the same bytes - and differs from what "each" wrote."""
    wavio, wavdev = pkg("wavio"), pkg("wavdev")
    multi, _, sources = directories
    tr = _trainer(weights, tmp_path / "out", wav_out="source")
    assert tr.channels == "mix"
    _seed(91)
    written = tr.generate_wav(load_pre_train=False, data_path=multi)
    _seed(91)
    shape = (1, 2, 21, 161)
    x_T = torch.randn(*shape, device=DEV, dtype=torch.float32)         # a.wav's draw, then its discards
    y = tr.enhance(torch.from_numpy(wavio.read_any(multi + "/a.wav"))[None], x_T=x_T)
    for _ in range(len(tr._pipes[next(reversed(tr._pipes))].schedule[0]) - 1):
        torch.randn(*shape, device=DEV, dtype=torch.float32)
    x_T = torch.randn(1, 2, 16, 161, device=DEV, dtype=torch.float32)
    y = tr.enhance(torch.from_numpy(wavio.read_any(multi + "/b.wav"))[None], x_T=x_T)
    (want,), _ = wavdev.encode(y, [2400], DEV, 48000, INT, 2, 2, n_keep=[7200])
    got, head = _channels_of(wavio, written[1])
    assert head == (48000, 2, 2, 7200, INT) and got.tobytes() == want
    assert got[:, 0].tobytes() == got[:, 1].tobytes()


def test_the_default_trainer_holds_the_contract_within_the_persistent_lstm_difference(L, weights, directories, tmp_path):
    """``exclusive=True``: ``enhance`` at B = 1 and the B = C ragged pass may take different LSTM launches, 1e-5 apart; channel c of
    b.wav and c.wav against the same trainer's files for the split directory, rel-L2 of the decoded samples within the suite's 1e-4."""
    wavio = pkg("wavio")
    multi, split, sources = directories
    outs = []
    for src, channels in ((split, "mix"), (multi, "each")):
        tr = _trainer(weights, tmp_path / channels, wav_out="source", channels=channels, exclusive=True)
        assert tr.exclusive
        _seed(91)
        outs.append({w.split("/")[-1]: w for w in tr.generate_wav(load_pre_train=False, data_path=src)})
    ref, got = outs
    for name in ("b.wav", "c.wav"):
        rate, ch = sources[name][:2]
        rows = wavio.read_channels(got[name], sr=rate)
        for c in range(ch):
            err = rel_l2(rows[c], wavio.read_any(ref["%s_c%d.wav" % (name[:-4], c)], sr=rate))
            print("%s channel %d: rel-L2 %.3e" % (name, c, err))
            assert err <= TOL, (name, c, err)


def test_a_db_aiat_prior_needs_masked_prior_and_then_matches_its_split_files(L, weights, directories, tmp_path):
    wavio = pkg("wavio")
    multi, split, sources = directories
    prior = "aia_complex_trans_ri"
    stereo, monos = tmp_path / "stereo", tmp_path / "monos"
    stereo.mkdir()
    monos.mkdir()
    (stereo / "b.wav").write_bytes(open(multi + "/b.wav", "rb").read())
    for c in range(2):
        (monos / ("b_c%d.wav" % c)).write_bytes(open(split + "/b_c%d.wav" % c, "rb").read())
    with pytest.raises(ValueError, match="bidirectional GRU"):
        _trainer(weights, tmp_path / "no", prior=prior, wav_out="source", channels="each").generate_wav(load_pre_train=False, data_path=str(stereo))
    outs = []
    for src, channels in ((monos, "mix"), (stereo, "each")):
        tr = _trainer(weights, tmp_path / channels, prior=prior, wav_out="source", channels=channels, masked_prior=True)
        _seed(92)
        outs.append(tr.generate_wav(load_pre_train=False, data_path=str(src)))
    got, head = _channels_of(wavio, outs[1][0])
    assert head == (48000, 2, 2, 7200, INT)
    for c in range(2):
        assert got[:, c].tobytes() == _channels_of(wavio, outs[0][c])[0].tobytes(), c
    assert got[:, 0].tobytes() != got[:, 1].tobytes()


def test_one_clip_warning_with_the_counts_per_channel(L, weights, directories, tmp_path, caplog):
    """The writer alone: 3 clipped samples in channel 1 of a stereo result, none in channel 0."""
    multi, _, _ = directories
    tr = _trainer(weights, tmp_path / "out", wav_out="pcm16", channels="each")
    (tmp_path / "out").mkdir()
    y = rows_signal(2, 2400, 8)
    y[1, [7, 900, 2399]] = [1.0, -3.0, np.nan]
    with caplog.at_level(logging.WARNING):
        tr._write_wav(str(tmp_path / "out" / "b.wav"), torch.from_numpy(y).to(DEV), multi + "/b.wav")
    warned = [r.getMessage() for r in caplog.records if "clipped" in r.getMessage()]
    assert len(warned) == 1 and "b.wav" in warned[0] and "0/3 of 2400 samples per channel" in warned[0]
    frames = pkg("wavio").read_frames(str(tmp_path / "out" / "b.wav"))
    assert frames[1:] == (2400, 2, 2, 16000, INT)
    for c in range(2):
        assert frames[0].reshape(2400, 2, 2)[:, c].tobytes() == pkg("wavio").encode(y[c], INT, 2, 1)[0]
