"""Wav input on the device: a file's raw PCM frames go to HBM as they are, and one launch (csrc/resample.hip, include/pdse.h:
pdse_resample_desc) decodes them, mixes two channels to mono and converts the rate to 16 kHz.  The result is bit-identical to
``wavio.read_wav`` - the kernel repeats its arithmetic operation for operation - without the host's float64 polyphase loop in
front of every pass (DESIGN.md 4.6 and profiles/wav_frontend_timing.txt hold the file-loop times measured on the MI355X machine).

    load(paths, device)                               -> (wav [B, Lmax] fp32 device tensor, lens)
    decode(pcm_list, channels, width, rate, device)   -> the same for callers that already hold frames

Files of one call that differ in rate or format take one launch per (channels, width, rate).  What the kernel does not cover -
more than two channels, a file without frames, a rate pair whose input window per workgroup passes the kernel's 64 KB of LDS
(input rates above about 900 kHz) - is read with ``wavio.read_wav`` and uploaded, as before.  There is no CPU
fallback for the kernel itself.  The tap table of a rate pair is uploaded once per device and kept; nothing else persists
between calls.

``load(..., formats="all")`` and ``decode(..., fmt=WAV_*)`` (opt-in; the defaults are the paragraph above, bit for bit) read what
else a RIFF/WAVE file holds - 24-bit PCM, IEEE float of 32 and 64 bits, G.711 A-law and mu-law, WAVE_FORMAT_EXTENSIBLE headers, up
to eight channels - with ``wavio.read_frames`` and the second kernel of csrc/resample.hip; the oracle is then ``wavio.read_any``.

The way back (opt-in: ``generate_wav`` of a trainer built with ``wav_out="source"``), at the end of the file:

    encode(rows, lens, device, rate, fmt, width, ch, n_keep=None)   -> (list of bytes objects, list of clip counts)

one launch of csrc/wavout.hip (include/pdse.h: pdse_wav_encode) converts enhanced waveforms to their sources' rate, encodes them
as 16-, 24- or 32-bit PCM or binary32 and interleaves the channels; the oracle is ``wavio.resample`` + ``wavio.encode``.

Per-channel enhancement (opt-in: a trainer built with ``channels="each"``) keeps a file's channels apart both ways:

    load(paths, device, formats=..., channels="each")                 -> (wav [R, Lmax], lens [R], chans [len(paths)])
    decode(..., split=True)                                           -> (wav [B * ch, Lmax], lens [B * ch])
    encode_channels(rows, lens, chans, device, rate, fmt, width, n_keep=None) -> (list of bytes objects, list of per-channel counts)

the split mode of the front end's second kernel (``L.WAV_SPLIT``; the oracle is ``wavio.read_channels``) and the channel encoder of
csrc/wavout.hip (pdse_wav_encode_channels; ``wavio.resample`` per row + ``wavio.encode_channels``)."""
import numpy as np

from . import _lib as L
from . import wavio

_TAPS = {}      # (device, sr_in, sr_out) -> (uploaded table or None, up, down, half)


def _device_taps(device, sr_in, sr_out):
    import torch

    key = (device.type, device.index if device.index is not None else torch.cuda.current_device(), int(sr_in), int(sr_out))
    if key not in _TAPS:
        h, up, down, half = wavio.taps(sr_in, sr_out)
        # pageable host memory: the copy returns only when the data is on the device (see metrics._device_tables)
        _TAPS[key] = (None if h is None else torch.from_numpy(h).to(device), up, down, half)
    return _TAPS[key]


def kernel_covers(channels, n_frames, rate, sr=16000, max_channels=2):
    """Whether csrc/resample.hip takes such a file: one or two channels (``max_channels``: ``L.WAV_MAX_CH`` for the kernel of
    fmt != 0), at least one frame, and an input window of one workgroup's
    outputs ((RESAMPLE_BLOCK - 1) down / up + 2 jmax + 2 fp32 samples, include/pdse.h) within 64 KB of LDS."""
    if channels > max_channels or n_frames < 1:
        return False
    up, down, half = _ratio(rate, sr)
    return up == down or 4 * ((L.RESAMPLE_BLOCK - 1) * down // up + 2 * (half // up + 1) + 2) <= 64 * 1024


def _ratio(rate, sr, half_width=16):
    """(up, down, half) of ``wavio.taps`` without building the table."""
    from math import gcd

    g = gcd(int(rate), int(sr))
    up, down = int(sr) // g, int(rate) // g
    return up, down, half_width * max(up, down)


def decode(pcm_list, channels, width, rate, device, sr=16000, fmt=0, split=False):
    """pcm_list: the interleaved little-endian PCM frames of B utterances of one format, each a uint8 array (or bytes) of whole
    frames (``wavio.read_pcm``); channels 1 or 2, width 1, 2 or 4 bytes, every utterance at least one frame long.
    Returns (wav, lens): wav [B, Lmax] fp32 on ``device`` with utterance b in wav[b, :lens[b]] - ``wavio.read_wav``'s samples bit
    for bit - and zeros behind it.  Two uploads and one launch on the current stream; asynchronous.
    fmt (default 0: the above): ``L.WAV_INT`` (width 1 .. 4), ``L.WAV_FLOAT`` (width 4 or 8), ``L.WAV_ALAW`` or ``L.WAV_ULAW``
    (width 1) with 1 .. 8 channels takes the kernel of the other encodings (``wavio.read_frames``); the rows are then
    ``wavio.read_any``'s bits.  The library refuses every other combination before the launch.
    split=True keeps the channels apart (``L.WAV_SPLIT``; fmt 0 is taken as ``L.WAV_INT``, which decodes the same widths): wav
    [B * channels, Lmax] and lens [B * channels], row b * channels + c being channel c of utterance b at the utterance's length -
    ``wavio.read_channels``'s rows bit for bit."""
    import torch

    device = torch.device(device)
    if device.type != "cuda":
        raise L.PdseError("wavdev.decode runs on the GPU only (no CPU fallback); wavio.read_wav is the host path")
    frame = int(channels) * int(width)
    bufs = [np.frombuffer(p, dtype=np.uint8) if isinstance(p, (bytes, bytearray, memoryview)) else
            np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in pcm_list]
    B = len(bufs)
    if B < 1:
        raise ValueError("an empty batch has nothing to decode")
    if any(p.size % frame for p in bufs):
        raise ValueError("pcm_list: whole frames only (%d bytes each)" % frame)
    n_in = np.array([p.size // frame for p in bufs], dtype=np.int64)
    if n_in.max() >= 2 ** 31:
        raise ValueError("an utterance of 2^31 frames or more")
    taps, up, down, half = _device_taps(device, rate, sr)
    lens = [wavio.out_len(int(n), rate, sr) for n in n_in]
    Lmax = max(max(lens), 1)
    # one int64 array carries both per-utterance tables: B byte offsets, then the B frame counts as int32
    meta = np.zeros(B + (B + 1) // 2, dtype=np.int64)
    meta[1:B] = np.cumsum([p.size for p in bufs])[:-1]
    n_in32 = meta[B:].view(np.int32)
    n_in32[:B] = n_in
    pcm = bufs[0] if B == 1 else np.concatenate(bufs)
    if pcm.size == 0:
        pcm = np.zeros(1, dtype=np.uint8)       # a non-null buffer; validation reports the empty utterance
    with torch.cuda.device(device):
        pcm_dev = torch.from_numpy(pcm if pcm.flags.writeable else pcm.copy()).to(device)
        meta_dev = torch.from_numpy(meta).to(device)
        if split:
            fmt = (int(fmt) or L.WAV_INT) | L.WAV_SPLIT
            lens = [n for n in lens for _ in range(int(channels))]
        out = torch.empty(len(lens) if split else B, Lmax, dtype=torch.float32, device=device)
        d = L.ResampleDesc()
        d.pcm, d.offs, d.n_in, d.n_in_host = pcm_dev.data_ptr(), meta_dev.data_ptr(), meta_dev.data_ptr() + 8 * B, n_in32.ctypes.data
        d.taps, d.out = (taps.data_ptr() if taps is not None else None), out.data_ptr()
        d.pcm_bytes, d.B, d.Lmax = int(pcm.size), B, Lmax
        d.up, d.down, d.half, d.width, d.ch, d.fmt = up, down, half, int(width), int(channels), int(fmt)
        L.launch(d, torch.cuda.current_stream(device).cuda_stream, device=device)
    return out, lens


def load(paths, device, sr=16000, formats="pcm", channels="mix"):
    """Read wav files and bring them to ``sr`` mono fp32 on the device: (wav [B, Lmax], lens) with file b in wav[b, :lens[b]],
    equal to ``wavio.read_wav(paths[b], sr)`` bit for bit, zeros behind it.  Raises what ``wavio.read_wav`` raises for a file it
    cannot read.
    formats="all": the files are opened with ``wavio.read_frames`` (24-bit, float, G.711, extensible headers, up to 8 channels on
    the device) and every row is ``wavio.read_any``'s; only files with more channels, without frames or with a rate pair beyond the
    kernel's window take ``read_any`` on the host.  A float file whose decoded samples are not all finite raises ValueError
    naming it (one ``isfinite().all()`` per float row, a synchronisation; integer files are not looked at).
    channels="each" (default "mix": the above, with the above's return value) keeps the channels apart: (wav [R, Lmax], lens [R],
    chans [len(paths)]) with one row per channel, in file order, then channel order - file i's rows start at sum(chans[:i]) - each
    ``wavio.read_channels``'s row bit for bit.  Every file is opened with ``wavio.read_frames`` and decoded by the kernel's split
    mode (``decode(split=True)``), whatever ``formats`` is; formats="pcm" still refuses, with the same exception, what
    ``wavio.read_wav`` refuses.  More than 8 channels, no frames or a rate pair beyond the kernel's window:
    ``wavio.read_channels`` on the host.  The finiteness check of float files applies per row."""
    import torch

    device = torch.device(device)
    if channels == "each":
        if formats not in ("pcm", "all"):
            raise ValueError("formats must be 'pcm' or 'all', got %r" % (formats,))
        return _load_each(paths, device, sr, formats)
    if channels != "mix":
        raise ValueError("channels must be 'mix' or 'each', got %r" % (channels,))
    if formats == "all":
        return _load_all(paths, device, sr)
    if formats != "pcm":
        raise ValueError("formats must be 'pcm' or 'all', got %r" % (formats,))
    rows, groups = [None] * len(paths), {}
    for i, path in enumerate(paths):
        frames, n, ch, width, rate = wavio.read_pcm(path)
        if not kernel_covers(ch, n, rate, sr):
            rows[i] = torch.from_numpy(wavio.read_wav(path, sr)).to(device)      # the host path, unchanged
        else:
            groups.setdefault((ch, width, rate), []).append((i, frames))
    if len(groups) == 1 and all(r is None for r in rows):                        # the common case: one launch is the result
        (ch, width, rate), items = next(iter(groups.items()))
        return decode([f for _, f in items], ch, width, rate, device, sr)
    for (ch, width, rate), items in groups.items():
        wav, lens = decode([f for _, f in items], ch, width, rate, device, sr)
        for (i, _), row, n in zip(items, wav, lens):
            rows[i] = row[:n]
    lens = [int(r.numel()) for r in rows]
    out = torch.zeros(len(rows), max(lens + [0]), dtype=torch.float32, device=device)
    for i, r in enumerate(rows):
        out[i, :lens[i]] = r
    return out, lens


def _load_all(paths, device, sr):
    """``load(formats="all")``: one launch per (fmt, channels, width, rate)."""
    import torch

    rows, groups = [None] * len(paths), {}
    for i, path in enumerate(paths):
        frames, n, ch, width, rate, fmt = wavio.read_frames(path)
        if not kernel_covers(ch, n, rate, sr, max_channels=L.WAV_MAX_CH):
            rows[i] = torch.from_numpy(wavio.read_any(path, sr)).to(device)
            if fmt == wavio.WAV_FLOAT:
                _finite(rows[i], path)
        else:
            groups.setdefault((fmt, ch, width, rate), []).append((i, frames))
    one = len(groups) == 1 and all(r is None for r in rows)
    for (fmt, ch, width, rate), items in groups.items():
        wav, lens = decode([f for _, f in items], ch, width, rate, device, sr, fmt=fmt)
        if fmt == wavio.WAV_FLOAT:
            for (i, _), row, n in zip(items, wav, lens):
                _finite(row[:n], paths[i])
        if one:
            return wav, lens
        for (i, _), row, n in zip(items, wav, lens):
            rows[i] = row[:n]
    lens = [int(r.numel()) for r in rows]
    out = torch.zeros(len(rows), max(lens + [0]), dtype=torch.float32, device=device)
    for i, r in enumerate(rows):
        out[i, :lens[i]] = r
    return out, lens


def _load_each(paths, device, sr, formats):
    """``load(channels="each")``: one split launch per (fmt, channels, width, rate)."""
    import torch

    files, groups, is_float = [None] * len(paths), {}, []    # files[i]: the [ch, n] rows of file i
    for i, path in enumerate(paths):
        if formats == "pcm":
            wavio.read_pcm(path)                             # raises what ``read_wav`` raises; the frames are read_frames' below
        frames, n, ch, width, rate, fmt = wavio.read_frames(path)
        is_float.append(fmt == wavio.WAV_FLOAT)
        if not kernel_covers(ch, n, rate, sr, max_channels=L.WAV_MAX_CH):
            files[i] = torch.from_numpy(wavio.read_channels(path, sr)).to(device)
        else:
            groups.setdefault((fmt, ch, width, rate), []).append((i, frames))
    chans = [None] * len(paths)
    one = len(groups) == 1 and all(f is None for f in files)
    for (fmt, ch, width, rate), items in groups.items():
        wav, lens = decode([f for _, f in items], ch, width, rate, device, sr, fmt=fmt, split=True)
        for k, (i, _) in enumerate(items):
            files[i] = wav[k * ch:(k + 1) * ch, :lens[k * ch]]
        if one:
            result = wav, lens
    for i, f in enumerate(files):
        chans[i] = int(f.shape[0])
        if is_float[i]:                                      # finite in every channel
            for c in range(chans[i]):
                _finite(f[c], "%s (channel %d)" % (paths[i], c) if chans[i] > 1 else paths[i])
    if one:
        return result[0], result[1], chans
    lens = [int(f.shape[1]) for f in files for _ in range(f.shape[0])]
    out = torch.zeros(len(lens), max(lens + [0]), dtype=torch.float32, device=device)
    r = 0
    for f in files:
        out[r:r + f.shape[0], :f.shape[1]] = f
        r += f.shape[0]
    return out, lens, chans


def _finite(row, path):
    import torch

    if not bool(torch.isfinite(row).all()):
        raise ValueError("%s: float samples that are not finite" % path)


# ---- the way back (opt-in: generate_wav(wav_out="source")): csrc/wavout.hip, include/pdse.h: the wav back end -------------------
def encoder_covers(rate, sr=16000, ch=None):
    """Whether csrc/wavout.hip converts ``sr`` to ``rate``: the input window of one workgroup's frames ((RESAMPLE_BLOCK - 1) down /
    up + 2 jmax + 2 fp32 samples) beside the 8 KB image of its bytes within 64 KB of LDS (output rates down to about 300 Hz).
    ch: the question for the channel encoder (``encode_channels``), which stages ``ch`` such windows."""
    up, down, half = _ratio(sr, rate)
    if ch is not None:
        return up == down or 4 * int(ch) * ((L.RESAMPLE_BLOCK - 1) * down // up + 2 * (half // up + 1) + 2) + L.WAVCH_STATIC_BYTES <= 64 * 1024
    return up == down or 4 * ((L.RESAMPLE_BLOCK - 1) * down // up + 2 * (half // up + 1) + 2) + L.WAVOUT_IMAGE_BYTES + 64 <= 64 * 1024


def encode(rows, lens, device, rate, fmt, width, ch, n_keep=None, sr=16000):
    """The frames of B waveforms at ``sr`` as their files hold them at ``rate``: (list of bytes objects, list of clip counts).
    rows: a [B, Lmax] fp32 tensor on ``device`` with waveform b in rows[b, :lens[b]] (what ``load`` returns, what ``enhance``
    gives back), or a list of 1-D tensors; fmt ``L.WAV_INT`` with width 2, 3 or 4 bytes or ``L.WAV_FLOAT`` with width 4; every one
    of the ``ch`` channels (1 .. 8) carries the waveform.  n_keep[b] (default: all ``wavio.out_len(lens[b], sr, rate)`` of them)
    cuts file b to its first frames.  Element b is ``wavio.encode(wavio.resample(row_b, sr, rate)[:n_keep[b]], fmt, width, ch)``
    byte for byte, and its clip count - the samples the integer clamp changed - is the host's.  One upload (the lengths), one
    launch on the current stream, one copy back that carries the frames and the per-workgroup clip counts together.  A rate pair
    the kernel's LDS window does not hold (``encoder_covers``) takes those host functions instead; the kernel itself has no CPU
    fallback."""
    out, keep, counts = encode_rows(rows, lens, device, rate, fmt, width, ch, n_keep, sr)
    fb = int(ch) * int(width)
    return [out[b, :keep[b] * fb].tobytes() for b in range(len(keep))], counts


def encode_rows(rows, lens, device, rate, fmt, width, ch, n_keep=None, sr=16000):
    """``encode`` before the rows are cut: (out, n_keep, clip counts) with out a uint8 array [B, stride] on the host, row b holding
    n_keep[b] * ch * width bytes of frames and zeros behind them (the kernel's buffer as it came back)."""
    import torch

    device = torch.device(device)
    if device.type != "cuda":
        raise L.PdseError("wavdev.encode runs on the GPU only (no CPU fallback); wavio.encode is the host path")
    wavio._check_target(fmt, width, ch)
    if not torch.is_tensor(rows):
        rows = torch.nn.utils.rnn.pad_sequence([torch.as_tensor(r, dtype=torch.float32).flatten().to(device) for r in rows], batch_first=True)
    rows = rows.to(device, torch.float32).contiguous()
    if rows.dim() != 2 or rows.shape[0] != len(lens) or rows.shape[0] < 1:
        raise ValueError("rows: [B, Lmax] with one length per row")
    B, Lmax = int(rows.shape[0]), int(rows.shape[1])
    lens = [int(n) for n in lens]
    if any(n < 1 or n > Lmax for n in lens):
        raise ValueError("lens: 1 .. %d samples per row" % Lmax)
    n_out = [wavio.out_len(n, sr, rate) for n in lens]
    keep = n_out if n_keep is None else [int(k) for k in n_keep]
    if len(keep) != B or any(k < 0 or k > n for k, n in zip(keep, n_out)):
        raise ValueError("n_keep: one count per row, at most the frames the row converts to")
    fb = int(ch) * int(width)
    stride = max(max(keep) * fb, 1)
    if not encoder_covers(rate, sr):
        host = rows.cpu().numpy()
        out, counts = np.zeros((B, stride), dtype=np.uint8), []
        for b in range(B):
            with np.errstate(over="ignore", invalid="ignore"):
                y = wavio.resample(host[b, :lens[b]], sr, rate)[:keep[b]]
            payload, clipped = wavio.encode(y, fmt, width, ch)
            out[b, :len(payload)] = np.frombuffer(payload, dtype=np.uint8)
            counts.append(clipped)
        return out, keep, counts
    taps, up, down, half = _device_taps(device, sr, rate)
    blocks = -(-stride // (L.RESAMPLE_BLOCK * fb))
    counts_at = -(-B * stride // 4) * 4                      # the int32 counts behind the rows, in the same buffer: one copy back
    meta = np.array(lens + keep, dtype=np.int32)
    with torch.cuda.device(device):
        meta_dev = torch.from_numpy(meta).to(device)
        buf = torch.empty(counts_at + 4 * B * blocks, dtype=torch.uint8, device=device)
        L.wav_encode(rows.data_ptr(), meta.ctypes.data, meta.ctypes.data + 4 * B, meta_dev.data_ptr(), meta_dev.data_ptr() + 4 * B,
                     taps.data_ptr() if taps is not None else None, buf.data_ptr(), buf.data_ptr() + counts_at,
                     stride, B, Lmax, up, down, half, fmt, width, ch,
                     stream=torch.cuda.current_stream(device).cuda_stream, device=device)
        host = buf.cpu().numpy()
    counts = host[counts_at:].view(np.int32).reshape(B, blocks).sum(axis=1)
    return host[:B * stride].reshape(B, stride), keep, [int(c) for c in counts]


def encode_channels(rows, lens, chans, device, rate, fmt, width, n_keep=None, sr=16000):
    """``encode`` for files whose channels differ: (list of bytes objects, list of per-channel clip-count lists), one of each per
    file.  rows: a [R, Lmax] fp32 tensor on ``device`` (or a list of 1-D tensors) with one row per channel, in file order, then
    channel order, as ``load(channels="each")`` returns them; lens [R]: the rows' lengths, equal within a file; chans: the files'
    channel counts (1 .. 8 each, sum R); n_keep[i] (per file; default: all ``wavio.out_len(len_i, sr, rate)`` frames) cuts file i
    to its first frames.  Element i is ``wavio.encode_channels`` of the file's rows after ``wavio.resample(row, sr, rate)[:n_keep[i]]``,
    bytes and counts.  One upload (the lengths), one launch of csrc/wavout.hip's channel encoder (include/pdse.h:
    pdse_wav_encode_channels) and one copy back per distinct channel count.  A rate pair whose ``ch`` windows the kernel's LDS
    does not hold (``encoder_covers(rate, sr, ch)``) takes those host functions; the kernel itself has no CPU fallback."""
    import torch

    device = torch.device(device)
    if device.type != "cuda":
        raise L.PdseError("wavdev.encode_channels runs on the GPU only (no CPU fallback); wavio.encode_channels is the host path")
    chans = [int(c) for c in chans]
    for ch in sorted(set(chans)):
        wavio._check_target(fmt, width, ch)
    if not torch.is_tensor(rows):
        rows = torch.nn.utils.rnn.pad_sequence([torch.as_tensor(r, dtype=torch.float32).flatten().to(device) for r in rows], batch_first=True)
    rows = rows.to(device, torch.float32).contiguous()
    if rows.dim() != 2 or rows.shape[0] != len(lens) or rows.shape[0] != sum(chans) or rows.shape[0] < 1:
        raise ValueError("rows: [R, Lmax] with one length per row and R the sum of the channel counts")
    Lmax = int(rows.shape[1])
    lens = [int(n) for n in lens]
    if any(n < 1 or n > Lmax for n in lens):
        raise ValueError("lens: 1 .. %d samples per row" % Lmax)
    first = [sum(chans[:i]) for i in range(len(chans))]      # a file's first row
    if any(len(set(lens[r:r + ch])) != 1 for r, ch in zip(first, chans)):
        raise ValueError("lens: the rows of a file have one length")
    flen = [lens[r] for r in first]
    n_out = [wavio.out_len(n, sr, rate) for n in flen]
    keep = n_out if n_keep is None else [int(k) for k in n_keep]
    if len(keep) != len(chans) or any(k < 0 or k > n for k, n in zip(keep, n_out)):
        raise ValueError("n_keep: one count per file, at most the frames the file converts to")
    payloads, counts = [None] * len(chans), [None] * len(chans)
    for ch in sorted(set(chans)):
        ids = [i for i, c in enumerate(chans) if c == ch]
        B, fb = len(ids), ch * int(width)
        k_ch, n_ch = [keep[i] for i in ids], [flen[i] for i in ids]
        x = rows if B == len(chans) else rows[[first[i] + c for i in ids for c in range(ch)]]
        if not encoder_covers(rate, sr, ch):
            host = x.cpu().numpy()
            for b, i in enumerate(ids):
                with np.errstate(over="ignore", invalid="ignore"):
                    y = [wavio.resample(host[b * ch + c, :n_ch[b]], sr, rate)[:k_ch[b]] for c in range(ch)]
                payloads[i], counts[i] = wavio.encode_channels(np.stack(y), fmt, width)
            continue
        stride = max(max(k_ch) * fb, 1)
        taps, up, down, half = _device_taps(device, sr, rate)
        blocks = -(-stride // (L.RESAMPLE_BLOCK * fb))
        counts_at = -(-B * stride // 4) * 4                  # the int32 counts behind the files' bytes, in the same buffer: one copy back
        meta = np.array(n_ch + k_ch, dtype=np.int32)
        with torch.cuda.device(device):
            meta_dev = torch.from_numpy(meta).to(device)
            buf = torch.empty(counts_at + 4 * B * blocks * ch, dtype=torch.uint8, device=device)
            L.wav_encode_channels(x.data_ptr(), meta.ctypes.data, meta.ctypes.data + 4 * B, meta_dev.data_ptr(), meta_dev.data_ptr() + 4 * B,
                                  taps.data_ptr() if taps is not None else None, buf.data_ptr(), buf.data_ptr() + counts_at,
                                  stride, B, Lmax, up, down, half, fmt, width, ch,
                                  stream=torch.cuda.current_stream(device).cuda_stream, device=device)
            host = buf.cpu().numpy()
        per = host[counts_at:].view(np.int32).reshape(B, blocks, ch).sum(axis=1)
        for b, i in enumerate(ids):
            payloads[i] = host[b * stride:b * stride + k_ch[b] * fb].tobytes()
            counts[i] = [int(c) for c in per[b]]
    return payloads, counts
