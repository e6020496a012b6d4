"""16-bit / float PCM wav read+write with the standard library only (the reference uses
librosa.load(sr=16000) and soundfile.write, trainer/complex_ddpm_trainer.py:921, :1018;
neither is a dependency of this package).  Precondition: RIFF/WAVE PCM (8/16/32-bit integer); files the ``wave``
module rejects (IEEE float, WAVE_FORMAT_EXTENSIBLE) raise and ``generate_wav`` skips them with a warning.  Other
sample rates are converted with a Kaiser-windowed-sinc polyphase filter; librosa's default (soxr_hq) is a
different filter of similar quality, so resampled inputs agree with the reference's to filter-design accuracy
(about -80 dB), not bit for bit.
``read_frames`` / ``read_any`` at the end of the file (opt-in: ``wav_formats="all"``) open the other RIFF/WAVE encodings -
24-bit PCM, IEEE float, G.711, WAVE_FORMAT_EXTENSIBLE - with a chunk walker of their own; ``read_wav`` / ``read_pcm`` do not."""
import wave
from math import gcd

import numpy as np


def resample(x, sr_in, sr_out, half_width=16, beta=8.6):
    """Rational-rate conversion: out[n] = sum_k h(n * down - k * up) x[k] with a Kaiser-windowed sinc low-pass at
    the narrower Nyquist band, evaluated polyphase (only the taps that meet a non-zero input sample)."""
    x = np.asarray(x, dtype=np.float64)
    if sr_in == sr_out or x.size == 0:
        return x.astype(np.float32)
    g = gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    m = max(up, down)
    half = half_width * m                                     # filter half length on the up-sampled grid
    n_h = np.arange(-half, half + 1)
    h = np.sinc(n_h / m) / m * np.kaiser(2 * half + 1, beta) * up
    n_out = int(np.ceil(x.size * up / down))
    out = np.zeros(n_out)
    n = np.arange(n_out)
    q = n * down                                              # position of output n on the up-sampled grid
    k_c, r = q // up, q % up                                  # nearest input sample at or before it, offset in between
    jmax = half // up + 1
    for j in range(-jmax, jmax + 1):                          # input sample k_c - j sits at grid offset r + j * up
        off = r + j * up
        k = k_c - j
        ok = (np.abs(off) <= half) & (k >= 0) & (k < x.size)
        out[ok] += h[off[ok] + half] * x[k[ok]]
    return out.astype(np.float32)


def read_wav(path, sr=16000):
    with wave.open(path, "rb") as f:
        n, ch, width, rate = f.getnframes(), f.getnchannels(), f.getsampwidth(), f.getframerate()
        raw = f.readframes(n)
    if width == 2:
        x = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif width == 4:
        x = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    elif width == 1:
        x = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    else:
        raise ValueError("unsupported sample width %d in %s" % (width, path))
    if ch > 1:
        x = x.reshape(-1, ch).mean(axis=1)  # librosa.load(mono=True)
    if rate != sr:
        x = resample(x, rate, sr)        # librosa.load(sr=16000) resamples (VoiceBank-DEMAND ships at 48 kHz)
    return x


def write_wav(path, x, sr=16000):
    """soundfile.write default subtype for .wav: PCM_16."""
    y = np.clip(np.asarray(x, dtype=np.float64), -1.0, 1.0 - 1.0 / 32768.0)
    pcm = np.round(y * 32768.0).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(pcm.tobytes())


# ---- the pieces of read_wav / resample the device front end needs (prior-diffuse_amd/wavdev.py, csrc/resample.hip) -------------
def taps(sr_in, sr_out, half_width=16, beta=8.6):
    """(h, up, down, half): the float64 tap table ``resample`` builds for this rate pair (the same expression, so the same
    bits), 2 * half + 1 values, and its polyphase constants.  ``up == down`` (equal rates) needs no filter; h is then None."""
    g = gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    m = max(up, down)
    half = half_width * m
    if up == down:
        return None, up, down, half
    n_h = np.arange(-half, half + 1)
    h = np.sinc(n_h / m) / m * np.kaiser(2 * half + 1, beta) * up
    return h, up, down, half


def out_len(n, sr_in, sr_out):
    """Samples ``resample`` returns for n input samples."""
    if sr_in == sr_out or n == 0:
        return int(n)
    g = gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    return int(np.ceil(n * up / down))


def read_pcm(path):
    """(frames, n_frames, channels, width, rate): the file's interleaved little-endian PCM frames as a uint8 array, undecoded.
    Goes through the ``wave`` module like ``read_wav`` and raises what it raises for the same files: wave.Error / EOFError for
    headers ``wave`` rejects, ValueError for a sample width other than 1, 2 or 4 bytes or a data chunk that ends inside a frame."""
    with wave.open(path, "rb") as f:
        n, ch, width, rate = f.getnframes(), f.getnchannels(), f.getsampwidth(), f.getframerate()
        raw = f.readframes(n)
    if width not in (1, 2, 4):
        raise ValueError("unsupported sample width %d in %s" % (width, path))
    if len(raw) % (ch * width):
        raise ValueError("%s: the data chunk ends inside a frame (%d bytes, %d per frame)" % (path, len(raw), ch * width))
    return np.frombuffer(raw, dtype=np.uint8), len(raw) // (ch * width), ch, width, rate


# ---- every RIFF/WAVE encoding libsndfile reads from such a file (``formats="all"``: wavdev.load, generate_wav(wav_formats="all")) ----
WAV_INT, WAV_FLOAT, WAV_ALAW, WAV_ULAW = 1, 2, 3, 4           # include/pdse.h: PDSE_WAV_*, pdse_resample_desc.fmt
_TAG_FMT = {1: WAV_INT, 3: WAV_FLOAT, 6: WAV_ALAW, 7: WAV_ULAW}      # wFormatTag: PCM, IEEE_FLOAT, ALAW, MULAW
_GUID_TAIL = bytes.fromhex("000000001000800000AA00389B71")           # KSDATAFORMAT_SUBTYPE_*: {tag, 0000-0010-8000-00AA00389B71}
_WIDTHS = {WAV_INT: (1, 2, 3, 4), WAV_FLOAT: (4, 8), WAV_ALAW: (1,), WAV_ULAW: (1,)}


def read_frames(path):
    """(frames, n_frames, channels, width, rate, fmt): the interleaved little-endian frames of a RIFF/WAVE file as a uint8 array,
    undecoded, with ``fmt`` one of WAV_INT (u8, s16, s24, s32), WAV_FLOAT (binary32, binary64), WAV_ALAW, WAV_ULAW (G.711, one
    byte).  A RIFF walker of its own - the ``wave`` module stops at everything but integer PCM: the chunks are walked with the pad
    byte behind an odd-sized one, format tags 1, 3, 6, 7 are taken from a plain ``fmt `` chunk (16 bytes or more) or from the
    SubFormat GUID of WAVE_FORMAT_EXTENSIBLE (40 bytes or more, cbSize >= 22); the container size decides the width and the
    valid-bits word is ignored, as libsndfile does.  A ``data`` size that runs past the end of the file - 0xFFFFFFFF from a
    writer on a pipe - is clamped to the end.  ValueError, naming the file, for everything else: RIFX, RF64, other tags, a block
    align that is not channels * width, a width the format does not have, a data chunk that ends inside a frame."""
    import struct

    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 12 or buf[:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file (%r)" % (path, buf[:4]))
    pos, fmt_chunk, data = 12, None, None
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], struct.unpack_from("<I", buf, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt " and fmt_chunk is None:
            fmt_chunk = buf[body:body + size]
            if len(fmt_chunk) < size:
                raise ValueError("%s: the file ends inside the fmt chunk" % path)
        elif cid == b"data":
            if fmt_chunk is None:
                raise ValueError("%s: data chunk before the fmt chunk" % path)
            data = buf[body:min(body + size, len(buf))]
            break
        pos = body + size + (size & 1)
    if fmt_chunk is None or data is None:
        raise ValueError("%s: no %s chunk" % (path, "fmt" if fmt_chunk is None else "data"))
    if len(fmt_chunk) < 16:
        raise ValueError("%s: fmt chunk of %d bytes" % (path, len(fmt_chunk)))
    tag, ch, rate, _, align, bits = struct.unpack_from("<HHIIHH", fmt_chunk)
    if tag == 0xFFFE:
        if len(fmt_chunk) < 40 or struct.unpack_from("<H", fmt_chunk, 16)[0] < 22:
            raise ValueError("%s: WAVE_FORMAT_EXTENSIBLE with a fmt chunk of %d bytes" % (path, len(fmt_chunk)))
        if fmt_chunk[26:40] != _GUID_TAIL:
            raise ValueError("%s: unknown SubFormat GUID %s" % (path, fmt_chunk[24:40].hex()))
        tag = struct.unpack_from("<H", fmt_chunk, 24)[0]
    if tag not in _TAG_FMT:
        raise ValueError("%s: unsupported format tag 0x%04X" % (path, tag))
    fmt = _TAG_FMT[tag]
    if bits % 8 or bits // 8 not in _WIDTHS[fmt]:
        raise ValueError("%s: %d bits per sample with format tag %d" % (path, bits, tag))
    width = bits // 8
    if ch < 1 or rate < 1:
        raise ValueError("%s: %d channels at %d Hz" % (path, ch, rate))
    if align != ch * width:
        raise ValueError("%s: block align %d with %d channels of %d bytes" % (path, align, ch, width))
    if len(data) % align:
        raise ValueError("%s: the data chunk ends inside a frame (%d bytes, %d per frame)" % (path, len(data), align))
    return np.frombuffer(data, dtype=np.uint8), len(data) // align, ch, width, rate, fmt


def _g711_tables():
    """The 256 linear 16-bit values of both G.711 laws, by the expansions of include/pdse.h (pdse_resample_desc)."""
    code = np.arange(256, dtype=np.int32)
    u = ~code & 0xFF
    mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84
    ulaw = np.where(u & 0x80, -mag, mag)
    a = code ^ 0x55
    e, m = (a >> 4) & 7, a & 15
    mag = np.where(e == 0, (m << 4) + 8, ((m << 4) + 0x108) << np.maximum(e - 1, 0))
    alaw = np.where(a & 0x80, mag, -mag)
    return alaw.astype(np.int32), ulaw.astype(np.int32)


def decode_frames(frames, ch, width, fmt):
    """The kernel's decode and mix (csrc/resample.hip: wav_kernel) in numpy: fp32 mono samples of interleaved frames.
    s24 is sign-extended and divided by 8388608; binary32 keeps its bits; binary64 is rounded to fp32 once (to nearest even,
    infinity beyond the range); G.711 expands to 16 bits and divides by 32768; the other integer widths as ``read_wav``.  More
    than one channel: the fp32 sum in channel order - an explicit loop, not ``mean(axis=1)``, whose order is numpy's business -
    then one division by float32(ch)."""
    raw = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1)
    if fmt == WAV_INT and width == 3:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        x = (v - ((v & 0x800000) << 1)).astype(np.float32) / np.float32(8388608.0)
    elif fmt == WAV_INT and width == 1:
        x = (raw.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    elif fmt == WAV_INT and width in (2, 4):
        x = raw.view("<i2" if width == 2 else "<i4").astype(np.float32) / np.float32(2.0 ** (8 * width - 1))
    elif fmt == WAV_FLOAT and width == 4:
        x = raw.view("<u4").astype(np.uint32).view(np.float32)          # the bits, never through arithmetic
    elif fmt == WAV_FLOAT and width == 8:
        with np.errstate(over="ignore", invalid="ignore"):
            x = raw.view("<f8").astype(np.float32)
    elif fmt in (WAV_ALAW, WAV_ULAW) and width == 1:
        x = _g711_tables()[0 if fmt == WAV_ALAW else 1][raw].astype(np.float32) / np.float32(32768.0)
    else:
        raise ValueError("no decode for fmt %d with %d bytes per sample" % (fmt, width))
    if ch == 1:
        return x
    x = x.reshape(-1, ch)
    with np.errstate(over="ignore", invalid="ignore"):
        s = x[:, 0].copy()
        for c in range(1, ch):
            s = s + x[:, c]
        return s / np.float32(ch)


def read_any(path, sr=16000):
    """``read_wav`` for every file ``read_frames`` opens: decode, mono mix (``decode_frames``) and ``resample`` to ``sr``.
    For a file ``read_wav`` accepts with one or two channels the result is ``read_wav``'s bit for bit.  With more channels the
    mix is the fp32 sum in channel order divided by the count, which may differ in the last bit from the ``mean(axis=1)``
    ``read_wav`` takes (numpy chooses that summation order); the device kernel follows this function."""
    frames, n, ch, width, rate, fmt = read_frames(path)
    x = decode_frames(frames, ch, width, fmt)
    if rate != sr:
        with np.errstate(over="ignore", invalid="ignore"):
            x = resample(x, rate, sr)
    return x


def read_channels(path, sr=16000):
    """fp32 [ch, n]: the channels of a file ``read_frames`` opens, kept apart (opt-in: ``wavdev.load(channels="each")``,
    ``generate_wav`` of a trainer built with ``channels="each"``).  Row c is channel c's samples de-interleaved, decoded alone
    (``decode_frames`` with ``ch == 1``) and run through ``resample``: ``read_any`` of a mono file that holds channel c's samples
    in the same encoding, bit for bit.  No mix arithmetic touches a sample, so binary32 NaN payloads survive as they do for a
    mono file; the single row of a mono file is ``read_any(path)``."""
    frames, n, ch, width, rate, fmt = read_frames(path)
    samples = frames.reshape(n, ch, width)
    rows = []
    for c in range(ch):
        x = decode_frames(np.ascontiguousarray(samples[:, c]), 1, width, fmt)
        if rate != sr:
            with np.errstate(over="ignore", invalid="ignore"):
                x = resample(x, rate, sr)
        rows.append(x)
    return np.stack(rows) if rows[0].size else np.zeros((ch, 0), dtype=np.float32)


# ---- the way back: a waveform at 16 kHz written in its source's rate and encoding (opt-in: generate_wav(wav_out="source")) ----
# The host oracle of csrc/wavout.hip (include/pdse.h: the wav back end; prior-diffuse_amd/wavdev.py: encode).
_FMT_TAG = {WAV_INT: 1, WAV_FLOAT: 3}                        # what write_any writes: WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT
_OUT_WIDTHS = {WAV_INT: (2, 3, 4), WAV_FLOAT: (4,)}
MAX_OUT_CH = 8                                               # PDSE_WAV_MAX_CH


def _check_target(fmt, width, ch):
    if fmt not in _OUT_WIDTHS or width not in _OUT_WIDTHS[fmt]:
        raise ValueError("no encoder for fmt %r with %r bytes per sample (WAV_INT: 2, 3, 4; WAV_FLOAT: 4)" % (fmt, width))
    if not 1 <= int(ch) <= MAX_OUT_CH:
        raise ValueError("%r channels (1 .. %d)" % (ch, MAX_OUT_CH))


def encode(x, fmt, width, ch):
    """(payload, clipped): the fp32 mono samples ``x`` as interleaved little-endian frames of ``ch`` equal channels (1 .. 8), and
    the number of samples the clamp changed.  WAV_INT, width 2 / 3 / 4: ``write_wav``'s arithmetic at that width - float64(x)
    clamped to [-1, 1 - 2^-(8 width - 1)], times 2^(8 width - 1) (exact), ``np.round`` (half to even); NaN is written as 0 and
    counts as clipped, an infinity clamps and counts.  WAV_FLOAT, width 4: the binary32 bits as they are, nothing clamped
    (clipped is 0).  The 16-bit mono payload is ``write_wav``'s data chunk byte for byte."""
    _check_target(fmt, width, ch)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if fmt == WAV_FLOAT:
        return np.repeat(x.view(np.uint32).astype("<u4"), ch).tobytes(), 0
    bits = 8 * width - 1
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        y = np.clip(x64, -1.0, 1.0 - 2.0 ** -bits)
        clipped = int(np.count_nonzero(y != x64))            # NaN != NaN: counted
    y[np.isnan(y)] = 0.0
    v = np.repeat(np.round(y * 2.0 ** bits).astype("<i4"), ch)
    if width == 2:
        return v.astype("<i2").tobytes(), clipped
    if width == 3:
        return np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).tobytes(), clipped
    return v.tobytes(), clipped


def encode_channels(rows, fmt, width):
    """(payload, clipped_per_channel): the fp32 rows [ch, n] as interleaved little-endian frames, channel c from row c (1 .. 8
    rows; the targets of ``encode``).  Every row goes through ``encode``'s arithmetic on its own - float64 clamp, exact scale,
    round half to even, NaN written as 0 and counted - and the samples are then interleaved in channel order:
    clipped_per_channel[c] is ``encode(rows[c], fmt, width, 1)[1]``, and ch equal rows give ``encode(row, fmt, width, ch)[0]``
    byte for byte.  The host oracle of csrc/wavout.hip's channel encoder (``wavdev.encode_channels``)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2:
        raise ValueError("rows: [ch, n], got shape %r" % (rows.shape,))
    ch, n = rows.shape
    _check_target(fmt, width, ch)
    image = np.zeros((n, ch, width), dtype=np.uint8)
    clipped = []
    for c in range(ch):
        payload, k = encode(rows[c], fmt, width, 1)
        image[:, c] = np.frombuffer(payload, dtype=np.uint8).reshape(n, width)
        clipped.append(k)
    return image.tobytes(), clipped


def wav_header(n_bytes, sr, fmt, width, ch):
    """The bytes in front of a data chunk of ``n_bytes``: RIFF, WAVE and a plain ``fmt `` chunk - tag 1 with the 16 bytes the
    ``wave`` module writes (a 16-bit mono file is that module's byte for byte), tag 3 with cbSize = 0 and a ``fact`` chunk holding
    the frame count - then the ``data`` chunk's own header.  An odd data chunk is followed by a pad byte (``wav_pad``), counted
    in the RIFF size."""
    import struct

    _check_target(fmt, width, ch)
    if n_bytes % (ch * width) or n_bytes + 64 >= 2 ** 32:
        raise ValueError("a data chunk of %d bytes (whole frames of %d bytes, below 4 GiB: RF64 is not written)" % (n_bytes, ch * width))
    body = struct.pack("<HHIIHH", _FMT_TAG[fmt], ch, int(sr), int(sr) * ch * width, ch * width, 8 * width)
    if fmt == WAV_FLOAT:
        chunks = b"fmt " + struct.pack("<I", 18) + body + struct.pack("<H", 0) + b"fact" + struct.pack("<II", 4, n_bytes // (ch * width))
    else:
        chunks = b"fmt " + struct.pack("<I", 16) + body
    chunks = b"WAVE" + chunks + b"data" + struct.pack("<I", n_bytes)
    return b"RIFF" + struct.pack("<I", len(chunks) + n_bytes + (n_bytes & 1)) + chunks


def write_payload(path, payload, sr, fmt, width, ch):
    """A RIFF/WAVE file around frames that are already encoded (``encode``, ``wavdev.encode``)."""
    head = wav_header(len(payload), sr, fmt, width, ch)
    with open(path, "wb") as f:
        f.write(head)
        f.write(payload)
        if len(payload) & 1:
            f.write(b"\0")


def write_any(path, x, sr, fmt, width, ch):
    """``write_wav`` for the other targets: ``encode(x, fmt, width, ch)`` in a file ``read_frames`` / ``read_any`` reads back.
    Returns the clip count.  ``write_any(path, x, sr, WAV_INT, 2, 1)`` writes ``write_wav(path, x, sr)``'s file."""
    payload, clipped = encode(x, fmt, width, ch)
    write_payload(path, payload, sr, fmt, width, ch)
    return clipped


def target_of(source):
    """(tag, width) a file is written with, from its source's (tag, width) - wFormatTag 1, 3, 6 or 7 as ``probe`` returns it:
    16-, 24- and 32-bit PCM as itself, binary32 and binary64 as binary32, and what is too narrow to hold an enhanced signal -
    8-bit PCM, A-law, mu-law - as 16-bit PCM."""
    tag, width = int(source[0]), int(source[1])
    if tag not in _TAG_FMT or width not in _WIDTHS[_TAG_FMT[tag]]:
        raise ValueError("no wav encoding with format tag %d and %d bytes per sample" % (tag, width))
    if tag == 3:
        return 3, 4
    if tag == 1 and width > 1:
        return 1, width
    return 1, 2


def probe(path):
    """(rate, channels, tag, width, n_frames) of a file ``read_frames`` opens, from its chunk headers alone: nothing of the data
    chunk is read.  tag is the wFormatTag behind a WAVE_FORMAT_EXTENSIBLE header (1 PCM, 3 IEEE float, 6 A-law, 7 mu-law),
    n_frames what ``read_frames`` returns (a data size beyond the end of the file is clamped to it).  ValueError for the files
    ``read_frames`` refuses."""
    import os
    import struct

    with open(path, "rb") as f:
        end = os.fstat(f.fileno()).st_size
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise ValueError("%s: not a RIFF/WAVE file (%r)" % (path, head[:4]))
        pos, fmt_chunk, n_data = 12, None, None
        while pos + 8 <= end:
            f.seek(pos)
            cid, size = struct.unpack("<4sI", f.read(8))
            body = pos + 8
            if cid == b"fmt " and fmt_chunk is None:
                fmt_chunk = f.read(size)
                if len(fmt_chunk) < size:
                    raise ValueError("%s: the file ends inside the fmt chunk" % path)
            elif cid == b"data":
                if fmt_chunk is None:
                    raise ValueError("%s: data chunk before the fmt chunk" % path)
                n_data = min(body + size, end) - body
                break
            pos = body + size + (size & 1)
    if fmt_chunk is None or n_data is None:
        raise ValueError("%s: no %s chunk" % (path, "fmt" if fmt_chunk is None else "data"))
    if len(fmt_chunk) < 16:
        raise ValueError("%s: fmt chunk of %d bytes" % (path, len(fmt_chunk)))
    tag, ch, rate, _, align, bits = struct.unpack_from("<HHIIHH", fmt_chunk)
    if tag == 0xFFFE:
        if len(fmt_chunk) < 40 or struct.unpack_from("<H", fmt_chunk, 16)[0] < 22:
            raise ValueError("%s: WAVE_FORMAT_EXTENSIBLE with a fmt chunk of %d bytes" % (path, len(fmt_chunk)))
        if fmt_chunk[26:40] != _GUID_TAIL:
            raise ValueError("%s: unknown SubFormat GUID %s" % (path, fmt_chunk[24:40].hex()))
        tag = struct.unpack_from("<H", fmt_chunk, 24)[0]
    if tag not in _TAG_FMT:
        raise ValueError("%s: unsupported format tag 0x%04X" % (path, tag))
    if bits % 8 or bits // 8 not in _WIDTHS[_TAG_FMT[tag]]:
        raise ValueError("%s: %d bits per sample with format tag %d" % (path, bits, tag))
    width = bits // 8
    if ch < 1 or rate < 1:
        raise ValueError("%s: %d channels at %d Hz" % (path, ch, rate))
    if align != ch * width:
        raise ValueError("%s: block align %d with %d channels of %d bytes" % (path, align, ch, width))
    if n_data % align:
        raise ValueError("%s: the data chunk ends inside a frame (%d bytes, %d per frame)" % (path, n_data, align))
    return rate, ch, tag, width, n_data // align


def restore(x16k, rate, n_src):
    """The samples a file of ``n_src`` frames at ``rate`` is written with, from its enhanced waveform at 16 kHz: ``resample`` back
    to the source's rate - the same taps, float64, one cast to fp32 - cut to ``n_src``.  ``resample`` returns ceil(n up / down)
    samples in each direction, so the way there and back never comes out shorter than the source (at most a few samples longer:
    tests/test_wavout_host.py walks the common rates) and the cut is all it takes."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = resample(np.asarray(x16k, dtype=np.float32), 16000, rate)
    if y.size < n_src:
        raise ValueError("%d samples at %d Hz from %d at 16 kHz: fewer than the %d the source holds" % (y.size, rate, np.size(x16k), n_src))
    return y[:n_src]
