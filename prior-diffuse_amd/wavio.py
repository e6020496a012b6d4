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
