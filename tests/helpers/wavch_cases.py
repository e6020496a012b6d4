"""Files and signals the host and the device tests of per-channel enhancement share (tests/test_wavch_host.py,
tests/test_gpu_wavch.py): a RIFF writer for every encoding ``wavio.read_frames`` opens, seeded payloads whose channels differ, and
the split of a multichannel file into the mono files of its channels."""
import struct

import numpy as np

INT, FLOAT, ALAW, ULAW = 1, 2, 3, 4                                  # wavio.WAV_*
TAG = {INT: 1, FLOAT: 3, ALAW: 6, ULAW: 7}
FORMATS = ((INT, 1), (INT, 2), (INT, 3), (INT, 4), (FLOAT, 4), (FLOAT, 8), (ALAW, 1), (ULAW, 1))      # every wav_kernel instantiation
NAMES = {(INT, 1): "u8", (INT, 2): "s16", (INT, 3): "s24", (INT, 4): "s32", (FLOAT, 4): "f32", (FLOAT, 8): "f64", (ALAW, 1): "alaw",
         (ULAW, 1): "ulaw"}
GUID_TAIL = bytes([0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])


def wav_bytes(fmt, width, ch, rate, data, extensible=False):
    """A RIFF/WAVE file around ``data`` (bytes of whole frames): a plain 16-byte fmt chunk or WAVE_FORMAT_EXTENSIBLE."""
    align = ch * width
    head = struct.pack("<HHIIHH", 0xFFFE if extensible else TAG[fmt], ch, rate, rate * align, align, 8 * width)
    if extensible:
        head += struct.pack("<HHIH", 22, 8 * width, 0, TAG[fmt]) + GUID_TAIL
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(head)) + head + b"data" + struct.pack("<I", len(data)) + data + b"\0" * (len(data) & 1)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def payload(rs, fmt, width, n, ch):
    """uint8 [n, ch, width]: n frames of ch channels of seeded samples - every channel its own - in the encoding (fmt, width).
    Integer and G.711 samples are random bytes (every code, both signs, the extremes); float samples are finite, 0.3 randn."""
    if fmt == FLOAT:
        x = (0.3 * rs.standard_normal((n, ch))).astype("<f4" if width == 4 else "<f8")
        return np.ascontiguousarray(x).view(np.uint8).reshape(n, ch, width)
    return rs.randint(0, 256, (n, ch, width)).astype(np.uint8)


def split_files(tmp, name, fmt, width, rate, frames, extensible=False):
    """Write the file ``name``.wav of ``frames`` [n, ch, width] and the mono files ``name``_c<c>.wav of its channels, same encoding;
    returns (path, [mono paths])."""
    n, ch, _ = frames.shape
    path = tmp / (name + ".wav")
    path.write_bytes(wav_bytes(fmt, width, ch, rate, frames.tobytes(), extensible))
    monos = []
    for c in range(ch):
        p = tmp / ("%s_c%d.wav" % (name, c))
        p.write_bytes(wav_bytes(fmt, width, 1, rate, np.ascontiguousarray(frames[:, c]).tobytes(), extensible))
        monos.append(str(p))
    return str(path), monos


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def rows_signal(ch, n, seed, clip_channel=None, width=2):
    """fp32 [ch, n]: 0.1 randn within +-0.4 per channel (a rate conversion's overshoot stays inside +-1), every row its own; ``clip_channel`` alone also holds values the integer clamp of
    ``width`` bytes changes - beyond +-1, +1.0 itself, NaN and both infinities."""
    x = (0.1 * np.random.RandomState(seed).standard_normal((ch, n))).clip(-0.4, 0.4).astype(np.float32)
    if clip_channel is not None and n >= 8:
        at = np.linspace(1, n - 2, 6).astype(np.int64)
        x[clip_channel, at] = np.array([1.0, -1.5, np.nan, np.inf, -np.inf, 2.5], dtype=np.float32)
    return x
