"""float64 numpy restatements of the spectral compression modes (``feat_type``: sqrt, normal, cubic, log_1x, none), written from
the table of include/pdse.h (pdse_compand_desc), for the tests of tests/test_feat_type_host.py and tests/test_gpu_feat_type.py.

A spectrogram is [B, 2, T, F] (real part, imaginary part).  m = |X|, the phase is kept: cos / sin of it are re / m and im / m,
(1, 0) at m == 0.  Every function takes any float array, works in float64 and returns float64.

    feat_type   compress        decompress
    sqrt        m ** 0.5        m ** 2
    normal      m               the spectrogram as it is
    cubic       m ** 0.3        m ** (10 / 3)
    log_1x      log(m + 1)      exp(m) - 1
    none        as it is        as it is
"""
import numpy as np

FEAT_TYPES = ("sqrt", "normal", "cubic", "log_1x", "none")

_COMPRESS = {
    "sqrt": lambda m: m ** 0.5,
    "normal": lambda m: m,
    "cubic": lambda m: m ** 0.3,
    "log_1x": lambda m: np.log(m + 1.0),
}
_DECOMPRESS = {
    "sqrt": lambda m: m ** 2,
    "cubic": lambda m: m ** (10.0 / 3.0),
    "log_1x": lambda m: np.exp(m) - 1.0,
}


def _through_phase(spec, f):
    s = np.asarray(spec, dtype=np.float64)
    re, im = s[:, 0], s[:, 1]
    m = np.sqrt(re * re + im * im)
    safe = np.where(m > 0, m, 1.0)
    cr, sr = np.where(m > 0, re / safe, 1.0), np.where(m > 0, im / safe, 0.0)
    with np.errstate(over="ignore"):
        g = f(m)
    return np.stack((g * cr, g * sr), axis=1)


def compress(spec, feat_type):
    """The front end's transform: the magnitude through ``feat_type``'s compression, the phase kept."""
    if feat_type not in FEAT_TYPES:
        raise ValueError(feat_type)
    if feat_type == "none":
        return np.asarray(spec, dtype=np.float64).copy()
    return _through_phase(spec, _COMPRESS[feat_type])


def decompress(spec, feat_type):
    """The back end's transform: the inverse of ``compress``."""
    if feat_type not in FEAT_TYPES:
        raise ValueError(feat_type)
    if feat_type in ("normal", "none"):
        return np.asarray(spec, dtype=np.float64).copy()
    return _through_phase(spec, _DECOMPRESS[feat_type])


def hann(n=320):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def frames_of(spec, feat_type, n_fft=320):
    """decompress, then the windowed inverse real DFT of every frame: [B, 2, T, n_fft / 2 + 1] -> [B, n_fft, T], what an
    inverse STFT overlaps and adds (the layout of pdse_spec_frames)."""
    d = decompress(spec, feat_type)
    z = d[:, 0] + 1j * d[:, 1]                                  # [B, T, F]
    return (np.fft.irfft(z, n=n_fft, axis=-1) * hann(n_fft)).transpose(0, 2, 1)


def wav_of(spec, feat_type, n_fft=320, hop=160):
    """decompress + the centred inverse STFT with a periodic Hann window: [B, 2, T, F] -> [B, (T - 1) * hop]."""
    fr = frames_of(spec, feat_type, n_fft)                      # [B, n_fft, T]
    B, _, T = fr.shape
    out, env = np.zeros((B, n_fft + hop * (T - 1))), np.zeros(n_fft + hop * (T - 1))
    w2 = hann(n_fft) ** 2
    for t in range(T):
        out[:, t * hop:t * hop + n_fft] += fr[:, :, t]
        env[t * hop:t * hop + n_fft] += w2
    half = n_fft // 2
    return out[:, half:half + (T - 1) * hop] / env[half:half + (T - 1) * hop]


def errors(got, want):
    """(rel-L2, max-abs) of ``got`` against ``want`` over the elements where ``want`` is finite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    ok = np.isfinite(want)
    d = got[ok] - want[ok]
    return float(np.linalg.norm(d) / max(np.linalg.norm(want[ok]), 1e-300)), float(np.abs(d).max()) if d.size else 0.0
