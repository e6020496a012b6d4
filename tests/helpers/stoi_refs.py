"""The oracle of the STOI tests: a float64 numpy statement of the measure, written from C. H. Taal et al., "An Algorithm for
Intelligibility Prediction of Time-Frequency Weighted Noisy Speech" (IEEE TASL 2011) and J. Jensen, C. H. Taal, "An Algorithm
for Predicting the Intelligibility of Speech Masked by Modulated Noise Maskers" (IEEE/ACM TASLP 2016).  It shares nothing with
the kernels but the 16 kHz -> 10 kHz converter, ``wavio.resample`` (step 1 of the measure): its own window, an FFT instead of a
basis product, all 257 bins, a 0/1 band matrix, a literal overlap-add of the kept frames.

Also the seeded inputs the host and GPU tests share (``CASES``), each with the margin of its keep mask."""
import numpy as np

from conftest import pkg

FS, FRAME, HOP, NFFT, NBAND, NSEG = 10000, 256, 128, 512, 15, 30
BETA, DYN_RANGE = -15.0, 40.0
EPS = np.finfo(np.float64).eps


def window():
    return np.hanning(FRAME + 2)[1:-1]


def third_octave_matrix():
    """([15][257] 0/1 matrix, centre frequencies): band k is centred at 150 * 2^(k/3) Hz and reaches a sixth of an octave to
    either side; each edge is moved to the nearest DFT bin, the upper one exclusive."""
    f = np.arange(NFFT // 2 + 1) * (FS / NFFT)
    k = np.arange(NBAND)
    cf = 150.0 * 2.0 ** (k / 3.0)
    obm = np.zeros((NBAND, f.size))
    for i in range(NBAND):
        lo = int(np.argmin(np.abs(f - cf[i] * 2.0 ** (-1 / 6.0))))
        hi = int(np.argmin(np.abs(f - cf[i] * 2.0 ** (1 / 6.0))))
        obm[i, lo:hi] = 1.0
    return obm, cf


def frames_of(x):
    """Whole windowed frames [nf][256] of a signal at 10 kHz."""
    nf = 0 if len(x) < FRAME else 1 + (len(x) - FRAME) // HOP
    w = window()
    return np.array([w * x[i * HOP:i * HOP + FRAME] for i in range(nf)]).reshape(nf, FRAME)


def remove_silent_frames(x, y):
    """-> (x', y', keep mask, energies in dB): frames of both signals whose clean energy lies within 40 dB of the loudest,
    overlap-added in order at hop 128."""
    xf, yf = frames_of(x), frames_of(y)
    en = 20 * np.log10(np.linalg.norm(xf, axis=1) + EPS)
    keep = (np.max(en) - DYN_RANGE - en) < 0 if len(en) else np.zeros(0, dtype=bool)
    xf, yf = xf[keep], yf[keep]
    n = (len(xf) - 1) * HOP + FRAME if len(xf) else 0
    xs, ys = np.zeros(n), np.zeros(n)
    for i in range(len(xf)):
        xs[i * HOP:i * HOP + FRAME] += xf[i]
        ys[i * HOP:i * HOP + FRAME] += yf[i]
    return xs, ys, keep, en


def band_amplitudes(x):
    """[M][15]: sqrt(OBM . |X|^2) of every whole frame of x."""
    obm, _ = third_octave_matrix()
    spec = np.fft.rfft(frames_of(x), n=NFFT, axis=1) if len(x) >= FRAME else np.zeros((0, NFFT // 2 + 1))
    return np.sqrt((np.abs(spec) ** 2) @ obm.T)


def _segments(a):
    """[M][15] -> [M - 29][15][30]"""
    return np.array([a[m:m + NSEG].T for m in range(len(a) - NSEG + 1)])


def measures(clean16, proc16):
    """-> dict: stoi, estoi (float64), frames (before removal), kept (frames after), margin_db (smallest distance of any
    frame's energy from the 40 dB threshold; inf without frames), keep (mask)."""
    wavio = pkg("wavio")
    x = wavio.resample(np.asarray(clean16, dtype=np.float32), 16000, FS).astype(np.float64)
    y = wavio.resample(np.asarray(proc16, dtype=np.float32), 16000, FS).astype(np.float64)
    xs, ys, keep, en = remove_silent_frames(x, y)
    margin = float(np.min(np.abs(np.max(en) - DYN_RANGE - en))) if len(en) else float("inf")
    res = {"frames": len(keep), "kept": int(keep.sum()), "margin_db": margin, "keep": keep}
    X, Y = band_amplitudes(xs), band_amplitudes(ys)
    if len(X) < NSEG:
        res["stoi"] = res["estoi"] = 1e-5
        return res
    xg, yg = _segments(X), _segments(Y)
    # STOI (2011, eqs. 3-6)
    alpha = np.linalg.norm(xg, axis=2, keepdims=True) / (np.linalg.norm(yg, axis=2, keepdims=True) + EPS)
    yp = np.minimum(yg * alpha, xg * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xm = xg - xg.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xm = xm / (np.linalg.norm(xm, axis=2, keepdims=True) + EPS)
    res["stoi"] = float(np.sum(yp * xm) / (xg.shape[0] * NBAND))

    # ESTOI (2016, eqs. 4-9): rows, then columns, mean- and norm-normalised
    def rowcol(a):
        a = a - a.mean(axis=2, keepdims=True)
        a = a / np.sqrt(np.sum(a * a, axis=2, keepdims=True))
        a = a - a.mean(axis=1, keepdims=True)
        return a / np.sqrt(np.sum(a * a, axis=1, keepdims=True))

    res["estoi"] = float(np.sum(rowcol(xg) * rowcol(yg) / NSEG) / xg.shape[0])
    return res


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def bursts(length, seed, gap=0.3, burst=0.4):
    """A speech-like signal at 16 kHz: ``synth.speechlike`` in bursts separated by ``gap`` seconds of a floor 60 dB down, so the
    silent-frame removal has something to remove."""
    synth = pkg("synth")
    x = synth.speechlike(1, length, seed)[0].astype(np.float64)
    t = np.arange(length) / 16000.0
    on = (t % (gap + burst)) < burst
    return (x * np.where(on, 1.0, 1e-3)).astype(np.float32)


def add_noise(clean, seed, snr_db):
    noise = np.random.RandomState(int(seed)).standard_normal(len(clean))
    c = clean.astype(np.float64)
    gain = np.sqrt((c ** 2).mean() / ((noise ** 2).mean() * 10.0 ** (snr_db / 10.0)))
    return (c + gain * noise).astype(np.float32)


# name -> (length, seed); the seeds were searched until every frame of every input lies at least MARGIN_DB from the threshold
# in this oracle (tests/test_stoi_host.py and tests/test_gpu_stoi.py assert it)
MARGIN_DB = 0.05
SEEDS = {"gap_L16000": 11, "snr10_L8000": 12, "min_L6400": 13, "short_L3000": 14}
CASES = ["gap_L16000", "snr10_L8000", "min_L6400", "short_L3000"]


def case(name):
    """(clean, proc) fp32 at 16 kHz.
    gap_L16000   16000 samples with 0.3 s of digital silence in both signals, 5 dB SNR outside it
    snr10_L8000  8000 samples at 10 dB
    min_L6400    6400 samples = 4000 at 10 kHz = 30 frames, none removed: one segment
    short_L3000  3000 samples: fewer than 30 frames, 1e-5"""
    synth = pkg("synth")
    seed = SEEDS[name]
    if name == "gap_L16000":
        clean = synth.speechlike(1, 16000, seed)[0]
        proc = add_noise(clean, seed + 1000, 5.0)
        clean[6000:10800] = 0.0
        proc[6000:10800] = 0.0
        return clean, proc
    n = int(name.rsplit("L", 1)[1])
    clean = synth.speechlike(1, n, seed)[0]
    return clean, add_noise(clean, seed + 1000, 10.0)


_ORACLE = {}


def oracle(name):
    """``measures`` of a case, computed once and shared."""
    if name not in _ORACLE:
        _ORACLE[name] = measures(*case(name))
    return _ORACLE[name]
