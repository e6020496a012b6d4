"""numpy restatement of the arithmetic of csrc/metrics.hip (not of the reference): the same framing, the same precision at
every step (float64 on the fp32 samples, the fp32 cast of the LPC vectors and fp32 Toeplitz forms as the reference has
them, fp32 per-frame values, float64 means rounded to fp32 once), the same trimming and rounding rule.  Only the order of the
sums differs from the kernels (numpy's pairwise / BLAS order), which is what the factor 10 of the parity tolerances covers
(profiles/metrics_parity.txt).  Also holds what the host and GPU tests share: the fixture list, the input recipe and the tolerances."""
import os

import numpy as np

from conftest import GOLDEN, pkg

CASES = ["snr0_L64000", "snr5_L47321", "snr10_L4000", "snr20_L160000", "snr40_L64000", "snr10_L600", "same_L4000",
         "silence_L32000"]
KEYS = ["ssnr", "llr", "wss", "fwsnrseg"]

# Absolute tolerances, each in the measure's own unit: 10 x the largest distance of ``emulate`` from the reference's float64
# results over CASES, scalars and per-frame values alike (measured values: profiles/metrics_parity.txt, written by
# tests/test_metrics_host.py::test_emulation_matches_the_reference_fixtures when PDSE_METRICS_PARITY names a file).
# All stay below the 1e-3 the reference's four-decimal reports resolve.
EMU_DISTANCE = {"ssnr": 2.0e-6, "llr": 2.2e-6, "wss": 3.7e-6, "fwsnrseg": 2.0e-6}      # half an fp32 ulp of a per-frame value, mostly
TOL = {k: 10.0 * v for k, v in EMU_DISTANCE.items()}
FRAME_OUTLIERS = 0.0       # fraction of an utterance's frames allowed outside TOL: what ``emulate`` shows against the reference (none), capped at 1 %


def load_case(name):
    g = np.load(os.path.join(GOLDEN, "metrics_%s.npz" % name))
    return {k: g[k] for k in g.files}


def case_inputs(g):
    """The pair a fixture was computed from, regenerated (or taken verbatim where stored) and checked against its sums."""
    synth = pkg("synth")
    snr = None if np.isnan(float(g["snr_db"])) else float(g["snr_db"])
    sil = tuple(int(v) for v in g["silence"])
    clean, proc = synth.noisy_pair(int(g["length"]), int(g["seed"]), snr, None if sil[0] < 0 else sil)
    c64, p64 = clean.astype(np.float64), proc.astype(np.float64)
    got = np.array([c64.sum(), (c64 ** 2).sum(), p64.sum(), (p64 ** 2).sum()])
    scale = np.sqrt(len(clean) * got[[1, 1, 3, 3]]) * [1, 0, 1, 0] + got[[1, 1, 3, 3]] * [0, 1, 0, 1]
    assert np.all(np.abs(got - g["checks"]) <= 1e-6 * scale), "the input generator drifted from the fixture"
    if "clean" in g:
        assert np.abs(clean - g["clean"]).max() <= 1e-6 and np.abs(proc - g["proc"]).max() <= 1e-6
        clean, proc = g["clean"].copy(), g["proc"].copy()
    return clean, proc


def _frames(x, m):
    idx = np.arange(m)[:, None] * 120 + np.arange(480)[None, :]
    return x[idx]


def _levinson(R):
    """[m, 17] float64 lags -> [m, 17] fp32 lpparams, the recursion of csrc/metrics.hip: levinson."""
    eps = np.finfo(np.float64).eps
    m = R.shape[0]
    a = np.zeros((m, 16))
    E = R[:, 0].copy()
    for i in range(16):
        s = np.zeros(m)
        for j in range(i):
            s += a[:, j] * R[:, i - j]
        rc = (R[:, i + 1] - s) / np.maximum(E, eps)
        if i > 0:
            a[:, :i] = a[:, :i] - rc[:, None] * a[:, :i][:, ::-1]
        a[:, i] = rc
        E = (1 - rc * rc) * E
    return np.concatenate([np.ones((m, 1)), -a], axis=1).astype(np.float32)


def _form(A, R):
    """A . toeplitz(R) . A^T per frame in fp32."""
    idx = np.abs(np.arange(17)[:, None] - np.arange(17)[None, :])
    T = R[:, idx]                                          # [m, 17, 17] fp32
    v = np.einsum("mij,mj->mi", T, A).astype(np.float32)
    return np.einsum("mi,mi->m", A, v).astype(np.float32)


def _peaks(le, ii):
    n = ii
    if le[ii + 1] - le[ii] > 0:
        while n < 24 and le[n + 1] - le[n] > 0:
            n += 1
        return le[n - 1]
    while n >= 0 and le[n + 1] - le[n] <= 0:
        n -= 1
    return le[n + 1]


def trimmed_mean(v):
    """Ascending sort (NaN last), mean of the first round-half-even(0.95 m)."""
    M = pkg("metrics")
    v = np.sort(np.asarray(v, dtype=np.float64))
    return float(np.mean(v[:M.kept_count(len(v))]))


def emulate(clean, proc, spectral=np.float64):
    """-> dict of the four scalars (float, after the kernel's final fp32 cast) and the four per-frame fp32 arrays.
    spectral=np.float32 restates the spectral stage as it was first planned (fp32 tables, fp32 DFT and everything after it in
    fp32): the study behind the kernel's float64 spectral stage, see test_metrics_host.py and profiles/metrics_parity.txt."""
    M, L = pkg("metrics"), pkg("_lib")
    f32 = np.float32
    tab = M.tables()
    win = tab[L.METRICS_OFF_WIN:L.METRICS_OFF_WIN + 480]
    basis = tab[L.METRICS_OFF_BASIS:L.METRICS_OFF_CRIT].reshape(480, 1024)
    crit = tab[L.METRICS_OFF_CRIT:L.METRICS_OFF_WEPS].reshape(25, 512)
    weps = tab[L.METRICS_OFF_WEPS:L.METRICS_OFF_BRANGE].reshape(2, 512)
    eps = np.finfo(np.float64).eps
    clean, proc = np.asarray(clean, dtype=f32), np.asarray(proc, dtype=f32)
    m = M.frame_count(len(clean))
    old = np.seterr(all="ignore")
    try:
        # ---- time-domain stage (float64 on the fp32 samples; the window is float64)
        fc = _frames(clean, m).astype(np.float64) * win
        fp = _frames(proc, m).astype(np.float64) * win
        Rc = np.stack([(fc[:, :480 - k] * fc[:, k:]).sum(-1) for k in range(17)], axis=1)
        Rp = np.stack([(fp[:, :480 - k] * fp[:, k:]).sum(-1) for k in range(17)], axis=1)
        en = ((fc - fp) ** 2).sum(-1)
        ssnr = np.clip(10 * np.log10(Rc[:, 0] / (en + eps) + eps), -10, 35)
        Ac, Ap, Rf = _levinson(Rc), _levinson(Rp), Rc.astype(f32)
        frac = _form(Ap, Rf).astype(np.float64) / _form(Ac, Rf).astype(np.float64)
        frac[frac <= 0] = 1000
        llr = np.log(frac)
        # ---- spectral stage (float64 on fp32 samples)
        sp = spectral
        basis, crit, weps = basis.astype(sp), crit.astype(sp), weps.astype(sp)
        wins = win.astype(sp)
        LE, EF = [], []
        for w in ((_frames(clean, m).astype(sp) * wins), (_frames(proc, m).astype(sp) * wins)):
            Z = w @ basis                                  # [m, 1024]
            re, im = Z[:, :512] + weps[0], Z[:, 512:] + weps[1]
            P = re * re + im * im
            Mg = np.sqrt(P)
            S = Mg.sum(-1)
            le = 10 * np.log10(P[:, :256] @ crit[:, :256].T)
            le[le < -100] = -100
            LE.append(le)
            EF.append((Mg[:, :256] @ crit[:, :256].T) / S[:, None])
        wss = np.zeros(m)
        lc, lp = LE
        mc, mp = lc.max(-1), lp.max(-1)
        for t in range(m):
            pc = np.array([_peaks(lc[t], i) for i in range(24)])
            pp = np.array([_peaks(lp[t], i) for i in range(24)])
            w_c = (20 / (20 + mc[t] - lc[t, :24])) * (1 / (1 + pc - lc[t, :24]))
            w_p = (20 / (20 + mp[t] - lp[t, :24])) * (1 / (1 + pp - lp[t, :24]))
            w_ = (w_c + w_p) / 2
            ds = np.diff(lc[t]) - np.diff(lp[t])
            wss[t] = (w_ * ds * ds).sum() / w_.sum()
        ec, ep = EF
        err = (ec - ep) ** 2
        err[err < sp(eps)] = sp(eps)
        wf = np.power(ec, sp(0.2))
        fw = (wf * (10 * np.log10(ec * ec / err))).sum(-1) / wf.sum(-1)
        fw[fw < -10] = -10
        fw[fw > 35] = 35
    finally:
        np.seterr(**old)
    frames = {"ssnr": ssnr.astype(f32), "llr": llr.astype(f32), "wss": wss.astype(f32), "fwsnrseg": fw.astype(f32)}
    res = {"ssnr": float(f32(frames["ssnr"].astype(np.float64).mean())),
           "fwsnrseg": float(f32(frames["fwsnrseg"].astype(np.float64).mean())),
           "llr": float(f32(trimmed_mean(frames["llr"]))), "wss": float(f32(trimmed_mean(frames["wss"])))}
    for k in KEYS:
        res[k + "_frames"] = frames[k]
    return res


def same(a, b, tol):
    """|a - b| <= tol where both are finite; NaN matches NaN, an infinity its own sign; never finite against non-finite."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    eq = np.where(fin, np.abs(np.where(fin, a, 0) - np.where(fin, b, 0)) <= tol, False)
    return eq | (np.isnan(a) & np.isnan(b)) | (np.isinf(a) & np.isinf(b) & (np.sign(a) == np.sign(b)))


def distance(a, b):
    """Largest |a - b| over the entries where both are finite (0 if none)."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    fin = np.isfinite(a) & np.isfinite(b)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0
