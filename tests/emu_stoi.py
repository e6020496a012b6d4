"""numpy restatement of the arithmetic of csrc/stoi.hip (not of the papers: that is tests/helpers/stoi_refs.py): the package's
tables (``metrics.stoi_tables``), the fp32 resampled signals, float64 frame energies and keep mask, the compacted frames gathered
through the kept-frame index list instead of an overlap-added signal, the DFT as a product with the cos|sin basis over bins
0..255, band sums over the edge table, the segment arithmetic band by band, one cast to fp32 at the end.  Only the order of the
sums differs from the kernels (numpy's pairwise / BLAS order), which is what the factor 10 of the GPU tolerance covers.
``spectral=np.float32`` restates the spectral stage (tables, windowed rows, DFT, band amplitudes) in fp32: the study behind the
kernel's choice of float64 (profiles/stoi_parity.txt).  Also holds the tolerances the host and GPU tests share."""
import numpy as np

from conftest import pkg

KEYS = ["stoi", "estoi"]
# Absolute distance of ``emulate`` from the float64 oracle over helpers/stoi_refs.py: CASES, both measures (measured values:
# profiles/stoi_parity.txt, written by tests/test_stoi_host.py when PDSE_METRICS_PARITY names a file).  With a float64 spectral
# stage the distance is the final fp32 rounding of a score below 1: half an ulp, 2^-25.
EMU_DISTANCE = 3.0e-8
TOL = 10.0 * EMU_DISTANCE
FP32_LIMIT = 1e-4          # an fp32 spectral stage further than this from the oracle on any input would have forced float64


def emulate(clean16, proc16, spectral=np.float64):
    """-> dict: stoi, estoi (float, after the kernel's fp32 cast), kept (frame count after removal)."""
    M, L, wavio = pkg("metrics"), pkg("_lib"), pkg("wavio")
    tab = M.stoi_tables()
    win = tab[L.STOI_OFF_WIN:L.STOI_OFF_WIN + 256]
    basis = tab[L.STOI_OFF_BASIS:L.STOI_OFF_BRANGE].reshape(256, 512)
    edges = tab[L.STOI_OFF_BRANGE:L.STOI_OFF_BRANGE + 30].reshape(15, 2).astype(int)
    eps = np.finfo(np.float64).eps
    f32 = np.float32
    x = wavio.resample(np.asarray(clean16, dtype=f32), 16000, 10000)          # fp32, what stoi_resample_kernel writes
    y = wavio.resample(np.asarray(proc16, dtype=f32), 16000, 10000)
    nf = L.stoi_frames(len(clean16))
    assert len(x) == L.stoi_n10(len(clean16))
    pos = np.arange(nf)[:, None] * 128 + np.arange(256)[None, :]
    # stoi_mask_kernel
    fx = win * x[pos].astype(np.float64)
    en = 20.0 * np.log10(np.sqrt((fx * fx).sum(-1)) + eps)
    keep = (en.max() - 40.0 - en) < 0.0 if nf else np.zeros(0, dtype=bool)
    idx = np.nonzero(keep)[0]
    K = len(idx)
    if K < 30:
        return {"stoi": float(f32(1e-5)), "estoi": float(f32(1e-5)), "kept": K}
    # stoi_spec_kernel: row j = w * (w x[k_j] + the overlapping half of the neighbouring kept frame)
    sp = spectral
    t = np.arange(256)
    u = t ^ 128
    amps = []
    for sig in (x, y):
        s64 = sig.astype(np.float64)
        cur = win * s64[idx[:, None] * 128 + t]
        prev = np.zeros_like(cur)
        nxt = np.zeros_like(cur)
        prev[1:] = win[u] * s64[idx[:-1, None] * 128 + u]
        nxt[:-1] = win[u] * s64[idx[1:, None] * 128 + u]
        rows = win * (cur + np.where(t < 128, prev, nxt))
        Z = rows.astype(sp) @ basis.astype(sp)
        P = Z[:, :256] * Z[:, :256] + Z[:, 256:] * Z[:, 256:]
        amps.append(np.stack([np.sqrt(P[:, lo:hi].sum(-1, dtype=sp)) for lo, hi in edges], axis=1).astype(np.float64))
    X, Y = amps
    # stoi_segment_kernel
    segs = K - 29
    clip = 1.0 + 5.623413251903491
    tot_s = tot_e = 0.0
    for s in range(segs):
        xs, ys = X[s:s + 30], Y[s:s + 30]                                       # [30][15]
        c = np.sqrt((xs * xs).sum(0)) / (np.sqrt((ys * ys).sum(0)) + eps)
        yp = np.minimum(ys * c, xs * clip)
        mx, my = xs.sum(0) / 30.0, yp.sum(0) / 30.0
        p, q = xs - mx, yp - my
        sxx, syy = (p * p).sum(0), (q * q).sum(0)
        tot_s += float((((q / (np.sqrt(syy) + eps)) * (p / (np.sqrt(sxx) + eps))).sum(0)).sum())
        ry = ys.sum(0) / 30.0
        qy = ys - ry
        ur, vr = p * (1.0 / np.sqrt(sxx)), qy * (1.0 / np.sqrt((qy * qy).sum(0)))
        uc = ur - (ur.sum(1) / 15.0)[:, None]
        vc = vr - (vr.sum(1) / 15.0)[:, None]
        iu, iv = 1.0 / np.sqrt((uc * uc).sum(1)), 1.0 / np.sqrt((vc * vc).sum(1))
        tot_e += float((((uc * iu[:, None]) * (vc * iv[:, None])).sum(1)).sum())
    return {"stoi": float(f32(tot_s / (15.0 * segs))), "estoi": float(f32(tot_e / (30.0 * segs))), "kept": K}
