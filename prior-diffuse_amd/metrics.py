"""Objective speech-quality scores on the device: the four measures the reference's utils/metrics.py implements itself
(SNRseg :36-55, llr :192-263, wss :266-427, fwSNRseg :58-174) and the ``composite`` arithmetic (:462-470), for batches that are
already in HBM (``ComplexDDPMTrainer.evaluate_batch``) or for two directories of wav files:

    python -m prior_diffuse_amd.metrics [--stoi] REF_DIR DEG_DIR

The reference takes PESQ and STOI from the ``pesq`` and ``pystoi`` packages, which are not dependencies of this one.  PESQ (ITU
code) is not computed.  STOI and ESTOI are, on request (``quality(stoi=True)``, ``--stoi``): csrc/stoi.hip, written from the
two papers (Taal et al. 2011, Jensen & Taal 2016).  The kernels are csrc/metrics.hip and csrc/stoi.hip (include/pdse.h:
pdse_metrics_desc); there is no CPU fallback."""
import glob
import os
import sys

import numpy as np

from . import _lib as L

FS, WINLEN, SKIP, NFFT, NBIN, NBAND, ORDER = 16000, 480, 120, 1024, 512, 25, 16
MIN_LEN = 600          # two time-domain frames: the reference drops the last one (:54, :247)

# Centre frequencies and bandwidths (Hz) of the 25 critical-band filters of Klatt's weighted spectral slope measure (D. Klatt,
# "Prediction of perceived phonetic distance from critical-band spectra", ICASSP 1982), with the values P. Loizou's composite
# measure code (comp_wss.m, "Speech Enhancement: Theory and Practice") publishes and the reference repeats at :75-124.  They
# are data of the measure; ``tables`` evaluates the measure's filter formula on them, as include/pdse.h requires of its caller.
CENT_FREQ = (50.0, 120.0, 190.0, 260.0, 330.0, 400.0, 470.0, 540.0, 617.372, 703.378, 798.717, 904.128, 1020.38, 1148.30,
             1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63)
BANDWIDTH = (70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 70.0, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914, 140.423,
             153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136)


def frame_count(length):
    """Frames every measure covers: the reference's (len - 360) // 120 time-domain frames less the dropped last one, which is
    also its spectral count int(len / 120 - 4)."""
    return (int(length) - WINLEN) // SKIP


def kept_count(m):
    """int(round(m * 0.95)) with Python's round (half to even): the values LLR and WSS average after sorting."""
    return int(round(m * 0.95))


def tables():
    """The constant tables of pdse_metrics_desc, built in float64 the way the reference's expressions build them.  Returns a
    float64 array of METRICS_TABLE_DOUBLES values (include/pdse.h lists the sections)."""
    hann = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, WINLEN + 1) / (WINLEN + 1)))
    max_freq = FS / 2
    min_factor = np.exp(-30.0 / (2.0 * 2.303))
    j = np.arange(NBIN)
    crit = np.zeros((NBAND, NBIN))
    for i in range(NBAND):
        f0 = (CENT_FREQ[i] / max_freq) * NBIN
        bw = (BANDWIDTH[i] / max_freq) * NBIN
        norm_factor = np.log(BANDWIDTH[0]) - np.log(BANDWIDTH[i])
        crit[i] = np.exp(-11 * (((j - np.floor(f0)) / bw) ** 2) + norm_factor)
        crit[i] = crit[i] * (crit[i] > min_factor)
    k = np.arange(WINLEN)[:, None]
    ang = ((k * j[None, :]) % NFFT) * (2 * np.pi / NFFT)
    basis = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)                      # [480][1024]
    weps = np.finfo(np.float64).eps * (hann[None, :] @ basis).reshape(2, NBIN)
    brange = np.zeros(64)
    for i in range(NBAND):
        nz = np.nonzero(crit[i])[0]
        brange[2 * i], brange[2 * i + 1] = nz[0], nz[-1]
    if brange.max() >= 256:
        raise AssertionError("a critical-band filter reaches bin 256: csrc/metrics.hip keeps bins 0..255 for the projection")
    out = np.zeros(L.METRICS_TABLE_DOUBLES)
    out[L.METRICS_OFF_WIN:L.METRICS_OFF_WIN + WINLEN] = hann
    out[L.METRICS_OFF_BASIS:L.METRICS_OFF_CRIT] = basis.reshape(-1)
    out[L.METRICS_OFF_CRIT:L.METRICS_OFF_WEPS] = crit.reshape(-1)
    out[L.METRICS_OFF_WEPS:L.METRICS_OFF_BRANGE] = weps.reshape(-1)
    out[L.METRICS_OFF_BRANGE:] = brange
    return out


# ---- STOI / ESTOI: the measure's constants (Taal et al. 2011, section II; they are properties of the measure) ----------------
STOI_FS, STOI_FRAME, STOI_HOP, STOI_NFFT, STOI_BANDS, STOI_SEG = 10000, 256, 128, 512, 15, 30
STOI_MIN_CF, STOI_BETA, STOI_DYN_RANGE = 150.0, -15.0, 40.0
STOI_BINS = 256        # DFT bins csrc/stoi.hip computes (0..255 of the 257): every band ends below


def stoi_band_edges():
    """[15][2] first bin and the bin after the last of every one-third-octave band: centre frequencies 150 * 2^(k / 3) Hz, edges
    a sixth of an octave to either side, each moved to the nearest bin of the 512-point DFT at 10 kHz."""
    f = np.linspace(0, STOI_FS, STOI_NFFT + 1)[:STOI_NFFT // 2 + 1]
    k = np.arange(STOI_BANDS)
    lo = STOI_MIN_CF * 2.0 ** ((2 * k - 1) / 6.0)
    hi = STOI_MIN_CF * 2.0 ** ((2 * k + 1) / 6.0)
    edges = np.zeros((STOI_BANDS, 2), dtype=np.int64)
    for i in range(STOI_BANDS):
        edges[i] = np.argmin((f - lo[i]) ** 2), np.argmin((f - hi[i]) ** 2)
    return edges


def stoi_tables():
    """The constant tables of pdse_metrics_desc.stoi_tables in float64: the analysis window hanning(258)[1:-1], the cos|sin
    basis of the 512-point DFT for bins 0..255, the band edges, and the taps of the 16 kHz -> 10 kHz converter
    (``wavio.taps``).  Returns a float64 array of STOI_TABLE_DOUBLES values (include/pdse.h lists the sections)."""
    from . import wavio

    win = 0.5 * (1 - np.cos(2 * np.pi * np.arange(1, STOI_FRAME + 1) / (STOI_FRAME + 1)))
    k = np.arange(STOI_FRAME)[:, None]
    j = np.arange(STOI_BINS)[None, :]
    ang = ((k * j) % STOI_NFFT) * (2 * np.pi / STOI_NFFT)
    basis = np.concatenate([np.cos(ang), np.sin(ang)], axis=1)                      # [256][512]
    edges = stoi_band_edges()
    if edges.max() > STOI_BINS or (edges[:, 0] >= edges[:, 1]).any():
        raise AssertionError("a one-third-octave band is empty or reaches bin 256: csrc/stoi.hip computes bins 0..255")
    h, up, down, half = wavio.taps(FS, STOI_FS)
    if (up, down, half, h.size) != (5, 8, 128, 257):
        raise AssertionError("csrc/stoi.hip holds the polyphase constants of 16 kHz -> 10 kHz: up 5, down 8, half 128")
    out = np.zeros(L.STOI_TABLE_DOUBLES)
    out[L.STOI_OFF_WIN:L.STOI_OFF_WIN + STOI_FRAME] = win
    out[L.STOI_OFF_BASIS:L.STOI_OFF_BRANGE] = basis.reshape(-1)
    out[L.STOI_OFF_BRANGE:L.STOI_OFF_BRANGE + 2 * STOI_BANDS] = edges.reshape(-1)
    out[L.STOI_OFF_TAPS:L.STOI_OFF_TAPS + h.size] = h
    return out


_TABLES = {}      # device -> uploaded tables
_STOI_TABLES = {}


def _device_tables(device):
    import torch

    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _TABLES:
        # pageable host memory: this copy returns only when the data is on the device, so a later call on another stream
        # cannot run ahead of the upload
        _TABLES[key] = torch.from_numpy(tables()).to(device)
    return _TABLES[key]


def _device_stoi_tables(device):
    import torch

    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _STOI_TABLES:
        _STOI_TABLES[key] = torch.from_numpy(stoi_tables()).to(device)      # pageable, as above
    return _STOI_TABLES[key]


def _check(clean, proc, lens):
    """Shape and length rules shared by ``quality`` and its callers; returns (B, Lmax, lens as int32 numpy)."""
    if getattr(clean, "ndim", 0) != 2 or tuple(clean.shape) != tuple(proc.shape):
        raise ValueError("clean, proc: two [B, L] tensors of one shape")
    B, Lmax = int(clean.shape[0]), int(clean.shape[1])
    if B < 1:
        raise ValueError("an empty batch has no scores")
    if lens is None:
        lens_np = np.full(B, Lmax, dtype=np.int32)
    else:
        if hasattr(lens, "detach"):
            lens = lens.detach().cpu().numpy()
        lens_np = np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(-1))
        if lens_np.size != B:
            raise ValueError("lens: one length per utterance")
        if lens_np.max() > Lmax:
            raise ValueError("lens: an utterance cannot be longer than the batch (%d > %d)" % (lens_np.max(), Lmax))
        lens_np = lens_np.astype(np.int32)
    if lens_np.min() < MIN_LEN:
        raise ValueError("utterances must hold two 480-sample frames (at least %d samples, got %d)" % (MIN_LEN, lens_np.min()))
    return B, Lmax, lens_np


def quality(clean, proc, lens=None, per_frame=False, stoi=False):
    """SSNR, LLR, WSS and fwSNRseg of every utterance pair of a batch, computed on the device the tensors live on.

    clean, proc: fp32 [B, L] device tensors (``proc`` is the enhanced or the noisy signal); lens: per-utterance lengths
    (list, array or tensor; host values - a device tensor is copied back first), default every utterance spans L.  Samples
    beyond an utterance's length are never read.  Returns a dict of device tensors ``ssnr``, ``llr``, ``wss``, ``fwsnrseg``,
    each [B]; with ``per_frame`` also ``frames`` ([4, B, M] in that order; entries beyond an utterance's own
    ``frame_count`` are undefined) and ``frame_counts`` (list).  Asynchronous on the current stream; the constant tables are
    uploaded once per device.  Raises ValueError for shape or length errors.

    stoi=True adds ``stoi`` and ``estoi`` ([B] device tensors): the short-time objective intelligibility measure of Taal et al.
    (2011) and its extended form (Jensen & Taal 2016) at 10 kHz, 256-sample frames every 128, 15 one-third-octave bands, segments
    of 30 frames (csrc/stoi.hip, four more launches).  An utterance left with fewer than 30 frames after the silent frames are
    removed scores 1e-5.  The 16 kHz -> 10 kHz conversion is this package's own Kaiser-windowed-sinc converter
    (``wavio.resample``, bit for bit); ``pystoi`` designs a different low-pass, so - like the wav front end against librosa -
    scores agree with it to filter-design accuracy, not bit for bit, and that agreement has not been measured.
    With the default the call, its launches and its result are what they were without the argument."""
    import torch

    B, Lmax, lens_np = _check(clean, proc, lens)
    if clean.dtype != torch.float32 or proc.dtype != torch.float32:
        raise ValueError("clean, proc must be fp32")
    if clean.device.type != "cuda" or proc.device != clean.device:
        raise L.PdseError("quality runs on the GPU only (no CPU fallback): both tensors on one cuda device")
    clean, proc = clean.contiguous(), proc.contiguous()
    dev = clean.device
    Mmax = frame_count(Lmax)
    tab = _device_tables(dev)
    lens_dev = torch.from_numpy(lens_np).to(dev)
    frames = torch.empty(4, B, Mmax, dtype=torch.float32, device=dev)
    work = torch.empty(2, B, Mmax, dtype=torch.float32, device=dev)
    out = torch.empty(B, 4, dtype=torch.float32, device=dev)
    d = L.MetricsDesc()
    d.clean, d.proc, d.lens_host, d.lens = clean.data_ptr(), proc.data_ptr(), lens_np.ctypes.data, lens_dev.data_ptr()
    d.tables, d.frames, d.sorted, d.out = tab.data_ptr(), frames.data_ptr(), work.data_ptr(), out.data_ptr()
    d.B, d.Lmax, d.Mmax = B, Lmax, Mmax
    if stoi:
        stab = _device_stoi_tables(dev)
        swork = torch.empty(L.stoi_work_doubles(B, Lmax), dtype=torch.float64, device=dev)
        sout = torch.empty(B, 2, dtype=torch.float32, device=dev)
        d.measures, d.stoi_tables, d.stoi_work, d.stoi_out = L.METRICS_STOI, stab.data_ptr(), swork.data_ptr(), sout.data_ptr()
    L.launch(d, torch.cuda.current_stream(dev).cuda_stream, device=dev)
    res = {"ssnr": out[:, 0], "llr": out[:, 1], "wss": out[:, 2], "fwsnrseg": out[:, 3]}
    if stoi:
        res["stoi"], res["estoi"] = sout[:, 0], sout[:, 1]
    if per_frame:
        res["frames"] = frames
        res["frame_counts"] = [frame_count(n) for n in lens_np]
    return res


def composite(llr, wss, ssnr, pesq):
    """(Csig, Cbak, Covl): the three linear forms of the composite measure, each limited to [1, 5] (:462-470).  Tensors
    (any device, broadcastable) or floats.  ``pesq`` comes from the caller: the reference obtains it from the ``pesq``
    package (ITU-T P.862 code), which this package neither contains nor depends on."""
    import torch

    if any(torch.is_tensor(v) for v in (llr, wss, ssnr, pesq)):
        lim = lambda v: torch.clamp(v, 1.0, 5.0)      # noqa: E731
    else:
        lim = lambda v: min(5.0, max(1.0, v))         # noqa: E731
    csig = 3.093 - 1.029 * llr + 0.603 * pesq - 0.009 * wss
    cbak = 1.634 + 0.478 * pesq - 0.007 * wss + 0.063 * ssnr
    covl = 1.594 + 0.805 * pesq - 0.512 * llr - 0.007 * wss
    return lim(csig), lim(cbak), lim(covl)


def pair_files(refdir, degdir):
    """Sorted ``*.wav`` of both directories paired by position, as the reference's ``compare`` does (:591-597)."""
    ref = sorted(glob.glob("%s/*.wav" % refdir))
    deg = sorted(glob.glob("%s/*.wav" % degdir))
    assert len(ref) == len(deg), "%d reference files, %d degraded files" % (len(ref), len(deg))
    return list(zip(ref, deg))


def load_pairs(pairs, formats="pcm"):
    """Read every pair at 16 kHz; both files of a pair must be equally long (:513).  Returns {length: [(clean, deg), ...]}.
    formats="all": ``wavio.read_any`` instead of ``wavio.read_wav`` (24-bit, float, G.711, extensible headers)."""
    from . import wavio

    read = {"pcm": wavio.read_wav, "all": wavio.read_any}[formats]
    groups = {}
    for r, g in pairs:
        c, p = read(r, FS), read(g, FS)
        assert len(c) == len(p), "c.shape=%r, p.shape=%r (%s, %s)" % (c.shape, p.shape, r, g)
        groups.setdefault(len(c), []).append((c, p))
    return groups


def load_pairs_device(pairs, device, chunk=32, formats="pcm"):
    """``load_pairs`` with the decoding and the 16 kHz conversion on the device (``wavdev.load``: the same samples bit for
    bit): {length: [(clean, deg), ...]} of 1-D device tensors, ``chunk`` pairs per launch.  The rows are copies of their own
    length: a chunk's padded [chunk, Lmax] tensors are released before the next chunk is loaded.  formats: ``wavdev.load``'s."""
    from . import wavdev

    groups = {}
    for i in range(0, len(pairs), chunk):
        part = pairs[i:i + chunk]
        c, cl = wavdev.load([r for r, _ in part], device, FS, formats=formats)
        p, pl = wavdev.load([g for _, g in part], device, FS, formats=formats)
        for k, (r, g) in enumerate(part):
            assert cl[k] == pl[k], "c.shape=%r, p.shape=%r (%s, %s)" % ((cl[k],), (pl[k],), r, g)
            groups.setdefault(cl[k], []).append((c[k, :cl[k]].clone(), p[k, :pl[k]].clone()))
    return groups


def main(argv=None, device=None, batch=32):
    """device: default the current cuda device."""
    import torch

    argv = list(sys.argv[1:] if argv is None else argv)
    stoi = "--stoi" in argv
    if stoi:
        argv.remove("--stoi")
    formats = "all" if "--all-wav" in argv else "pcm"
    if formats == "all":
        argv.remove("--all-wav")
    if len(argv) != 2:
        print("usage: python -m prior_diffuse_amd.metrics [--stoi] [--all-wav] REF_DIR DEG_DIR")
        return 2
    pairs = pair_files(argv[0], argv[1])
    if not pairs:
        print("no *.wav files in %s" % argv[0])
        return 1
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    groups = load_pairs_device(pairs, device, batch, formats=formats)
    rows = []
    for length in sorted(groups):
        items = groups[length]
        for i in range(0, len(items), batch):       # files of one length share a batch
            c = torch.stack([a for a, _ in items[i:i + batch]])
            p = torch.stack([a for _, a in items[i:i + batch]])
            q = quality(c, p, stoi=True) if stoi else quality(c, p)
            keys = ["ssnr", "llr", "wss", "fwsnrseg"] + (["stoi", "estoi"] if stoi else [])
            rows.append(torch.stack([q[k] for k in keys], dim=1).double().cpu().numpy())
    pm = np.concatenate(rows).mean(axis=0)
    print("ref=", argv[0])
    print("deg=", argv[1])
    if stoi:
        print("ssnr:%6.4f llr:%6.4f wss:%6.4f fwsnrseg:%6.4f stoi:%6.4f estoi:%6.4f" % tuple(pm))
        print("PESQ is not computed (the reference takes it from the pesq package).")
    else:
        print("ssnr:%6.4f llr:%6.4f wss:%6.4f fwsnrseg:%6.4f" % tuple(pm))
        print("PESQ and STOI are not computed (the reference takes them from the pesq and pystoi packages).")
    return 0


if __name__ == "__main__":
    sys.exit(main())
