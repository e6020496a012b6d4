// metrics.hip — objective speech-quality scores on the device: segmental SNR, log-likelihood ratio, weighted spectral
// slope and frequency-weighted segmental SNR of the reference's utils/metrics.py (SNRseg :36-55, llr + lpcoeff :192-263,
// wss + findLocPeaks :266-427, fwSNRseg :58-174) at fs = 16000: 480-sample frames every 120 samples, a 1024-point
// DFT of which bins 0..511 are used, LPC order 16, 25 critical bands.
//
// Three launches on the caller's stream, no host synchronisation:
//   metrics_time_kernel   one wave per frame: windowing, energies, autocorrelation lags 0..16 of both signals,
//                         Levinson-Durbin, the two Toeplitz forms -> per-frame SSNR and LLR.  The reference does all of
//                         this in float64 up to the fp32 cast of :221-227, and so does the kernel: the work is tiny
//                         (17 lags x 480 samples per frame) and the recursion is where fp32 would cost accuracy.
//   metrics_spec_kernel   8 frames x 2 signals = the 16 rows of v_mfma_f64_16x16x4_f64 tiles: [16 x 480] windowed frames
//                         times the [480 x 1024] cos|sin basis, magnitude in the epilogue, power of the 256 bins the
//                         critical-band filters reach kept in LDS, the 25-band projections, then the per-frame WSS and
//                         fwSNRseg values, all in float64.  The spectrum never leaves the workgroup.
//   metrics_reduce_kernel one workgroup per utterance: the means, and for LLR / WSS the ascending order (rank count, NaN
//                         last like numpy.sort) and the mean of the first round(0.95 m) values.
// pdse_metrics_desc.measures = PDSE_METRICS_STOI adds STOI and ESTOI behind them: csrc/stoi.hip, four launches of its own.
// Every sum has a fixed order and every frame is computed from its own samples at a position in its tile that depends on
// the frame index alone, so an utterance's scores do not depend on scheduling, on B or on its place in the batch.
//
// Frames: the reference counts n = (len - 360) / 120 time-domain frames and drops the last one (:54, :247), and its
// spectral measures use int(len / 120 - 4) = n - 1 frames of the signal cut to that many (:145-152).  All four measures
// therefore cover frames 0 .. m-1, m = (len - 480) / 120, and only those are computed.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pdse.h"
#include "pdse_internal.h"

#define REQ(cond, msg)          \
  do {                          \
    if (!(cond)) {              \
      pdse_set_error(msg);      \
      return 1;                 \
    }                           \
  } while (0)

namespace {

constexpr int WIN = 480, HOP = 120, ORDER = 16, NBAND = 25, NBIN = 512;
constexpr double EPS64 = 2.220446049250313e-16;   // np.finfo(np.float64).eps
constexpr int TFR = 4;                            // frames per workgroup, time-domain kernel (one per wave)
constexpr int XW = 528;                           // 480 windowed samples + zeros up to 64 * 8 + 16
constexpr int SFR = 8;                            // frames per workgroup, spectral kernel (x 2 signals = 16 tile rows)
constexpr int SSAMP = SFR * HOP + WIN - HOP;      // 1320 samples feed 8 frames
constexpr int PBIN = 256;                         // the critical-band filters end below this bin (checked on the host side)
constexpr int PROW = PBIN + 1;

__device__ __forceinline__ int utt_frames(const pdse_metrics_desc& d, int b) {
  const int len = min(max(d.lens[b], 0), d.Lmax);
  return min(max((len - WIN) / HOP, 0), d.Mmax);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;   // every lane holds the same bits
}

// lpcoeff :202-227: Levinson-Durbin in float64 with the max(E, eps) guard, then lpparams = [1, -a] in fp32
__device__ __forceinline__ void levinson(const double (&R)[ORDER + 1], float (&A)[ORDER + 1]) {
  double a[ORDER], E = R[0];
#pragma unroll
  for (int i = 0; i < ORDER; ++i) {
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < i; ++j) sum += a[j] * R[i - j];
    const double rc = (R[i + 1] - sum) / fmax(E, EPS64);
    double nw[ORDER];
#pragma unroll
    for (int j = 0; j < i; ++j) nw[j] = a[j] - rc * a[i - 1 - j];
#pragma unroll
    for (int j = 0; j < i; ++j) a[j] = nw[j];
    a[i] = rc;
    E = (1.0 - rc * rc) * E;
  }
  A[0] = 1.0f;
#pragma unroll
  for (int j = 0; j < ORDER; ++j) A[j + 1] = (float)(-a[j]);
}

// A . toeplitz(R) . A^T in fp32, as :254-255 has it
__device__ __forceinline__ float toeplitz_form(const float (&A)[ORDER + 1], const float (&R)[ORDER + 1]) {
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i <= ORDER; ++i) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j <= ORDER; ++j) v = fmaf(R[i > j ? i - j : j - i], A[j], v);
    q = fmaf(A[i], v, q);
  }
  return q;
}

__global__ __launch_bounds__(256) void metrics_time_kernel(const pdse_metrics_desc d) {
  __shared__ double xw[TFR][2][XW];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = utt_frames(d, b);
  if ((int)blockIdx.x * TFR >= m) return;
  const int f = blockIdx.x * TFR + wave;
  const bool live = f < m;
  const double* win = d.tables + PDSE_METRICS_OFF_WIN;
  const int64_t base = (int64_t)b * d.Lmax + (int64_t)f * HOP;   // f * 120 + 479 < len for every live frame
  for (int j = lane; j < XW; j += 64) {
    double c = 0.0, p = 0.0;
    if (live && j < WIN) {
      const double w = win[j];
      c = w * (double)d.clean[base + j];
      p = w * (double)d.proc[base + j];
    }
    xw[wave][0][j] = c;
    xw[wave][1][j] = p;
  }
  __syncthreads();
  if (!live) return;
  const double* xc = xw[wave][0];
  const double* xp = xw[wave][1];
  double Rc[ORDER + 1], Rp[ORDER + 1], en = 0.0;
#pragma unroll
  for (int k = 0; k <= ORDER; ++k) Rc[k] = Rp[k] = 0.0;
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    const int j = lane + 64 * t;               // j + 16 <= 527; samples beyond 479 are zeros
    const double c0 = xc[j], p0 = xp[j], e = c0 - p0;
    en += e * e;
#pragma unroll
    for (int k = 0; k <= ORDER; ++k) {
      Rc[k] += c0 * xc[j + k];
      Rp[k] += p0 * xp[j + k];
    }
  }
#pragma unroll
  for (int k = 0; k <= ORDER; ++k) {
    Rc[k] = wave_sum(Rc[k]);
    Rp[k] = wave_sum(Rp[k]);
  }
  en = wave_sum(en);
  // SNRseg :48-53 (signal energy = lag 0 of the clean frame)
  double snr = 10.0 * log10(Rc[0] / (en + EPS64) + EPS64);
  if (snr < -10.0) snr = -10.0;
  if (snr > 35.0) snr = 35.0;
  // llr :250-259
  float Ac[ORDER + 1], Ap[ORDER + 1], Rf[ORDER + 1];
  levinson(Rc, Ac);
  levinson(Rp, Ap);
#pragma unroll
  for (int k = 0; k <= ORDER; ++k) Rf[k] = (float)Rc[k];
  const float num = toeplitz_form(Ap, Rf), den = toeplitz_form(Ac, Rf);
  double frac = (double)num / (double)den;      // 0 / 0 of a silent frame stays NaN, as in the reference
  if (frac <= 0.0) frac = 1000.0;
  const double dist = log(frac);
  if (lane == 0) {
    const int64_t plane = (int64_t)d.B * d.Mmax, o = (int64_t)b * d.Mmax + f;
    d.frames[PDSE_METRICS_SSNR * plane + o] = (float)snr;
    d.frames[PDSE_METRICS_LLR * plane + o] = (float)dist;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Spectral stage, in float64 throughout.  Measured on the fixtures, an fp32 spectrum left single fwSNRseg frames 2.5e-2 dB
// from the reference (the measure takes the difference of two nearly equal band energies, :165) - more than the 1e-3 the
// reference's four-decimal reports resolve - so the DFT runs on v_mfma_f64_16x16x4_f64 and everything after it stays double.
// Tile rows 0..7: clean frames f0..f0+7, rows 8..15: the processed signal's.  Wave w owns bins 128 w .. 128 w + 127 in two
// passes of 64 bins (re and im of four 16-bin chunks: eight accumulator tiles, 64 VGPRs).
// A operand of k-step kk: lane l holds row l & 15, k = 4 kk + (l >> 4); B: basis[k][bin0 + (l & 15)].
// C/D: column = l & 15, row = (l >> 4) + 4 r, r = 0..3.
// The reference adds float64 eps to both signals before its STFT (:62-63, :292-293).  On fp32 samples that addition is a
// no-op and is not made; its exact effect on the spectrum, eps times the window's own transform, is added in the
// epilogue instead (table WEPS).  It is far below the rounding of any frame that holds signal and is what the reference's
// spectrum of a digitally silent frame consists of, so silent frames normalise to the same finite values there and here.
// ---------------------------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct spec_lds {
  double P[2 * SFR][PROW];     // |Z|^2 of bins 0..255
  double Sp[4][2 * SFR];       // per wave: sum of |Z| over its 128 bins, per row
  double LE[2 * SFR][NBAND];   // 10 log10 of the band energies of |Z|^2, floored at -100 (wss :392-397)
  double EF[2 * SFR][NBAND];   // band energies of |Z| / sum |Z| (fwSNRseg :163-164)
  double win[WIN];
  float xs[2][SSAMP];
};

__device__ __forceinline__ double find_peak(const double* le, int ii) {
  // findLocPeaks :266-282 for one band; slope[n] = le[n + 1] - le[n], n = 0..23
  int n = ii;
  if (le[ii + 1] - le[ii] > 0.0) {
    while (n < NBAND - 1 && le[n + 1] - le[n] > 0.0) ++n;
    return le[n - 1];
  }
  while (n >= 0 && le[n + 1] - le[n] <= 0.0) --n;
  return le[n + 1];
}

__global__ __launch_bounds__(256) void metrics_spec_kernel(const pdse_metrics_desc d) {
  __shared__ spec_lds s;
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = utt_frames(d, b);
  const int f0 = blockIdx.x * SFR;
  if (f0 >= m) return;
  const int limit = m * HOP + (WIN - HOP);      // the signal is cut to its whole frames (:150)
  const double* tab = d.tables;
  for (int i = tid; i < SSAMP; i += 256) {
    const int idx = f0 * HOP + i;
    const bool in = idx < limit;
    const int64_t g = (int64_t)b * d.Lmax + idx;
    s.xs[0][i] = in ? d.clean[g] : 0.0f;
    s.xs[1][i] = in ? d.proc[g] : 0.0f;
  }
  for (int i = tid; i < WIN; i += 256) s.win[i] = tab[PDSE_METRICS_OFF_WIN + i];
  __syncthreads();

  const int row = lane & 15, kq = lane >> 4;
  const float* xrow = &s.xs[row / SFR][(row % SFR) * HOP];
  const double* basis = tab + PDSE_METRICS_OFF_BASIS;
  const double* weps = tab + PDSE_METRICS_OFF_WEPS;
  double ssum[4] = {0.0, 0.0, 0.0, 0.0};
  for (int pass = 0; pass < 2; ++pass) {
    const int bin0 = wave * 128 + pass * 64;
    f64x4 re[4], im[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) re[c][r] = im[c][r] = 0.0;
    const double* bp = basis + (int64_t)kq * 1024 + bin0 + row;
#pragma unroll 2
    for (int kk = 0; kk < WIN / 4; ++kk) {
      const int k = 4 * kk + kq;
      const double a = s.win[k] * (double)xrow[k];
      const double* q = bp + (int64_t)kk * 4096;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        re[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, q[16 * c], re[c], 0, 0, 0);
        im[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, q[NBIN + 16 * c], im[c], 0, 0, 0);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int bin = bin0 + 16 * c + row;
      const double ec = weps[bin], es = weps[NBIN + bin];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double x = re[c][r] + ec, y = im[c][r] + es;
        const double p = x * x + y * y;
        ssum[r] += sqrt(p);
        if (bin0 < PBIN) s.P[kq + 4 * r][bin] = p;   // wave-uniform condition
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double v = ssum[r];
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);   // over the 16 lanes (bins) of this quarter-wave
    if (row == 0) s.Sp[wave][kq + 4 * r] = v;
  }
  __syncthreads();

  // 25-band projections of every row (crit_filter.dot(spec), :163-164 and :392-395); the filters are zero outside
  // [lo, hi], so the shortened sum adds the same non-zero terms in the same order
  const double* crit = tab + PDSE_METRICS_OFF_CRIT;
  const double* brange = tab + PDSE_METRICS_OFF_BRANGE;
  for (int idx = tid; idx < 2 * SFR * NBAND; idx += 256) {
    const int r = idx / NBAND, band = idx - r * NBAND;
    const int lo = min(max((int)brange[2 * band], 0), PBIN - 1), hi = min(max((int)brange[2 * band + 1], 0), PBIN - 1);
    double ew = 0.0, ef = 0.0;
    for (int bin = lo; bin <= hi; ++bin) {
      const double c = crit[band * NBIN + bin], p = s.P[r][bin];
      ew += c * p;
      ef += c * sqrt(p);
    }
    const double S = ((s.Sp[0][r] + s.Sp[1][r]) + s.Sp[2][r]) + s.Sp[3][r];
    double le = 10.0 * log10(ew);
    if (le < -100.0) le = -100.0;
    s.LE[r][band] = le;
    s.EF[r][band] = ef / S;
  }
  __syncthreads();

  // one thread per (frame, measure): WSS on threads 0..7, fwSNRseg on threads 64..71 (another wave)
  const int fr = tid & 63;
  if (fr < SFR && f0 + fr < m && (tid >> 6) < 2) {
    const int64_t plane = (int64_t)d.B * d.Mmax, o = (int64_t)b * d.Mmax + f0 + fr;
    if ((tid >> 6) == 0) {
      // wss :399-424, Kmax = 20, Klocmax = 1
      const double* lc = s.LE[fr];
      const double* lp = s.LE[SFR + fr];
      double mc = lc[0], mp = lp[0];
      for (int i = 1; i < NBAND; ++i) {
        if (lc[i] > mc || lc[i] != lc[i]) mc = lc[i];
        if (lp[i] > mp || lp[i] != lp[i]) mp = lp[i];
      }
      double num = 0.0, den = 0.0;
      for (int i = 0; i < NBAND - 1; ++i) {
        const double pc = find_peak(lc, i), pp = find_peak(lp, i);
        const double wc = (20.0 / (20.0 + mc - lc[i])) * (1.0 / (1.0 + pc - lc[i]));
        const double wp = (20.0 / (20.0 + mp - lp[i])) * (1.0 / (1.0 + pp - lp[i]));
        const double w = (wc + wp) / 2.0;
        const double ds = (lc[i + 1] - lc[i]) - (lp[i + 1] - lp[i]);
        num += w * (ds * ds);
        den += w;
      }
      d.frames[PDSE_METRICS_WSS * plane + o] = (float)(num / den);
    } else {
      // fwSNRseg :165-172, gamma = 0.2
      const double* ec = s.EF[fr];
      const double* ep = s.EF[SFR + fr];
      double fn = 0.0, fd = 0.0;
      for (int i = 0; i < NBAND; ++i) {
        const double e = ec[i] - ep[i];
        double err = e * e;
        if (err < EPS64) err = EPS64;
        const double wf = pow(ec[i], 0.2);
        fn += wf * (10.0 * log10(ec[i] * ec[i] / err));
        fd += wf;
      }
      double fw = fn / fd;
      if (fw < -10.0) fw = -10.0;
      if (fw > 35.0) fw = 35.0;
      d.frames[PDSE_METRICS_FWSNRSEG * plane + o] = (float)fw;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-utterance reduction: fixed-order sums in double.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum(double v, double* lds) {
  v = wave_sum(v);
  __syncthreads();                              // lds may still be read from the previous call
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ double strided_sum(const float* v, int n) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += (double)v[i];
  return acc;
}

// numpy.sort order with ties and NaNs (last) broken by index
__device__ __forceinline__ bool before(float vj, int j, float vi, int i) {
  const bool nj = vj != vj, ni = vi != vi;
  if (nj || ni) return (!nj && ni) || (nj && ni && j < i);
  return vj < vi || (vj == vi && j < i);
}

// rank count against LDS-staged chunks of the values (every thread reads the same chunk entry: a broadcast)
constexpr int CHUNK = 1024;
__device__ void sort_into(const float* v, float* sorted, int m, float* chunk) {
  for (int i0 = 0; i0 < m; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const float vi = i < m ? v[i] : 0.0f;
    int rank = 0;
    for (int c0 = 0; c0 < m; c0 += CHUNK) {
      const int n = min(CHUNK, m - c0);
      __syncthreads();
      for (int t = threadIdx.x; t < n; t += 256) chunk[t] = v[c0 + t];
      __syncthreads();
      if (i < m)
        for (int j = 0; j < n; ++j) rank += before(chunk[j], c0 + j, vi, i) ? 1 : 0;
    }
    if (i < m) sorted[rank] = vi;                // ranks are a permutation of 0..m-1
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void metrics_reduce_kernel(const pdse_metrics_desc d) {
  __shared__ double lds[4];
  __shared__ float chunk[CHUNK];
  const int b = blockIdx.x;
  const int m = utt_frames(d, b);
  const int64_t plane = (int64_t)d.B * d.Mmax, o = (int64_t)b * d.Mmax;
  const int keep = (int)rint((double)m * 0.95);   // int(round(len * alpha)), Python's round: half to even (:262, :426)
  const double ssnr = block_sum(strided_sum(d.frames + PDSE_METRICS_SSNR * plane + o, m), lds) / (double)m;
  const double fw = block_sum(strided_sum(d.frames + PDSE_METRICS_FWSNRSEG * plane + o, m), lds) / (double)m;
  float* s0 = d.sorted + o;
  float* s1 = d.sorted + plane + o;
  sort_into(d.frames + PDSE_METRICS_LLR * plane + o, s0, m, chunk);
  sort_into(d.frames + PDSE_METRICS_WSS * plane + o, s1, m, chunk);
  const double llr = block_sum(strided_sum(s0, keep), lds) / (double)keep;
  const double wss = block_sum(strided_sum(s1, keep), lds) / (double)keep;
  if (threadIdx.x == 0) {
    d.out[4 * b + PDSE_METRICS_SSNR] = (float)ssnr;
    d.out[4 * b + PDSE_METRICS_LLR] = (float)llr;
    d.out[4 * b + PDSE_METRICS_WSS] = (float)wss;
    d.out[4 * b + PDSE_METRICS_FWSNRSEG] = (float)fw;
  }
}

}  // namespace

int pdse_metrics_launch(const pdse_metrics_desc* d, hipStream_t s) {
  REQ(d && d->clean && d->proc && d->lens_host && d->lens && d->tables && d->frames && d->sorted && d->out,
      "metrics: null pointer");
  REQ(d->B >= 1 && d->B <= 65535, "metrics: B < 1 (or above 65535)");
  REQ(d->Lmax >= 600, "metrics: len < 600 (Lmax holds fewer than two frames)");
  int longest = 0;
  for (int b = 0; b < d->B; ++b) {
    REQ(d->lens_host[b] >= 600, "metrics: len < 600 (fewer than two frames)");
    REQ(d->lens_host[b] <= d->Lmax, "metrics: len > Lmax");
    longest = d->lens_host[b] > longest ? d->lens_host[b] : longest;
  }
  REQ(d->Mmax >= (longest - WIN) / HOP && d->Mmax <= (d->Lmax - WIN) / HOP, "metrics: Mmax does not match the lengths");
  // measures: 0 is the four measures above alone; the STOI fields are looked at only when it selects them
  REQ(d->measures == 0 || d->measures == PDSE_METRICS_STOI, "metrics: unknown measure selector");
  if (d->measures & PDSE_METRICS_STOI) {
    REQ(d->stoi_tables && d->stoi_work && d->stoi_out, "metrics: null STOI pointer (stoi_tables, stoi_work or stoi_out) with STOI selected");
    REQ(((uintptr_t)d->stoi_tables & 7) == 0 && ((uintptr_t)d->stoi_work & 7) == 0, "metrics: stoi_tables and stoi_work must be 8-byte aligned");
  }
  hipLaunchKernelGGL(metrics_time_kernel, dim3((d->Mmax + TFR - 1) / TFR, d->B), dim3(256), 0, s, *d);
  hipLaunchKernelGGL(metrics_spec_kernel, dim3((d->Mmax + SFR - 1) / SFR, d->B), dim3(256), 0, s, *d);
  hipLaunchKernelGGL(metrics_reduce_kernel, dim3(d->B), dim3(256), 0, s, *d);
  if (pdse_check_launch("metrics")) return 1;
  return (d->measures & PDSE_METRICS_STOI) ? pdse_stoi_launch(d, s) : 0;
}
