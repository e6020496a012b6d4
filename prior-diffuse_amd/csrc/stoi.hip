// stoi.hip — short-time objective intelligibility on the device: STOI (C. H. Taal, R. C. Hendriks, R. Heusdens, J. Jensen,
// "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy Speech", IEEE TASL 19(7), 2011) and its
// extended form ESTOI (J. Jensen, C. H. Taal, "An Algorithm for Predicting the Intelligibility of Speech Masked by Modulated
// Noise Maskers", IEEE/ACM TASLP 24(11), 2016) for B utterance pairs at 16 kHz, written from the two papers.  Reached through
// pdse_metrics_launch when pdse_metrics_desc.measures selects it (include/pdse.h lists the steps and the tables).
//
// Four launches on the caller's stream, no host synchronisation, no atomics:
//   stoi_resample_kernel  16 kHz -> 10 kHz of both signals with the wav front end's polyphase converter (csrc/resample.hip:
//                         the same loop over the same taps, float64, product rounded before the add, one cast to fp32), the
//                         input window of 256 outputs staged in LDS.  The fp32 result is wavio.resample's bit for bit.
//   stoi_mask_kernel      one workgroup per utterance: energy 20 log10(|w x| + eps) of every clean frame (one wave per frame),
//                         the maximum, the keep mask (within 40 dB of it), and the kept frames' indices in order - a ballot
//                         prefix over 256 frames at a time, whole numbers, so the kept set is the same whatever runs when.
//   stoi_spec_kernel      8 kept frames x 2 signals = the 16 rows of v_mfma_f64_16x16x4_f64 tiles.  The silent-frame removal
//                         overlap-adds the kept windowed frames at hop 128, so frame j of the compacted signal is kept frame
//                         j plus the second half of kept frame j - 1 (samples 0..127) or the first half of kept frame j + 1
//                         (samples 128..255): the rows are gathered through the index list and the compacted signal is never
//                         stored.  [16 x 256] windowed rows times the [256 x 512] cos|sin basis, |X|^2 of bins 0..255 into
//                         LDS (the highest one-third-octave band ends at bin 219), the 15 band amplitudes to the workspace.
//   stoi_segment_kernel   one workgroup per utterance, one wave per segment of 30 frames: the clipped, mean-removed, normalised
//                         correlation of every band (one lane per band) and the row-then-column normalised inner product of
//                         ESTOI (one lane per band, then one lane per frame); each wave adds its segments in ascending order
//                         and the four partial sums are added in wave order.
// The spectral stage and everything after it is float64.  tests/emu_stoi.py restates this file in numpy with the spectral
// stage in either precision: in fp32 (tables, DFT, band amplitudes) it stays 4.2e-8 from the float64 statement of the measure
// on the test inputs, far inside the 1e-4 that would have forced float64, so by that rule either would do
// (profiles/stoi_parity.txt).  float64 is used because with it the distance from the oracle is the rounding of the fp32 result
// alone (2.6e-8 measured, half an ulp is 3.0e-8), so the tolerance the GPU test gets - ten times that - is a statement about this file and not
// about how the MFMA's k-ordered fp32 chain differs from numpy's pairwise sums, which the restatement cannot bound; and because
// the DFT is small: 16 x 256 x 512 multiply-adds per workgroup, the tiles csrc/metrics.hip runs in float64 at four times the
// length.  What an fp32 stage would save has not been measured.
// Every sum has a fixed order and every value is computed from its own utterance at a position that depends on the frame or
// segment index alone, so a score does not depend on scheduling, on B or on the utterance's place in the batch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "pdse.h"
#include "pdse_internal.h"

// No floating-point contraction: the resampling must round the product before the add, as the host path does
// (csrc/resample.hip), and the rest of the file then rounds like its numpy restatement.
#pragma clang fp contract(off)

namespace {

constexpr int UP = 5, DOWN = 8, HALF = 128, JMAX = HALF / UP + 1;         // wavio.taps(16000, 10000)
constexpr int RS_BLOCK = 256;                                             // outputs per workgroup
constexpr int RS_WIN = ((RS_BLOCK - 1) * DOWN) / UP + 2 * JMAX + 2;       // 462 input samples feed them
constexpr int FL = 256, FHOP = 128, NBAND = 15, NSEG = 30, NBIN = 256;
constexpr int SFR = 8;                                                    // kept frames per workgroup (x 2 signals = 16 tile rows)
constexpr int AROW = FL + 2;                                              // row stride of the A tile: rows 4 dwords apart in the banks
constexpr int PROW = NBIN + 1;
constexpr double EPS64 = 2.220446049250313e-16;                           // np.finfo(np.float64).eps
constexpr double DYN_RANGE = 40.0;
constexpr double CLIP = 1.0 + 5.623413251903491;                          // 1 + 10^(-beta / 20), beta = -15 dB

typedef double f64x4 __attribute__((ext_vector_type(4)));

// the slices of pdse_metrics_desc.stoi_work (PDSE_STOI_WORK_DOUBLES)
struct stoi_ws {
  float* x10;       // [2][B][N10] both signals at 10 kHz
  double* en;       // [B][F] clean frame energies in dB
  int32_t* idx;     // [B][IS]: indices of the kept frames in order, their count at [F]
  double* bands;    // [2][B][F][15] band amplitudes of the compacted signals
  int64_t N10;
  int F, IS;
};

__device__ __forceinline__ stoi_ws workspace(const pdse_metrics_desc& d) {
  stoi_ws w;
  w.N10 = PDSE_STOI_N10(d.Lmax);
  w.F = (int)PDSE_STOI_FRAMES(d.Lmax);
  w.IS = 2 * ((w.F + 3) / 2);
  double* p = d.stoi_work;
  w.x10 = (float*)p;
  p += (int64_t)d.B * w.N10;
  w.en = p;
  p += (int64_t)d.B * w.F;
  w.idx = (int32_t*)p;
  p += (int64_t)d.B * (w.IS / 2);
  w.bands = p;
  return w;
}

__device__ __forceinline__ int utt_len(const pdse_metrics_desc& d, int b) { return min(max(d.lens[b], 0), d.Lmax); }

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;   // every lane holds the same bits
}

// ---------------------------------------------------------------------------------------------------------------------
// 16 kHz -> 10 kHz: csrc/resample.hip's convert step on fp32 samples that are already in memory
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_BLOCK) void stoi_resample_kernel(const pdse_metrics_desc d) {
  __shared__ float xs[RS_WIN];   // input samples k_lo .. k_lo + RS_WIN - 1 (0 outside the utterance)
  const int b = blockIdx.y, sig = blockIdx.z, tid = threadIdx.x;
  const stoi_ws w = workspace(d);
  const int64_t n_in = utt_len(d, b);
  const int64_t n_out = PDSE_STOI_N10(n_in);
  const int64_t n0 = (int64_t)blockIdx.x * RS_BLOCK;
  if (n0 >= n_out) return;       // uniform over the workgroup; nothing reads beyond n_out
  const float* src = (sig ? d.proc : d.clean) + (int64_t)b * d.Lmax;
  const double* taps = d.stoi_tables + PDSE_STOI_OFF_TAPS;
  const int64_t k_lo = (n0 * DOWN) / UP - JMAX;
  for (int i = tid; i < RS_WIN; i += RS_BLOCK) {
    const int64_t k = k_lo + i;
    xs[i] = (k >= 0 && k < n_in) ? src[k] : 0.0f;
  }
  __syncthreads();
  const int64_t n = n0 + tid;
  if (n >= n_out) return;
  const int64_t q = n * DOWN;
  const int64_t k_c = q / UP;
  const int r = (int)(q - k_c * UP);
  const int c = (int)(k_c - k_lo);              // JMAX <= c < RS_WIN - JMAX
  int j_lo = -JMAX, j_hi = JMAX;
  if (k_c - j_hi < 0) j_hi = (int)k_c;                        // k_c - j >= 0
  if (k_c - j_lo >= n_in) j_lo = (int)(k_c - n_in + 1);       // k_c - j < n_in
  double acc = 0.0;
  for (int j = j_lo; j <= j_hi; ++j) {
    const int off = r + j * UP;
    if (off < -HALF || off > HALF) continue;
    const double p = taps[off + HALF] * (double)xs[c - j];
    acc = acc + p;
  }
  w.x10[((int64_t)sig * d.B + b) * w.N10 + n] = (float)acc;   // n < n_out <= N10
}

// ---------------------------------------------------------------------------------------------------------------------
// Silent-frame removal: which frames stay
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_mask_kernel(const pdse_metrics_desc d) {
  __shared__ double red[4];
  __shared__ int wtot[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const stoi_ws w = workspace(d);
  const int nf = (int)PDSE_STOI_FRAMES(utt_len(d, b));          // <= F
  const float* x = w.x10 + (int64_t)b * w.N10;                  // the clean signal
  double* en = w.en + (int64_t)b * w.F;
  int32_t* idx = w.idx + (int64_t)b * w.IS;
  const double* win = d.stoi_tables + PDSE_STOI_OFF_WIN;
  for (int f = wave; f < nf; f += 4) {                          // f * 128 + 255 < n10 for every whole frame
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < FL / 64; ++i) {
      const int t = lane + 64 * i;
      const double v = win[t] * (double)x[(int64_t)f * FHOP + t];
      a += v * v;
    }
    a = wave_sum(a);
    if (lane == 0) en[f] = 20.0 * log10(sqrt(a) + EPS64);
  }
  __syncthreads();
  double mx = -INFINITY;
  for (int f = tid; f < nf; f += 256) mx = fmax(mx, en[f]);
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  int base = 0;
  for (int f0 = 0; f0 < nf; f0 += 256) {
    const int f = f0 + tid;
    const bool keep = f < nf && (mx - DYN_RANGE - en[f]) < 0.0;
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int v = 0; v < wave; ++v) off += wtot[v];
    if (keep) idx[off + before] = f;                            // off + before < nf <= F
    base += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (tid == 0) idx[w.F] = base;
}

// ---------------------------------------------------------------------------------------------------------------------
// Short-time spectrum of the compacted signals and the band amplitudes.
// A operand of k-step kk: lane l holds row l & 15, k = 4 kk + (l >> 4); B: basis[k][bin0 + (l & 15)].
// C/D: column = l & 15, row = (l >> 4) + 4 r, r = 0..3.  Wave w owns bins 64 w .. 64 w + 63: re and im of four 16-bin chunks.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_spec_kernel(const pdse_metrics_desc d) {
  __shared__ double buf[2 * SFR * AROW];     // the A tile [16][AROW]; afterwards |X|^2 [16][PROW]
  __shared__ double win[FL];
  __shared__ int ks[SFR + 2];                // kept-frame index of compacted frames j0 - 1 .. j0 + 8, -1 outside 0 .. K - 1
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const stoi_ws w = workspace(d);
  const int nf = (int)PDSE_STOI_FRAMES(utt_len(d, b));
  const int32_t* idx = w.idx + (int64_t)b * w.IS;
  const int K = min(max(idx[w.F], 0), nf);
  const int j0 = blockIdx.x * SFR;
  if (j0 >= K) return;
  const double* tab = d.stoi_tables;
  if (tid < SFR + 2) {
    const int j = j0 - 1 + tid;
    ks[tid] = (j >= 0 && j < K) ? min(max(idx[j], 0), nf - 1) : -1;
  }
  win[tid] = tab[PDSE_STOI_OFF_WIN + tid];
  __syncthreads();
  {
    const int t = tid, u = tid ^ FHOP;         // u: this position inside the neighbouring frame that overlaps it
    const double wt = win[t], wu = win[u];
#pragma unroll 4
    for (int r = 0; r < 2 * SFR; ++r) {
      const int jj = r & (SFR - 1);
      const float* x = w.x10 + ((int64_t)(r / SFR) * d.B + b) * w.N10;
      const int kc = ks[jj + 1], kn = t < FHOP ? ks[jj] : ks[jj + 2];
      double v = 0.0;
      if (kc >= 0) {
        v = wt * (double)x[(int64_t)kc * FHOP + t];
        if (kn >= 0) v = v + wu * (double)x[(int64_t)kn * FHOP + u];
      }
      buf[r * AROW + t] = wt * v;              // the analysis window on the overlap-added signal
    }
  }
  __syncthreads();

  const int row = lane & 15, kq = lane >> 4;
  const double* arow = buf + row * AROW;
  const double* bp = tab + PDSE_STOI_OFF_BASIS + kq * (2 * NBIN) + wave * 64 + row;
  f64x4 re[4], im[4];
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) re[c][r] = im[c][r] = 0.0;
#pragma unroll 2
  for (int kk = 0; kk < FL / 4; ++kk) {
    const double a = arow[4 * kk + kq];
    const double* q = bp + kk * (4 * 2 * NBIN);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      re[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, q[16 * c], re[c], 0, 0, 0);
      im[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, q[NBIN + 16 * c], im[c], 0, 0, 0);
    }
  }
  __syncthreads();                             // every wave has read its A rows: the buffer becomes |X|^2
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int bin = wave * 64 + 16 * c + row;
#pragma unroll
    for (int r = 0; r < 4; ++r) buf[(kq + 4 * r) * PROW + bin] = re[c][r] * re[c][r] + im[c][r] * im[c][r];
  }
  __syncthreads();

  const double* brange = tab + PDSE_STOI_OFF_BRANGE;
  if (tid < 2 * SFR * NBAND) {
    const int r = tid / NBAND, band = tid - r * NBAND;
    const int lo = min(max((int)brange[2 * band], 0), NBIN), hi = min(max((int)brange[2 * band + 1], 0), NBIN);
    double e = 0.0;
    for (int bin = lo; bin < hi; ++bin) e += buf[r * PROW + bin];
    const int j = j0 + (r & (SFR - 1));
    if (j < K) w.bands[(((int64_t)(r / SFR) * d.B + b) * w.F + j) * NBAND + band] = sqrt(e);   // j < K <= F
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Segments of 30 frames, hop 1: x, y [30][15] band amplitudes of the clean and the processed signal
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_segment_kernel(const pdse_metrics_desc d) {
  __shared__ double seg[4][2][NSEG * NBAND];
  __shared__ double rows[4][4][16];            // per wave: mean and 1 / norm of every row of x, then of y
  __shared__ double part[4][2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const stoi_ws w = workspace(d);
  const int nf = (int)PDSE_STOI_FRAMES(utt_len(d, b));
  const int K = min(max((w.idx + (int64_t)b * w.IS)[w.F], 0), nf);
  const int segs = K - NSEG + 1;
  if (segs < 1) {                              // fewer than 30 frames left: the published implementation's convention
    if (tid < 2) d.stoi_out[2 * b + tid] = 1e-5f;
    return;
  }
  const double* xb = w.bands + (int64_t)b * w.F * NBAND;
  const double* yb = w.bands + ((int64_t)d.B + b) * w.F * NBAND;
  double acc_s = 0.0, acc_e = 0.0;
  for (int s0 = 0; s0 < segs; s0 += 4) {       // the same trip count in every wave
    const int s = s0 + wave;
    const bool live = s < segs;
    double* X = seg[wave][0];
    double* Y = seg[wave][1];
    __syncthreads();
    if (live)
      for (int i = lane; i < NSEG * NBAND; i += 64) {           // frames s .. s + 29 are contiguous: (s + 29) < K
        X[i] = xb[(int64_t)s * NBAND + i];
        Y[i] = yb[(int64_t)s * NBAND + i];
      }
    __syncthreads();
    double ds = 0.0, de = 0.0;
    if (live && lane < NBAND) {
      const int j = lane;
      // STOI: scale y to x's norm, clip, remove the means, normalise, correlate
      double sx = 0.0, sy = 0.0;
      for (int n = 0; n < NSEG; ++n) {
        const double x = X[n * NBAND + j], y = Y[n * NBAND + j];
        sx += x * x;
        sy += y * y;
      }
      const double c = sqrt(sx) / (sqrt(sy) + EPS64);
      double mx = 0.0, my = 0.0;
      for (int n = 0; n < NSEG; ++n) {
        const double x = X[n * NBAND + j];
        mx += x;
        my += fmin(Y[n * NBAND + j] * c, x * CLIP);
      }
      mx = mx / (double)NSEG;
      my = my / (double)NSEG;
      double sxx = 0.0, syy = 0.0;
      for (int n = 0; n < NSEG; ++n) {
        const double x = X[n * NBAND + j];
        const double p = x - mx, q = fmin(Y[n * NBAND + j] * c, x * CLIP) - my;
        sxx += p * p;
        syy += q * q;
      }
      const double nx = sqrt(sxx) + EPS64, ny = sqrt(syy) + EPS64;
      for (int n = 0; n < NSEG; ++n) {
        const double x = X[n * NBAND + j];
        const double p = x - mx, q = fmin(Y[n * NBAND + j] * c, x * CLIP) - my;
        ds += (q / ny) * (p / nx);
      }
      // ESTOI, rows: mean and norm of band j over the 30 frames
      double ry = 0.0;
      for (int n = 0; n < NSEG; ++n) ry += Y[n * NBAND + j];
      ry = ry / (double)NSEG;
      double ryy = 0.0;
      for (int n = 0; n < NSEG; ++n) {
        const double q = Y[n * NBAND + j] - ry;
        ryy += q * q;
      }
      rows[wave][0][j] = mx;
      rows[wave][1][j] = 1.0 / sqrt(sxx);
      rows[wave][2][j] = ry;
      rows[wave][3][j] = 1.0 / sqrt(ryy);
    }
    __syncthreads();
    if (live && lane < NSEG) {
      // ESTOI, columns: frame n of the row-normalised segment over the 15 bands
      const int n = lane;
      const double* R = &rows[wave][0][0];
      double mu = 0.0, mv = 0.0;
      for (int j = 0; j < NBAND; ++j) {
        mu += (X[n * NBAND + j] - R[j]) * R[16 + j];
        mv += (Y[n * NBAND + j] - R[32 + j]) * R[48 + j];
      }
      mu = mu / (double)NBAND;
      mv = mv / (double)NBAND;
      double suu = 0.0, svv = 0.0;
      for (int j = 0; j < NBAND; ++j) {
        const double u = (X[n * NBAND + j] - R[j]) * R[16 + j] - mu, v = (Y[n * NBAND + j] - R[32 + j]) * R[48 + j] - mv;
        suu += u * u;
        svv += v * v;
      }
      const double iu = 1.0 / sqrt(suu), iv = 1.0 / sqrt(svv);
      for (int j = 0; j < NBAND; ++j) {
        const double u = (X[n * NBAND + j] - R[j]) * R[16 + j] - mu, v = (Y[n * NBAND + j] - R[32 + j]) * R[48 + j] - mv;
        de += (u * iu) * (v * iv);
      }
    }
    ds = wave_sum(ds);
    de = wave_sum(de);
    if (live) {
      acc_s += ds;
      acc_e += de;
    }
  }
  if (lane == 0) {
    part[wave][0] = acc_s;
    part[wave][1] = acc_e;
  }
  __syncthreads();
  if (tid < 2) {
    const double sum = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    d.stoi_out[2 * b + tid] = (float)(sum / ((double)(tid == 0 ? NBAND : NSEG) * (double)segs));
  }
}

}  // namespace

// validated by pdse_metrics_launch before its own launches: pointers and their alignment, B, Lmax >= 600 (so F >= 1) and the lengths
int pdse_stoi_launch(const pdse_metrics_desc* d, hipStream_t s) {
  const int64_t n10 = PDSE_STOI_N10(d->Lmax);
  const int64_t F = PDSE_STOI_FRAMES(d->Lmax);
  hipLaunchKernelGGL(stoi_resample_kernel, dim3((unsigned)((n10 + RS_BLOCK - 1) / RS_BLOCK), d->B, 2), dim3(RS_BLOCK), 0, s, *d);
  hipLaunchKernelGGL(stoi_mask_kernel, dim3(d->B), dim3(256), 0, s, *d);
  hipLaunchKernelGGL(stoi_spec_kernel, dim3((unsigned)((F + SFR - 1) / SFR), d->B), dim3(256), 0, s, *d);
  hipLaunchKernelGGL(stoi_segment_kernel, dim3(d->B), dim3(256), 0, s, *d);
  return pdse_check_launch("metrics (stoi)");
}
