// valid.hip — the two memory-rate passes of the validation epoch (trainer/complex_ddpm_trainer.py:399-580) that the sampling
// path does not have: the (noisy, clean) pair front end of Collate.collate_fn (utils/dataset.py:45-58) and the masked losses of
// utils/loss.py (com_mse_loss :34-44, mag_mse_loss :10-19, com_mag_mse_loss :59-71).  Plain arguments, no descriptor and no
// operator kind: the calls are additive within the ABI version and cannot be recorded in a plan.
#include <hip/hip_runtime.h>
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

// ---------------------------------------------------------------------------------------
// Pair front end: one workgroup per utterance.  c = sqrt(sum x^2 / len) of the NOISY row over its own len samples - the
// statements, the strides and the summation tree of wavprep_kernel's batched mode (csrc/misc.hip), so that c and the noisy
// row come out bit for bit as pdse_wavprep_f32 writes them - then both rows divided by that one c and reflect-padded.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void pair_pad_row(const float* x, float* o, const float c, const int L, const int pad, const int len_own,
                                             const bool own, const int tid) {
  const int Lp = L + 2 * pad;
  if (own) {
    // exact ragged batches: reflect at the utterance's own end, zeros behind the reflected tail
    for (int i = tid; i < Lp; i += 1024) {
      int k = i - pad;
      if (k < 0) k = -k;
      const bool tail = k >= len_own + pad;
      if (k >= len_own) k = tail ? 0 : 2 * (len_own - 1) - k;
      o[i] = tail ? 0.f : x[k] / c;
    }
    return;
  }
  for (int i = tid; i < Lp; i += 1024) {
    int k = i - pad;
    if (k < 0) k = -k;
    if (k >= L) k = 2 * (L - 1) - k;
    o[i] = x[k] / c;
  }
}

__global__ __launch_bounds__(1024) void pair_prep_kernel(const float* __restrict__ noisy, const float* __restrict__ clean,
                                                         const int32_t* __restrict__ lens, float* __restrict__ noisy_pad,
                                                         float* __restrict__ clean_pad, float* __restrict__ cout, const int L, const int pad,
                                                         const int reflect_own) {
  __shared__ float red[16];
  __shared__ float cval;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = noisy + (size_t)b * L;
  const int len = min(max(lens[b], 1), L);
  float ss = 0.f;
  for (int i = tid; i < len; i += 1024) ss += x[i] * x[i];
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_down(ss, o);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int w = 0; w < 16; ++w) tot += red[w];
    cval = sqrtf(tot / (float)len);
  }
  __syncthreads();
  const float c = cval;
  if (tid == 0) cout[b] = c;
  const int Lp = L + 2 * pad;
  const int len_own = min(max(lens[b], pad + 1), L);   // every index below stays inside [0, L): 2 (len_own - 1) - k >= 0 for k < len_own + pad
  pair_pad_row(x, noisy_pad + (size_t)b * Lp, c, L, pad, len_own, reflect_own != 0, tid);
  pair_pad_row(clean + (size_t)b * L, clean_pad + (size_t)b * Lp, c, L, pad, len_own, reflect_own != 0, tid);
}

int pdse_pair_prep_launch(const float* noisy, const float* clean, const int32_t* lens, float* noisy_pad, float* clean_pad, float* c,
                          int32_t B, int32_t L, int32_t pad, int32_t reflect_own, hipStream_t s) {
  REQ(noisy && clean && lens && noisy_pad && clean_pad && c, "pair_prep: null pointer");
  REQ(B > 0 && L > 0 && pad >= 0, "pair_prep: bad sizes (B > 0, L > 0, pad >= 0)");
  REQ(pad < L, "pair_prep: reflect padding needs pad < L");
  REQ(reflect_own == 0 || reflect_own == 1, "pair_prep: reflect_own is 0 or 1");
  hipLaunchKernelGGL(pair_prep_kernel, dim3(B), dim3(1024), 0, s, noisy, clean, lens, noisy_pad, clean_pad, c, L, pad, reflect_own);
  return pdse_check_launch("pair_prep");
}

// ---------------------------------------------------------------------------------------
// Masked losses of [B][2][T][F] over frames t < frames[b].  A thread takes quads of four consecutive (t, f) positions of an
// utterance's live region - the re and the im plane of esti and of label at the same index - so that the magnitude term has
// both parts in registers.  Every term is an fp32 value (the reference's tensor operations: difference, square, norm over the
// channel axis) widened to double and added to the thread's running sum; the thread sums go through a shuffle tree and four
// LDS slots (block_sum), PDSE_SPECLOSS_BLOCKS workgroups per utterance leave partials, one workgroup adds them in index
// order.  Nothing is added atomically: the value depends on the data and on (frames[b], F) alone - not on B, T, the
// utterance's place in the batch, the alignment of its planes or the schedule.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double vl_block_sum(double v, double* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();   // the slots may still be read from the previous sum
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) r = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  return r;   // valid on thread 0
}

// four consecutive floats from p, of which the first n (1 .. 4) exist; one 16-byte load where the address allows it (uniform
// over a workgroup: a quad starts a multiple of four floats behind its plane)
__device__ __forceinline__ float4 vl_quad(const float* p, const int n, const bool aligned) {
  if (n == 4 && aligned) return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[0];
  if (n > 1) v.y = p[1];
  if (n > 2) v.z = p[2];
  if (n > 3) v.w = p[3];
  return v;
}

__device__ __forceinline__ void vl_term(const float er, const float ei, const float lr, const float li, double& com, double& mag) {
#pragma clang fp contract(off)
  const float dr = er - lr, di = ei - li;
  const float qr = dr * dr, qi = di * di;
  com += (double)qr;
  com += (double)qi;
  const float e2 = er * er, e3 = ei * ei, l2 = lr * lr, l3 = li * li;
  const float me = sqrtf(e2 + e3), ml = sqrtf(l2 + l3);
  const float dm = me - ml;
  const float qm = dm * dm;
  mag += (double)qm;
}

__global__ __launch_bounds__(256) void speclosses_partial_kernel(const float* __restrict__ esti, const float* __restrict__ label,
                                                                 const int32_t* __restrict__ frames, double* __restrict__ partial,
                                                                 const int T, const int F) {
  __shared__ double lds[4];
  const int b = blockIdx.y;
  const int fr = min(max(frames[b], 0), T);
  const int64_t plane = (int64_t)T * F, live = (int64_t)fr * F;
  const float* er = esti + (int64_t)b * 2 * plane;
  const float* ei = er + plane;
  const float* lr = label + (int64_t)b * 2 * plane;
  const float* li = lr + plane;
  const bool a_er = ((uintptr_t)er & 15) == 0, a_ei = ((uintptr_t)ei & 15) == 0;
  const bool a_lr = ((uintptr_t)lr & 15) == 0, a_li = ((uintptr_t)li & 15) == 0;
  double com = 0.0, mag = 0.0;
  const int64_t quads = (live + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)PDSE_SPECLOSS_BLOCKS * 256) {
    const int64_t i = q << 2;
    const int n = (int)min((int64_t)4, live - i);
    const float4 v0 = vl_quad(er + i, n, a_er), v1 = vl_quad(ei + i, n, a_ei);
    const float4 w0 = vl_quad(lr + i, n, a_lr), w1 = vl_quad(li + i, n, a_li);
    vl_term(v0.x, v1.x, w0.x, w1.x, com, mag);
    if (n > 1) vl_term(v0.y, v1.y, w0.y, w1.y, com, mag);
    if (n > 2) vl_term(v0.z, v1.z, w0.z, w1.z, com, mag);
    if (n > 3) vl_term(v0.w, v1.w, w0.w, w1.w, com, mag);
  }
  const double tc = vl_block_sum(com, lds);
  const double tm = vl_block_sum(mag, lds);
  if (threadIdx.x == 0) {
    double* o = partial + ((int64_t)b * PDSE_SPECLOSS_BLOCKS + blockIdx.x) * 2;
    o[0] = tc;
    o[1] = tm;
  }
}

__global__ __launch_bounds__(256) void speclosses_final_kernel(const int32_t* __restrict__ frames, const double* __restrict__ partial,
                                                               double* __restrict__ per_utt, float* __restrict__ loss, const int B,
                                                               const int T, const int F) {
  // numerator k of utterance b: its partials in workgroup order
  for (int idx = threadIdx.x; idx < 2 * B; idx += 256) {
    const int b = idx >> 1, k = idx & 1;
    double s = 0.0;
    for (int j = 0; j < PDSE_SPECLOSS_BLOCKS; ++j) s += partial[((int64_t)b * PDSE_SPECLOSS_BLOCKS + j) * 2 + k];
    per_utt[idx] = s;
  }
  __syncthreads();   // the workgroup's own global stores are visible to it behind the barrier
  if (threadIdx.x == 0) {
    double com = 0.0, mag = 0.0, fsum = 0.0;
    for (int b = 0; b < B; ++b) {   // utterances in batch order
      com += per_utt[2 * b];
      mag += per_utt[2 * b + 1];
      fsum += (double)min(max(frames[b], 0), T);
    }
    const double c = com / (2.0 * (double)F * fsum), m = mag / ((double)F * fsum);
    loss[0] = (float)c;
    loss[1] = (float)m;
    loss[2] = (float)(0.5 * (c + m));
  }
}

int pdse_spec_losses_launch(const float* esti, const float* label, const int32_t* frames_host, const int32_t* frames, double* partial,
                            double* per_utt, float* loss, int32_t B, int32_t T, int32_t F, hipStream_t s) {
  REQ(esti && label && frames_host && frames && partial && per_utt && loss, "spec_losses: null pointer");
  REQ(B > 0 && B <= 65535 && T > 0 && F > 0, "spec_losses: bad sizes (0 < B <= 65535, T > 0, F > 0)");
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    REQ(frames_host[b] >= 0 && frames_host[b] <= T, "spec_losses: frames outside [0, T]");
    total += frames_host[b];
  }
  REQ(total > 0, "spec_losses: no frame in the batch (the sum of frames is 0: the losses have no denominator)");
  hipLaunchKernelGGL(speclosses_partial_kernel, dim3(PDSE_SPECLOSS_BLOCKS, B), dim3(256), 0, s, esti, label, frames, partial, T, F);
  hipLaunchKernelGGL(speclosses_final_kernel, dim3(1), dim3(256), 0, s, frames, partial, per_utt, loss, B, T, F);
  return pdse_check_launch("spec_losses");
}

// ---------------------------------------------------------------------------------------
// Decompression and windowed inverse DFT of [B][2][T][161] for the waveforms the quality measures compare
// (utils/metrics.py:531-561: |X|^2 with the phase kept, torch.istft's frames).  The sampling path's own back end does this
// with fp32 arithmetic (compand_kernel, fp32 GEMM): 2e-6 from torch.istft, which a score of 20 - 27 dB over a few frames shows
// in its fifth decimal.  Here every frame sample is one double sum: |X| X = sqrt(re^2 + im^2) (re, im) in double from the fp32
// spectrogram, 322 products with a double basis (window and 1 / n_fft folded in) added in k order, one rounding to fp32.
// A workgroup takes VF_ROWS frames of one utterance, thread r the sample r of each; the decompressed rows sit in LDS.
// ---------------------------------------------------------------------------------------
#define VF_F 161
#define VF_N 320
#define VF_ROWS 4

// MODE: the decompress mode of pdse_compand_desc (the other feat_type values, utils/metrics.py:534-551), a template parameter:
// the sqrt case keeps its code.  COPY takes the spectrogram as it is; POW103 and EXPM1 scale (re, im) by f(m) / m in double.
template <int MODE>
__device__ __forceinline__ void spec_decompress(const double re, const double im, double& vr, double& vi) {
  if constexpr (MODE == PDSE_COMPAND_COPY) {
    vr = re;
    vi = im;
  } else {
    const double mag = sqrt(re * re + im * im);
    if constexpr (MODE == PDSE_COMPAND_SQUARE) {
      vr = mag * re;   // |X|^2 cos(phase) = |X| re
      vi = mag * im;
    } else {
      const double g = MODE == PDSE_COMPAND_POW103 ? pow(mag, 10.0 / 3.0) : exp(mag) - 1.0;
      vr = mag > 0.0 ? g * (re / mag) : 0.0;     // f(0) = 0 for both
      vi = mag > 0.0 ? g * (im / mag) : 0.0;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(VF_N) void spec_frames_kernel(const float* __restrict__ spec, const double* __restrict__ basis,
                                                           float* __restrict__ frames, const int T) {
  __shared__ double dec[VF_ROWS][2 * VF_F];
  const int b = blockIdx.y, t0 = blockIdx.x * VF_ROWS, r = threadIdx.x;
  const int64_t plane = (int64_t)T * VF_F;
  const float* re_p = spec + (int64_t)b * 2 * plane;
  const float* im_p = re_p + plane;
  for (int idx = r; idx < VF_ROWS * VF_F; idx += VF_N) {
    const int row = idx / VF_F, f = idx - row * VF_F, t = t0 + row;
    double vr = 0.0, vi = 0.0;
    if (t < T) {
      const double re = (double)re_p[(int64_t)t * VF_F + f], im = (double)im_p[(int64_t)t * VF_F + f];
      spec_decompress<MODE>(re, im, vr, vi);
    }
    dec[row][f] = vr;
    dec[row][VF_F + f] = vi;
  }
  __syncthreads();
  double acc[VF_ROWS];
#pragma unroll
  for (int j = 0; j < VF_ROWS; ++j) acc[j] = 0.0;
  for (int k = 0; k < 2 * VF_F; ++k) {
    const double w = basis[(int64_t)k * VF_N + r];
#pragma unroll
    for (int j = 0; j < VF_ROWS; ++j) acc[j] += dec[j][k] * w;
  }
#pragma unroll
  for (int j = 0; j < VF_ROWS; ++j)
    if (t0 + j < T) frames[((int64_t)b * VF_N + r) * T + t0 + j] = (float)acc[j];
}

int pdse_spec_frames_mode_launch(const float* spec, const double* basis, float* frames, int32_t B, int32_t T, int32_t F, int32_t mode,
                                 hipStream_t s) {
  REQ(spec && basis && frames, "spec_frames: null pointer");
  REQ(B > 0 && B <= 65535 && T > 0, "spec_frames: bad sizes (0 < B <= 65535, T > 0)");
  REQ(F == VF_F, "spec_frames: F must be 161 (n_fft 320)");
  REQ(mode == PDSE_COMPAND_SQUARE || mode == PDSE_COMPAND_COPY || mode == PDSE_COMPAND_POW103 || mode == PDSE_COMPAND_EXPM1,
      "spec_frames: mode must be a decompress mode: 1 (mag**2), 3 (copy), 5 (mag**(10/3)) or 7 (exp(mag)-1)");
  const dim3 grid((T + VF_ROWS - 1) / VF_ROWS, B), block(VF_N);
  switch (mode) {
    case PDSE_COMPAND_SQUARE: hipLaunchKernelGGL(spec_frames_kernel<PDSE_COMPAND_SQUARE>, grid, block, 0, s, spec, basis, frames, T); break;
    case PDSE_COMPAND_COPY: hipLaunchKernelGGL(spec_frames_kernel<PDSE_COMPAND_COPY>, grid, block, 0, s, spec, basis, frames, T); break;
    case PDSE_COMPAND_POW103: hipLaunchKernelGGL(spec_frames_kernel<PDSE_COMPAND_POW103>, grid, block, 0, s, spec, basis, frames, T); break;
    default: hipLaunchKernelGGL(spec_frames_kernel<PDSE_COMPAND_EXPM1>, grid, block, 0, s, spec, basis, frames, T); break;
  }
  return pdse_check_launch("spec_frames");
}

int pdse_spec_frames_launch(const float* spec, const double* basis, float* frames, int32_t B, int32_t T, int32_t F, hipStream_t s) {
  return pdse_spec_frames_mode_launch(spec, basis, frames, B, T, F, PDSE_COMPAND_SQUARE, s);
}
