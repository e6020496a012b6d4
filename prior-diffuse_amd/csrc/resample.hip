// resample.hip — the wav front end on the device: integer PCM decode, mono mix and polyphase Kaiser-windowed-sinc rate
// conversion of a ragged batch of utterances that share one sample format and one rate, in one launch.  The arithmetic is
// that of prior-diffuse_amd/wavio.py (read_wav + resample) operation for operation, so the fp32 result is bit-identical
// to the host path:
//   decode   fp32: i16 / 32768, float(i32) / 2147483648 (the conversion rounds to nearest even), (u8 - 128) / 128; every
//            division is by a power of two and exact
//   mix      two channels: (a + b) rounded to fp32, then / 2 (numpy's fp32 mean over an axis of two)
//   convert  out[n] = sum over j = -jmax .. +jmax (ascending) of h[r + j up + half] * x[k_c - j] with q = n down,
//            k_c = q / up, r = q % up, jmax = half / up + 1; a term is skipped when |r + j up| > half or k_c - j is
//            outside [0, n_in).  float64 throughout, the product rounded before the add (contraction is switched off for
//            this file: a fused multiply-add rounds once), accumulator started at +0.0, one cast to fp32 at the end.
//            numpy's `out[ok] += h[...] * x[...]` over the same ascending j does exactly this per output.
// The tap table h is built on the host (wavio.taps) and read through L2: it holds 97 doubles for 48 kHz -> 16 kHz but
// 14113 for 44.1 kHz, and the lanes of a wave read neighbouring phases.  A workgroup computes RS_BLOCK consecutive outputs
// of one utterance and first decodes the input window they reach (RS_BLOCK down / up samples plus the filter's two
// half lengths) into LDS, so every input sample is decoded once per workgroup instead of once per tap.
// Row b of out[B][Lmax] holds n_out[b] = ceil(n_in[b] up / down) samples and zeros behind them; every element of the
// row is written.  A row is computed from its own utterance alone, at positions that depend on the output index alone:
// it does not depend on B or on the utterance's place in the batch.  No atomics, no scratch, no host synchronisation.
// All sample positions are 64-bit: n down passes 2^31 for a ten-minute 44.1 kHz file.
// Two kernel templates run the same steps behind the decode (window, convert, zero tail).  resample_kernel<WIDTH, CH>
// is the operator of fmt == 0 - integer PCM, one or two channels - as it was.  wav_kernel<FMT, WIDTH> (fmt != 0) decodes what
// else a RIFF/WAVE file holds - 24-bit PCM, binary32 / binary64, G.711 A-law and mu-law - with the channel count, 1 .. 8, as a
// runtime loop; its arithmetic is wavio.read_any's (include/pdse.h lists it):
//   s24      the three bytes sign-extended, / 8388608 (exact)
//   binary32 the bits as they are, moved as an integer (no arithmetic touches a mono sample: NaN payloads survive)
//   binary64 one conversion to fp32, round to nearest even (v_cvt_f32_f64); beyond the fp32 range: infinity
//   G.711    the 16-bit linear value of the code, / 32768
//   mix      fp32 sum of the channels in channel order, one division by (float)ch (correctly rounded: hipcc's default)
// wav_split_kernel<FMT, WIDTH> (fmt | PDSE_WAV_SPLIT) is wav_kernel without the mix: out has B ch rows, row b ch + c is channel
// c of utterance b decoded alone (wavio.read_channels) and converted by the same steps; the row index comes from the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pdse.h"
#include "pdse_internal.h"

// No floating-point contraction anywhere in this file: hipcc fuses a * b + c by default, also through __dmul_rn / __dadd_rn
// (plain operators in HIP's headers), and the host path rounds the product before the add.
#pragma clang fp contract(off)

#define REQ(cond, msg)          \
  do {                          \
    if (!(cond)) {              \
      pdse_set_error(msg);      \
      return 1;                 \
    }                           \
  } while (0)

namespace {

constexpr int RS_BLOCK = PDSE_RESAMPLE_BLOCK;   // outputs per workgroup = threads per workgroup
constexpr int RS_LDS_MAX = 64 * 1024;           // bytes of input window a workgroup may stage

// one integer sample, little endian, from single bytes: an utterance may start at any byte offset
template <int WIDTH>
__device__ __forceinline__ float pcm_sample(const uint8_t* p) {
  if (WIDTH == 1) return ((float)p[0] - 128.0f) / 128.0f;
  if (WIDTH == 2) return (float)(int16_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8)) / 32768.0f;
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  return (float)(int32_t)v / 2147483648.0f;
}

// frame k of the utterance that starts at byte `base`: decoded and mixed to mono; 0 for a frame that would end beyond the buffer
template <int WIDTH, int CH>
__device__ __forceinline__ float pcm_frame(const pdse_resample_desc& d, int64_t base, int64_t k) {
  const int64_t at = base + k * (int64_t)(WIDTH * CH);
  if (at < 0 || at + WIDTH * CH > d.pcm_bytes) return 0.0f;
  const uint8_t* p = d.pcm + at;
  if (CH == 1) return pcm_sample<WIDTH>(p);
  const float s = pcm_sample<WIDTH>(p) + pcm_sample<WIDTH>(p + WIDTH);
  return s / 2.0f;
}

template <int WIDTH, int CH>
__global__ __launch_bounds__(RS_BLOCK) void resample_kernel(const pdse_resample_desc d, const int jmax, const int win) {
  extern __shared__ float xs[];   // [win] decoded samples k_lo .. k_lo + win - 1 (0 outside the utterance)
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * RS_BLOCK;
  const int64_t n_in = d.n_in[b];
  const int64_t base = d.offs[b];
  const int64_t up = d.up, down = d.down;
  const int64_t n_full = (n_in * up + down - 1) / down;
  const int64_t n_out = n_full < d.Lmax ? n_full : (int64_t)d.Lmax;
  float* const row = d.out + (int64_t)b * d.Lmax;
  const int64_t n = n0 + tid;
  if (n0 >= n_out || n_in < 1) {   // the whole block lies in the row's zero tail (uniform over the workgroup)
    if (n < d.Lmax) row[n] = 0.0f;
    return;
  }
  if (up == down) {                // ratio 1: decode and mix only
    if (n < d.Lmax) row[n] = n < n_out ? pcm_frame<WIDTH, CH>(d, base, n) : 0.0f;
    return;
  }
  // the window of this block: the first output's k_c - jmax up to the last output's k_c + jmax
  const int64_t k_lo = (n0 * down) / up - jmax;
  for (int i = tid; i < win; i += RS_BLOCK) {
    const int64_t k = k_lo + i;
    xs[i] = (k >= 0 && k < n_in) ? pcm_frame<WIDTH, CH>(d, base, k) : 0.0f;
  }
  __syncthreads();
  if (n >= d.Lmax) return;
  if (n >= n_out) {
    row[n] = 0.0f;
    return;
  }
  const int64_t q = n * down;
  const int64_t k_c = q / up;
  const int r = (int)(q - k_c * up);
  const int half = d.half, iup = d.up;
  const int c = (int)(k_c - k_lo);            // position of k_c in the window: jmax <= c < win - jmax
  // j runs over the terms that pass both tests, in ascending order: the sum is the one the host forms
  int j_lo = -jmax, j_hi = jmax;
  if (k_c - j_hi < 0) j_hi = (int)k_c;                        // k_c - j >= 0
  if (k_c - j_lo >= n_in) j_lo = (int)(k_c - n_in + 1);       // k_c - j < n_in
  double acc = 0.0;
  for (int j = j_lo; j <= j_hi; ++j) {
    const int off = r + j * iup;
    if (off < -half || off > half) continue;
    const double p = d.taps[off + half] * (double)xs[c - j];
    acc = acc + p;
  }
  row[n] = (float)acc;
}

// ---- fmt != 0: the encodings of RIFF/WAVE beyond one- and two-channel integer PCM ------------------------------------------
template <int FMT, int WIDTH>
__device__ __forceinline__ float wav_sample(const uint8_t* p) {
  if constexpr (FMT == PDSE_WAV_INT && WIDTH == 3) {
    const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    return (float)((int32_t)(v << 8) >> 8) / 8388608.0f;
  } else if constexpr (FMT == PDSE_WAV_INT) {
    return pcm_sample<WIDTH>(p);
  } else if constexpr (FMT == PDSE_WAV_FLOAT && WIDTH == 4) {
    return __uint_as_float((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
  } else if constexpr (FMT == PDSE_WAV_FLOAT) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | (uint64_t)p[i];
    return (float)__longlong_as_double((long long)v);
  } else if constexpr (FMT == PDSE_WAV_ULAW) {
    const int u = ~(int)p[0] & 0xFF;
    const int mag = ((((u & 15) << 3) + 0x84) << ((u >> 4) & 7)) - 0x84;
    return (float)((u & 0x80) ? -mag : mag) / 32768.0f;
  } else {
    const int a = (int)p[0] ^ 0x55, e = (a >> 4) & 7, m = a & 15;
    const int mag = e == 0 ? (m << 4) + 8 : ((m << 4) + 0x108) << (e - 1);
    return (float)((a & 0x80) ? mag : -mag) / 32768.0f;
  }
}

template <int FMT, int WIDTH>
struct WavFrame {
  __device__ __forceinline__ float operator()(const pdse_resample_desc& d, int64_t base, int64_t k) const {
    const int ch = d.ch;
    const int64_t at = base + k * (int64_t)(WIDTH * ch);
    if (at < 0 || at + WIDTH * ch > d.pcm_bytes) return 0.0f;
    const uint8_t* p = d.pcm + at;
    float s = wav_sample<FMT, WIDTH>(p);
    if (ch == 1) return s;
    for (int c = 1; c < ch; ++c) s = s + wav_sample<FMT, WIDTH>(p + c * WIDTH);
    return s / (float)ch;
  }
};

// resample_kernel's steps behind the decode - zero tail, ratio 1, the LDS window, the float64 polyphase sum - statement for statement,
// with the frame decode as a parameter: frame(d, base, k) is frame k of the utterance at byte `base`, mixed to mono.  resample_kernel
// itself is kept as written rather than rebuilt on this function: going through it changes the register allocation of the six
// instantiations fmt == 0 launches, and those are to stay the code they were.
// b is the utterance (n_in, offs) and y the row of out; the dense kernel passes blockIdx.y for both.
template <class Frame>
__device__ __forceinline__ void resample_block(const pdse_resample_desc& d, const int jmax, const int win, const Frame& frame, const int b,
                                               const int y) {
  extern __shared__ float xs[];   // [win] decoded samples k_lo .. k_lo + win - 1 (0 outside the utterance)
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * RS_BLOCK;
  const int64_t n_in = d.n_in[b];
  const int64_t base = d.offs[b];
  const int64_t up = d.up, down = d.down;
  const int64_t n_full = (n_in * up + down - 1) / down;
  const int64_t n_out = n_full < d.Lmax ? n_full : (int64_t)d.Lmax;
  float* const row = d.out + (int64_t)y * d.Lmax;
  const int64_t n = n0 + tid;
  if (n0 >= n_out || n_in < 1) {   // the whole block lies in the row's zero tail (uniform over the workgroup)
    if (n < d.Lmax) row[n] = 0.0f;
    return;
  }
  if (up == down) {                // ratio 1: decode and mix only
    if (n < d.Lmax) row[n] = n < n_out ? frame(d, base, n) : 0.0f;
    return;
  }
  // the window of this block: the first output's k_c - jmax up to the last output's k_c + jmax
  const int64_t k_lo = (n0 * down) / up - jmax;
  for (int i = tid; i < win; i += RS_BLOCK) {
    const int64_t k = k_lo + i;
    xs[i] = (k >= 0 && k < n_in) ? frame(d, base, k) : 0.0f;
  }
  __syncthreads();
  if (n >= d.Lmax) return;
  if (n >= n_out) {
    row[n] = 0.0f;
    return;
  }
  const int64_t q = n * down;
  const int64_t k_c = q / up;
  const int r = (int)(q - k_c * up);
  const int half = d.half, iup = d.up;
  const int c = (int)(k_c - k_lo);            // position of k_c in the window: jmax <= c < win - jmax
  // j runs over the terms that pass both tests, in ascending order: the sum is the one the host forms
  int j_lo = -jmax, j_hi = jmax;
  if (k_c - j_hi < 0) j_hi = (int)k_c;                        // k_c - j >= 0
  if (k_c - j_lo >= n_in) j_lo = (int)(k_c - n_in + 1);       // k_c - j < n_in
  double acc = 0.0;
  for (int j = j_lo; j <= j_hi; ++j) {
    const int off = r + j * iup;
    if (off < -half || off > half) continue;
    const double p = d.taps[off + half] * (double)xs[c - j];
    acc = acc + p;
  }
  row[n] = (float)acc;
}

template <int FMT, int WIDTH>
__global__ __launch_bounds__(RS_BLOCK) void wav_kernel(const pdse_resample_desc d, const int jmax, const int win) {
  resample_block(d, jmax, win, WavFrame<FMT, WIDTH>(), blockIdx.y, blockIdx.y);
}

// ---- fmt | PDSE_WAV_SPLIT: the channels kept apart ---------------------------------------------------------------------------------
// Channel c of frame k, decoded alone: no mix arithmetic touches the sample (wavio.read_channels).  The frame test is the dense
// kernel's - a frame that would end beyond the buffer reads as zero in every channel.
template <int FMT, int WIDTH>
struct WavChannel {
  int c;
  __device__ __forceinline__ float operator()(const pdse_resample_desc& d, int64_t base, int64_t k) const {
    const int ch = d.ch;
    const int64_t at = base + k * (int64_t)(WIDTH * ch);
    if (at < 0 || at + WIDTH * ch > d.pcm_bytes) return 0.0f;
    return wav_sample<FMT, WIDTH>(d.pcm + at + c * WIDTH);
  }
};

// Row blockIdx.y = b ch + c of out[B ch][Lmax] is channel c of utterance b: the dense kernel's steps on that channel's samples.
template <int FMT, int WIDTH>
__global__ __launch_bounds__(RS_BLOCK) void wav_split_kernel(const pdse_resample_desc d, const int jmax, const int win) {
  const int y = blockIdx.y, b = y / d.ch;
  resample_block(d, jmax, win, WavChannel<FMT, WIDTH>{y - b * d.ch}, b, y);
}

template <int WIDTH, int CH>
void launch(const pdse_resample_desc& d, int jmax, int win, hipStream_t s) {
  const dim3 grid((unsigned)((d.Lmax + RS_BLOCK - 1) / RS_BLOCK), (unsigned)d.B);
  const size_t lds = d.up == d.down ? 0 : (size_t)win * sizeof(float);
  hipLaunchKernelGGL((resample_kernel<WIDTH, CH>), grid, dim3(RS_BLOCK), lds, s, d, jmax, win);
}

template <int FMT, int WIDTH>
void launch_wav(const pdse_resample_desc& d, int jmax, int win, hipStream_t s) {
  const dim3 grid((unsigned)((d.Lmax + RS_BLOCK - 1) / RS_BLOCK), (unsigned)d.B);
  const size_t lds = d.up == d.down ? 0 : (size_t)win * sizeof(float);
  hipLaunchKernelGGL((wav_kernel<FMT, WIDTH>), grid, dim3(RS_BLOCK), lds, s, d, jmax, win);
}

template <int FMT, int WIDTH>
void launch_split(const pdse_resample_desc& d, int jmax, int win, hipStream_t s) {
  const dim3 grid((unsigned)((d.Lmax + RS_BLOCK - 1) / RS_BLOCK), (unsigned)(d.B * d.ch));
  const size_t lds = d.up == d.down ? 0 : (size_t)win * sizeof(float);
  hipLaunchKernelGGL((wav_split_kernel<FMT, WIDTH>), grid, dim3(RS_BLOCK), lds, s, d, jmax, win);
}

}  // namespace

int pdse_resample_launch(const pdse_resample_desc* d, hipStream_t s) {
  REQ(d && d->pcm && d->offs && d->n_in_host && d->n_in && d->out, "resample: null pointer");
  REQ(d->B >= 1 && d->B <= 65535, "resample: B < 1 (or above 65535)");
  REQ(d->up >= 1 && d->down >= 1 && d->half >= 0, "resample: up < 1, down < 1 or half < 0");
  // fmt | PDSE_WAV_SPLIT (fmt one of PDSE_WAV_*): the channels kept apart, out[B ch][Lmax]
  const bool split = d->fmt > 0 && (d->fmt & PDSE_WAV_SPLIT) != 0;
  const int fmt = split ? d->fmt & ~PDSE_WAV_SPLIT : d->fmt;
  if (d->fmt == 0) {
    REQ(d->width == 1 || d->width == 2 || d->width == 4, "resample: width must be 1, 2 or 4 bytes");
    REQ(d->ch == 1 || d->ch == 2, "resample: ch must be 1 or 2");
  } else {
    const int w = d->width;
    REQ(fmt >= PDSE_WAV_INT && fmt <= PDSE_WAV_ULAW, "resample: unknown fmt (0 or PDSE_WAV_INT, _FLOAT, _ALAW, _ULAW)");
    REQ(fmt != PDSE_WAV_INT || (w >= 1 && w <= 4), "resample: fmt PDSE_WAV_INT takes a width of 1, 2, 3 or 4 bytes");
    REQ(fmt != PDSE_WAV_FLOAT || w == 4 || w == 8, "resample: fmt PDSE_WAV_FLOAT takes a width of 4 or 8 bytes");
    REQ((fmt != PDSE_WAV_ALAW && fmt != PDSE_WAV_ULAW) || w == 1, "resample: fmt PDSE_WAV_ALAW / _ULAW takes a width of 1 byte");
    REQ(d->ch >= 1 && d->ch <= PDSE_WAV_MAX_CH, "resample: with fmt != 0 ch must be 1 .. 8");
    REQ(!split || (int64_t)d->B * d->ch <= 65535, "resample: with PDSE_WAV_SPLIT B ch must not pass 65535 rows");
  }
  REQ(d->Lmax >= 1 && d->pcm_bytes >= 0, "resample: Lmax < 1 or pcm_bytes < 0");
  for (int b = 0; b < d->B; ++b) {
    REQ(d->n_in_host[b] >= 1, "resample: n_in < 1");
    const int64_t n_out = ((int64_t)d->n_in_host[b] * d->up + d->down - 1) / d->down;
    REQ(n_out <= d->Lmax, "resample: n_out > Lmax");
  }
  REQ(d->up == d->down || d->taps, "resample: null taps with up != down");
  const int jmax = d->half / d->up + 1;
  const int64_t win = ((int64_t)(RS_BLOCK - 1) * d->down) / d->up + 2 * (int64_t)jmax + 2;
  REQ(d->up == d->down || win * (int64_t)sizeof(float) <= RS_LDS_MAX,
      "resample: the input window of one block of outputs does not fit the LDS budget (down / up or half too large)");
  if (split) {
    switch (fmt * 16 + d->width) {
      case PDSE_WAV_INT * 16 + 1: launch_split<PDSE_WAV_INT, 1>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_INT * 16 + 2: launch_split<PDSE_WAV_INT, 2>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_INT * 16 + 3: launch_split<PDSE_WAV_INT, 3>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_INT * 16 + 4: launch_split<PDSE_WAV_INT, 4>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_FLOAT * 16 + 4: launch_split<PDSE_WAV_FLOAT, 4>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_FLOAT * 16 + 8: launch_split<PDSE_WAV_FLOAT, 8>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_ALAW * 16 + 1: launch_split<PDSE_WAV_ALAW, 1>(*d, jmax, (int)win, s); break;
      default: launch_split<PDSE_WAV_ULAW, 1>(*d, jmax, (int)win, s); break;
    }
    return pdse_check_launch("resample");
  }
  if (d->fmt != 0) {
    switch (d->fmt * 16 + d->width) {
      case PDSE_WAV_INT * 16 + 1: launch_wav<PDSE_WAV_INT, 1>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_INT * 16 + 2: launch_wav<PDSE_WAV_INT, 2>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_INT * 16 + 3: launch_wav<PDSE_WAV_INT, 3>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_INT * 16 + 4: launch_wav<PDSE_WAV_INT, 4>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_FLOAT * 16 + 4: launch_wav<PDSE_WAV_FLOAT, 4>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_FLOAT * 16 + 8: launch_wav<PDSE_WAV_FLOAT, 8>(*d, jmax, (int)win, s); break;
      case PDSE_WAV_ALAW * 16 + 1: launch_wav<PDSE_WAV_ALAW, 1>(*d, jmax, (int)win, s); break;
      default: launch_wav<PDSE_WAV_ULAW, 1>(*d, jmax, (int)win, s); break;
    }
    return pdse_check_launch("resample");
  }
  const int key = d->width * 4 + d->ch;
  switch (key) {
    case 1 * 4 + 1: launch<1, 1>(*d, jmax, (int)win, s); break;
    case 1 * 4 + 2: launch<1, 2>(*d, jmax, (int)win, s); break;
    case 2 * 4 + 1: launch<2, 1>(*d, jmax, (int)win, s); break;
    case 2 * 4 + 2: launch<2, 2>(*d, jmax, (int)win, s); break;
    case 4 * 4 + 1: launch<4, 1>(*d, jmax, (int)win, s); break;
    default: launch<4, 2>(*d, jmax, (int)win, s); break;
  }
  return pdse_check_launch("resample");
}
