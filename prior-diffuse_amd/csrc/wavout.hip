// wavout.hip — the wav back end on the device: a ragged batch of fp32 mono waveforms at 16 kHz is converted to the rate of the
// files it came from, encoded in their sample format and interleaved into ch equal channels, in one launch.  The mirror of
// resample.hip, and like it bit-identical to its host path, prior-diffuse_amd/wavio.py (resample + encode), whose arithmetic
// it repeats operation for operation:
//   convert  resample.hip's convert step, read from the fp32 row instead of decoded frames: out[n] = sum over j = -jmax .. +jmax
//            (ascending) of h[r + j up + half] * x[k_c - j] with q = n down, k_c = q / up, r = q % up, jmax = half / up + 1; a
//            term is skipped when |r + j up| > half or k_c - j is outside [0, n_in).  float64 throughout, the product rounded
//            before the add (contraction is switched off for this file), accumulator started at +0.0, one cast to fp32,
//            64-bit positions.  up == down: the sample as it is.
//   encode   integer targets of 2, 3 and 4 bytes: y = float64(x) clamped to [-1, 1 - 2^-(8 width - 1)], v = rint(y * 2^(8 width - 1))
//            (the product is exact, rint rounds half to even as np.round does), stored little endian; NaN is written as 0.  A
//            sample counts as clipped when the clamp changed it (y != x: NaN and the infinities count).  binary32: the bits as
//            they are, nothing clamped.
// A workgroup computes WO_BLOCK consecutive frames of one row: it stages the fp32 input window they reach in LDS (resample.hip's
// window: (WO_BLOCK - 1) down / up + 2 jmax + 2 samples), a lane converts and encodes one whole frame and writes its ch * width
// bytes into an LDS image of the block's bytes, and the workgroup then stores that image with one aligned 32-bit word per lane,
// neighbouring lanes neighbouring words; only the words that straddle an end of the block's byte range go out byte by byte, so two
// workgroups never write the same word.  The image is laid out at the row's own misalignment (a row may start at any byte: stride
// need not be a multiple of 4), which makes every word of it an aligned word of the buffer.  The tap table is read through L2 as
// in the front end (97 doubles for 48 kHz, 14113 for 44.1 kHz).
// Row b of out[B][stride] holds n_keep[b] * ch * width bytes - the first n_keep[b] <= ceil(n_in[b] up / down) frames: a file is
// cut to its source's length - and zeros behind them up to stride; every byte of the row is written.  clipped[b][k] is the
// number of clipped samples (not counted once per channel) among the kept frames of workgroup k, written by every workgroup with
// a plain store; the host sums a row.  A row is computed from its own waveform alone at positions that depend on the frame index
// alone: it does not depend on B or on its place in the batch.  No atomics, no scratch, no host synchronisation.
// A second kernel, wavch_kernel (pdse_wav_encode_channels, at the end of the file), encodes files whose ch channels differ:
// x[B ch][Lmax], a lane taking the ch samples of its frame one after the other; its host path is wavio.encode_channels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pdse.h"
#include "pdse_internal.h"

// As in resample.hip: hipcc fuses a * b + c by default, and the host path rounds the product before the add.
#pragma clang fp contract(off)

#define REQ(cond, msg)          \
  do {                          \
    if (!(cond)) {              \
      pdse_set_error(msg);      \
      return 1;                 \
    }                           \
  } while (0)

namespace {

constexpr int WO_BLOCK = PDSE_RESAMPLE_BLOCK;                       // frames per workgroup = threads per workgroup
constexpr int WO_IMAGE = WO_BLOCK * PDSE_WAV_MAX_CH * 4 + 16;       // bytes of a block's frames at 8 channels of 4 bytes, plus the misalignment
constexpr int WO_LDS_MAX = 64 * 1024;                               // LDS of a workgroup: the image, the wave counts and the input window

template <int FMT, int WIDTH>
__global__ __launch_bounds__(WO_BLOCK) void wavout_kernel(const float* __restrict__ x, const int32_t* __restrict__ n_in_p,
                                                          const int32_t* __restrict__ n_keep_p, const double* __restrict__ taps,
                                                          uint8_t* __restrict__ out, int32_t* __restrict__ clipped, const int64_t stride,
                                                          const int Lmax, const int iup, const int idown, const int half, const int ch,
                                                          const int jmax, const int win) {
  extern __shared__ float xs[];                  // [win] samples k_lo .. k_lo + win - 1 of the row (0 outside it)
  __shared__ uint32_t image[WO_IMAGE / 4];       // the block's bytes, byte i at sh + i
  __shared__ int wave_clips[WO_BLOCK / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int fb = ch * WIDTH;                     // bytes per frame
  const int64_t n0 = (int64_t)blockIdx.x * WO_BLOCK;
  const int64_t g0 = n0 * fb;                    // the block's first byte in the row
  if (g0 >= stride) {                            // not reached with the launcher's grid
    if (tid == 0) clipped[(int64_t)b * gridDim.x + blockIdx.x] = 0;
    return;
  }
  int64_t n_in = n_in_p[b];
  if (n_in > Lmax) n_in = Lmax;                  // never read beyond the row
  const int64_t up = iup, down = idown;
  const int64_t n_full = n_in < 1 ? 0 : (n_in * up + down - 1) / down;
  int64_t keep = n_keep_p[b];
  keep = keep < 0 ? 0 : (keep > n_full ? n_full : keep);
  const float* const row = x + (int64_t)b * Lmax;
  const int64_t n = n0 + tid;
  float xv = 0.0f;
  if (n0 < keep) {                               // uniform over the workgroup: otherwise the block lies in the row's zero tail
    if (up == down) {                            // ratio 1: n < keep <= n_in
      if (n < keep) xv = row[n];
    } else {
      // the window of this block: the first frame's k_c - jmax up to the last frame's k_c + jmax
      const int64_t k_lo = (n0 * down) / up - jmax;
      for (int i = tid; i < win; i += WO_BLOCK) {
        const int64_t k = k_lo + i;
        xs[i] = (k >= 0 && k < n_in) ? row[k] : 0.0f;
      }
      __syncthreads();
      if (n < keep) {
        const int64_t q = n * down;
        const int64_t k_c = q / up;
        const int r = (int)(q - k_c * up);
        const int c = (int)(k_c - k_lo);            // position of k_c in the window: jmax <= c < win - jmax
        // j runs over the terms that pass both tests, in ascending order: the sum is the one the host forms
        int j_lo = -jmax, j_hi = jmax;
        if (k_c - j_hi < 0) j_hi = (int)k_c;                        // k_c - j >= 0
        if (k_c - j_lo >= n_in) j_lo = (int)(k_c - n_in + 1);       // k_c - j < n_in
        double acc = 0.0;
        for (int j = j_lo; j <= j_hi; ++j) {
          const int off = r + j * iup;
          if (off < -half || off > half) continue;
          const double p = taps[off + half] * (double)xs[c - j];
          acc = acc + p;
        }
        xv = (float)acc;
      }
    }
  }
  // encode: the frame's sample as WIDTH little-endian bytes in v (0 behind the kept frames)
  uint32_t v = 0;
  bool clip = false;
  if (n < keep) {
    if constexpr (FMT == PDSE_WAV_FLOAT) {
      v = __float_as_uint(xv);
    } else {
      constexpr double scale = (double)(1ull << (8 * WIDTH - 1));
      constexpr double hi = 1.0 - 1.0 / scale;
      const double xd = (double)xv;
      const double y = xd < -1.0 ? -1.0 : (xd > hi ? hi : xd);      // NaN passes both tests, as through np.clip
      const bool nan = xd != xd;
      clip = y != xd;                                               // true for NaN
      v = nan ? 0u : (uint32_t)(int32_t)rint(y * scale);
    }
  }
  // the lane's frame into the image: ch copies of the sample
  uint8_t* const dst_row = out + (int64_t)b * stride;
  const int sh = (int)((uintptr_t)(dst_row + g0) & 3);
  uint8_t* const img = reinterpret_cast<uint8_t*>(image);
  {
    uint8_t* p = img + sh + tid * fb;
    for (int c = 0; c < ch; ++c, p += WIDTH) {
#pragma unroll
      for (int k = 0; k < WIDTH; ++k) p[k] = (uint8_t)(v >> (8 * k));
    }
  }
  const unsigned long long vote = __ballot(clip);
  if ((tid & 63) == 0) wave_clips[tid >> 6] = __popcll(vote);
  __syncthreads();
  // the image to the row: word w of the image is the aligned word at dst_row + g0 - sh + 4 w
  const int64_t left = stride - g0;
  const int nbytes = left < (int64_t)WO_BLOCK * fb ? (int)left : WO_BLOCK * fb;
  uint8_t* const dst = dst_row + g0 - sh;
  const int nw = (sh + nbytes + 3) >> 2;
  for (int w = tid; w < nw; w += WO_BLOCK) {
    const int lo = 4 * w - sh;                   // the block's byte in the word's first place
    const uint32_t word = image[w];
    if (lo >= 0 && lo + 4 <= nbytes) {
      *reinterpret_cast<uint32_t*>(dst + 4 * (int64_t)w) = word;
    } else {
      for (int k = 0; k < 4; ++k)
        if (lo + k >= 0 && lo + k < nbytes) dst[4 * (int64_t)w + k] = (uint8_t)(word >> (8 * k));
    }
  }
  if (tid == 0) {
    int total = 0;
    for (int i = 0; i < WO_BLOCK / 64; ++i) total += wave_clips[i];
    clipped[(int64_t)b * gridDim.x + blockIdx.x] = total;
  }
}

template <int FMT, int WIDTH>
void launch(const float* x, const int32_t* n_in, const int32_t* n_keep, const double* taps, uint8_t* out, int32_t* clipped,
            int64_t stride, int B, int Lmax, int up, int down, int half, int ch, int jmax, int win, int64_t blocks, hipStream_t s) {
  const dim3 grid((unsigned)blocks, (unsigned)B);
  const size_t lds = up == down ? 0 : (size_t)win * sizeof(float);
  hipLaunchKernelGGL((wavout_kernel<FMT, WIDTH>), grid, dim3(WO_BLOCK), lds, s, x, n_in, n_keep, taps, out, clipped, stride, Lmax, up,
                     down, half, ch, jmax, win);
}

// ---- the channel encoder (pdse_wav_encode_channels): ch different rows per file ------------------------------------------------------
// x[B ch][Lmax]: row b ch + c is channel c of file b; all ch rows of a file hold n_in[b] samples.  The steps are wavout_kernel's, a
// lane taking its frame's channels one after the other: the workgroup stages ch input windows, xs[c][win], a lane converts and
// encodes sample c of its frame - the float64 sum of each channel in the host's order - and writes it at its place in the frame,
// and the image goes out by the same aligned-word scheme.  wavout_kernel itself is kept as written (the mono encoder's four
// instantiations stay the code they were).  clipped[b][k][c]: clipped samples of channel c among the kept frames of workgroup k.
constexpr int WO_CH_STATIC = WO_IMAGE + 256;                        // static LDS of the channel encoder: the image and the wave counts

template <int FMT, int WIDTH>
__global__ __launch_bounds__(WO_BLOCK) void wavch_kernel(const float* __restrict__ x, const int32_t* __restrict__ n_in_p,
                                                         const int32_t* __restrict__ n_keep_p, const double* __restrict__ taps,
                                                         uint8_t* __restrict__ out, int32_t* __restrict__ clipped, const int64_t stride,
                                                         const int Lmax, const int iup, const int idown, const int half, const int ch,
                                                         const int jmax, const int win) {
  extern __shared__ float xs[];                  // [ch][win] samples k_lo .. k_lo + win - 1 of the file's rows (0 outside them)
  __shared__ uint32_t image[WO_IMAGE / 4];       // the block's bytes, byte i at sh + i
  __shared__ int wave_clips[WO_BLOCK / 64][PDSE_WAV_MAX_CH];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int fb = ch * WIDTH;                     // bytes per frame
  const int64_t n0 = (int64_t)blockIdx.x * WO_BLOCK;
  const int64_t g0 = n0 * fb;                    // the block's first byte in the file's row of out
  int32_t* const counts = clipped + ((int64_t)b * gridDim.x + blockIdx.x) * ch;
  if (g0 >= stride) {                            // not reached with the launcher's grid
    if (tid < ch) counts[tid] = 0;
    return;
  }
  int64_t n_in = n_in_p[b];
  if (n_in > Lmax) n_in = Lmax;                  // never read beyond a row
  const int64_t up = iup, down = idown;
  const int64_t n_full = n_in < 1 ? 0 : (n_in * up + down - 1) / down;
  int64_t keep = n_keep_p[b];
  keep = keep < 0 ? 0 : (keep > n_full ? n_full : keep);
  const float* const rows = x + (int64_t)b * ch * Lmax;
  const int64_t n = n0 + tid;
  const bool live = n0 < keep;                   // uniform over the workgroup: otherwise the block lies in the file's zero tail
  const int64_t k_lo = (n0 * down) / up - jmax;  // the window of this block: the first frame's k_c - jmax up to the last frame's k_c + jmax
  if (live && up != down) {
    for (int c = 0; c < ch; ++c) {
      const float* const row = rows + (int64_t)c * Lmax;
      for (int i = tid; i < win; i += WO_BLOCK) {
        const int64_t k = k_lo + i;
        xs[c * win + i] = (k >= 0 && k < n_in) ? row[k] : 0.0f;
      }
    }
    __syncthreads();
  }
  // the frame's position in every channel's window; j runs over the terms that pass both tests, in ascending order
  const int64_t q = n * down;
  const int64_t k_c = q / up;
  const int r = (int)(q - k_c * up);
  const int cw = (int)(k_c - k_lo);              // position of k_c in a window: jmax <= cw < win - jmax
  int j_lo = -jmax, j_hi = jmax;
  if (k_c - j_hi < 0) j_hi = (int)k_c;                        // k_c - j >= 0
  if (k_c - j_lo >= n_in) j_lo = (int)(k_c - n_in + 1);       // k_c - j < n_in
  const uint8_t* const dst_row = out + (int64_t)b * stride;
  const int sh = (int)((uintptr_t)(dst_row + g0) & 3);
  uint8_t* p = reinterpret_cast<uint8_t*>(image) + sh + tid * fb;
  for (int c = 0; c < ch; ++c, p += WIDTH) {
    float xv = 0.0f;
    if (live && n < keep) {
      if (up == down) {                          // ratio 1: n < keep <= n_in
        xv = rows[(int64_t)c * Lmax + n];
      } else {
        const float* const w = xs + c * win;
        double acc = 0.0;
        for (int j = j_lo; j <= j_hi; ++j) {
          const int off = r + j * iup;
          if (off < -half || off > half) continue;
          const double pr = taps[off + half] * (double)w[cw - j];
          acc = acc + pr;
        }
        xv = (float)acc;
      }
    }
    // encode: the sample as WIDTH little-endian bytes in v (0 behind the kept frames)
    uint32_t v = 0;
    bool clip = false;
    if (n < keep) {
      if constexpr (FMT == PDSE_WAV_FLOAT) {
        v = __float_as_uint(xv);
      } else {
        constexpr double scale = (double)(1ull << (8 * WIDTH - 1));
        constexpr double hi = 1.0 - 1.0 / scale;
        const double xd = (double)xv;
        const double y = xd < -1.0 ? -1.0 : (xd > hi ? hi : xd);      // NaN passes both tests, as through np.clip
        const bool nan = xd != xd;
        clip = y != xd;                                               // true for NaN
        v = nan ? 0u : (uint32_t)(int32_t)rint(y * scale);
      }
    }
#pragma unroll
    for (int k = 0; k < WIDTH; ++k) p[k] = (uint8_t)(v >> (8 * k));
    const unsigned long long vote = __ballot(clip);
    if ((tid & 63) == 0) wave_clips[tid >> 6][c] = __popcll(vote);
  }
  __syncthreads();
  // the image to the row: word w of the image is the aligned word at dst_row + g0 - sh + 4 w
  const int64_t left = stride - g0;
  const int nbytes = left < (int64_t)WO_BLOCK * fb ? (int)left : WO_BLOCK * fb;
  uint8_t* const dst = out + (int64_t)b * stride + g0 - sh;
  const int nw = (sh + nbytes + 3) >> 2;
  for (int w = tid; w < nw; w += WO_BLOCK) {
    const int lo = 4 * w - sh;                   // the block's byte in the word's first place
    const uint32_t word = image[w];
    if (lo >= 0 && lo + 4 <= nbytes) {
      *reinterpret_cast<uint32_t*>(dst + 4 * (int64_t)w) = word;
    } else {
      for (int k = 0; k < 4; ++k)
        if (lo + k >= 0 && lo + k < nbytes) dst[4 * (int64_t)w + k] = (uint8_t)(word >> (8 * k));
    }
  }
  if (tid < ch) {
    int total = 0;
    for (int i = 0; i < WO_BLOCK / 64; ++i) total += wave_clips[i][tid];
    counts[tid] = total;
  }
}

template <int FMT, int WIDTH>
void launch_channels(const float* x, const int32_t* n_in, const int32_t* n_keep, const double* taps, uint8_t* out, int32_t* clipped,
                     int64_t stride, int B, int Lmax, int up, int down, int half, int ch, int jmax, int win, int64_t blocks, hipStream_t s) {
  const dim3 grid((unsigned)blocks, (unsigned)B);
  const size_t lds = up == down ? 0 : (size_t)win * ch * sizeof(float);
  hipLaunchKernelGGL((wavch_kernel<FMT, WIDTH>), grid, dim3(WO_BLOCK), lds, s, x, n_in, n_keep, taps, out, clipped, stride, Lmax, up,
                     down, half, ch, jmax, win);
}

}  // namespace

int pdse_wavch_launch(const float* x, const int32_t* n_in_host, const int32_t* n_keep_host, const int32_t* n_in, const int32_t* n_keep,
                      const double* taps, uint8_t* out, int32_t* clipped, int64_t stride, int32_t B, int32_t Lmax, int32_t up,
                      int32_t down, int32_t half, int32_t fmt, int32_t width, int32_t ch, hipStream_t s) {
  REQ(x && n_in_host && n_keep_host && n_in && n_keep && out && clipped, "wav_encode_channels: null pointer");
  REQ(ch >= 1 && ch <= PDSE_WAV_MAX_CH, "wav_encode_channels: ch must be 1 .. 8");
  REQ(B >= 1 && (int64_t)B * ch <= 65535, "wav_encode_channels: B < 1 (or B ch above 65535 rows)");
  REQ(up >= 1 && down >= 1 && half >= 0, "wav_encode_channels: up < 1, down < 1 or half < 0");
  REQ(fmt == PDSE_WAV_INT || fmt == PDSE_WAV_FLOAT, "wav_encode_channels: fmt must be PDSE_WAV_INT or PDSE_WAV_FLOAT");
  REQ(fmt != PDSE_WAV_INT || (width >= 2 && width <= 4), "wav_encode_channels: fmt PDSE_WAV_INT takes a width of 2, 3 or 4 bytes");
  REQ(fmt != PDSE_WAV_FLOAT || width == 4, "wav_encode_channels: fmt PDSE_WAV_FLOAT takes a width of 4 bytes");
  REQ(Lmax >= 1, "wav_encode_channels: Lmax < 1");
  const int64_t fb = (int64_t)ch * width;
  int64_t need = 1;
  for (int b = 0; b < B; ++b) {
    REQ(n_in_host[b] >= 1, "wav_encode_channels: n_in < 1");
    REQ(n_in_host[b] <= Lmax, "wav_encode_channels: n_in > Lmax");
    const int64_t n_out = ((int64_t)n_in_host[b] * up + down - 1) / down;
    REQ(n_keep_host[b] >= 0 && n_keep_host[b] <= n_out, "wav_encode_channels: n_keep outside 0 .. ceil(n_in up / down)");
    if (n_keep_host[b] * fb > need) need = n_keep_host[b] * fb;
  }
  REQ(stride >= need, "wav_encode_channels: stride below the bytes of the longest file (n_keep ch width)");
  REQ(up == down || taps, "wav_encode_channels: null taps with up != down");
  const int jmax = half / up + 1;
  const int64_t win = ((int64_t)(WO_BLOCK - 1) * down) / up + 2 * (int64_t)jmax + 2;
  REQ(up == down || win * ch * (int64_t)sizeof(float) + WO_CH_STATIC <= WO_LDS_MAX,
      "wav_encode_channels: the ch input windows of one block of frames do not fit the LDS budget (down / up, half or ch too large)");
  const int64_t blocks = (stride + WO_BLOCK * fb - 1) / (WO_BLOCK * fb);
  REQ(blocks <= 0x7fffffff, "wav_encode_channels: stride too large");
  if (fmt == PDSE_WAV_FLOAT) {
    launch_channels<PDSE_WAV_FLOAT, 4>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  } else if (width == 2) {
    launch_channels<PDSE_WAV_INT, 2>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  } else if (width == 3) {
    launch_channels<PDSE_WAV_INT, 3>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  } else {
    launch_channels<PDSE_WAV_INT, 4>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  }
  return pdse_check_launch("wav_encode_channels");
}

int pdse_wavout_launch(const float* x, const int32_t* n_in_host, const int32_t* n_keep_host, const int32_t* n_in, const int32_t* n_keep,
                       const double* taps, uint8_t* out, int32_t* clipped, int64_t stride, int32_t B, int32_t Lmax, int32_t up,
                       int32_t down, int32_t half, int32_t fmt, int32_t width, int32_t ch, hipStream_t s) {
  REQ(x && n_in_host && n_keep_host && n_in && n_keep && out && clipped, "wav_encode: null pointer");
  REQ(B >= 1 && B <= 65535, "wav_encode: B < 1 (or above 65535)");
  REQ(up >= 1 && down >= 1 && half >= 0, "wav_encode: up < 1, down < 1 or half < 0");
  REQ(fmt == PDSE_WAV_INT || fmt == PDSE_WAV_FLOAT, "wav_encode: fmt must be PDSE_WAV_INT or PDSE_WAV_FLOAT");
  REQ(fmt != PDSE_WAV_INT || (width >= 2 && width <= 4), "wav_encode: fmt PDSE_WAV_INT takes a width of 2, 3 or 4 bytes");
  REQ(fmt != PDSE_WAV_FLOAT || width == 4, "wav_encode: fmt PDSE_WAV_FLOAT takes a width of 4 bytes");
  REQ(ch >= 1 && ch <= PDSE_WAV_MAX_CH, "wav_encode: ch must be 1 .. 8");
  REQ(Lmax >= 1, "wav_encode: Lmax < 1");
  const int64_t fb = (int64_t)ch * width;
  int64_t need = 1;
  for (int b = 0; b < B; ++b) {
    REQ(n_in_host[b] >= 1, "wav_encode: n_in < 1");
    REQ(n_in_host[b] <= Lmax, "wav_encode: n_in > Lmax");
    const int64_t n_out = ((int64_t)n_in_host[b] * up + down - 1) / down;
    REQ(n_keep_host[b] >= 0 && n_keep_host[b] <= n_out, "wav_encode: n_keep outside 0 .. ceil(n_in up / down)");
    if (n_keep_host[b] * fb > need) need = n_keep_host[b] * fb;
  }
  REQ(stride >= need, "wav_encode: stride below the bytes of the longest row (n_keep ch width)");
  REQ(up == down || taps, "wav_encode: null taps with up != down");
  const int jmax = half / up + 1;
  const int64_t win = ((int64_t)(WO_BLOCK - 1) * down) / up + 2 * (int64_t)jmax + 2;
  REQ(up == down || win * (int64_t)sizeof(float) + WO_IMAGE + 64 <= WO_LDS_MAX,
      "wav_encode: the input window of one block of frames does not fit the LDS budget (down / up or half too large)");
  const int64_t blocks = (stride + WO_BLOCK * fb - 1) / (WO_BLOCK * fb);
  REQ(blocks <= 0x7fffffff, "wav_encode: stride too large");
  if (fmt == PDSE_WAV_FLOAT) {
    launch<PDSE_WAV_FLOAT, 4>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  } else if (width == 2) {
    launch<PDSE_WAV_INT, 2>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  } else if (width == 3) {
    launch<PDSE_WAV_INT, 3>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  } else {
    launch<PDSE_WAV_INT, 4>(x, n_in, n_keep, taps, out, clipped, stride, B, Lmax, up, down, half, ch, jmax, (int)win, blocks, s);
  }
  return pdse_check_launch("wav_encode");
}
