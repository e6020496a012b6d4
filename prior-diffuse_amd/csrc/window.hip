// Gather and scatter of the windowed passes (include/pdse.h: pdse_window_gather / pdse_window_scatter).  Plain
// arguments, no descriptor and no operator kind: the calls are additive within the ABI, like the ensemble statistics.
//
// Both tensors are fp32 [B][C][.][F] - the layout in which the networks read x_t, the condition and the feature and write eps and
// X_init - so frames [a, a + W) of one (b, c) plane are ONE contiguous run of W F floats in the whole-file tensor and the whole plane
// of the window tensor: either kernel is a copy of contiguous runs, one run per (b, c).  A workgroup walks its share of a run with
// consecutive lanes on consecutive floats, 256 bytes per wave and instruction, whole cache lines whatever a F is (F = 161 is odd: a
// run starts on a 4-byte boundary only, so 16-byte accesses would split lines at every odd a); WIN_UNROLL independent accesses per
// lane are in flight before the first store.  Nothing is reduced and nothing is converted: bit patterns arrive unchanged.
#include <hip/hip_runtime.h>

#include "pdse_internal.h"

#define REQ(cond, msg)     \
  if (!(cond)) {           \
    pdse_set_error(msg);   \
    return 1;              \
  }

constexpr int WIN_THREADS = 256;
constexpr int WIN_UNROLL = 4;
constexpr int WIN_MAX_BLOCKS = 1024;      // per (b, c) run: 4 K floats a workgroup and pass

// win[plane][i] = whole[plane][a F + i] where that lies inside the plane, else 0;  i < W F
__global__ __launch_bounds__(WIN_THREADS) void window_gather_kernel(const float* __restrict__ whole, float* __restrict__ win,
                                                                    const int64_t plane_whole, const int64_t plane_win,
                                                                    const int64_t shift) {
  const float* src = whole + (int64_t)blockIdx.y * plane_whole;
  float* dst = win + (int64_t)blockIdx.y * plane_win;
  const int64_t stride = (int64_t)gridDim.x * WIN_THREADS * WIN_UNROLL;
  for (int64_t base = (int64_t)blockIdx.x * WIN_THREADS * WIN_UNROLL + threadIdx.x; base < plane_win; base += stride) {
    float v[WIN_UNROLL];
#pragma unroll
    for (int k = 0; k < WIN_UNROLL; ++k) {
      const int64_t i = base + (int64_t)k * WIN_THREADS, g = i + shift;
      v[k] = (i < plane_win && g >= 0 && g < plane_whole) ? src[g] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < WIN_UNROLL; ++k) {
      const int64_t i = base + (int64_t)k * WIN_THREADS;
      if (i < plane_win) dst[i] = v[k];
    }
  }
}

// whole[plane][a F + i] = win[plane][i] for lo <= i < hi (the kept frames' floats; the caller has checked that they lie inside both)
__global__ __launch_bounds__(WIN_THREADS) void window_scatter_kernel(const float* __restrict__ win, float* __restrict__ whole,
                                                                     const int64_t plane_whole, const int64_t plane_win,
                                                                     const int64_t shift, const int64_t lo, const int64_t hi) {
  const float* src = win + (int64_t)blockIdx.y * plane_win;
  float* dst = whole + (int64_t)blockIdx.y * plane_whole + shift;
  const int64_t stride = (int64_t)gridDim.x * WIN_THREADS * WIN_UNROLL;
  for (int64_t base = lo + (int64_t)blockIdx.x * WIN_THREADS * WIN_UNROLL + threadIdx.x; base < hi; base += stride) {
    float v[WIN_UNROLL];
#pragma unroll
    for (int k = 0; k < WIN_UNROLL; ++k) {
      const int64_t i = base + (int64_t)k * WIN_THREADS;
      v[k] = i < hi ? src[i] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < WIN_UNROLL; ++k) {
      const int64_t i = base + (int64_t)k * WIN_THREADS;
      if (i < hi) dst[i] = v[k];
    }
  }
}

static int win_blocks(int64_t n) {
  const int64_t per = (int64_t)WIN_THREADS * WIN_UNROLL;
  const int64_t nb = (n + per - 1) / per;
  return (int)(nb < 1 ? 1 : nb > WIN_MAX_BLOCKS ? WIN_MAX_BLOCKS : nb);
}

static int win_sizes(const char* what, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W) {
  if (B < 1 || C < 1 || T < 1 || F < 1 || W < 1 || (int64_t)B * C > 65535) {
    pdse_set_error(what);
    return 1;
  }
  return 0;
}

int pdse_window_gather_launch(const float* whole, float* win, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t a,
                              hipStream_t s) {
  REQ(whole && win, "window_gather: null pointer");
  if (win_sizes("window_gather: bad sizes (B, C, T, F, W >= 1, B C <= 65535)", B, C, T, F, W)) return 1;
  REQ((int64_t)a + W > 0 && a < T, "window_gather: the window [a, a + W) holds no frame of [0, T)");
  const int64_t pw = (int64_t)T * F, pn = (int64_t)W * F;
  hipLaunchKernelGGL(window_gather_kernel, dim3(win_blocks(pn), B * C), dim3(WIN_THREADS), 0, s, whole, win, pw, pn, (int64_t)a * F);
  return pdse_check_launch("window_gather");
}

int pdse_window_scatter_launch(const float* win, float* whole, int32_t B, int32_t C, int32_t T, int32_t F, int32_t W, int32_t a,
                               int32_t keep_lo, int32_t keep_hi, hipStream_t s) {
  REQ(whole && win, "window_scatter: null pointer");
  if (win_sizes("window_scatter: bad sizes (B, C, T, F, W >= 1, B C <= 65535)", B, C, T, F, W)) return 1;
  const int64_t lo_min = a > 0 ? a : 0, hi_max = (int64_t)a + W < T ? (int64_t)a + W : T;
  REQ(lo_min <= keep_lo && keep_lo <= keep_hi && keep_hi <= hi_max,
      "window_scatter: kept frames outside max(a, 0) <= keep_lo <= keep_hi <= min(a + W, T)");
  if (keep_lo == keep_hi) return 0;
  const int64_t pw = (int64_t)T * F, pn = (int64_t)W * F;
  const int64_t lo = ((int64_t)keep_lo - a) * F, hi = ((int64_t)keep_hi - a) * F;
  hipLaunchKernelGGL(window_scatter_kernel, dim3(win_blocks(hi - lo), B * C), dim3(WIN_THREADS), 0, s, win, whole, pw, pn,
                     (int64_t)a * F, lo, hi);
  return pdse_check_launch("window_scatter");
}
