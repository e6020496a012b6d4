// range.hip — the range audit of the f16x2 window: per-tensor histograms of the fp16 binade of |x| * 2^e, for a table of
// tensors in one launch (include/pdse.h: pdse_range_desc, PDSE_OP_RANGE).
//
// The bin map (PDSE_RANGE_BINS = 32 counters per tensor; prior-diffuse_amd/_lib.py exports it as RANGE_BINADE):
//   bin 0        x == 0 (either sign)
//   bin 1        0 < |x| 2^e < 2^-14                  (hi would be an fp16 subnormal)
//   bin E + 16   2^E <= |x| 2^e < 2^(E+1), E = -14 .. 14  (bins 2 .. 30: one bin per normal fp16 binade, nothing is merged)
//   bin 31       |x| 2^e >= 2^15, infinities and NaN
// PDSE_RANGE_F32 rows bin by the fp32 exponent field plus e (integer arithmetic: no multiply that could round or overflow;
// an fp32 subnormal lands in bin 1), PDSE_RANGE_F16HI rows by the exponent field of the stored hi plane (e = 0: the planes
// are scaled already; lo is never read).  An F16HI row walks the logical box n0 x n1 x n2 x n3 of 8-element vectors of the
// hi plane only, so margins, pad frames, the lo plane and the kernels' dump item are not counted.
//
// Why replicated LDS sub-histograms: real tensors put nearly all their mass in three or four binades, so one histogram per
// workgroup would serialise every ds_add of a wave on three or four addresses.  Here every wave owns RH_COPIES = 8 copies
// of the 32 counters and lane l adds to copy l & 7; the copies of one bin are adjacent words (eight different banks), so a
// wave whose 64 lanes hit ONE bin is spread over eight addresses in eight banks - 8 lanes deep instead of 64 - and waves
// never contend with each other.  4 waves x 8 copies x 32 bins x 4 B = 4 KB of LDS.  (Counting the hot bins with wave
// ballots costs one scalar round per distinct binade and element slot, which is slower than this for the spread-out
// tensors and no faster for the concentrated ones.)  A workgroup folds its 32 copies at the end and adds the non-zero totals
// to global memory with atomicAdd on unsigned: integer counts, so the result does not depend on the order.
// Streaming side: 16-byte loads (four fp32 or eight fp16 per lane), grid-stride over the row, a scalar tail for n % 4.
// No scratch, no inline assembly.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

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

constexpr int RH_THREADS = 256;
constexpr int RH_WAVES = RH_THREADS / 64;
constexpr int RH_COPIES = 8;
constexpr int RH_BINS = PDSE_RANGE_BINS;

// bin of an fp32 bit pattern scaled by 2^e
__device__ __forceinline__ int bin_f32(uint32_t u, int e) {
  const uint32_t a = u & 0x7fffffffu;
  if (a == 0u) return 0;
  const int be = (int)(a >> 23);
  if (be == 255) return 31;
  if (be == 0) return 1;               // fp32 subnormal: below 2^-126, far under 2^-14 for every accepted e
  const int E = be - 127 + e;
  return E < -14 ? 1 : (E > 14 ? 31 : E + 16);
}

// bin of an fp16 bit pattern (the hi plane as stored)
__device__ __forceinline__ int bin_f16(uint32_t h) {
  const uint32_t a = h & 0x7fffu;
  if (a == 0u) return 0;
  const int he = (int)(a >> 10);       // 0: subnormal, 1 .. 30: E = he - 15, 31: inf / NaN
  return he == 0 ? 1 : (he >= 30 ? 31 : he + 1);
}

__global__ __launch_bounds__(RH_THREADS) void range_hist_kernel(const pdse_range_desc d) {
  __shared__ unsigned hist[RH_WAVES][RH_BINS][RH_COPIES];
  const pdse_range_row r = d.rows[blockIdx.y];
  // rows were validated when the op was recorded or launched directly; a table overwritten since then is skipped, never followed
  if (r.ptr == nullptr || r.out_row < 0 || r.out_row >= d.out_rows || r.n < 0) return;
  const int tid = threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * RH_THREADS;
  const int64_t stride = (int64_t)gridDim.x * RH_THREADS;
  int64_t nvec;
  if (r.kind == PDSE_RANGE_F32) {
    nvec = r.n >> 2;
  } else if (r.kind == PDSE_RANGE_F16HI) {
    if (r.n0 < 1 || r.n1 < 1 || r.n2 < 1 || r.n3 < 1) return;
    nvec = (int64_t)r.n0 * r.n1 * r.n2 * r.n3;
    if (nvec > 0x7fffffff) return;
  } else {
    return;
  }
  if (first >= nvec && !(blockIdx.x == 0 && r.kind == PDSE_RANGE_F32 && (r.n & 3))) return;   // uniform over the workgroup

  for (int i = tid; i < RH_WAVES * RH_BINS * RH_COPIES; i += RH_THREADS) (&hist[0][0][0])[i] = 0u;
  __syncthreads();
  unsigned* const my = &hist[tid >> 6][0][tid & (RH_COPIES - 1)];   // counter of bin b: my[b * RH_COPIES]

  if (r.kind == PDSE_RANGE_F32) {
    const uint32_t* const p = static_cast<const uint32_t*>(r.ptr);
    const int e = r.exp;
    if ((reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
      const uint4* const p4 = reinterpret_cast<const uint4*>(p);
      for (int64_t v = first + tid; v < nvec; v += stride) {
        const uint4 q = p4[v];
        atomicAdd(my + bin_f32(q.x, e) * RH_COPIES, 1u);
        atomicAdd(my + bin_f32(q.y, e) * RH_COPIES, 1u);
        atomicAdd(my + bin_f32(q.z, e) * RH_COPIES, 1u);
        atomicAdd(my + bin_f32(q.w, e) * RH_COPIES, 1u);
      }
    } else {   // a view that does not start on 16 bytes: the same elements, one at a time
      for (int64_t v = first + tid; v < nvec; v += stride)
        for (int j = 0; j < 4; ++j) atomicAdd(my + bin_f32(p[4 * v + j], e) * RH_COPIES, 1u);
    }
    if (blockIdx.x == 0 && tid < (int)(r.n & 3)) atomicAdd(my + bin_f32(p[4 * nvec + tid], e) * RH_COPIES, 1u);
  } else {
    const uint16_t* const p = static_cast<const uint16_t*>(r.ptr);
    const uint32_t n1 = (uint32_t)r.n1, n2 = (uint32_t)r.n2, n3 = (uint32_t)r.n3;
    for (int64_t v = first + tid; v < nvec; v += stride) {
      uint32_t t = (uint32_t)v;
      const uint32_t i3 = t % n3;
      t /= n3;
      const uint32_t i2 = t % n2;
      t /= n2;
      const uint32_t i1 = t % n1;
      const uint32_t i0 = t / n1;
      const uint32_t i = i3 + (uint32_t)r.i0;
      const uint32_t pos = r.par_half ? (i & 1u) * (uint32_t)r.par_half + (i >> 1) : i;
      const uint4 q = *reinterpret_cast<const uint4*>(p + (int64_t)i0 * r.s0 + (int64_t)i1 * r.s1 + (int64_t)i2 * r.s2 + (int64_t)pos * 8);
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        atomicAdd(my + bin_f16(w[j] & 0xffffu) * RH_COPIES, 1u);
        atomicAdd(my + bin_f16(w[j] >> 16) * RH_COPIES, 1u);
      }
    }
  }
  __syncthreads();
  if (tid < RH_BINS) {
    unsigned sum = 0;
    for (int w = 0; w < RH_WAVES; ++w)
      for (int c = 0; c < RH_COPIES; ++c) sum += hist[w][tid][c];
    if (sum) atomicAdd(d.out + (int64_t)r.out_row * RH_BINS + tid, sum);
  }
}

}  // namespace

// the descriptor's own fields (no device access)
static int range_check_desc(const pdse_range_desc* d) {
  REQ(d && d->out, "range: null descriptor or output");
  REQ(d->mode == 0 || d->mode == 1, "range: mode must be 0 (clear) or 1 (accumulate)");
  REQ(d->out_rows >= 1, "range: out_rows < 1");
  if (d->mode == 0) return 0;
  REQ(d->rows, "range: null row table");
  REQ(d->nrows >= 1 && d->nrows <= 65535, "range: zero rows (or more than 65535)");
  REQ(d->blocks >= 1 && d->blocks <= 65535, "range: blocks must be 1 .. 65535");
  return 0;
}

// Reads the row table back (synchronous) and checks every row: called once per direct launch and once when a plan records the op.
int pdse_range_validate(const pdse_range_desc* d) {
  if (range_check_desc(d)) return 1;
  if (d->mode == 0) return 0;
  std::vector<pdse_range_row> rows((size_t)d->nrows);
  if (pdse_check_hip(hipMemcpy(rows.data(), d->rows, rows.size() * sizeof(pdse_range_row), hipMemcpyDeviceToHost), "range: reading the row table")) return 1;
  for (const pdse_range_row& r : rows) {
    REQ(r.ptr, "range: null tensor pointer in a row");
    REQ(r.kind == PDSE_RANGE_F32 || r.kind == PDSE_RANGE_F16HI, "range: unknown element kind");
    REQ(r.n >= 0, "range: n < 0");
    REQ(r.out_row >= 0 && r.out_row < d->out_rows, "range: out_row outside the output table");
    REQ(r.exp >= -64 && r.exp <= 64, "range: exponent outside -64 .. 64");
    if (r.kind == PDSE_RANGE_F32) {
      REQ((reinterpret_cast<uintptr_t>(r.ptr) & 3u) == 0, "range: fp32 tensor not aligned to 4 bytes");
    } else {
      REQ(r.exp == 0, "range: hi planes are scaled already (exp must be 0)");
      REQ(r.n0 >= 1 && r.n1 >= 1 && r.n2 >= 1 && r.n3 >= 1, "range: empty layout");
      const int64_t nv = (int64_t)r.n0 * r.n1 * r.n2 * r.n3;
      REQ(nv <= 0x7fffffff && r.n == 8 * nv, "range: n does not match the layout (or more than 2^31 vectors)");
      REQ(r.s0 >= 0 && r.s1 >= 0 && r.s2 >= 0 && ((r.s0 | r.s1 | r.s2) & 7) == 0 && (reinterpret_cast<uintptr_t>(r.ptr) & 15u) == 0,
          "range: hi-plane vectors must be 16-byte aligned (pointer and strides)");
      REQ(r.i0 >= 0 && r.par_half >= 0, "range: negative bin offset or parity split");
    }
  }
  return 0;
}

int pdse_range_launch(const pdse_range_desc* d, hipStream_t s) {
  if (range_check_desc(d)) return 1;
  if (d->mode == 0)   // clear: every counter of the table, no tensor is read
    return pdse_check_hip(hipMemsetAsync(d->out, 0, (size_t)d->out_rows * RH_BINS * sizeof(uint32_t), s), "range: clear");
  hipLaunchKernelGGL(range_hist_kernel, dim3((unsigned)d->blocks, (unsigned)d->nrows), dim3(RH_THREADS), 0, s, *d);
  return pdse_check_launch("range");
}
