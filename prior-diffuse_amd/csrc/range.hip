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
//
// PDSE_RANGE_NONFINITE (mode 2) is the finiteness verdict of a pass, not a histogram: bin 31 above counts every value from 2^15
// up together with Inf and NaN, so it cannot say whether a result is finite.  Row r of the table is an fp32 tensor (ptr, n; the
// other row fields are not read); out[r][0] grows by the number of its elements whose exponent field is all ones, found by an
// integer test on the bit pattern.  ptr is only 4-byte aligned: the elements up to the first 16-byte boundary and the n % 4
// behind the last whole vector are read one by one by workgroup 0, everything between with 16-byte loads, grid-stride.  A lane
// keeps its count in a register; the counts are summed within the wave by shuffles, across the workgroup's waves through LDS,
// and one thread adds the total with ONE atomicAdd - none when it is 0, so a clean pass does no atomics.  Bins 1 .. 31 are
// not written.  An integer count: independent of scheduling.
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

// mode 0: zero the n counters of a table
__global__ __launch_bounds__(RH_THREADS) void range_clear_kernel(uint32_t* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RH_THREADS + threadIdx.x;
  if (i < n) out[i] = 0u;
}

// 1 when the fp32 bit pattern is an infinity or a NaN (exponent field all ones), else 0
__device__ __forceinline__ unsigned nonfinite_f32(uint32_t u) { return (u & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

__global__ __launch_bounds__(RH_THREADS) void range_nonfinite_kernel(const pdse_range_desc d) {
  __shared__ unsigned part[RH_WAVES];
  const int row = (int)blockIdx.y;
  if (row >= d.out_rows) return;                                                   // uniform over the workgroup, like all returns below
  const pdse_range_row r = d.rows[row];
  // rows were validated when the op was recorded or launched directly; a table overwritten since then is skipped, never followed
  if (r.ptr == nullptr || r.n <= 0 || (reinterpret_cast<uintptr_t>(r.ptr) & 3u) != 0) return;
  const uint32_t* const p = static_cast<const uint32_t*>(r.ptr);
  const int tid = threadIdx.x;
  int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);   // 0 .. 3 elements before the boundary
  if (head > r.n) head = r.n;
  const int64_t nvec = (r.n - head) >> 2;
  const int tail = (int)((r.n - head) & 3);
  const int64_t first = (int64_t)blockIdx.x * RH_THREADS;
  const int64_t stride = (int64_t)gridDim.x * RH_THREADS;
  if (blockIdx.x != 0 && first >= nvec) return;

  unsigned c = 0;
  const uint4* const p4 = reinterpret_cast<const uint4*>(p + head);                // 16-byte aligned by the choice of head
  for (int64_t v = first + tid; v < nvec; v += stride) {
    const uint4 q = p4[v];
    c += nonfinite_f32(q.x) + nonfinite_f32(q.y) + nonfinite_f32(q.z) + nonfinite_f32(q.w);
  }
  if (blockIdx.x == 0) {   // the scalar ends: head on the first lanes of wave 0, tail on the first lanes of wave 1
    if (tid < (int)head) c += nonfinite_f32(p[tid]);
    if (tid >= 64 && tid - 64 < tail) c += nonfinite_f32(p[head + 4 * nvec + (tid - 64)]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
  if ((tid & 63) == 0) part[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < RH_WAVES; ++w) sum += part[w];
    if (sum) atomicAdd(d.out + (int64_t)row * RH_BINS, sum);
  }
}

}  // namespace

// the descriptor's own fields (no device access)
static int range_check_desc(const pdse_range_desc* d) {
  REQ(d && d->out, "range: null descriptor or output");
  REQ(d->mode == 0 || d->mode == 1 || d->mode == PDSE_RANGE_NONFINITE, "range: mode must be 0 (clear), 1 (accumulate) or 2 (non-finite count)");
  REQ(d->out_rows >= 1, "range: out_rows < 1");
  if (d->mode == 0) return 0;
  REQ(d->rows, "range: null row table");
  REQ(d->nrows >= 1 && d->nrows <= 65535, "range: zero rows (or more than 65535)");
  REQ(d->blocks >= 1 && d->blocks <= 65535, "range: blocks must be 1 .. 65535");
  if (d->mode == PDSE_RANGE_NONFINITE) REQ(d->nrows <= d->out_rows, "range: more rows than the output table has (non-finite count: row r adds to out[r][0])");
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
    if (d->mode == PDSE_RANGE_NONFINITE) {   // an fp32 tensor (ptr, n): nothing else of the row is read
      REQ(r.n >= 0, "range: n < 0");
      REQ((reinterpret_cast<uintptr_t>(r.ptr) & 3u) == 0, "range: fp32 tensor not aligned to 4 bytes");
      continue;
    }
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
  if (d->mode == 0) {   // clear: every counter of the table, no tensor is read
    // A kernel, not hipMemsetAsync: a memset node in a captured graph was seen to fill its table with other data once a second
    // graph that holds memset nodes had been launched in the process; kernel nodes replay as recorded.
    const int64_t n = (int64_t)d->out_rows * RH_BINS;
    hipLaunchKernelGGL(range_clear_kernel, dim3((unsigned)((n + RH_THREADS - 1) / RH_THREADS)), dim3(RH_THREADS), 0, s, d->out, n);
    return pdse_check_launch("range: clear");
  }
  if (d->mode == PDSE_RANGE_NONFINITE) {
    hipLaunchKernelGGL(range_nonfinite_kernel, dim3((unsigned)d->blocks, (unsigned)d->nrows), dim3(RH_THREADS), 0, s, *d);
    return pdse_check_launch("range");
  }
  hipLaunchKernelGGL(range_hist_kernel, dim3((unsigned)d->blocks, (unsigned)d->nrows), dim3(RH_THREADS), 0, s, *d);
  return pdse_check_launch("range");
}
