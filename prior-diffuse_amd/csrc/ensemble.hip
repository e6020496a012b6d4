// ensemble.hip — statistics of a posterior ensemble: K reverse trajectories of the same B utterances, member-major
// [K][B][2][T][F], reduced to their mean, a per-bin spread map and the sums behind the relative spread and the medoid
// (include/pdse.h: pdse_ensemble_stats).  Plain arguments, no descriptor and no operator kind: the call is additive within the
// ABI version and cannot be recorded in a plan.
//
// Memory-bound: K n floats are read once, 1.5 n written (n = B 2 T F).  A thread owns NP (t, f) positions of one utterance - four
// up to K = 8, two above - and takes the re plane, then the im plane: the K values of its positions of a plane sit in registers
// for both passes over them (the mean, then the deviations), NP K floats at a time - 32 - beside K + 2 double accumulators.  K is
// a template parameter (a switch in the launcher): with K as a run-time bound the value array is indexed dynamically and goes to
// scratch.  VEC: the NP positions are consecutive and every plane is read with one 16- or 8-byte load - possible only where
// every plane starts on such a boundary, i.e. T F is a multiple of NP (F = 161 is odd: T is) and the bases are aligned; the
// launcher decides from the pointer values.  Otherwise the positions are 256 apart and a wave's loads are consecutive dwords.
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

#define ENS_THREADS 256

template <int NP>
struct ens_vec_of;
template <>
struct ens_vec_of<4> {
  typedef float4 type;
};
template <>
struct ens_vec_of<2> {
  typedef float2 type;
};
template <int NP>
using ens_vec = typename ens_vec_of<NP>::type;

// NP doubles rounded to fp32 once and stored at the thread's positions: one 16- or 8-byte store where VEC allows it
template <int NP, bool VEC>
__device__ __forceinline__ void ens_store(float* __restrict__ dst, const int64_t (&pos)[NP], const bool (&in)[NP], const double (&x)[NP]) {
  alignas(16) float f[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) f[j] = (float)x[j];
  if (VEC) {
    if (in[0]) *reinterpret_cast<ens_vec<NP>*>(dst + pos[0]) = *reinterpret_cast<const ens_vec<NP>*>(f);
  } else {
#pragma unroll
    for (int j = 0; j < NP; ++j)
      if (in[j]) dst[pos[j]] = f[j];
  }
}

// One plane (re or im) of the thread's NP positions: mean in double (members added in order k = 0 .. K-1, one division),
// rounded to fp32 once and stored; squared deviations from the double mean added to the positions' sums (dev) and, for live
// positions, to the utterance's sums.
template <int K, int NP, bool VEC>
__device__ __forceinline__ void ens_plane(const float* __restrict__ src, const int64_t kstride, float* __restrict__ mean,
                                          const int64_t (&pos)[NP], const bool (&in)[NP], const bool (&live)[NP], double (&dev)[NP],
                                          double& s_dev, double& s_mean, double (&s_mem)[K]) {
#pragma clang fp contract(off)
  alignas(16) float v[K][NP];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float* p = src + (int64_t)k * kstride;
    if (VEC) {   // the plane is a multiple of NP long: the NP positions are inside it together
      ens_vec<NP> q = {};
      if (in[0]) q = *reinterpret_cast<const ens_vec<NP>*>(p + pos[0]);
      *reinterpret_cast<ens_vec<NP>*>(v[k]) = q;
    } else {
#pragma unroll
      for (int j = 0; j < NP; ++j) v[k][j] = in[j] ? p[pos[j]] : 0.f;
    }
  }
  double m[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) s += (double)v[k][j];
    m[j] = s / (double)K;
    if (live[j]) s_mean += m[j] * m[j];
  }
  ens_store<NP, VEC>(mean, pos, in, m);
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      // an empty statement the compiler cannot see through: the values are widened again here, not kept as NP K doubles from
      // the mean's pass
      asm volatile("" : "+v"(v[k][j]));
      const double d = (double)v[k][j] - m[j];
      const double q = d * d;
      dev[j] += q;
      if (live[j]) {
        s_dev += q;
        s_mem[k] += q;
      }
    }
  }
}

template <int K, int NP, bool VEC>
__global__ __launch_bounds__(ENS_THREADS) void ensemble_partial_kernel(const float* __restrict__ members, float* __restrict__ mean,
                                                                       float* __restrict__ spread, const int32_t* __restrict__ frames,
                                                                       double* __restrict__ partial, const int B, const int T,
                                                                       const int F) {
  __shared__ double lds[ENS_THREADS / 64][K + 2];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t plane = (int64_t)T * F;
  const int64_t nlive = (int64_t)min(max(frames[b], 0), T) * F;
  const int64_t kstride = (int64_t)B * 2 * plane;   // member k + 1 behind member k
  const float* src = members + (int64_t)b * 2 * plane;
  float* mout = mean + (int64_t)b * 2 * plane;
  float* sout = spread + (int64_t)b * plane;
  double s_dev = 0.0, s_mean = 0.0, s_mem[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s_mem[k] = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * (NP * ENS_THREADS); base < plane; base += (int64_t)PDSE_ENSEMBLE_BLOCKS * (NP * ENS_THREADS)) {
    int64_t pos[NP];
    bool in[NP], live[NP];
    double dev[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      pos[j] = VEC ? base + NP * tid + j : base + j * ENS_THREADS + tid;
      in[j] = pos[j] < plane;
      live[j] = pos[j] < nlive;
      dev[j] = 0.0;
    }
    ens_plane<K, NP, VEC>(src, kstride, mout, pos, in, live, dev, s_dev, s_mean, s_mem);
    __builtin_amdgcn_sched_barrier(0);   // the im plane's loads stay behind the re plane's arithmetic: one plane's values in registers at a time
    ens_plane<K, NP, VEC>(src + plane, kstride, mout + plane, pos, in, live, dev, s_dev, s_mean, s_mem);
    double sp[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) sp[j] = K > 1 ? sqrt(dev[j] / (double)(K > 1 ? K - 1 : 1)) : 0.0;
    ens_store<NP, VEC>(sout, pos, in, sp);
  }
  // the workgroup's K + 2 sums: a shuffle tree per wave, the four waves in index order
  double mine[K + 2];
  mine[0] = s_dev;
  mine[1] = s_mean;
#pragma unroll
  for (int k = 0; k < K; ++k) mine[2 + k] = s_mem[k];
#pragma unroll
  for (int i = 0; i < K + 2; ++i) {
    double v = mine[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((tid & 63) == 0) lds[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < K + 2) {
    double* o = partial + ((int64_t)b * PDSE_ENSEMBLE_BLOCKS + blockIdx.x) * (K + 2);
    o[tid] = ((lds[0][tid] + lds[1][tid]) + lds[2][tid]) + lds[3][tid];
  }
}

// sum j of utterance b: one thread adds the utterance's partials in workgroup order
__global__ __launch_bounds__(ENS_THREADS) void ensemble_final_kernel(const double* __restrict__ partial, double* __restrict__ per_utt,
                                                                     double* __restrict__ per_member, const int K, const int B) {
  const int idx = blockIdx.x * ENS_THREADS + threadIdx.x;
  if (idx >= B * (K + 2)) return;
  const int b = idx / (K + 2), j = idx - b * (K + 2);
  double s = 0.0;
  for (int w = 0; w < PDSE_ENSEMBLE_BLOCKS; ++w) s += partial[((int64_t)b * PDSE_ENSEMBLE_BLOCKS + w) * (K + 2) + j];
  if (j < 2)
    per_utt[2 * b + j] = s;
  else
    per_member[(int64_t)(j - 2) * B + b] = s;
}

template <int K>
static void ens_launch(const float* members, float* mean, float* spread, const int32_t* frames, double* partial, int B, int T, int F,
                       hipStream_t s) {
  const dim3 grid(PDSE_ENSEMBLE_BLOCKS, B), block(ENS_THREADS);
  constexpr int NP = K > 8 ? 2 : 4;   // positions per thread: NP K values of a plane in registers (the compiler's figures)
  // NP x 4-byte accesses: every plane of the three tensors starts on such a boundary
  const bool vec = ((int64_t)T * F) % NP == 0 && (((uintptr_t)members | (uintptr_t)mean | (uintptr_t)spread) & (4 * NP - 1)) == 0;
  if (vec)
    hipLaunchKernelGGL((ensemble_partial_kernel<K, NP, true>), grid, block, 0, s, members, mean, spread, frames, partial, B, T, F);
  else
    hipLaunchKernelGGL((ensemble_partial_kernel<K, NP, false>), grid, block, 0, s, members, mean, spread, frames, partial, B, T, F);
}

int pdse_ensemble_stats_launch(const float* members, float* mean, float* spread, const int32_t* frames_host, const int32_t* frames,
                               double* partial, double* per_utt, double* per_member, int32_t K, int32_t B, int32_t T, int32_t F,
                               hipStream_t s) {
  REQ(members && mean && spread && frames_host && frames && partial && per_utt && per_member, "ensemble_stats: null pointer");
  REQ(K >= 1 && K <= PDSE_ENSEMBLE_MAX, "ensemble_stats: K outside [1, 16] (a thread holds its K values in registers)");
  REQ(B >= 1 && B <= 65535, "ensemble_stats: B outside [1, 65535]");
  REQ(T >= 1 && F >= 1, "ensemble_stats: bad sizes (T >= 1, F >= 1)");
  for (int b = 0; b < B; ++b) REQ(frames_host[b] >= 0 && frames_host[b] <= T, "ensemble_stats: frames outside [0, T]");
  switch (K) {
#define ENS_CASE(k) \
  case k: ens_launch<k>(members, mean, spread, frames, partial, B, T, F, s); break;
    ENS_CASE(1) ENS_CASE(2) ENS_CASE(3) ENS_CASE(4) ENS_CASE(5) ENS_CASE(6) ENS_CASE(7) ENS_CASE(8)
    ENS_CASE(9) ENS_CASE(10) ENS_CASE(11) ENS_CASE(12) ENS_CASE(13) ENS_CASE(14) ENS_CASE(15) ENS_CASE(16)
#undef ENS_CASE
  }
  const int sums = B * (K + 2);
  hipLaunchKernelGGL(ensemble_final_kernel, dim3((sums + ENS_THREADS - 1) / ENS_THREADS), dim3(ENS_THREADS), 0, s, partial, per_utt,
                     per_member, K, B);
  return pdse_check_launch("ensemble_stats");
}
