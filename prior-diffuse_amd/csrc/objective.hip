// objective.hip — the two memory-rate passes of the denoising objective (trainer/complex_ddpm_trainer.py:699-738) that neither the
// sampling path nor the validation epoch has: the forward noising of a whole batch at per-utterance diffusion steps, with the
// --sigma mask and its target, and the --sigma loss com_mse_sigma_loss (utils/loss.py:46-56).  Plain arguments, no descriptor and
// no operator kind, like csrc/valid.hip: the calls are additive within the ABI version and cannot be recorded in a plan.
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

// four consecutive floats at p, of which the first n (1 .. 4) exist; one 16-byte access where the address allows it (uniform over
// a workgroup: a quad starts a multiple of four floats behind its utterance).  F = 161 rows are not 16-byte aligned, so the
// kernels below index the flat planes.
__device__ __forceinline__ float4 ob_load(const float* p, const int n, const bool aligned) {
  if (n == 4 && aligned) return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[0];
  if (n > 1) v.y = p[1];
  if (n > 2) v.z = p[2];
  if (n > 3) v.w = p[3];
  return v;
}

__device__ __forceinline__ void ob_store(float* p, const float4 v, const int n, const bool aligned) {
  if (n == 4 && aligned) {
    *reinterpret_cast<float4*>(p) = v;
    return;
  }
  p[0] = v.x;
  if (n > 1) p[1] = v.y;
  if (n > 2) p[2] = v.z;
  if (n > 3) p[3] = v.w;
}

__device__ __forceinline__ bool ob_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// mask = |init| / max / 2 + 0.5 (:713-715), three separately rounded fp32 operations; x / 2 and x * 0.5 are the same value
__device__ __forceinline__ float ob_mask(const float in, const float mx) {
#pragma clang fp contract(off)
  float m = fabsf(in) / mx;
  m = m * 0.5f;
  return m + 0.5f;
}

// ---------------------------------------------------------------------------------------
// max |init| per (b, channel) plane, over the WHOLE padded plane as the reference takes it (torch.max over the flattened
// [T F] axis, :713-714).  |x| >= 0, so the float bit pattern orders like an unsigned integer: an integer atomicMax on the bits,
// whose result does not depend on the order of arrival.  maxbuf is zeroed on the stream ahead of the launch.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void objective_max_kernel(const float* __restrict__ init, float* __restrict__ maxbuf, const int64_t plane) {
  const int pl = blockIdx.y;
  const float* x = init + (int64_t)pl * plane;
  const bool al = ob_aligned(x);
  const int64_t quads = (plane + 3) >> 2;
  float m = 0.f;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q << 2;
    const int n = (int)min((int64_t)4, plane - i);
    const float4 v = ob_load(x + i, n, al);   // lanes that do not exist read as 0, which no maximum of magnitudes notices
    m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
  }
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_down(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<unsigned int*>(maxbuf) + pl, __float_as_uint(m));
}

// ---------------------------------------------------------------------------------------
// Forward noising (:709-733).  One workgroup column per utterance: a = sqrt(alpha_bar_t), s = sqrt(1 - alpha_bar_t) from the two
// tables at the utterance's own step t[b] - walked without a clamp, like the step embedding - and per element
//   SIGMA: target = noise * sqrt(mask)           (:717)     else target = noise
//   MODE 0 (pirorgrad): noisy = a * (label - init) + s * target            (:726)
//   MODE 1 (deltamu):   noisy = a * label + s * (target + init)            (:729)
//   MODE 2 (plain):     noisy = a * label + s * target                     (:732)
// every operation rounded to fp32 on its own, in the reference's order (nothing contracted into an fma).  An utterance's two
// channel planes are one flat run of 2 plane floats; a quad that straddles the channel boundary takes each element's own maximum.
// ---------------------------------------------------------------------------------------
template <int MODE, bool SIGMA>
__device__ __forceinline__ void ob_elem(const float lb, const float in, const float nz, const float a, const float s, const float mx,
                                        float& noisy, float& target) {
#pragma clang fp contract(off)
  float tg = nz;
  if (SIGMA) {
    const float root = sqrtf(ob_mask(in, mx));
    tg = nz * root;
  }
  float t1, t2;
  if (MODE == 0) {
    const float diff = lb - in;
    t1 = a * diff;
    t2 = s * tg;
  } else if (MODE == 1) {
    t1 = a * lb;
    const float ni = tg + in;
    t2 = s * ni;
  } else {
    t1 = a * lb;
    t2 = s * tg;
  }
  noisy = t1 + t2;
  target = tg;
}

template <int MODE, bool SIGMA>
__global__ __launch_bounds__(256) void objective_noise_kernel(const float* __restrict__ label, const float* __restrict__ init,
                                                              const float* __restrict__ noise, const int32_t* __restrict__ t,
                                                              const float* __restrict__ atab, const float* __restrict__ stab,
                                                              const float* __restrict__ maxbuf, float* __restrict__ noisy,
                                                              float* __restrict__ target, const int64_t plane) {
  const int b = blockIdx.y;
  const int32_t step = t[b];
  const float a = atab[step], s = stab[step];
  const float mx0 = SIGMA ? maxbuf[2 * b] : 1.f, mx1 = SIGMA ? maxbuf[2 * b + 1] : 1.f;
  const int64_t n2 = 2 * plane, off = (int64_t)b * n2;
  label += off, init += off, noise += off, noisy += off, target += off;
  const bool a_lb = ob_aligned(label), a_in = ob_aligned(init), a_nz = ob_aligned(noise), a_ny = ob_aligned(noisy), a_tg = ob_aligned(target);
  const int64_t quads = (n2 + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    const int64_t i = q << 2;
    const int n = (int)min((int64_t)4, n2 - i);
    const float4 lb = ob_load(label + i, n, a_lb), nz = ob_load(noise + i, n, a_nz);
    const float4 in = (MODE != 2 || SIGMA) ? ob_load(init + i, n, a_in) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 ny, tg;
    ob_elem<MODE, SIGMA>(lb.x, in.x, nz.x, a, s, i < plane ? mx0 : mx1, ny.x, tg.x);
    ob_elem<MODE, SIGMA>(lb.y, in.y, nz.y, a, s, i + 1 < plane ? mx0 : mx1, ny.y, tg.y);
    ob_elem<MODE, SIGMA>(lb.z, in.z, nz.z, a, s, i + 2 < plane ? mx0 : mx1, ny.z, tg.z);
    ob_elem<MODE, SIGMA>(lb.w, in.w, nz.w, a, s, i + 3 < plane ? mx0 : mx1, ny.w, tg.w);
    ob_store(noisy + i, ny, n, a_ny);
    ob_store(target + i, tg, n, a_tg);
  }
}

// workgroups of a launch over `quads` quads per row of `rows` rows: enough to give every CU a few, no more than there is work
static inline int ob_blocks(const int64_t quads, const int rows) {
  int64_t bx = (quads + 255) / 256;
  const int64_t cap = (4 * 256 + rows - 1) / rows;   // about four workgroups per CU over the whole grid
  if (bx > cap) bx = cap;
  return (int)(bx < 1 ? 1 : bx);
}

int pdse_objective_noise_launch(const float* label, const float* init, const float* noise, const int32_t* t, const float* a_tab,
                                const float* s_tab, float* noisy, float* target, float* maxbuf, int32_t B, int32_t T, int32_t F,
                                int32_t mode, int32_t sigma, hipStream_t s) {
  REQ(label && init && noise && t && a_tab && s_tab && noisy && target && maxbuf, "objective_noise: null pointer");
  REQ(B > 0 && B <= 32767 && T > 0 && F > 0, "objective_noise: bad sizes (0 < B <= 32767, T > 0, F > 0)");
  REQ(mode >= 0 && mode <= 2, "objective_noise: mode is 0 (pirorgrad), 1 (deltamu) or 2 (plain)");
  REQ(sigma == 0 || sigma == 1, "objective_noise: sigma is 0 or 1");
  const int64_t plane = (int64_t)T * F;
  if (pdse_check_hip(hipMemsetAsync(maxbuf, 0, sizeof(float) * 2 * B, s), "objective_noise memset")) return 1;
  if (sigma) {
    const dim3 g(ob_blocks((plane + 3) >> 2, 2 * B), 2 * B);
    hipLaunchKernelGGL(objective_max_kernel, g, dim3(256), 0, s, init, maxbuf, plane);
  }
  const dim3 grid(ob_blocks((2 * plane + 3) >> 2, B), B);
#define OB_LAUNCH(M, S) \
  hipLaunchKernelGGL((objective_noise_kernel<M, S>), grid, dim3(256), 0, s, label, init, noise, t, a_tab, s_tab, maxbuf, noisy, target, plane)
  switch (mode * 2 + sigma) {
    case 0: OB_LAUNCH(0, false); break;
    case 1: OB_LAUNCH(0, true); break;
    case 2: OB_LAUNCH(1, false); break;
    case 3: OB_LAUNCH(1, true); break;
    case 4: OB_LAUNCH(2, false); break;
    default: OB_LAUNCH(2, true); break;
  }
#undef OB_LAUNCH
  return pdse_check_launch("objective_noise");
}

// ---------------------------------------------------------------------------------------
// com_mse_sigma_loss (utils/loss.py:46-56) over the frames t < frames[b]: per element d = predicted - target and the term
// (((d m) / mask) d) m of :55 with m = 1 inside the live frames - d m and the trailing m are exact, so the term is (d / mask) d,
// two fp32 roundings behind the subtraction - and mask recomputed from init and maxbuf as the noising formed it.  The fp32 terms
// are widened to double and added in a fixed order: a thread its own quads ascending, the re plane before the im plane; a
// workgroup through a shuffle tree and four LDS slots; PDSE_SPECLOSS_BLOCKS workgroups per utterance leave partials and one
// workgroup adds them in index order (the scheme of speclosses_partial_kernel / speclosses_final_kernel, csrc/valid.hip).
// Nothing is added atomically.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double ob_block_sum(double v, double* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) r = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  return r;   // valid on thread 0
}

__device__ __forceinline__ void ob_term(const float p, const float tg, const float in, const float mx, double& acc) {
#pragma clang fp contract(off)
  const float d = p - tg;
  const float q = d / ob_mask(in, mx);
  const float term = q * d;
  acc += (double)term;
}

__global__ __launch_bounds__(256) void sigmaloss_partial_kernel(const float* __restrict__ predicted, const float* __restrict__ target,
                                                                const float* __restrict__ init, const float* __restrict__ maxbuf,
                                                                const int32_t* __restrict__ frames, double* __restrict__ partial,
                                                                const int T, const int F) {
  __shared__ double lds[4];
  const int b = blockIdx.y;
  const int fr = min(max(frames[b], 0), T);
  const int64_t plane = (int64_t)T * F, live = (int64_t)fr * F;
  const int64_t quads = (live + 3) >> 2;
  double acc = 0.0;
  for (int ch = 0; ch < 2; ++ch) {
    const int64_t off = ((int64_t)b * 2 + ch) * plane;
    const float* pp = predicted + off;
    const float* tp = target + off;
    const float* ip = init + off;
    const bool a_p = ob_aligned(pp), a_t = ob_aligned(tp), a_i = ob_aligned(ip);
    const float mx = maxbuf[2 * b + ch];
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)PDSE_SPECLOSS_BLOCKS * 256) {
      const int64_t i = q << 2;
      const int n = (int)min((int64_t)4, live - i);
      const float4 p = ob_load(pp + i, n, a_p), tg = ob_load(tp + i, n, a_t), in = ob_load(ip + i, n, a_i);
      ob_term(p.x, tg.x, in.x, mx, acc);
      if (n > 1) ob_term(p.y, tg.y, in.y, mx, acc);
      if (n > 2) ob_term(p.z, tg.z, in.z, mx, acc);
      if (n > 3) ob_term(p.w, tg.w, in.w, mx, acc);
    }
  }
  const double tot = ob_block_sum(acc, lds);
  if (threadIdx.x == 0) partial[(int64_t)b * PDSE_SPECLOSS_BLOCKS + blockIdx.x] = tot;
}

__global__ __launch_bounds__(256) void sigmaloss_final_kernel(const int32_t* __restrict__ frames, const double* __restrict__ partial,
                                                              double* __restrict__ per_utt, float* __restrict__ loss, const int B,
                                                              const int T, const int F) {
  for (int b = threadIdx.x; b < B; b += 256) {   // the numerator of utterance b: its partials in workgroup order
    double s = 0.0;
    for (int j = 0; j < PDSE_SPECLOSS_BLOCKS; ++j) s += partial[(int64_t)b * PDSE_SPECLOSS_BLOCKS + j];
    per_utt[b] = s;
  }
  __syncthreads();   // the workgroup's own global stores are visible to it behind the barrier
  if (threadIdx.x == 0) {
    double num = 0.0, fsum = 0.0;
    for (int b = 0; b < B; ++b) {   // utterances in batch order
      num += per_utt[b];
      fsum += (double)min(max(frames[b], 0), T);
    }
    loss[0] = (float)(num / (2.0 * (double)F * fsum));
  }
}

int pdse_sigma_loss_launch(const float* predicted, const float* target, const float* init, const float* maxbuf,
                           const int32_t* frames_host, const int32_t* frames, double* partial, double* per_utt, float* loss, int32_t B,
                           int32_t T, int32_t F, hipStream_t s) {
  REQ(predicted && target && init && maxbuf && frames_host && frames && partial && per_utt && loss, "sigma_loss: null pointer");
  REQ(B > 0 && B <= 32767 && T > 0 && F > 0, "sigma_loss: bad sizes (0 < B <= 32767, T > 0, F > 0)");
  int64_t total = 0;
  for (int b = 0; b < B; ++b) {
    REQ(frames_host[b] >= 0 && frames_host[b] <= T, "sigma_loss: frames outside [0, T]");
    total += frames_host[b];
  }
  REQ(total > 0, "sigma_loss: no frame in the batch (the sum of frames is 0: the loss has no denominator)");
  hipLaunchKernelGGL(sigmaloss_partial_kernel, dim3(PDSE_SPECLOSS_BLOCKS, B), dim3(256), 0, s, predicted, target, init, maxbuf, frames,
                     partial, T, F);
  hipLaunchKernelGGL(sigmaloss_final_kernel, dim3(1), dim3(256), 0, s, frames, partial, per_utt, loss, B, T, F);
  return pdse_check_launch("sigma_loss");
}
