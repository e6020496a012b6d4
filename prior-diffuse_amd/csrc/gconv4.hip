// gconv4.hip — the GEMM-shaped gather convolutions (korder 3) on the bf16 matrix cores with exact three-way bf16
// operand splits: GCRN's gated (transposed) convolutions and LSTM input projection, DB-AIAT's dilated dense blocks.
// Same descriptors, same fp32 tensors in HBM and the same LINEAR / GLU epilogues as gconv2.hip (gconv_common.h); only
// the contraction changes (arithmetic: see gconv3.hip / packing.split_bf16x3 - six bf16 products per fp32
// multiply-add, fp32 accumulation, fp32-level accuracy at 16/6 of the fp32 MFMA rate).
//
// Unlike the eps-net blocks (gconv3.hip: K <= 192, all weights of a launch in one LDS image) these layers have K up to
// 1024 and up to 2 x 256 output channels, i.e. up to 1.5 MB of split weights: a GEMM main loop.
//   * workgroup = 8 waves = 8 tiles of 32 positions of one batch item x MT channel tiles (x 2 branches for GLU);
//   * K is walked in chunks of G4_CH 16-channel blocks of one (source, tap); the chunk's A fragments
//     ([block][branch][tile][3 planes][64 lanes] uint4) are streamed into a double-buffered LDS ring by LDS-DMA
//     (global_load_lds_dwordx4) while the previous chunk is multiplied; one barrier per chunk;
//   * B operand: lane (position, half h) gathers channels 16 cb + 8h .. +7 of its position (eight 4-byte loads per block,
//     scalar channel base + 32-bit lane offset), ELU-on-load for GCRN's skip source, exact split in registers; the next
//     chunk's requests are issued before the current chunk's matrix work;
//   * every (branch, tile) accumulator of the wave reuses the split B operand: 6 x branches x MT MFMAs per block.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pdse.h"
#include "pdse_internal.h"

#include "gconv_common.h"

// 16-channel K blocks per LDS chunk.  The ring (2 buffers x G4_CH x fragments x 3 KB) decides how many workgroups share
// a CU: with 4 blocks the four-fragment launches (GLU with two channel tiles, LINEAR with four) need 96 KB, i.e. ONE
// workgroup = 8 waves per CU although their registers allow two; 3 blocks = 72 KB lets two workgroups cover each
// other's chunk barriers and epilogues.
#ifndef G4_CH
#define G4_CH 3
#endif

// One gathered activation: global_load_dword (scalar base + 32-bit lane offset) written as inline asm.  While an LDS-DMA is
// in flight hipcc puts s_waitcnt vmcnt(0) in front of the first use of ANY compiler-visible load result
// (cdna_hip_programming.md §5, "Pipelining across barriers"), which made every K block wait for the next chunk's DMA and
// gather.  The compiler does not see these loads; what orders them is the chunk barrier: a chunk's values are requested
// one barrier before they are used, and __syncthreads() drains vmcnt (the DMA is compiler-visible) before it releases.
__device__ __forceinline__ float g4_load(const float* sbase, const unsigned byte_off) {
  float v;
  asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(byte_off), "s"(sbase) : "memory");
  return v;
}
// channel-blocked sources (pdse_src.blk = 8): the lane's eight channels of a K block are 32 contiguous bytes
typedef float g4_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ g4_f32x4 g4_load16(const float* sbase, const unsigned byte_off) {
  g4_f32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(v) : "v"(byte_off), "s"(sbase) : "memory");
  return v;
}
// The gathered values of one chunk.  A load written as inline asm returns before its data: between the request and the
// chunk barrier NOTHING may touch the destination registers - not even a copy - so every load writes the registers the
// values are read from later: scalars for plain sources, whole 16-byte vectors for channel-blocked ones (extracting the
// elements of a vector right behind its load made hipcc copy them at once, i.e. before they had landed, and re-use the
// vector's registers while the load was still in flight).
template <bool BLK>
struct g4_raw {
  float v[G4_CH][8];
  __device__ __forceinline__ float get(const int i, const int e) const { return v[i][e]; }
};
template <>
struct g4_raw<true> {
  g4_f32x4 v[G4_CH][2];
  __device__ __forceinline__ float get(const int i, const int e) const { return v[i][e >> 2][e & 3]; }
};
// no instruction: pins the point after which the values may be read (register-only uses could otherwise be scheduled above
// the barrier that makes them valid)
__device__ __forceinline__ void g4_landed(g4_raw<false>& raw) {
#pragma unroll
  for (int i = 0; i < G4_CH; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) asm volatile("" : "+v"(raw.v[i][e]));
}
__device__ __forceinline__ void g4_landed(g4_raw<true>& raw) {
#pragma unroll
  for (int i = 0; i < G4_CH; ++i)
#pragma unroll
    for (int e = 0; e < 2; ++e) asm volatile("" : "+v"(raw.v[i][e]));
}

// A fragments are read from the ring with ds_read_b128 written as inline asm too: the compiler cannot tell the ring
// buffer being read from the one an LDS-DMA in flight is filling, and put s_waitcnt vmcnt(0) in front of every K
// block's ring reads - each chunk then waited for the NEXT chunk's DMA and gathers before its first MFMA.  The chunk
// barrier orders the DMA of a buffer before its reads; the wait below orders the reads before their use.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // a register quad the inline asm can name (uint4 is a struct)
// the NP planes of one fragment (NP = 3: exact three-way split; NP = 1: plain bf16, the opt-in bf16 mode - korder 4)
__device__ __forceinline__ void g4_lds_read3(const unsigned addr, u32x4 (&a)[3]) {
  asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:1024\n\tds_read_b128 %2, %3 offset:2048"
               : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2])
               : "v"(addr)
               : "memory");
}
__device__ __forceinline__ void g4_lds_read3(const unsigned addr, u32x4 (&a)[2]) {   // f16x2: hi and lo planes
  asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024" : "=&v"(a[0]), "=&v"(a[1]) : "v"(addr) : "memory");
}
__device__ __forceinline__ void g4_lds_read3(const unsigned addr, u32x4 (&a)[1]) {
  asm volatile("ds_read_b128 %0, %1" : "=&v"(a[0]) : "v"(addr) : "memory");
}
template <int N, int NP>
__device__ __forceinline__ void g4_lds_wait(u32x4 (&a)[N][NP]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int p = 0; p < NP; ++p) asm volatile("" : "+v"(a[i][p]));
}
// planes.h: plane_mma on A fragments held as the register quads above
template <int NP>
__device__ __forceinline__ f32x16 g4_mma(const u32x4 (&a)[NP], const uint4 (&b)[NP], f32x16 acc) {
  uint4 a4[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) a4[p] = make_uint4(a[p][0], a[p][1], a[p][2], a[p][3]);
  return plane_mma<NP>(a4, b, acc);
}

struct g4_chunk {
  int s, tap, cb0, n, kb0;   // source, tap, first 16-channel block, blocks in the chunk, first K block in the packed weights
};

__device__ long long* g_trace4 = nullptr;   // PDSE_G4_TRACE=1 (diagnostic): [workgroup][wave][8] clock sums

// BLK: every source is channel-blocked (pdse_src.blk = 8) / none is
template <int EPI, int MT, bool BLK, int NP = 3>
__global__ __launch_bounds__(512, 2) void gconv4_kernel(const pdse_gconv_desc d) {
  constexpr int FB = 64 * NP;   // uint4 entries per fragment (NP planes of 64 lanes)
#ifdef PDSE_DIAG
  long long* const trace = g_trace4;
#else
  long long* const trace = nullptr;
#endif
  const long long c_start = trace ? clock64() : 0;
  long long c_req = 0, c_cmp = 0, c_bar = 0;
  constexpr bool DUAL = (EPI != PDSE_EPI_LINEAR);
  constexpr int NBR = DUAL ? 2 : 1, FR = NBR * MT;   // fragments (3 planes each) per K block and workgroup
  extern __shared__ uint4 ring[];                     // [2 buffers][G4_CH blocks][FR][FB]
  const unsigned ring_base = (unsigned)(uintptr_t)ring;   // LDS byte address (the low half of the flat address)
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int b = blockIdx.y;
  const int P = d.Tout * d.Fout;
  const int p = (blockIdx.x * 8 + wave) * 32 + col;
  const bool pvalid = p < P;
  const int t = pvalid ? p / d.Fout : 0;
  const int j = pvalid ? p - t * d.Fout : 0;
  const int mtiles = (d.Cout + 31) >> 5;
  const int mt0 = blockIdx.z * MT;

  const int cbn0 = d.in0.C >> 4, cbn1 = d.in1.C >> 4;                    // 16-channel blocks per source
  const int cps0 = (cbn0 + G4_CH - 1) / G4_CH, cps1 = (cbn1 + G4_CH - 1) / G4_CH;   // chunks per (source, tap)
  const int nch0 = d.ntaps * cps0, nch = nch0 + d.ntaps * cps1;

  // Everything about a chunk is wave-uniform; readfirstlane says so to the compiler (without it the source select and the
  // channel bases were treated as per-lane values and every gather load sat in a waterfall loop)
  auto uni = [](const int v) { return __builtin_amdgcn_readfirstlane(v); };
  auto decode = [&](const int ci) {
    g4_chunk c;
    c.s = uni(ci >= nch0);
    const int q = c.s ? ci - nch0 : ci, cps = c.s ? cps1 : cps0, cbn = c.s ? cbn1 : cbn0;
    c.tap = uni(q / cps);
    c.cb0 = uni((q - c.tap * cps) * G4_CH);
    c.n = uni(min(G4_CH, cbn - c.cb0));
    c.kb0 = uni((c.s ? d.ntaps * cbn0 : 0) + c.tap * cbn + c.cb0);
    return c;
  };
  // A fragments of a chunk -> ring buffer `buf`: one 1 KB piece (= one plane of one fragment) per wave instruction
  auto dma = [&](const g4_chunk& c, const int buf) {
    const int npieces = c.n * FR * NP;
    for (int pc = __builtin_amdgcn_readfirstlane(wave); pc < npieces; pc += 8) {
      const int i = pc / (FR * NP), rem = pc - i * (FR * NP), f = rem / NP, part = rem - f * NP;
      const int br = f / MT, m = f - br * MT;
      if (mt0 + m < mtiles) {   // tiles past Cout keep stale fragments: their accumulators are never stored
        const uint4* src = reinterpret_cast<const uint4*>(br ? d.w1 : d.w0) + ((size_t)(c.kb0 + i) * mtiles + mt0 + m) * FB +
                           part * 64 + lane;
        glds16(src, ring + ((buf * G4_CH + i) * FR + f) * FB + part * 64);
      }
    }
  };
  // B operand of a chunk: raw[i][e] = channel 16 (cb0 + i) + 8h + e of this lane's position at the chunk's tap
  auto gather = [&](const g4_chunk& c, g4_raw<BLK>& raw, bool& inb) {
    const bool s1 = c.s != 0;   // field-by-field scalar selects (a reference to one of two kernel-argument structs is not)
    const float* const sptr = s1 ? d.in1.ptr : d.in0.ptr;
    const int64_t ssb = s1 ? d.in1.sb : d.in0.sb, ssc = s1 ? d.in1.sc : d.in0.sc, sst = s1 ? d.in1.st : d.in0.st,
                  ssf = s1 ? d.in1.sf : d.in0.sf;
    int dt = 0, df = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {   // kernel-argument table, scalar compares instead of a dynamically indexed load
      dt = c.tap == k ? d.tap_dt[k] : dt;
      df = c.tap == k ? d.tap_df[k] : df;
    }
    const int tin = t + dt, fin = j * d.sf_in + df;
    inb = pvalid && fin >= 0 && fin < d.Fin && tin >= 0 && tin < d.Tin;
    if constexpr (BLK) {   // [B][C/8][T][F][8]: block 2 (cb0 + i) + h, two 16-byte loads per K block
      const unsigned off = 4u * (unsigned)((inb ? (int64_t)b * ssb + (int64_t)tin * sst + (int64_t)fin * ssf : 0) + (int64_t)h * ssc);
#pragma unroll
      for (int i = 0; i < G4_CH; ++i) {
        if (i < c.n) {
          const float* base = sptr + (int64_t)(2 * (c.cb0 + i)) * ssc;
          raw.v[i][0] = g4_load16(base, off);
          raw.v[i][1] = g4_load16(base + 4, off);
        }
      }
    } else {
    const unsigned off = 4u * (unsigned)((inb ? (int64_t)b * ssb + (int64_t)tin * sst + (int64_t)fin * ssf : 0) + (int64_t)(8 * h) * ssc);
#pragma unroll
    for (int i = 0; i < G4_CH; ++i) {
      if (i < c.n) {   // wave-uniform
        const float* base = sptr + (int64_t)(16 * (c.cb0 + i)) * ssc;
#pragma unroll
        for (int e = 0; e < 8; ++e) raw.v[i][e] = g4_load(base + (int64_t)e * ssc, off);
      }
    }
    }
  };

  f32x16 acc0[MT], acc1[DUAL ? MT : 1];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      acc0[m][r] = 0.f;
      if (DUAL) acc1[m][r] = 0.f;
    }
  }
  // One chunk.  The ring reads of K block i+1 are issued fragment by fragment right behind the six MFMAs that were the last
  // readers of that fragment's registers in block i, so they fly under the remaining MFMAs of block i instead of in front of
  // block i+1's (an MFMA reads its A / B operands when it issues; the LDS data returns ~100 cycles later).  Before round 3's
  // end every block waited for its twelve ring reads with an idle matrix pipe: 5.3k cycles per chunk for 3.1k of MFMAs.
  auto compute = [&](const g4_chunk& c, const g4_raw<BLK>& raw, const bool inb, const int buf) {
    const bool elu = uni((c.s ? d.in1.act : d.in0.act) == PDSE_ACT_ELU) != 0;   // GCRN re-applies ELU to the skip half (gcrn.py:152-155)
    u32x4 af[FR][NP];
    const unsigned wa0 = ring_base + (unsigned)((((buf * G4_CH) * FR) * FB + lane) * 16);
#pragma unroll
    for (int f = 0; f < FR; ++f) g4_lds_read3(wa0 + f * (FB * 16), af[f]);
#pragma unroll
    for (int i = 0; i < G4_CH; ++i) {
      if (i < c.n) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = inb ? raw.get(i, e) : 0.f;
        if (elu) {   // wave-uniform; exp2-based like the epilogues' ELU (act_c); elu(0) = 0 keeps masked lanes zero
#pragma unroll
          for (int e = 0; e < 8; ++e) x[e] = x[e] < 0.f ? fast_exp(x[e]) - 1.0f : x[e];
        }
        uint4 bp[NP];
        split_planes<NP>(x, bp, pow2i(PDSE_F16_ACT_EXP));         // runs under the LDS latency of the block's fragments
        g4_lds_wait(af);
        const bool more = i + 1 < c.n;   // wave-uniform
        const unsigned wn = ring_base + (unsigned)((((buf * G4_CH + i + 1) * FR) * FB + lane) * 16);
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          const int m = f % MT;
          if (f < MT) acc0[m] = g4_mma<NP>(af[f], bp, acc0[m]);
          else acc1[m] = g4_mma<NP>(af[f], bp, acc1[m]);
          // (i + 1 < G4_CH is a compile-time fact once the loop is unrolled: no read is emitted behind the last possible block,
          // whose destination registers would be dead - free for the compiler to re-use - while the read is still in flight)
          if (i + 1 < G4_CH && more) g4_lds_read3(wn + f * (FB * 16), af[f]);
        }
      }
    }
  };

  g4_raw<BLK> rawA, rawB;
  bool inbA = false, inbB = false;
  g4_chunk cA = decode(0), cB = cA;
  gather(cA, rawA, inbA);
  dma(cA, 0);
  __syncthreads();   // DMA and gather of chunk 0 have landed (the fence waits vmcnt(0) while LDS-DMA is in flight)
  g4_landed(rawA);
  const long long c_pro = trace ? clock64() : 0;
  for (int ci = 0; ci < nch; ci += 2) {
    const bool hasB = ci + 1 < nch;
    const long long k0 = trace ? clock64() : 0;
    if (hasB) {      // chunk ci+1: requests and DMA go out before chunk ci's matrix work
      cB = decode(ci + 1);
      gather(cB, rawB, inbB);
      dma(cB, 1);
    }
    const long long k1 = trace ? clock64() : 0;
    compute(cA, rawA, inbA, 0);
    const long long k2 = trace ? clock64() : 0;
    __syncthreads();   // buffer 1 complete; every wave is done reading buffer 0
    const long long k3 = trace ? clock64() : 0;
    c_req += k1 - k0, c_cmp += k2 - k1, c_bar += k3 - k2;
    if (!hasB) break;
    g4_landed(rawB);
    const bool hasA = ci + 2 < nch;
    if (hasA) {
      cA = decode(ci + 2);
      gather(cA, rawA, inbA);
      dma(cA, 0);
    }
    const long long k4 = trace ? clock64() : 0;
    compute(cB, rawB, inbB, 1);
    const long long k5 = trace ? clock64() : 0;
    __syncthreads();
    const long long k6 = trace ? clock64() : 0;
    c_req += k4 - k3, c_cmp += k5 - k4, c_bar += k6 - k5;
    g4_landed(rawA);
  }
  const long long c_loop = trace ? clock64() : 0;
  if constexpr (NP == 2) {   // f16x2: the accumulators hold (true value) * 2^(activation exponent + weight exponent)
    const float us = pow2i(-(PDSE_F16_ACT_EXP + d.wexp));
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        acc0[m][r] *= us;
        if (DUAL) acc1[m][r] *= us;
      }
  }
  gconv_epilogue<EPI, MT>(d, tail_from_desc(d), acc0, acc1, b, t, j, pvalid, lane, h, mt0, mtiles);
  if (trace && lane == 0) {
    long long* q = trace + ((size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + wave) * 8;
    q[0] = c_pro - c_start;
    q[1] = c_req;
    q[2] = c_cmp;
    q[3] = c_bar;
    q[4] = nch;
    q[5] = clock64() - c_loop;
    q[6] = clock64() - c_start;
  }
}

template <int EPI, int MT, bool BLK, int NP>
static int launch4b(const pdse_gconv_desc* d, hipStream_t s, const int mtiles) {
  const int P = d->Tout * d->Fout;
  const dim3 grid(((P + 31) / 32 + 7) / 8, d->B, (mtiles + MT - 1) / MT), block(512);
  constexpr int FR = (EPI == PDSE_EPI_LINEAR ? 1 : 2) * MT;
  const size_t lds = (size_t)2 * G4_CH * FR * 64 * NP * sizeof(uint4);
  static unsigned long long attr_mask = 0;   // per instantiation and device
  if (lds > 64 * 1024 && pdse_lds_attr((const void*)gconv4_kernel<EPI, MT, BLK, NP>, &attr_mask, "gconv4 lds attribute")) return 1;
  static const bool tracing = PDSE_DIAG_ENV("PDSE_G4_TRACE") != nullptr;
  static long long* tbuf = nullptr;
  const size_t nw = (size_t)grid.x * grid.y * grid.z * 8;
  if (tracing) {
    if (!tbuf) {
      (void)hipMalloc(&tbuf, (size_t)1 << 24);
      (void)hipMemcpyToSymbol(HIP_SYMBOL(g_trace4), &tbuf, sizeof(tbuf));
    }
    (void)hipMemsetAsync(tbuf, 0, nw * 64, s);
  }
  hipLaunchKernelGGL((gconv4_kernel<EPI, MT, BLK, NP>), grid, block, lds, s, *d);
  if (tracing && nw * 64 <= ((size_t)1 << 24)) {   // diagnostic: per-wave averages in shader clocks
    (void)hipStreamSynchronize(s);
    long long* h = (long long*)malloc(nw * 64);
    (void)hipMemcpy(h, tbuf, nw * 64, hipMemcpyDeviceToHost);
    double sum[7] = {0};
    for (size_t i = 0; i < nw; ++i)
      for (int k = 0; k < 7; ++k) sum[k] += (double)h[i * 8 + k];
    fprintf(stderr, "gconv4 trace EPI %d MT %d taps %d cin %d+%d cout %d %dx%d grid %ux%ux%u: prologue %.0f | per chunk: request %.0f compute %.0f barrier %.0f | chunks %.1f | epilogue %.0f total %.0f\n",
            EPI, MT, d->ntaps, d->in0.C, d->in1.C, d->Cout, d->Tout, d->Fout, grid.x, grid.y, grid.z, sum[0] / nw, sum[1] / sum[4], sum[2] / sum[4], sum[3] / sum[4],
            sum[4] / nw, sum[5] / nw, sum[6] / nw);
    free(h);
  }
  return pdse_check_launch("gconv4");
}

template <int EPI, int MT>
static int launch4(const pdse_gconv_desc* d, hipStream_t s, const int mtiles) {
  if (d->korder == 5)   // two planes: fp16 hi + lo of the power-of-two scaled operands, three f16 products (f16x2)
    return d->in0.blk ? launch4b<EPI, MT, true, 2>(d, s, mtiles) : launch4b<EPI, MT, false, 2>(d, s, mtiles);
  if (d->korder == 4)   // one plane: plain bf16 operands, one product (the opt-in bf16 mode)
    return d->in0.blk ? launch4b<EPI, MT, true, 1>(d, s, mtiles) : launch4b<EPI, MT, false, 1>(d, s, mtiles);
  return d->in0.blk ? launch4b<EPI, MT, true, 3>(d, s, mtiles) : launch4b<EPI, MT, false, 3>(d, s, mtiles);
}

// ---------------------------------------------------------------------------------------------------------------
// Flat form (pdse_gconv_desc.flat; the LSTM input projections: LINEAR, one source, Fout == 1, K <= 512, Cout = 2048).
// gconv4_kernel runs these as 16 channel groups x 8 column tiles per workgroup: every group gathers and splits the same
// activations again, and the column tiles are cut per batch item.  Here
//   * the columns are n = b Tout + t over all B Tout positions; a lane derives (b, t) of its own column, so a tile may
//     straddle batch items: each column addresses its own item and masks its own taps;
//   * the workgroup gathers its 32 columns once for the WHOLE K, splits them and keeps the planes in LDS in B-fragment order,
//     [K block][plane][64 lanes] uint4 (64 KB for K = 512 in the two-plane form); one barrier, none afterwards;
//   * its 8 waves then walk MTW channel tiles each (8 MTW = 32 tiles of 32 rows per workgroup) over all K blocks: the A
//     fragments come straight from global memory into registers (the packed weights are read in 1 KB rows and are shared by
//     every workgroup, so they stay in L2), the B fragments from LDS.
// Every accumulator sees its K blocks in the order of gconv4_kernel ((tap, channel block)) and each product is the same
// instruction on the same operands; the epilogue is the same function: results are bit for bit those of the tiled form.
// ---------------------------------------------------------------------------------------------------------------
template <int MTW, bool BLK, int NP>
__global__ __launch_bounds__(512, NP == 2 ? 4 : 2) void gconv4_flat_kernel(const pdse_gconv_desc d) {
  extern __shared__ uint4 bimg[];   // [K blocks][NP][64]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int n = blockIdx.x * 32 + col;
  const bool pvalid = n < d.B * d.Tout;
  const int b = pvalid ? n / d.Tout : 0;
  const int t = pvalid ? n - b * d.Tout : 0;
  const int mtiles = (d.Cout + 31) >> 5;
  const int cbn = d.in0.C >> 4, nkb = d.ntaps * cbn;   // K blocks of 16 channels, order (tap, channel block)
  const bool elu = d.in0.act == PDSE_ACT_ELU;

  for (int kb = wave; kb < nkb; kb += 8) {   // wave-uniform
    const int tap = kb / cbn, cb = kb - tap * cbn;
    int dt = 0, df = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      dt = tap == k ? d.tap_dt[k] : dt;
      df = tap == k ? d.tap_df[k] : df;
    }
    const int tin = t + dt, fin = df;   // Fout == 1: output bin 0
    const bool inb = pvalid && fin >= 0 && fin < d.Fin && tin >= 0 && tin < d.Tin;
    // a column without a value at this tap reads element 0 of the source (always there) and drops it
    const int64_t pos = inb ? (int64_t)b * d.in0.sb + (int64_t)tin * d.in0.st + (int64_t)fin * d.in0.sf : 0;
    float x[8];
    if constexpr (BLK) {   // [B][C/8][T][F][8]: block 2 cb + h
      const float* q = d.in0.ptr + pos + (int64_t)(2 * cb + h) * d.in0.sc;
      const float4 v0 = *reinterpret_cast<const float4*>(q), v1 = *reinterpret_cast<const float4*>(q + 4);
      x[0] = v0.x, x[1] = v0.y, x[2] = v0.z, x[3] = v0.w, x[4] = v1.x, x[5] = v1.y, x[6] = v1.z, x[7] = v1.w;
    } else {
      const float* q = d.in0.ptr + pos + (int64_t)(16 * cb + 8 * h) * d.in0.sc;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = q[(int64_t)e * d.in0.sc];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = inb ? x[e] : 0.f;
    if (elu) {
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = x[e] < 0.f ? fast_exp(x[e]) - 1.0f : x[e];
    }
    uint4 bp[NP];
    split_planes<NP>(x, bp, pow2i(PDSE_F16_ACT_EXP));
#pragma unroll
    for (int p = 0; p < NP; ++p) bimg[(kb * NP + p) * 64 + lane] = bp[p];
  }
  __syncthreads();

  const int mt0 = (blockIdx.y * 8 + wave) * MTW;
  if (mt0 >= mtiles) return;   // (behind the only barrier)
  const uint4* const wl = reinterpret_cast<const uint4*>(d.w0) + lane;
  u32x4 a[MTW][NP];   // (Cout is a multiple of 256: every tile mt0 .. mt0 + MTW - 1 exists)
  auto lda = [&](const int kb, const int m) {
    const u32x4* src = reinterpret_cast<const u32x4*>(wl + ((size_t)kb * mtiles + mt0 + m) * (NP * 64));
#pragma unroll
    for (int p = 0; p < NP; ++p) a[m][p] = src[p * 64];
  };
  f32x16 acc[MTW];
#pragma unroll
  for (int m = 0; m < MTW; ++m) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    lda(0, m);
  }
  for (int kb = 0; kb < nkb; ++kb) {
    uint4 bp[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) bp[p] = bimg[(kb * NP + p) * 64 + lane];
    const int kn = min(kb + 1, nkb - 1);   // (the last block is requested once more instead of a branch in the loop)
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
      acc[m] = g4_mma<NP>(a[m], bp, acc[m]);
      lda(kn, m);   // the next block's fragments of this tile, into the registers its products have just read
    }
  }
  if constexpr (NP == 2) {
    const float us = pow2i(-(PDSE_F16_ACT_EXP + d.wexp));
#pragma unroll
    for (int m = 0; m < MTW; ++m)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][r] *= us;
  }
  gconv_epilogue_impl<PDSE_EPI_LINEAR, MTW, true>(d, tail_from_desc(d), acc, acc, b, t, 0, pvalid, lane, h, mt0, mtiles, 0);   // out_cr == 1
}

template <bool BLK, int NP>
static int launch4f(const pdse_gconv_desc* d, hipStream_t s) {
  constexpr int MTW = 4;
  const int mtiles = (d->Cout + 31) / 32, nkb = d->ntaps * (d->in0.C >> 4);
  const long long N = (long long)d->B * d->Tout;
  const dim3 grid((unsigned)((N + 31) / 32), (mtiles + 8 * MTW - 1) / (8 * MTW)), block(512);
  const size_t lds = (size_t)nkb * NP * 64 * sizeof(uint4);
  static unsigned long long attr_mask = 0;
  if (lds > 64 * 1024 && pdse_lds_attr((const void*)gconv4_flat_kernel<MTW, BLK, NP>, &attr_mask, "gconv4 flat lds attribute")) return 1;
  hipLaunchKernelGGL((gconv4_flat_kernel<MTW, BLK, NP>), grid, block, lds, s, *d);
  return pdse_check_launch("gconv4 flat");
}

// korder 3: LINEAR / GLU, one or two sources of a multiple of 16 channels, no load transform; validated by pdse_gconv_launch
static int check4(const pdse_gconv_desc* d) {
  const bool two = d->in1.C > 0;
  // lane offsets are 32-bit BYTE offsets from a scalar channel base
  const long long span0 = 4 * ((long long)d->B * d->in0.sb + 40ll * d->in0.sc), span1 = two ? 4 * ((long long)d->B * d->in1.sb + 40ll * d->in1.sc) : 0;
  auto blk_ok = [](const pdse_src& x) {   // 16-byte loads: every stride a multiple of 4 floats, the base 16-byte aligned
    return x.blk == 0 || (x.blk == 8 && !((x.sb | x.sc | x.st | x.sf) & 3) && (reinterpret_cast<uintptr_t>(x.ptr) & 15) == 0);
  };
  if (!blk_ok(d->in0) || (two && !blk_ok(d->in1)) || (two && d->in0.blk != d->in1.blk)) {
    pdse_set_error("gconv4: a channel-blocked source has blk = 8, strides in multiples of 4 floats and a 16-byte aligned base; "
                   "two sources are both blocked or both plain");
    return 1;
  }
  if (!(d->epi == PDSE_EPI_LINEAR || d->epi == PDSE_EPI_GLU) || (d->in0.C & 15) || (d->in1.C & 15) || d->in0.C == 0 || d->cin1 ||
      d->xf_mode != 0 || d->padrow != nullptr || d->ntaps > 12 || span0 >= (1ll << 32) || span1 >= (1ll << 32) ||
      (d->epi == PDSE_EPI_GLU && !d->w1) || (d->korder == 5 && (d->wexp < -40 || d->wexp > 40))) {
    pdse_set_error("gconv4: split-bf16 GEMM convolutions need LINEAR / GLU, channel counts in multiples of 16, <= 12 taps, "
                   "no load transform / pad row, 32-bit gather offsets");
    return 1;
  }
  if (d->flat && (d->flat != 1 || !(d->korder == 3 || d->korder == 5) || d->epi != PDSE_EPI_LINEAR || two || d->Fout != 1 ||
                  d->ntaps * (d->in0.C >> 4) > 32 || (d->Cout & 255) || d->out_cr != 1 || (long long)d->B * d->Tout > (1ll << 30))) {
    pdse_set_error("gconv4: the flat form takes korder 3 / 5 LINEAR launches of one source with Fout = 1, ntaps * C <= 512, "
                   "Cout in multiples of 256 and out_cr = 1");
    return 1;
  }
  return 0;
}

int pdse_gconv4_launch(const pdse_gconv_desc* d, hipStream_t s) {
  if (check4(d)) return 1;
  if (d->flat) {
    if (d->korder == 5) return d->in0.blk ? launch4f<true, 2>(d, s) : launch4f<false, 2>(d, s);
    return d->in0.blk ? launch4f<true, 3>(d, s) : launch4f<false, 3>(d, s);
  }
  const int mtiles = (d->Cout + 31) / 32;
  if (d->epi == PDSE_EPI_GLU) return mtiles >= 2 ? launch4<PDSE_EPI_GLU, 2>(d, s, mtiles) : launch4<PDSE_EPI_GLU, 1>(d, s, mtiles);
  if (mtiles >= 4) return launch4<PDSE_EPI_LINEAR, 4>(d, s, mtiles);
  if (mtiles >= 2) return launch4<PDSE_EPI_LINEAR, 2>(d, s, mtiles);
  return launch4<PDSE_EPI_LINEAR, 1>(d, s, mtiles);
}

// ---------------------------------------------------------------------------------------------------------------
// Phase pair of a stride-(1,2) transposed convolution (GLU, f16x2) as one launch.  d: the even output bins 2j (taps {j, j-1}),
// e: the odd bins 2j+1 (tap {j}, which is d's tap 0).  The workgroup walks d's chunks; in the chunks of tap 0 the ring also
// carries e's fragments of the same K blocks, and the split B operand the wave holds for d's products is multiplied by them
// as well: one gather and three product sets where the two launches gathered 2 + 1 times.  e's accumulators see their K
// blocks in the order of e's own launch ((source, channel block), the order d's tap-0 chunks come in) and each product is
// the same instruction on the same operands, so every element equals the separate launch bit for bit.  Positions are d's;
// the odd bin of a lane exists while j < e.Fout (one bin fewer when the output row length is odd) and is masked on the
// store.  Ring: [2 buffers][G4_CH blocks][2 phases x 2 branches x MT][2 planes x 64] uint4.
// ---------------------------------------------------------------------------------------------------------------
template <int MT, bool BLK>
__global__ __launch_bounds__(512, 2) void gconv4_pair_kernel(const pdse_gconv_desc d, const pdse_gconv_desc e) {
  constexpr int NP = 2, FB = 64 * NP;
  constexpr int FR = 2 * MT, FR2 = 2 * FR;   // fragments per K block: d's alone, d's and e's
  extern __shared__ uint4 ring[];
  const unsigned ring_base = (unsigned)(uintptr_t)ring;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int b = blockIdx.y;
  const int P = d.Tout * d.Fout;
  const int p = (blockIdx.x * 8 + wave) * 32 + col;
  const bool pvalid = p < P;
  const int t = pvalid ? p / d.Fout : 0;
  const int j = pvalid ? p - t * d.Fout : 0;
  const int mtiles = (d.Cout + 31) >> 5;
  const int mt0 = blockIdx.z * MT;

  const int cbn0 = d.in0.C >> 4, cbn1 = d.in1.C >> 4;
  const int cps0 = (cbn0 + G4_CH - 1) / G4_CH, cps1 = (cbn1 + G4_CH - 1) / G4_CH;
  const int nch0 = d.ntaps * cps0, nch = nch0 + d.ntaps * cps1;

  auto uni = [](const int v) { return __builtin_amdgcn_readfirstlane(v); };
  auto decode = [&](const int ci) {
    g4_chunk c;
    c.s = uni(ci >= nch0);
    const int q = c.s ? ci - nch0 : ci, cps = c.s ? cps1 : cps0, cbn = c.s ? cbn1 : cbn0;
    c.tap = uni(q / cps);
    c.cb0 = uni((q - c.tap * cps) * G4_CH);
    c.n = uni(min(G4_CH, cbn - c.cb0));
    c.kb0 = uni((c.s ? d.ntaps * cbn0 : 0) + c.tap * cbn + c.cb0);
    return c;
  };
  // fragments f < FR: d's (branch f / MT, tile f % MT); FR <= f < FR2, in the chunks of tap 0 only: e's, K block
  // (source, channel block) of its one-tap weights
  auto dma = [&](const g4_chunk& c, const int buf) {
    const int nf = c.tap == 0 ? FR2 : FR;
    const int kb1 = (c.s ? cbn0 : 0) + c.cb0;
    const int npieces = c.n * nf * NP;
    for (int pc = __builtin_amdgcn_readfirstlane(wave); pc < npieces; pc += 8) {
      const int i = pc / (nf * NP), rem = pc - i * (nf * NP), f = rem / NP, part = rem - f * NP;
      const bool odd = f >= FR;
      const int g = odd ? f - FR : f, br = g / MT, m = g - br * MT;
      if (mt0 + m < mtiles) {
        const float* const w = odd ? (br ? e.w1 : e.w0) : (br ? d.w1 : d.w0);
        const uint4* src = reinterpret_cast<const uint4*>(w) + ((size_t)((odd ? kb1 : c.kb0) + i) * mtiles + mt0 + m) * FB + part * 64 + lane;
        glds16(src, ring + ((buf * G4_CH + i) * FR2 + f) * FB + part * 64);
      }
    }
  };
  auto gather = [&](const g4_chunk& c, g4_raw<BLK>& raw, bool& inb) {
    const bool s1 = c.s != 0;
    const float* const sptr = s1 ? d.in1.ptr : d.in0.ptr;
    const int64_t ssb = s1 ? d.in1.sb : d.in0.sb, ssc = s1 ? d.in1.sc : d.in0.sc, sst = s1 ? d.in1.st : d.in0.st,
                  ssf = s1 ? d.in1.sf : d.in0.sf;
    int dt = 0, df = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      dt = c.tap == k ? d.tap_dt[k] : dt;
      df = c.tap == k ? d.tap_df[k] : df;
    }
    const int tin = t + dt, fin = j * d.sf_in + df;
    inb = pvalid && fin >= 0 && fin < d.Fin && tin >= 0 && tin < d.Tin;
    if constexpr (BLK) {
      const unsigned off = 4u * (unsigned)((inb ? (int64_t)b * ssb + (int64_t)tin * sst + (int64_t)fin * ssf : 0) + (int64_t)h * ssc);
#pragma unroll
      for (int i = 0; i < G4_CH; ++i) {
        if (i < c.n) {
          const float* base = sptr + (int64_t)(2 * (c.cb0 + i)) * ssc;
          raw.v[i][0] = g4_load16(base, off);
          raw.v[i][1] = g4_load16(base + 4, off);
        }
      }
    } else {
      const unsigned off = 4u * (unsigned)((inb ? (int64_t)b * ssb + (int64_t)tin * sst + (int64_t)fin * ssf : 0) + (int64_t)(8 * h) * ssc);
#pragma unroll
      for (int i = 0; i < G4_CH; ++i) {
        if (i < c.n) {
          const float* base = sptr + (int64_t)(16 * (c.cb0 + i)) * ssc;
#pragma unroll
          for (int e_ = 0; e_ < 8; ++e_) raw.v[i][e_] = g4_load(base + (int64_t)e_ * ssc, off);
        }
      }
    }
  };

  f32x16 acc[FR2];   // [phase][branch][tile]
#pragma unroll
  for (int f = 0; f < FR2; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[f][r] = 0.f;

  // NF = FR2: a chunk of tap 0 (both phases); NF = FR: any other chunk.  Two instantiations instead of a run-time
  // fragment count: which registers a ring read writes, and which are live across a K block, stays a compile-time fact
  // (see compute() of gconv4_kernel on reads into dead registers).  The fragment registers hold ONE phase's FR fragments: d's
  // products of a K block are followed by the reads of e's fragments of the same block into the registers they free, and
  // e's products by the reads of d's fragments of the next block.
  auto compute = [&](auto nf_tag, const g4_chunk& c, const g4_raw<BLK>& raw, const bool inb, const int buf) {
    constexpr int NF = decltype(nf_tag)::value;
    const bool elu = uni((c.s ? d.in1.act : d.in0.act) == PDSE_ACT_ELU) != 0;
    u32x4 af[FR][NP];
    const unsigned wa0 = ring_base + (unsigned)((((buf * G4_CH) * FR2) * FB + lane) * 16);
#pragma unroll
    for (int f = 0; f < FR; ++f) g4_lds_read3(wa0 + f * (FB * 16), af[f]);
#pragma unroll
    for (int i = 0; i < G4_CH; ++i) {
      if (i < c.n) {
        float x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = inb ? raw.get(i, q) : 0.f;
        if (elu) {
#pragma unroll
          for (int q = 0; q < 8; ++q) x[q] = x[q] < 0.f ? fast_exp(x[q]) - 1.0f : x[q];
        }
        uint4 bp[NP];
        split_planes<NP>(x, bp, pow2i(PDSE_F16_ACT_EXP));
        g4_lds_wait(af);
        const bool more = i + 1 < c.n;
        const unsigned wi = ring_base + (unsigned)((((buf * G4_CH + i) * FR2) * FB + lane) * 16);
        const unsigned wn = wi + FR2 * FB * 16;
        if constexpr (NF == FR2) {
#pragma unroll
          for (int f = 0; f < FR; ++f) {
            acc[f] = g4_mma<NP>(af[f], bp, acc[f]);
            g4_lds_read3(wi + (FR + f) * (FB * 16), af[f]);
          }
          g4_lds_wait(af);
        }
#pragma unroll
        for (int f = 0; f < FR; ++f) {
          acc[NF - FR + f] = g4_mma<NP>(af[f], bp, acc[NF - FR + f]);
          if (i + 1 < G4_CH && more) g4_lds_read3(wn + f * (FB * 16), af[f]);
        }
      }
    }
  };
  auto compute_chunk = [&](const g4_chunk& c, const g4_raw<BLK>& raw, const bool inb, const int buf) {
    if (c.tap == 0) compute(std::integral_constant<int, FR2>{}, c, raw, inb, buf);
    else compute(std::integral_constant<int, FR>{}, c, raw, inb, buf);
  };

  g4_raw<BLK> rawA, rawB;
  bool inbA = false, inbB = false;
  g4_chunk cA = decode(0), cB = cA;
  gather(cA, rawA, inbA);
  dma(cA, 0);
  __syncthreads();
  g4_landed(rawA);
  for (int ci = 0; ci < nch; ci += 2) {
    const bool hasB = ci + 1 < nch;
    if (hasB) {
      cB = decode(ci + 1);
      gather(cB, rawB, inbB);
      dma(cB, 1);
    }
    compute_chunk(cA, rawA, inbA, 0);
    __syncthreads();
    if (!hasB) break;
    g4_landed(rawB);
    if (ci + 2 < nch) {
      cA = decode(ci + 2);
      gather(cA, rawA, inbA);
      dma(cA, 0);
    }
    compute_chunk(cB, rawB, inbB, 1);
    __syncthreads();
    g4_landed(rawA);
  }
  const float us0 = pow2i(-(PDSE_F16_ACT_EXP + d.wexp)), us1 = pow2i(-(PDSE_F16_ACT_EXP + e.wexp));
#pragma unroll
  for (int f = 0; f < FR2; ++f)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[f][r] *= f < FR ? us0 : us1;
  gconv_epilogue<PDSE_EPI_GLU, MT>(d, tail_from_desc(d), acc, acc + MT, b, t, j, pvalid, lane, h, mt0, mtiles);
  gconv_epilogue<PDSE_EPI_GLU, MT>(e, tail_from_desc(e), acc + FR, acc + FR + MT, b, t, j, pvalid && j < e.Fout, lane, h, mt0, mtiles);
}

template <int MT, bool BLK>
static int launch4p(const pdse_gconv_desc* d, const pdse_gconv_desc* e, hipStream_t s, const int mtiles) {
  const int P = d->Tout * d->Fout;
  const dim3 grid(((P + 31) / 32 + 7) / 8, d->B, (mtiles + MT - 1) / MT), block(512);
  const size_t lds = (size_t)2 * G4_CH * 4 * MT * 64 * 2 * sizeof(uint4);
  static unsigned long long attr_mask = 0;
  if (lds > 64 * 1024 && pdse_lds_attr((const void*)gconv4_pair_kernel<MT, BLK>, &attr_mask, "gconv4 pair lds attribute")) return 1;
  hipLaunchKernelGGL((gconv4_pair_kernel<MT, BLK>), grid, block, lds, s, *d, *e);
  return pdse_check_launch("gconv4 pair");
}

// That d and e are the two phases of one transposed convolution this kernel takes (each validated by itself before:
// pdse_gconv_pair_check).  Checked once, when the pair enters a plan.
int pdse_gconv4_pair_check(const pdse_gconv_desc* d, const pdse_gconv_desc* e) {
  if (check4(d) || check4(e)) return 1;
  auto same_src = [](const pdse_src& x, const pdse_src& y) {
    return x.ptr == y.ptr && x.sb == y.sb && x.sc == y.sc && x.st == y.st && x.sf == y.sf && x.C == y.C && x.act == y.act && x.blk == y.blk;
  };
  const bool ok = d->korder == 5 && e->korder == 5 && d->epi == PDSE_EPI_GLU && e->epi == PDSE_EPI_GLU && d->w2 == nullptr &&
                  e->w2 == nullptr && d->p1mask == 1 && d->Fout1 == e->Fout && same_src(d->in0, e->in0) && same_src(d->in1, e->in1) &&
                  d->Tin == e->Tin && d->Fin == e->Fin && d->sf_in == e->sf_in && d->ntaps >= 1 && e->ntaps == 1 &&
                  d->tap_dt[0] == e->tap_dt[0] && d->tap_df[0] == e->tap_df[0] && d->B == e->B && d->Tout == e->Tout &&
                  d->Cout == e->Cout && e->Fout >= 1 && e->Fout <= d->Fout;
  if (!ok) {
    pdse_set_error("gconv4: p1mask on a korder 5 GLU launch says that the next launch is its odd phase: the same sources, batch, frames and "
                   "channels, one tap that is this launch's tap 0, Fout1 bins (at most this launch's)");
    return 1;
  }
  // One channel tile per workgroup only: with two (eight accumulators) the kernel needs more than the 256 registers a wave of a
  // 512-thread workgroup can have and spills, and one tile per workgroup over several tiles would gather MORE often than the two
  // launches do.  Stages of more than 32 channels stay two launches (nets.GcrnPlan marks none of them).
  if (d->Cout > 32) {
    pdse_set_error("gconv4: a phase pair runs as one launch for Cout <= 32 only");
    return 1;
  }
  return 0;
}

// a pair that passed pdse_gconv4_pair_check
int pdse_gconv4_pair_launch(const pdse_gconv_desc* d, const pdse_gconv_desc* e, hipStream_t s) {
  return d->in0.blk ? launch4p<1, true>(d, e, s, 1) : launch4p<1, false>(d, e, s, 1);
}
