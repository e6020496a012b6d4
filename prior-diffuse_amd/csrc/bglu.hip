// bglu.hip - BiConvGLU / BiConvTransGLU blocks of the eps-net on PLANE tensors (include/pdse.h: pdse_bglu_desc).
// Reference semantics: model/diff3.py:307-326 (BiConvGLU), :329-351 (BiConvTransGLU), the BatchNorm2d + PReLU behind
// every stage (:122-141, :172-203) and the next stage's 1x1 conv1 (:146-149, :343-345).
//
// Round 3 redesign of csrc/gconv3.hip, from measurements of that kernel (profiles/r03_*):
//   * one tile of 32 positions cost 288 bf16 MFMAs (9.2k matrix-pipe cycles) and ~2450 vector instructions (9.8k issue
//     cycles), and the time per tile on a SIMD was their SUM plus ~5k of waits, scalar work and ~70 exec-mask branches:
//     vector instructions of one wave do not hide behind matrix instructions of the other wave of the SIMD, only behind
//     matrix instructions of their own stream (MI355X_MICROARCH.md: <= 5 vector instructions per 32x32x16 gap);
//   * so a tile's instruction order is spelled out by hand (csrc/bglu_sched.inc: slots of one product beside one chunk of
//     vector work) - the K loop is matrix instructions and LDS reads only, because the input arrives as the producer's
//     bf16 split planes - in one basic block (no exec-mask branches: out-of-range taps are zero margins, lanes beyond
//     the last position compute on position 0 and only the final stores are predicated), 8 waves per workgroup.  The
//     4-wave form that overlapped the K loop of tile i+1 with the tail of tile i, and the 12/16-wave and spread-issue
//     forms, measured slower and left the tree after commit ae0a628;
//   * vector work removed from the tail: BatchNorm folded into conv2, -log2 e into l_conv / r_conv, biases seed the
//     accumulators from LDS, PReLU is mul + max.
// NP = 3: exact three-way bf16 split of every operand, six products per multiply-add (fp32-equivalent);
// NP = 1: plain bf16 operands, one product (the opt-in bf16 mode; its own tolerance).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "pdse.h"
#include "pdse_internal.h"

#include "gconv_common.h"

// Cache policy of the plane / skip stores (gconv_common.h: bstore16).  0 = write-back through the XCD's L2.  Measured: written
// through (17 = sc0 sc1) or non-temporal (2) the same launches take 3-7 x as long (encoder 401x79: 183 -> 1203 / 1352 us;
// decoder 401x40: 153 -> 566 / 1033 us) - the L2 assembling full lines before they go to HBM is worth that much here.
#ifndef BGLU_ST_AUX
#define BGLU_ST_AUX 0
#endif

namespace {

#ifdef BGLU_DIAG   // diagnostic build only (-DBGLU_DIAG, timed with tools/time_bglu.py)
__device__ unsigned long long g_bglu_slots[97];   // BGLU_SLOTSTAMP: shader cycles per slot, summed over waves and tiles; [96]: tiles
#endif

constexpr int popc(int m) { return m ? (m & 1) + popc(m >> 1) : 0; }
constexpr int rank_of(int m, int tap) { return popc(m & ((1 << tap) - 1)); }

// planes.h: split_planes behind this file's timing ablation
template <int NP>
__device__ __forceinline__ void split8p(const float (&x)[8], uint4 (&p)[NP], const float sc = 1.0f) {
#if defined(BGLU_DIAG) && defined(BGLU_NO_SPLIT)   // timing ablation: no split arithmetic (results wrong)
  p[0] = make_uint4(__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3]));
  if constexpr (NP == 3) {
    p[1] = make_uint4(__float_as_uint(x[4]), __float_as_uint(x[5]), __float_as_uint(x[6]), __float_as_uint(x[7]));
    p[2] = p[0];
  }
  return;
#endif
  split_planes<NP>(x, p, sc);
}

__device__ __forceinline__ float sigm2(const float m) {   // sigmoid of a pre-activation that is already scaled by -log2 e
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(m));
}

__device__ __forceinline__ float vmax(const float a, const float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

#define BGLU_FLOATS 512
// float operands behind the fragment areas: bl 0, br 32, bl0 64, br0 96, blc 128, brc 160, bc2 192 (64), nxb 256 (96), wc2v 352
enum { F_BL = 0, F_BR = 32, F_BL0 = 64, F_BR0 = 96, F_BLC = 128, F_BRC = 160, F_BC2 = 192, F_NXB = 256, F_WC2V = 352 };

template <int NT, int P1MASK, int C2, int NXN, bool IN4, int NP>
struct bglu_cfg {
  static constexpr int WV = 8;
  static constexpr int NB = IN4 ? 3 : 2 * NT;
  static constexpr int NT1 = popc(P1MASK), NB1 = 2 * NT1;
  static constexpr bool DUAL = P1MASK != 0;
  static constexpr int BS = NP * 64;   // uint4 per fragment block
  static constexpr int o_gL = 0, o_gR = NB * BS, o_gL1 = 2 * NB * BS, o_gR1 = o_gL1 + NB1 * BS, o_lc = o_gR1 + NB1 * BS,
                       o_rc = o_lc + 2 * BS, o_c2 = o_rc + 2 * BS, o_nx = o_c2 + (C2 == 64 ? 4 * BS : 0),
                       o_f = o_nx + NXN * 4 * BS;
  static constexpr size_t lds_bytes = (size_t)o_f * sizeof(uint4) + BGLU_FLOATS * sizeof(float);
};

// 8 waves (two per SIMD, 256 registers), K loop and tail of the same tile one after the other - a wave issues at most one
// instruction per four cycles, so two waves per SIMD double the issue rate and cover each other's stalls.
template <int NT, int P1MASK, int C2, int NXN, bool IN4, int NP>
__global__ __launch_bounds__(512, 2) void bglu_kernel(const pdse_bglu_desc d) {
  using CF = bglu_cfg<NT, P1MASK, C2, NXN, IN4, NP>;
  constexpr int WV = CF::WV, NB = CF::NB, NB1 = CF::NB1, BS = CF::BS;
  constexpr bool DUAL = CF::DUAL;
  extern __shared__ uint4 img[];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int col = lane & 31, h = lane >> 5;
  const int b = blockIdx.y;
  const int P = d.Tout * d.Fout;
  // NP == 2 (f16x2): the powers of two between the exponents of the planes (2^PDSE_F16_ACT_EXP), of the four weight groups
  // (d.qexp: gather, l_conv / r_conv, conv2, chained tiles) and of the accumulators (plane exponent + weight exponent)
  constexpr int PE = NP == 2 ? PDSE_F16_ACT_EXP : 0;
  const int qG = NP == 2 ? d.qexp[0] : 0, qLC = NP == 2 ? d.qexp[1] : 0, qC2 = NP == 2 ? d.qexp[2] : 0, qNX = NP == 2 ? d.qexp[3] : 0;
  [[maybe_unused]] const float s_in = pow2i(PE), s_G = pow2i(-qG), s_LC = pow2i(-(PE + qLC)), s_C2 = pow2i(-qC2), s_NX = pow2i(-qNX),
                               s_C2out = pow2i(-(PE + qC2)), s_NXout = pow2i(-(PE + qNX)), s_NXin = pow2i(PE + qNX);

  // ---- the LDS image: every weight fragment of the launch by LDS-DMA (1 KB per wave instruction), then the floats
  {
    const uint4* const srcs[8] = {reinterpret_cast<const uint4*>(d.w0), reinterpret_cast<const uint4*>(d.w1),
                                  reinterpret_cast<const uint4*>(d.w2), reinterpret_cast<const uint4*>(d.w3),
                                  reinterpret_cast<const uint4*>(d.wlc), reinterpret_cast<const uint4*>(d.wrc),
                                  reinterpret_cast<const uint4*>(d.wc2), reinterpret_cast<const uint4*>(d.nx_w)};
    const int cnt[8] = {NB * NP, NB * NP, NB1 * NP, NB1 * NP, 2 * NP, 2 * NP, C2 == 64 ? 4 * NP : 0, NXN * 4 * NP};
    constexpr int total = CF::o_f >> 6;
    for (int c = __builtin_amdgcn_readfirstlane(wave); c < total; c += WV) {
      int cc = c;
      const uint4* src = nullptr;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (src == nullptr) {
          if (cc < cnt[k]) src = srcs[k] + cc * 64;
          else cc -= cnt[k];
        }
      }
      glds16(src + lane, img + c * 64);
    }
    float* const fo = reinterpret_cast<float*>(img + CF::o_f);
    for (int s = tid; s < BGLU_FLOATS; s += 64 * WV) {
      const int k = s & 31;
      float v = 0.f;
      if (s < 32) v = d.bias0[(int64_t)b * d.bias_sb + k];
      else if (s < 64) v = d.bias1[(int64_t)b * d.bias_sb + k];
      else if (s < 96) v = (d.bias0_t0 ? d.bias0_t0 : d.bias0)[(int64_t)b * d.bias_sb + k];
      else if (s < 128) v = (d.bias1_t0 ? d.bias1_t0 : d.bias1)[(int64_t)b * d.bias_sb + k];
      else if (s < 160) v = d.blc[k];
      else if (s < 192) v = d.brc[k];
      else if (s < 256) v = (s - 192) < C2 ? d.bc2[s - 192] : 0.f;
      else if (s < 352) {
        const int i = (s - 256) >> 5;
        v = (i < NXN && d.nx_bias[i]) ? d.nx_bias[i][(int64_t)b * d.nx_bias_sb[i] + k] : 0.f;
      } else if (s < 384) v = (C2 == 1) ? d.wc2v[k] : 0.f;
      if constexpr (NP == 2) {   // biases seed accumulators: they carry the accumulator's exponent (exact: powers of two)
        v *= s < 128 ? pow2i(PE + qG) : s < 192 ? pow2i(PE + qLC) : s < 256 ? (C2 == 64 ? pow2i(PE + qC2) : 1.0f)
             : s < 352 ? pow2i(PE + qNX) : pow2i(-(PE + qG));   // wc2v (C2 == 1) multiplies G, which is at the gather exponent
      }
      fo[s] = v;
    }
  }
  __syncthreads();
  const float* const fop = reinterpret_cast<const float*>(img + CF::o_f);
  const int ntiles = (P + 31) >> 5;
  const int nrounds = (ntiles + WV - 1) / WV;

  // ---- per-tile lane state
  struct pos_t {
    int t, j;
    bool valid;
    uint32_t vin;   // lane part of the input address: BYTE offset into the item's hp (planes) / unused (IN4)
  };
  const int Fp = d.hp_Fp;
  auto locate = [&](const int rd, pos_t& ps) {
    const int p = (rd * WV + wave) * 32 + col;
    ps.valid = p < P;
    const int pp = ps.valid ? p : 0;   // branch-free: lanes without a position work on position 0
    ps.t = pp / d.Fout;
    ps.j = pp - ps.t * d.Fout;
    // hp_par (sf_in == 2, validated): bin 2 j + df + f0 lives at ((df + f0) & 1) * Fh + j + ((df + f0) >> 1) - the lane part is j
    ps.vin = (uint32_t)(ps.t * (4 * NP * Fp) + h * (NP * Fp) + (d.hp_par ? ps.j : ps.j * d.sf_in)) << 4;
  };
  const int Fh = (Fp + 1) >> 1;
  // (tap, K block q, plane pl) of a lane = buffer resource of this item's hp + the lane's byte offset (pos_t::vin) + a
  // wave-uniform byte offset in a scalar register
  auto soff_in = [&](const int tap, const int q, const int pl) -> int {
    const int bin0 = d.tap_df[tap] + d.hp_f0;
    return (((d.tap_dt[tap] + d.hp_t0) * 4 + 2 * q) * (NP * Fp) + pl * Fp + (d.hp_par ? (bin0 & 1) * Fh + (bin0 >> 1) : bin0)) << 4;
  };
  // input operands of one tile: planes [tap][q][plane] (or, stage 1, the raw fp32 gathers [slot][4])
  struct in_t {
    uint4 pl[IN4 ? 1 : NT][2][NP];
    float raw[IN4 ? 6 : 1][4];
    unsigned live;
  };
  auto request_tap = [&](const pos_t& ps, in_t& in, const int tap) {
#if defined(BGLU_DIAG) && defined(BGLU_HALF_REQ)   // timing ablation (results wrong): every other tap re-uses its neighbour's registers
    if (tap & 1) {
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) in.pl[tap][q][pl] = in.pl[tap - 1][q][pl];
      return;
    }
#endif
    const __amdgpu_buffer_rsrc_t r_in = make_rsrc(d.hp + (int64_t)b * d.hp_sb, (uint32_t)d.hp_Tp * 4u * NP * (uint32_t)Fp * 16u);
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) in.pl[tap][q][pl] = bload16(r_in, ps.vin, soff_in(tap, q, pl));
  };
  auto request_in4 = [&](const pos_t& ps, in_t& in) {
    // slot s = 2q + w: tap 4q + 2h + w of the ten (2,5) taps, channels (x 0, x 1, x_init 0, x_init 1); taps >= 10: zero
    in.live = 0;
    const __amdgpu_buffer_rsrc_t r_x0 = make_rsrc(d.x0.ptr, 0xfffffffcu), r_x1 = make_rsrc(d.x1.ptr, 0xfffffffcu);
#pragma unroll
    for (int s_ = 0; s_ < 6; ++s_) {
      const int ta = 4 * (s_ >> 1) + (s_ & 1), tb = ta + 2;
      const bool has_b = tb < 10, has_a = ta < 10;
      const int dt = h ? (has_b ? d.tap_dt[tb < 10 ? tb : 0] : 0) : (has_a ? d.tap_dt[ta < 10 ? ta : 0] : 0);
      const int df = h ? (has_b ? d.tap_df[tb < 10 ? tb : 0] : 0) : (has_a ? d.tap_df[ta < 10 ? ta : 0] : 0);
      const bool has = h ? has_b : has_a;
      const int tin = ps.t + dt, fin = ps.j * d.sf_in + df;
      const bool inb = has && ps.valid && fin >= 0 && fin < d.Fin && tin >= 0 && tin < d.Tin;
      if (inb) in.live |= 1u << s_;
      const uint32_t o0 = inb ? (unsigned)((int64_t)b * d.x0.sb + (int64_t)tin * d.x0.st + (int64_t)fin * d.x0.sf) : 0u;
      const uint32_t o1 = inb ? (unsigned)((int64_t)b * d.x1.sb + (int64_t)tin * d.x1.st + (int64_t)fin * d.x1.sf) : 0u;
      in.raw[s_][0] = bload4(r_x0, o0 << 2, 0);
      in.raw[s_][1] = bload4(r_x0, o0 << 2, (int)(d.x0.sc << 2));
      in.raw[s_][2] = bload4(r_x1, o1 << 2, 0);
      in.raw[s_][3] = bload4(r_x1, o1 << 2, (int)(d.x1.sc << 2));
    }
  };

  struct acc_t {
    f32x16 L, R, L1, R1;
  };
  // accumulators start from the gather biases (frame 0 of the composed stage 1 has its own)
  auto seed = [&](const pos_t& ps, acc_t& a) {
    const bool f0 = ps.t == 0;
    a.L = ld16(fop + (f0 ? F_BL0 : F_BL) + 4 * h);
    a.R = ld16(fop + (f0 ? F_BR0 : F_BR) + 4 * h);
    if constexpr (DUAL) {
      a.L1 = a.L;
      a.R1 = a.R;
    }
  };

  // ---- stores.  Plane and skip-half stores are UNCONDITIONAL (lanes without a position write to the dump item B of the
  // target tensor, which is allocated with B + 1 items), so they leave the tail as soon as their values exist and the iteration stays one basic block; only
  // the few fp32 stores of the stages without a dump frame (last decoder stage, encoder stage 5) are predicated.
  const int nFp = d.nx_Fp;
  // dump targets: item B of the tensor (allocated with B + 1 items); all offsets are bytes from the start of the tensor
  const uint32_t item_hp = NXN > 0 ? (uint32_t)(d.nx_hp_sb * 2) : 0u;
  const __amdgpu_buffer_rsrc_t r_nx = make_rsrc(NXN > 0 ? d.nx_hp : nullptr, NXN > 0 ? (uint32_t)(d.B + 1) * item_hp : 0u);
  auto store_planes = [&](const uint4 (&zp)[2][NP], const bool ok, const int t, const int bin) {
    // (frame t, bin) of the next stage's hp: lane half h owns groups g = 2q + h
    const int bi = bin + d.nx_f0;
    const int bpos = d.nx_par ? (bi & 1) * ((nFp + 1) >> 1) + (bi >> 1) : bi;
    const uint32_t o = ok ? (uint32_t)b * item_hp + ((uint32_t)(((t + d.nx_t0) * 4 + h) * (NP * nFp) + bpos) << 4)
                          : (uint32_t)d.B * item_hp + ((uint32_t)(h * (NP * nFp)) << 4);
#if defined(BGLU_DIAG) && defined(BGLU_ONE_STORER)   // timing ablation (results wrong): wave 7 issues the plane stores of all eight waves
    if (wave != 7) return;
#pragma unroll
    for (int k_ = 0; k_ < 8; ++k_)
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int pl = 0; pl < NP; ++pl) bstore16<BGLU_ST_AUX>(zp[q][pl], r_nx, o + (uint32_t)(k_ * 4 * NP * nFp * 16), ((2 * q * NP + pl) * nFp) << 4);
    return;
#endif
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int pl = 0; pl < NP; ++pl) bstore16<BGLU_ST_AUX>(zp[q][pl], r_nx, o, ((2 * q * NP + pl) * nFp) << 4);
  };
  const __amdgpu_buffer_rsrc_t r_sk0 = make_rsrc(NXN > 1 ? d.nx_out[0] : nullptr, NXN > 1 ? (uint32_t)((d.B + 1) * d.nx_sb[0] * 4) : 0u);
  const __amdgpu_buffer_rsrc_t r_sk1 = make_rsrc(NXN > 2 ? d.nx_out[1] : nullptr, NXN > 2 ? (uint32_t)((d.B + 1) * d.nx_sb[1] * 4) : 0u);
  // fp32 skip halves in groups of four channels, [B + 1 (dump item)][8 groups][T][F][4]: accumulator rows 4q..4q+3 of lane
  // half h are channels 8q + 4h..+3 = group 2q + h, 16 contiguous bytes - four 16-byte stores per tile where
  // [B][32][T][F] took sixteen 4-byte ones (a 4-byte and a 16-byte wave access cost the addresser about the same)
  auto store_skip = [&](const f32x16& z, const int i, const pos_t& ps) {
    const int jp = d.skip_Fh ? (ps.j & 1) * d.skip_Fh + (ps.j >> 1) : ps.j;   // bins split by parity (pdse_bglu_desc.skip_Fh)
    const uint32_t o = (uint32_t)(((int64_t)(ps.valid ? b : d.B) * d.nx_sb[i] + (ps.valid ? (int64_t)ps.t * d.nx_st[i] + (int64_t)jp * d.nx_sf[i] : 0) +
                                   (int64_t)h * d.nx_sc[i]) << 2);
    // NP == 2: HBM holds true values - all sixteen are re-scaled into registers of their own BEFORE the first store.  (Scaled four at
    // a time into one temporary, hipcc re-used that temporary right behind each 16-byte store, and on gfx950 a v_pk_mul_f32 issued
    // directly behind a buffer_store_dwordx4 with a scalar offset overwrote dword 1 of the store's data: LLVM models that hazard
    // for stores without a scalar offset only.  tests/test_isa_guards.py checks every kernel for the pattern.)
    f32x16 zs = z;
    if constexpr (NP == 2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) zs[r] = z[r] * s_NXout;
      asm volatile("" : "+v"(zs));
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      bstore16<BGLU_ST_AUX>(make_uint4(__float_as_uint(zs[4 * q]), __float_as_uint(zs[4 * q + 1]), __float_as_uint(zs[4 * q + 2]), __float_as_uint(zs[4 * q + 3])),
               i == 0 ? r_sk0 : r_sk1, o, (int)((2 * q * d.nx_sc[i]) << 2));
  };
  auto stores_masked = [&](const pos_t& ps, const auto& o0, const auto& o1) {
    if (!ps.valid) return;
    const int t = ps.t, j = ps.j;
    const bool two = DUAL && j < d.Fout1;
    float* const po = d.out + ((int64_t)b * d.out_sb + (int64_t)t * d.out_st + (int64_t)j * d.out_sf + d.out_off);
    if constexpr (C2 == 1) {
      if (h == 0) {
        if constexpr (DUAL) {
          const int64_t bin = d.out_sf >> 1;
          if (two && bin == 1) store_pair(po, o0.v, o1.v);
          else {
            po[0] = o0.v;
            if (two) po[bin] = o1.v;
          }
        } else {
          po[0] = o0.v;
        }
      }
    } else if constexpr (NXN == 0) {   // no chained tile: the 64-channel block output itself (encoder stage 5 -> TCM)
#pragma unroll
      for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int r = 0; r < 16; ++r) po[(int64_t)(32 * m2 + 4 * h + PDSE_KR(r)) * d.out_sc] = (m2 ? o0.O1 : o0.O0)[r] * (NP == 2 ? s_C2out : 1.0f);
    }
  };

  // ---- the tail of one output phase as separately schedulable pieces (vocabulary of csrc/bglu_sched.inc).
  // PReLU slope <= 1 (validated at launch): PReLU(v) = max(v, slope v).
  const float slope = d.slope;
  struct ph_t {
    f32x16 L, R, mL, mR, G, O0, O1, Z0, Z1, Z2;
    uint4 lp[2][NP], rp[2][NP], gp[2][NP], yp[2][2][NP], zp[2][NP];
    float v;
  };
  auto split_half = [&](const f32x16& X, const int s_, uint4 (&p)[NP], const float sc = 1.0f) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = X[8 * s_ + j];
    split8p<NP>(x, p, sc);
  };
  // addend of chained tile 0 (decoders: the encoder's skip half of this conv1; its bias is part of it).  Lanes without a
  // valid position (or without an odd bin) read a position that exists.
  const __amdgpu_buffer_rsrc_t r_add = make_rsrc((DUAL && NXN > 0) ? d.nx_add : nullptr, (DUAL && NXN > 0) ? (uint32_t)(d.B * d.add_sb * 4) : 0u);
  auto zseed = [&](const pos_t& ps, const int ph, f32x16& z) {
    const bool two = ph == 0 || ps.j < d.Fout1;
    const int bin0 = 2 * ps.j + (two ? ph : 0);
    const int bin = d.skip_Fh ? (two ? ph : 0) * d.skip_Fh + ps.j : bin0;   // parity-split bins: phase ph reads a contiguous run
    const uint32_t o = (uint32_t)(((int64_t)b * d.add_sb + (int64_t)ps.t * d.add_st + (int64_t)bin * d.add_sf + (int64_t)h * d.add_sc) << 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) {   // groups of four channels (store_skip's layout): four 16-byte loads
      const uint4 v = bload16(r_add, o, (int)((2 * q * d.add_sc) << 2));
      z[4 * q] = __uint_as_float(v.x), z[4 * q + 1] = __uint_as_float(v.y), z[4 * q + 2] = __uint_as_float(v.z), z[4 * q + 3] = __uint_as_float(v.w);
      if constexpr (NP == 2) z[4 * q] *= s_NXin, z[4 * q + 1] *= s_NXin, z[4 * q + 2] *= s_NXin, z[4 * q + 3] *= s_NXin;   // seeds an accumulator
    }
  };

#define FRAG(buf, ptr)                                         \
  {                                                            \
    _Pragma("unroll") for (int pl_ = 0; pl_ < NP; ++pl_) fr[buf][pl_] = (ptr)[64 * pl_]; \
  }
#if defined(BGLU_DIAG) && defined(BGLU_NO_MM)   // timing ablation: no matrix instructions in the loop (results wrong)
#define MM(buf, acc_, bp_) acc_[0] += __uint_as_float(fr[buf][0].x ^ bp_[0].x)
#else
#define MM(buf, acc_, bp_) acc_ = plane_mma<NP>(fr[buf], bp_, acc_)
#endif
#define GL(tap, q) (img + CF::o_gL + ((tap) * 2 + (q)) * BS + lane)
#define GR(tap, q) (img + CF::o_gR + ((tap) * 2 + (q)) * BS + lane)
#define GL1(rk, q) (img + CF::o_gL1 + ((rk) * 2 + (q)) * BS + lane)
#define GR1(rk, q) (img + CF::o_gR1 + ((rk) * 2 + (q)) * BS + lane)
#define GLI(q) (img + CF::o_gL + (q) * BS + lane)
#define GRI(q) (img + CF::o_gR + (q) * BS + lane)
#define LCW(s_) (img + CF::o_lc + (s_) * BS + lane)
#define RCW(s_) (img + CF::o_rc + (s_) * BS + lane)
#define C2W(m2, s_) (img + CF::o_c2 + ((m2) * 2 + (s_)) * BS + lane)
#define NXW(i, m2, s_) (img + CF::o_nx + ((i) * 4 + (m2) * 2 + (s_)) * BS + lane)
#define V_SL(S, s_)                                      \
  {                                                      \
    if ((s_) == 0) S.mL = ld16(fop + F_BLC + 4 * h);     \
    split_half(S.L, s_, S.lp[s_], s_G);                  \
  }
#define V_SR(S, s_)                                      \
  {                                                      \
    if ((s_) == 0) S.mR = ld16(fop + F_BRC + 4 * h);     \
    split_half(S.R, s_, S.rp[s_], s_G);                  \
  }
#define V_SG(S, lo, hi)                                                                                       \
  {                                                                                                           \
    _Pragma("unroll") for (int r = lo; r < hi; ++r) S.G[r] = S.L[r] * sigm2(NP == 2 ? S.mR[r] * s_LC : S.mR[r]) + S.R[r] * sigm2(NP == 2 ? S.mL[r] * s_LC : S.mL[r]); \
  }
#define V_SPG(S, s_)                                          \
  {                                                           \
    if ((s_) == 0) {                                          \
      S.O0 = ld16(fop + F_BC2 + 4 * h);                       \
      S.O1 = ld16(fop + F_BC2 + 32 + 4 * h);                  \
    }                                                         \
    split_half(S.G, s_, S.gp[s_], s_G);                       \
  }
#define V_PR(S, m2)                                                                                        \
  {                                                                                                        \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) S.O##m2[r] = vmax(S.O##m2[r], slope * S.O##m2[r]);       \
  }
#define V_SY(S, m2, s_)                                                     \
  {                                                                         \
    if ((m2) == 0 && (s_) == 0) {                                           \
      if constexpr (!DUAL && NXN > 0) S.Z0 = ld16(fop + F_NXB + 4 * h);     \
      if constexpr (NXN > 1) S.Z1 = ld16(fop + F_NXB + 32 + 4 * h);         \
      if constexpr (NXN > 2) S.Z2 = ld16(fop + F_NXB + 64 + 4 * h);         \
    }                                                                       \
    split_half(S.O##m2, s_, S.yp[m2][s_], s_C2);                            \
  }
#define V_ZSEED(S, ph) zseed(pc, ph, S.Z0);
#define V_SZ(S, s_) split_half(S.Z0, s_, S.zp[s_], s_NX);
#define V_ST0(S, ph)                                                                                   \
  {                                                                                                    \
    if constexpr (DUAL) {                                                                              \
      store_planes(S.zp, pc.valid && ((ph) == 0 || pc.j < d.Fout1), pc.t, 2 * pc.j + (ph));            \
    } else {                                                                                           \
      store_planes(S.zp, pc.valid, pc.t, pc.j);                                                        \
      if (d.nx_row0) { /* uniform: the explicit pad frame of the next encoder stage = the folded bias */ \
        uint4 bp_[2][NP];                                                                              \
        split_tile<NP>(ld16(fop + F_NXB + 4 * h), bp_, s_NX);                                            \
        store_planes(bp_, pc.valid && pc.t == 0, -1, pc.j);                                            \
      }                                                                                                \
    }                                                                                                  \
  }
#define V_STSKIP(S, i) store_skip(S.Z##i, (i)-1, pc);
#define V_DOT(S, ph)                                                              \
  {                                                                               \
    const f32x16 vw_ = ld16(fop + F_WC2V + 4 * h);                                \
    float part_ = 0.f;                                                            \
    _Pragma("unroll") for (int r = 0; r < 16; ++r) part_ += vw_[r] * S.G[r];      \
    const float v_ = part_ + __shfl_xor(part_, 32) + fop[F_BC2];                  \
    S.v = vmax(v_, slope * v_);                                                   \
  }
#define V_KEEP(S)
#define V_KSPLIT(q)                                                                                                               \
  {                                                                                                                               \
    float x_[8];                                                                                                                  \
    _Pragma("unroll") for (int e = 0; e < 8; ++e) x_[e] = ((in.live >> (2 * (q) + (e >> 2))) & 1u) ? in.raw[2 * (q) + (e >> 2)][e & 3] : 0.f; \
    split8p<NP>(x_, kb[q], s_in);                                                                                                 \
  }
#define REQ(tap) request_tap(p_req, in, tap);
#define REQ_CUR(tap) request_tap(pc, in, tap);
#define REQ_IN4() request_in4(p_req, in);
#define V_TAKE()          \
  {                       \
    SA.L = acc.L;         \
    SA.R = acc.R;         \
    if constexpr (DUAL) { \
      SB.L = acc.L1;      \
      SB.R = acc.R1;      \
    }                     \
  }
#ifndef BGLU_VPER
#define BGLU_VPER 9   // vector instructions placed behind each MFMA of a slot (tuning: tools/time_bglu.py with PDSE_LIB builds)
#endif
#define FRAG_FENCE __builtin_amdgcn_sched_barrier(0);
#if defined(BGLU_DIAG) && defined(BGLU_NO_V)
#undef V_SL
#undef V_SR
#undef V_SG
#undef V_SPG
#undef V_PR
#undef V_SY
#undef V_SZ
#undef V_ST0
#undef V_STSKIP
#undef V_DOT
#undef V_KSPLIT
#define V_SL(S, s_)
#define V_SR(S, s_)
#define V_SG(S, lo, hi)
#define V_SPG(S, s_)
#define V_PR(S, m2)
#define V_SY(S, m2, s_)
#define V_SZ(S, s_)
#undef V_ZSEED
#define V_ZSEED(S, ph)
#define V_ST0(S, ph)
#define V_STSKIP(S, i)
#define V_DOT(S, ph)
#define V_KSPLIT(q)
#endif
#if defined(BGLU_DIAG) && defined(BGLU_NO_ST)   // timing ablation: no plane / skip stores
#undef V_ST0
#undef V_STSKIP
#define V_ST0(S, ph) if (d.slope == 12345.f) { store_planes(S.zp, pc.valid, pc.t, DUAL ? 2 * pc.j + (ph) : pc.j); }
#define V_STSKIP(S, i) if (d.slope == 12345.f) { store_skip(S.Z##i, (i)-1, pc); }
#endif
#if defined(BGLU_DIAG) && defined(BGLU_NO_ZSEED)   // timing ablation: no addend loads
#undef V_ZSEED
#define V_ZSEED(S, ph)
#endif
#if defined(BGLU_DIAG) && defined(BGLU_NO_REQ)
#undef REQ
#undef REQ_CUR
#undef REQ_IN4
#define REQ(tap)
#define REQ_CUR(tap)
#define REQ_IN4()
#endif
#if defined(BGLU_DIAG) && defined(BGLU_NO_FRAG)
#undef FRAG
#define FRAG(buf, ptr)
#endif
#define SLOT_BEGIN {
  // one slot: the LDS reads of the next slot's fragments first, then each MFMA followed by the vector instructions
  // that fit its shadow; nothing crosses the slot boundary
#define SLOT_END(hasm, hasv)                                                       \
  if constexpr (NP == 3) {                                                         \
    _Pragma("unroll") for (int g_ = 0; g_ < 6; ++g_) {                             \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                           \
      __builtin_amdgcn_sched_group_barrier(0x002, BGLU_VPER, 0);                   \
    }                                                                              \
  } else if constexpr (NP == 2) {                                                  \
    _Pragma("unroll") for (int g_ = 0; g_ < 3; ++g_) {                             \
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                           \
      __builtin_amdgcn_sched_group_barrier(0x002, BGLU_VPER, 0);                   \
    }                                                                              \
  } else {                                                                         \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                             \
  }                                                                                \
  __builtin_amdgcn_sched_barrier(0);                                               \
  DG_SLOT(__COUNTER__)                                                             \
  }
#if defined(BGLU_DIAG) && defined(BGLU_SLOTSTAMP)
  // per-slot shader-clock stamps (s_memtime waits for lgkmcnt(0): the slot's own LDS reads have been consumed by then)
  unsigned dg_slot[96];
#pragma unroll
  for (int k_ = 0; k_ < 96; ++k_) dg_slot[k_] = 0;
  unsigned long long dg_prev = 0;
  unsigned dg_tiles = 0;
#define DG_SLOT(c_)                                                                 \
  {                                                                                 \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                     \
    dg_slot[(c_) - dg_base - 1] += (unsigned)(t_ - dg_prev);                        \
    dg_prev = t_;                                                                   \
  }
#else
#define DG_SLOT(c_)
#endif

  // ---- this workgroup's rounds r_k = blockIdx.x + k gridDim.x: K loop, then tail, per tile; the first two taps of the next
  // tile are in flight during the tail
  const int stride = gridDim.x;
  int rd = blockIdx.x;
  if (rd >= nrounds) return;
  pos_t pc, pn;
  in_t in;
  acc_t acc;
  locate(rd, pc);
  if constexpr (IN4) {
    request_in4(pc, in);
  } else {
    request_tap(pc, in, 0);
    request_tap(pc, in, 1);
  }
  constexpr int SCHED = 10 + (IN4 ? 5 : (DUAL ? (C2 == 64 ? 1 : 2) : (NXN == 3 ? 3 : 4)));
  while (true) {
    locate(rd + stride, pn);
    const pos_t& p_req = pn;
    ph_t SA, SB;
    uint4 fr[2][NP];
    uint4 kb[IN4 ? 3 : 1][NP];
    seed(pc, acc);
    __builtin_amdgcn_sched_barrier(0);
#if defined(BGLU_DIAG) && defined(BGLU_SLOTSTAMP)
    dg_prev = __builtin_amdgcn_s_memtime();
    ++dg_tiles;
#endif
    if constexpr (SCHED == 11) {
#define BGLU_SCHED 11
    [[maybe_unused]] constexpr int dg_base = __COUNTER__;
#include "bglu_sched.inc"
#undef BGLU_SCHED
    } else if constexpr (SCHED == 12) {
#define BGLU_SCHED 12
    [[maybe_unused]] constexpr int dg_base = __COUNTER__;
#include "bglu_sched.inc"
#undef BGLU_SCHED
    } else if constexpr (SCHED == 13) {
#define BGLU_SCHED 13
    [[maybe_unused]] constexpr int dg_base = __COUNTER__;
#include "bglu_sched.inc"
#undef BGLU_SCHED
    } else if constexpr (SCHED == 14) {
#define BGLU_SCHED 14
    [[maybe_unused]] constexpr int dg_base = __COUNTER__;
#include "bglu_sched.inc"
#undef BGLU_SCHED
    } else {
#define BGLU_SCHED 15
    [[maybe_unused]] constexpr int dg_base = __COUNTER__;
#include "bglu_sched.inc"
#undef BGLU_SCHED
    }
    if constexpr (C2 == 1 || NXN == 0) stores_masked(pc, SA, SB);
    rd += stride;
    if (rd >= nrounds) break;
    pc = pn;
  }
#if defined(BGLU_DIAG) && defined(BGLU_SLOTSTAMP)
  if (lane == 0) {
#pragma unroll
    for (int k_ = 0; k_ < 96; ++k_)
      if (dg_slot[k_]) atomicAdd(&g_bglu_slots[k_], (unsigned long long)dg_slot[k_]);
    atomicAdd(&g_bglu_slots[96], (unsigned long long)dg_tiles);
  }
#endif
}

// fp32 [B, 32, T, F] -> planes (the first decoder stage's standalone conv1 output)
template <int NP>
__global__ __launch_bounds__(256) void planes_kernel(const pdse_planes_desc d) {
  const int64_t n = (int64_t)d.B * d.T * d.F * 4;   // one thread per (b, t, g, f): 8 channels
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int f = (int)(i % d.F);
  const int g = (int)((i / d.F) & 3);
  const int64_t bt = i / ((int64_t)4 * d.F);
  const int t = (int)(bt % d.T), b = (int)(bt / d.T);
  const int q = g >> 1, h = g & 1;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = 16 * q + 8 * (e >> 2) + 4 * h + (e & 3);
    x[e] = d.in[(int64_t)b * d.in_sb + (int64_t)c * d.in_sc + (int64_t)t * d.in_st + (int64_t)f * d.in_sf];
  }
  uint4 p[NP];
  split8p<NP>(x, p, NP == 2 ? pow2i(PDSE_F16_ACT_EXP) : 1.0f);
  uint4* const base = reinterpret_cast<uint4*>(d.hp + (int64_t)b * d.hp_sb) + ((int64_t)(t + d.hp_t0) * 4 + g) * (NP * d.hp_Fp) + f + d.hp_f0;
#pragma unroll
  for (int pl = 0; pl < NP; ++pl) base[pl * d.hp_Fp] = p[pl];
}

// The same planes, of a 1x1 convolution computed here (pdse_planes_desc.w; F == 4): a wave owns 8 frames x 4 bins = 32 positions and all
// 32 output channels on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32, one fmaf chain in k order per output - the
// arithmetic of the gather-GEMM launch this replaces); the accumulator registers of lane half h ARE plane groups h and 2 + h, so the
// split and the 64-byte-per-frame plane stores are those of the block kernels' tails.  (As a vector kernel - one thread per position,
// wave-uniform weights from scalar loads or broadcast LDS reads - the launch took 52-55 us: 256 dependent scalar loads, or an LDS
// array busy with 1024 broadcast reads, per thread.)
template <int NP>
__global__ __launch_bounds__(256) void planes_conv_kernel(const pdse_planes_desc d) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, h = lane >> 5;
  const int di = blockIdx.z, b = blockIdx.y;
  const int t = (blockIdx.x * 4 + wave) * 8 + (col >> 2), f = col & 3;
  const bool live = t < d.T;
  const int64_t xo = (int64_t)b * d.in_sb + (int64_t)(live ? t : d.T - 1) * d.in_st + (int64_t)f * d.in_sf;
  const float* const w = d.w[di] + col;                 // A operand: lane (row = output channel, k = 2 i + h)
  f32x16 acc;
  if (d.bias[di]) {
    acc = ld16(d.bias[di] + (int64_t)b * d.bias_sb + 4 * h);
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  }
  const int K = d.cin0 + d.cin1;                        // multiples of 32 per source (validated)
  float av[2][16], bv[2][16];
  auto request = [&](const int k0, const int s_) {      // the 32 loads of a chunk of 32 input channels
    const float* const src = (k0 < d.cin0 ? d.in + (int64_t)k0 * d.in_sc : d.in1 + (int64_t)(k0 - d.cin0) * d.in_sc) + xo;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      av[s_][i] = w[(k0 + 2 * i + h) * 32];
      bv[s_][i] = src[(int64_t)(2 * i + h) * d.in_sc];
    }
  };
  request(0, 0);
  for (int k0 = 0; k0 < K; k0 += 64) {                  // two chunks per iteration: the next chunk's loads fly under this chunk's MFMAs
    if (k0 + 32 < K) request(k0 + 32, 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][i], bv[0][i], acc, 0, 0, 0);
    if (k0 + 32 >= K) break;
    if (k0 + 64 < K) request(k0 + 64, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][i], bv[1][i], acc, 0, 0, 0);
  }
  if (!live) return;
  uint4 p[2][NP];
  split_tile<NP>(acc, p, NP == 2 ? pow2i(PDSE_F16_ACT_EXP) : 1.0f);
  uint4* const base = reinterpret_cast<uint4*>((di ? d.hp1 : d.hp) + (int64_t)b * d.hp_sb) + ((int64_t)(t + d.hp_t0) * 4 + h) * (NP * d.hp_Fp) + f + d.hp_f0;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int pl = 0; pl < NP; ++pl) base[(2 * q * NP + pl) * d.hp_Fp] = p[q][pl];
}

template <int NT, int P1MASK, int C2, int NXN, bool IN4, int NP>
int launch(const pdse_bglu_desc* d, hipStream_t s) {
  using CF = bglu_cfg<NT, P1MASK, C2, NXN, IN4, NP>;
  const int P = d->Tout * d->Fout;
  const int rounds = (((P + 31) >> 5) + CF::WV - 1) / CF::WV;
  static const int wgs = PDSE_DIAG_ENV("PDSE_BGLU_WGS") ? atoi(PDSE_DIAG_ENV("PDSE_BGLU_WGS")) : 256;
  int gx = (wgs + d->B - 1) / d->B;
  if (gx > rounds) gx = rounds;
  if (gx < 1) gx = 1;
  if (CF::lds_bytes > 160 * 1024) {
    pdse_set_error("bglu: LDS image too large");
    return 1;
  }
  const void* fn = (const void*)bglu_kernel<NT, P1MASK, C2, NXN, IN4, NP>;
  static unsigned long long attr_mask = 0;   // per instantiation and device
  if (pdse_lds_attr(fn, &attr_mask, "bglu lds attribute")) return 1;
#ifdef BGLU_DIAG
  static unsigned long long zs[97];
  for (int k = 0; k < 97; ++k) zs[k] = 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bglu_slots), zs, sizeof(zs));
#endif
  hipLaunchKernelGGL((bglu_kernel<NT, P1MASK, C2, NXN, IN4, NP>), dim3(gx, d->B, 1), dim3(64 * CF::WV), CF::lds_bytes, s, *d);
#ifdef BGLU_DIAG
  (void)hipStreamSynchronize(s);
  (void)hipMemcpyFromSymbol(zs, HIP_SYMBOL(g_bglu_slots), sizeof(zs));
  if (zs[96]) {
    fprintf(stderr, "bglu slots NT %d P1 %d C2 %d NXN %d NP %d (cycles per slot and tile, %llu tiles):", NT, P1MASK, C2, NXN, NP, zs[96]);
    double tot = 0;
    for (int k = 0; k < 96; ++k)
      if (zs[k]) {
        fprintf(stderr, " %d:%.0f", k, (double)zs[k] / (double)zs[96]);
        tot += (double)zs[k] / (double)zs[96];
      }
    fprintf(stderr, " | sum %.0f\n", tot);
  }
#endif
  return pdse_check_launch("bglu");
}

template <int NP>
int dispatch(const pdse_bglu_desc* d, hipStream_t s) {
  if (d->x0.ptr) {   // encoder stage 1
    if (d->nx_n == 3) return launch<10, 0, 64, 3, true, NP>(d, s);
  } else if (d->p1mask) {
    if (d->ntaps == 4 && d->p1mask == 5 && d->C2 == 64 && d->nx_n == 1) return launch<4, 5, 64, 1, false, NP>(d, s);
    if (d->ntaps == 6 && d->p1mask == 27 && d->C2 == 1 && d->nx_n == 0) return launch<6, 27, 1, 0, false, NP>(d, s);
  } else {
    if (d->ntaps == 6 && d->C2 == 64 && d->nx_n == 3) return launch<6, 0, 64, 3, false, NP>(d, s);
    if (d->ntaps == 6 && d->C2 == 64 && d->nx_n == 0) return launch<6, 0, 64, 0, false, NP>(d, s);
  }
  pdse_set_error("bglu: no instantiation for this (taps, phases, C2, chained tiles)");
  return 1;
}

}   // namespace

int pdse_bglu_launch(const pdse_bglu_desc* d, hipStream_t s) {
  if (!d || !d->w0 || !d->w1 || !d->wlc || !d->wrc || !d->bias0 || !d->bias1 || !d->blc || !d->brc || !d->bc2) {
    pdse_set_error("bglu: null operand");
    return 1;
  }
  if (!(d->slope <= 1.0f)) {
    pdse_set_error("bglu: PReLU slope must be <= 1 (max form); use the korder 2 kernels otherwise");
    return 1;
  }
  if (d->B < 1 || d->Tout < 1 || d->Fout < 1 || !(d->np == 3 || d->np == 2 || d->np == 1) || !(d->C2 == 64 || d->C2 == 1) || d->nx_n < 0 ||
      d->nx_n > 3 || d->ntaps < 1 || d->ntaps > 10) {
    pdse_set_error("bglu: bad geometry (np in {1, 2, 3}, C2 in {64, 1}, nx_n <= 3, ntaps <= 10)");
    return 1;
  }
  if (d->p1mask && d->Fout1 > d->Fout) {
    pdse_set_error("bglu: Fout1 > Fout");
    return 1;
  }
  if ((d->C2 == 64 && !d->wc2) || (d->C2 == 1 && (!d->wc2v || !d->out)) || (d->C2 == 64 && d->nx_n == 0 && !d->out) || (d->nx_n > 0 && (!d->nx_w || !d->nx_hp)) ||
      (d->nx_n > 1 && !d->nx_out[0]) || (d->nx_n > 2 && !d->nx_out[1]) || (d->p1mask && (!d->w2 || !d->w3))) {
    pdse_set_error("bglu: an operand of the selected form is missing");
    return 1;
  }
  if (!d->x0.ptr) {
    // plane input: every tap must stay inside the margins of hp, and the lane offsets must fit 32 bits
    if (!d->hp || d->hp_Fp < 1) {
      pdse_set_error("bglu: null hp");
      return 1;
    }
    const long long frame = 4ll * d->np * d->hp_Fp;
    if ((long long)d->hp_Tp * frame * 16 >= (1ll << 32)) {
      pdse_set_error("bglu: hp item exceeds 32-bit lane offsets");
      return 1;
    }
    if (d->hp_par && (d->hp_par != 1 || d->sf_in != 2)) {
      pdse_set_error("bglu: parity-split input planes (hp_par = 1) are for stride-2 taps (sf_in == 2)");
      return 1;
    }
    for (int i = 0; i < d->ntaps; ++i) {
      const int tlo = d->tap_dt[i] + d->hp_t0, thi = d->Tout - 1 + d->tap_dt[i] + d->hp_t0;
      const int flo = d->tap_df[i] + d->hp_f0, fhi = (d->Fout - 1) * d->sf_in + d->tap_df[i] + d->hp_f0;
      if (tlo < 0 || thi >= d->hp_Tp || flo < 0 || fhi >= d->hp_Fp) {
        pdse_set_error("bglu: a tap leaves the margins of hp");
        return 1;
      }
    }
  } else if (!d->x1.ptr || d->ntaps != 10 || d->p1mask || (long long)d->B * d->x0.sb * 4 >= (1ll << 32) || (long long)d->B * d->x1.sb * 4 >= (1ll << 32)) {
    pdse_set_error("bglu: encoder stage 1 needs two fp32 sources and the ten (2,5) taps");
    return 1;
  }
  if (d->nx_n > 0) {
    if (d->nx_items < d->B + 1) {
      pdse_set_error("bglu: nx_hp / nx_out need B + 1 allocated items (nx_items): item B is the dump target of lanes beyond the last position");
      return 1;
    }
    const long long frame = 4ll * d->np * d->nx_Fp;
    int maxbin = d->Fout - 1;
    if (d->p1mask) maxbin = 2 * (d->Fout - 1) > 2 * (d->Fout1 - 1) + 1 ? 2 * (d->Fout - 1) : 2 * (d->Fout1 - 1) + 1;
    if (d->nx_t0 + d->Tout > d->nx_Tp || d->nx_t0 - (d->nx_row0 ? 1 : 0) < 0 || d->nx_f0 < 0 || maxbin + d->nx_f0 >= d->nx_Fp ||
        (long long)d->nx_Tp * frame >= (1ll << 31) || (d->p1mask != 0) != (d->nx_add != nullptr) ||
        (long long)(d->B + 1) * d->nx_hp_sb * 2 >= (1ll << 32)) {
      pdse_set_error("bglu: the chained tile does not fit its hp tensor");
      return 1;
    }
    if (d->nx_add && (long long)d->B * d->add_sb * 4 >= (1ll << 32)) {
      pdse_set_error("bglu: addend exceeds 32-bit lane offsets");
      return 1;
    }
    auto c4_ok = [](const void* p, const int64_t sb, const int64_t sc, const int64_t st, const int64_t sf) {
      return ((sb | sc | st | sf) & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    };
    if (d->nx_add && !c4_ok(d->nx_add, d->add_sb, d->add_sc, d->add_st, d->add_sf)) {
      pdse_set_error("bglu: the addend is kept in groups of four channels: strides in multiples of 4 floats, 16-byte aligned base");
      return 1;
    }
    for (int i = 0; i + 1 < d->nx_n; ++i) {
      if ((long long)(d->B + 1) * d->nx_sb[i] * 4 >= (1ll << 32)) {
        pdse_set_error("bglu: skip tensor exceeds 32-bit lane offsets");
        return 1;
      }
      if (!c4_ok(d->nx_out[i], d->nx_sb[i], d->nx_sc[i], d->nx_st[i], d->nx_sf[i])) {
        pdse_set_error("bglu: skip tensors are kept in groups of four channels: strides in multiples of 4 floats, 16-byte aligned base");
        return 1;
      }
    }
  }
  if (d->np == 2) {
    for (int i = 0; i < 4; ++i)
      if (d->qexp[i] < -40 || d->qexp[i] > 40) {
        pdse_set_error("bglu: qexp (f16x2 weight exponents) out of range");
        return 1;
      }
    return dispatch<2>(d, s);
  }
  return d->np == 3 ? dispatch<3>(d, s) : dispatch<1>(d, s);
}

int pdse_bglu_set_form(int form) {
  static int cur = -1;   // the library holds one form (8 waves): -1 and 0 both name it
  if (form < -1 || form > 0) return -2;
  const int prev = cur;
  cur = form;
  return prev;
}

int pdse_planes_launch(const pdse_planes_desc* d, hipStream_t s) {
  if (!d || !d->in || !d->hp || d->B < 1 || d->T < 1 || d->F < 1 || !(d->np == 3 || d->np == 2 || d->np == 1)) {
    pdse_set_error("planes: bad argument");
    return 1;
  }
  if (d->hp_t0 < 0 || d->hp_f0 < 0 || d->hp_t0 + d->T > d->hp_Tp || d->hp_f0 + d->F > d->hp_Fp) {
    pdse_set_error("planes: the tensor does not fit hp");
    return 1;
  }
  if (d->w[0]) {   // the planes of a 1x1 convolution computed here
    if (d->nd < 1 || d->nd > 2 || d->cin0 < 32 || d->cin1 < 0 || (d->cin0 & 31) || (d->cin1 & 31) || d->cin0 + d->cin1 > 128 || (d->cin1 > 0 && !d->in1) || (d->nd == 2 && (!d->w[1] || !d->hp1)) ||
        d->B > 65535) {
      pdse_set_error("planes: the convolution form takes 1 or 2 weight sets, up to 128 input channels (multiples of 32) over one or two sources");
      return 1;
    }
    if (d->F != 4 || (reinterpret_cast<uintptr_t>(d->bias[0]) & 15) || (reinterpret_cast<uintptr_t>(d->bias[1]) & 15) || (d->bias_sb & 3)) {
      pdse_set_error("planes: the convolution form is built for F == 4 (decoder stage 5) and 16-byte aligned bias rows");
      return 1;
    }
    const dim3 cgrid((unsigned)((d->T + 31) / 32), (unsigned)d->B, (unsigned)d->nd), cblock(256);
    if (d->np == 3) hipLaunchKernelGGL(planes_conv_kernel<3>, cgrid, cblock, 0, s, *d);
    else if (d->np == 2) hipLaunchKernelGGL(planes_conv_kernel<2>, cgrid, cblock, 0, s, *d);
    else hipLaunchKernelGGL(planes_conv_kernel<1>, cgrid, cblock, 0, s, *d);
    return pdse_check_launch("planes (conv)");
  }
  const int64_t n = (int64_t)d->B * d->T * d->F * 4;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (d->np == 3) hipLaunchKernelGGL(planes_kernel<3>, grid, block, 0, s, *d);
  else if (d->np == 2) hipLaunchKernelGGL(planes_kernel<2>, grid, block, 0, s, *d);
  else hipLaunchKernelGGL(planes_kernel<1>, grid, block, 0, s, *d);
  return pdse_check_launch("planes");
}
