// planes.h — the split-operand arithmetic of every matrix-core kernel, defined once: an fp32 value is carried as NP operand
// planes and a product is a fixed sequence of plane products on the matrix cores with fp32 accumulation.
//   NP = 3: exact three-way bf16 split, six products (fp32-equivalent);
//   NP = 2: f16x2 - fp16 hi + lo of the power-of-two scaled value, three products;
//   NP = 1: plain bf16 operands (round to nearest even), one product (the opt-in bf16 mode; its own tolerance).
// Which cross terms are kept and their order (plane_terms), how a value is split (split_planes) and how bf16 is rounded
// (pack_bf16_rne) are what the tolerances of the tests rest on.  Included through gconv_common.h.
#ifndef PDSE_PLANES_H
#define PDSE_PLANES_H
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------------------------
// Split-bf16 operands (csrc/gconv3.hip, packing.split_bf16x3): an fp32 value is the exact sum of three bf16 numbers
// (8 + 8 + 8 significand bits, by truncation), and a product is evaluated as its six leading cross terms on the bf16
// matrix cores with fp32 accumulation.  Fragments are 8 bf16 per lane (one uint4) per plane.
// ---------------------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma_bf16(const uint4& a, const uint4& b, const f32x16 c) {
  union { uint4 u; bf16x8 v; } A, B;
  A.u = a;
  B.u = b;
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(A.v, B.v, c, 0, 0, 0);
}

// x[0..7] -> three planes of 8 bf16 (element j in the low / high half of dword j >> 1), x == p1 + p2 + p3 exactly.
// 11 VALU instructions per pair of values: two masked residuals each, and one v_perm_b32 per plane picks the high
// halves of the pair (the bf16 of a truncation IS the high half, masked or not); 15 per pair with shift / or packing.
// Two thirds of the VALU instructions of a block kernel's tail are this function, yet a quarter fewer of them moved
// the tail by 5 % only (22.4k -> 21.1k cycles per round, PDSE_S3_TRACE): the tail is a serial chain of split ->
// fragment read -> six dependent MFMAs, not an issue-bound stream.
__device__ __forceinline__ void split8(const float (&x)[8], uint4& p1, uint4& p2, uint4& p3) {
#ifdef PDSE_ABLATE_SPLIT   // diagnostic build only (wrong results): the cost of the splits
  p1 = make_uint4(__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3]));
  p2 = make_uint4(__float_as_uint(x[4]), __float_as_uint(x[5]), __float_as_uint(x[6]), __float_as_uint(x[7]));
  p3 = make_uint4(p1.x ^ p2.x, p1.y ^ p2.y, p1.z ^ p2.z, p1.w ^ p2.w);
  return;
#endif
  uint32_t q1[4], q2[4], q3[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = x[2 * i], b = x[2 * i + 1];
    const float ra = a - __uint_as_float(__float_as_uint(a) & 0xffff0000u);
    const float rb = b - __uint_as_float(__float_as_uint(b) & 0xffff0000u);
    const float sa = ra - __uint_as_float(__float_as_uint(ra) & 0xffff0000u);
    const float sb = rb - __uint_as_float(__float_as_uint(rb) & 0xffff0000u);
    q1[i] = __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
    q2[i] = __builtin_amdgcn_perm(__float_as_uint(rb), __float_as_uint(ra), 0x07060302u);
    q3[i] = __builtin_amdgcn_perm(__float_as_uint(sb), __float_as_uint(sa), 0x07060302u);
  }
  p1 = make_uint4(q1[0], q1[1], q1[2], q1[3]);
  p2 = make_uint4(q2[0], q2[1], q2[2], q2[3]);
  p3 = make_uint4(q3[0], q3[1], q3[2], q3[3]);
}

// four values -> their three bf16 planes, 8 bytes each (element i in half i & 1 of dword i >> 1)
__device__ __forceinline__ void split4(const float (&x)[4], uint2& p1, uint2& p2, uint2& p3) {
  uint32_t q[3][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const float a = x[2 * i], b = x[2 * i + 1];
    const uint32_t a1 = __float_as_uint(a) & 0xffff0000u, b1 = __float_as_uint(b) & 0xffff0000u;
    const float ra = a - __uint_as_float(a1), rb = b - __uint_as_float(b1);
    const uint32_t a2 = __float_as_uint(ra) & 0xffff0000u, b2 = __float_as_uint(rb) & 0xffff0000u;
    const float sa = ra - __uint_as_float(a2), sb = rb - __uint_as_float(b2);
    q[0][i] = (a1 >> 16) | b1;
    q[1][i] = (a2 >> 16) | b2;
    q[2][i] = (__float_as_uint(sa) >> 16) | (__float_as_uint(sb) & 0xffff0000u);
  }
  p1 = make_uint2(q[0][0], q[0][1]);
  p2 = make_uint2(q[1][0], q[1][1]);
  p3 = make_uint2(q[2][0], q[2][1]);
}

// ---------------------------------------------------------------------------------------------------------------
// Split-f16 operands (round 4; include/pdse.h "f16x2"): an fp32 value x, scaled by a power of two into the fp16 range,
// is carried as hi = RN16(x), lo = RN16(x - hi): 11 + 11 significand bits and the sign of lo, |x - hi - lo| <= 2^-23 |x|
// (half an fp32 ulp at worst) while lo is a normal fp16, i.e. for |x| >= 2^-2 in scaled units; below that the absolute
// error is <= 2^-25 of the scaled unit.  A product is its three leading cross terms (a1 b1, a1 b2, a2 b1; what is dropped
// is a2 b2 <= 2^-22 |a b|) on the f16 matrix cores with fp32 accumulation: half the matrix instructions and two thirds
// of the operand bytes of the three-plane bf16 split.  Every product of two fp16 numbers is exact in fp32.
// Scaling is by exact powers of two: activations by 2^PDSE_F16_ACT_EXP, every weight matrix by its own 2^q chosen on
// the host (packing.f16_wexp); accumulators therefore hold (true value) * 2^(P + q) and are re-scaled where they are
// split for the next contraction (one multiply, merged with the split's own).
// ---------------------------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x16 mfma_f16(const uint4& a, const uint4& b, const f32x16 c) {
  union { uint4 u; f16x8 v; } A, B;
  A.u = a;
  B.u = b;
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(A.v, B.v, c, 0, 0, 0);
}

// 2^e as a float (|e| < 127)
__device__ __forceinline__ float pow2i(const int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }

// Conversions are IEEE (MODE.FP16_OVFL stays 0): a scaled value beyond the fp16 range becomes an infinity in its planes and a
// non-finite number in every sum it enters - it surfaces at the end of the path (SamplerPipeline.check) instead of passing for a value.

// x[0..7] * sc -> two planes of 8 fp16 (element j in the low / high half of dword j >> 1): v_pk_mul, v_cvt_pk_f16_f32,
// two v_cvt_f32_f16, v_pk_add, v_cvt_pk_f16_f32 per pair of values (the bf16 three-way split takes eleven)
__device__ __forceinline__ void split8h(const float (&x)[8], const float sc, uint4& p1, uint4& p2) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  uint32_t q1[4], q2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 t = {x[2 * i] * sc, x[2 * i + 1] * sc};
    union { f16x2 h; uint32_t u; } hi, lo;
    hi.h = __builtin_convertvector(t, f16x2);
    const f32x2 r = t - __builtin_convertvector(hi.h, f32x2);
    lo.h = __builtin_convertvector(r, f16x2);
    q1[i] = hi.u;
    q2[i] = lo.u;
  }
  p1 = make_uint4(q1[0], q1[1], q1[2], q1[3]);
  p2 = make_uint4(q2[0], q2[1], q2[2], q2[3]);
}

// four values * sc -> fp16 hi / lo planes, 8 bytes each
__device__ __forceinline__ void split4h(const float (&x)[4], const float sc, uint2& p1, uint2& p2) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  uint32_t q1[2], q2[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x2 t = {x[2 * i] * sc, x[2 * i + 1] * sc};
    union { f16x2 h; uint32_t u; } hi, lo;
    hi.h = __builtin_convertvector(t, f16x2);
    const f32x2 r = t - __builtin_convertvector(hi.h, f32x2);
    lo.h = __builtin_convertvector(r, f16x2);
    q1[i] = hi.u;
    q2[i] = lo.u;
  }
  p1 = make_uint2(q1[0], q1[1]);
  p2 = make_uint2(q2[0], q2[1]);
}

// round-to-nearest-even bf16 of two floats, packed (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_bf16_rne(const float a, const float b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const f32x2 v = {a, b};
  union { bf16x2 h; uint32_t u; } c;
  c.h = __builtin_convertvector(v, bf16x2);
  return c.u;
}

// ---------------------------------------------------------------------------------------------------------------
// The NP forms behind one name.
// ---------------------------------------------------------------------------------------------------------------
// x -> its NP planes; sc: the power of two that takes the values to the plane exponent (NP == 2 only)
template <int NP>
__device__ __forceinline__ void split_planes(const float (&x)[8], uint4 (&p)[NP], const float sc = 1.0f) {
  if constexpr (NP == 3) split8(x, p[0], p[1], p[2]);
  else if constexpr (NP == 2) split8h(x, sc, p[0], p[1]);
  else p[0] = make_uint4(pack_bf16_rne(x[0], x[1]), pack_bf16_rne(x[2], x[3]), pack_bf16_rne(x[4], x[5]), pack_bf16_rne(x[6], x[7]));
}
template <int NP>
__device__ __forceinline__ void split_planes(const float (&x)[4], uint2 (&p)[NP], const float sc = 1.0f) {
  if constexpr (NP == 3) split4(x, p[0], p[1], p[2]);
  else if constexpr (NP == 2) split4h(x, sc, p[0], p[1]);
  else p[0] = make_uint2(pack_bf16_rne(x[0], x[1]), pack_bf16_rne(x[2], x[3]));
}

// The plane products of a multiply-add, in the order they are accumulated: term q is (plane a[q] of A) x (plane b[q] of B),
// smallest first.  NP = 3 keeps a0 b2, a2 b0, a1 b1, a0 b1, a1 b0, a0 b0 and drops a1 b2, a2 b1, a2 b2 (below 2^-23 |a b|);
// NP = 2 keeps a1 b0, a0 b1, a0 b0 and drops a1 b1.
template <int NP>
struct plane_terms;
template <>
struct plane_terms<3> {
  static constexpr int n = 6;
  static constexpr int a[6] = {0, 2, 1, 0, 1, 0}, b[6] = {2, 0, 1, 1, 0, 0};
};
template <>
struct plane_terms<2> {
  static constexpr int n = 3;
  static constexpr int a[3] = {1, 0, 0}, b[3] = {0, 1, 0};
};
template <>
struct plane_terms<1> {
  static constexpr int n = 1;
  static constexpr int a[1] = {0}, b[1] = {0};
};

// one plane product on the matrix cores of the form's number format
template <int NP>
__device__ __forceinline__ f32x16 plane_mfma(const uint4& a, const uint4& b, const f32x16 c) {
  if constexpr (NP == 2) return mfma_f16(a, b, c);
  else return mfma_bf16(a, b, c);
}

// acc += A B, both operands as NP planes in registers
template <int NP>
__device__ __forceinline__ f32x16 plane_mma(const uint4 (&a)[NP], const uint4 (&b)[NP], f32x16 acc) {
  using T = plane_terms<NP>;
#pragma unroll
  for (int q = 0; q < T::n; ++q) acc = plane_mfma<NP>(a[T::a[q]], b[T::b[q]], acc);
  return acc;
}

// the same with A given as NP fragment planes at w[0], w[64], w[128] (uint4 units, this lane's entry)
template <int NP>
__device__ __forceinline__ f32x16 plane_mma_frag(const uint4* w, const uint4 (&b)[NP], f32x16 acc) {
  uint4 a[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) a[p] = w[64 * p];
  return plane_mma<NP>(a, b, acc);
}

// A 32-channel accumulator tile X as the B operand of the next contraction: two K blocks of 8 registers each, p[K block][plane]
template <int NP>
__device__ __forceinline__ void split_tile(const f32x16& X, uint4 (&p)[2][NP], const float sc = 1.0f) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = X[8 * s + j];
    split_planes<NP>(x, p[s], sc);
  }
}

// Y = W X over the two K blocks; w: LDS fragments [2 blocks][NP planes][64 lanes] of this output tile, already offset by the lane
template <int NP>
__device__ __forceinline__ f32x16 chain_tile(const uint4* w, const uint4 (&p)[2][NP], f32x16 acc) {
#pragma unroll
  for (int s = 0; s < 2; ++s) acc = plane_mma_frag<NP>(w + s * NP * 64, p[s], acc);
  return acc;
}

// The same for an operand used once: each K block is split right in front of its products
template <int NP>
__device__ __forceinline__ f32x16 chain_tile(const uint4* w, const f32x16& X, f32x16 acc, const float sc = 1.0f) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = X[8 * s + j];
    uint4 b[NP];
    split_planes<NP>(x, b, sc);
    acc = plane_mma_frag<NP>(w + s * NP * 64, b, acc);
  }
  return acc;
}

#endif
