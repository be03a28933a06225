// qblock.h -- the quantised weight formats of the decode kernels, stated once: each format's packed
// layout, the per-lane register image of a packed block with its fetch, and the arithmetic that
// turns the image into MFMA fragments.  k_qgemv.hip (loader kernels, dequant-fused GEMV) and
// k_qdgemm.hip (packed-row skinny GEMM) include it; nothing else knows a byte offset.  The byte
// counts per 256 weights (kQ4KBytes, ...) are in kernels.h: host code uses them.
//
// Every format is counted in units of 256 weights of one row ("super-block"; 8 sub-blocks s of 32).
// A wave reads 16 rows x one unit per step: lane = 16 g + fr, row fr, lane group g.  The packed
// layouts put what lane group g needs of one unit in 16-B pieces at 16 g, so one wave load
// instruction reads 64 contiguous bytes of each row.  In the Q4_K / Q5_K / Q8_0 order lane group g
// owns weights k = 32 s + 8 g + i (i < 8) of every sub-block s -- MFMA s of the unit takes them with
// the X elements of the same k (a k permutation applied to both operands: dot products unchanged).
//
// Q4_K (ggml type 12; raw {fp16 d, dmin; scales[12]; qs[128]} = 144 B, y = d1 q - m1 with
// d1 = d sc_s, m1 = dmin m_s, get_scale_min_k4).  Packed, 144 B:
//   bytes 0..15     the ggml header as is
//   byte 16 + 64 (s >> 2) + 16 g + 4 (s & 3) + i = nib(k) | nib(k + 4) << 4, k = 32 s + 8 g + i, i < 4:
//                   lane group g's sub-blocks 0-3 in the 16 B at 16 + 16 g, 4-7 at 80 + 16 g, one
//                   dword per sub-block
// Q5_K (type 13; raw {d, dmin; scales[12]; qh[32]; qs[128]} = 176 B; weight t = 32 s + l has the code
// nibble(t) + 16 ((qh[l] >> s) & 1) in 0..31, and Q4_K's d1, m1).  Packed, 176 B:
//   bytes 0..143    Q4_K's packed block of the header and the nibbles
//   bytes 144..175  qh in its raw order: lane group g reads the 8 bytes at 144 + 8 g as two dwords
//                   Hlo, Hhi; sub-block s's fifth bits are ((H >> s) & 0x01010101) << 4
// Q6_K (type 14; raw {ql[128]; qh[64]; int8 scales[16]; fp16 d} = 210 B, y = (d sc) (q - 32)).
// Packed, 224 B, every field 16-B aligned:
//   bytes 0..127    ql regrouped by the GEMV's lane group g = 2 hh + p (half hh of the block, positions
//                   l in [16 p, 16 p + 16), each giving the weights 128 hh + {0, 32, 64, 96} + l): raw
//                   ql[64 hh + 16 p ..] (low nibbles: weights + 0, high: + 64) at 16 g, raw
//                   ql[64 hh + 32 + 16 p ..] (+ 32, + 96) at 64 + 16 g
//   bytes 128..191  qh unmoved (raw 128 + 32 hh + 16 p = 128 + 16 g: already in that order)
//   bytes 192..207  the 16 scales; 208..209 d; 210..223 zero
// Q8_0 (type 8; 8 consecutive ggml blocks {fp16 d; int8 qs[32]} = 272 raw bytes, y = d q).  Packed
// unit, 272 B:
//   bytes 0..15     the 8 fp16 scales d_0 .. d_7 in block order
//   byte 16 + 64 (s >> 1) + 16 g + 8 (s & 1) + i = q[32 s + 8 g + i], i < 8: piece c of lane group g
//                   (16 B at 16 + 64 c + 16 g) holds its 8 weights of blocks 2c and 2c + 1
#pragma once
#include "gemv_common.h"

namespace ms {

// packed Q4_K / Q5_K: header, the two nibble pieces (+ 16 g), Q5_K's qh (+ 8 g); their raw fields
constexpr int kKqHdr = 0, kKqNib0 = 16, kKqNib1 = 80, kQ5Qh = 144;
constexpr int kQ4RawQs = 16, kQ5RawQh = 16, kQ5RawQs = 48;
// packed Q6_K: the two ql halves (+ 16 g), qh, scales, d (raw: ql 0, the rest at the same offsets)
constexpr int kQ6Ql0 = 0, kQ6Ql1 = 64, kQ6Qh = 128, kQ6Sc = 192, kQ6D = 208;
// packed Q8_0: scales, quant pieces (+ 64 c + 16 g); a raw block is {d, qs[32]}
constexpr int kQ8Sc = 0, kQ8Q = 16, kQ8RawBlock = 34;

__device__ __forceinline__ float h2f_lo(uint32_t h16) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)(h16 & 0xFFFFu));
}
// Q5_K's 8-B qh piece, loaded through a function returning by value as the skinny GEMM always did: as
// a struct copy through the cast pointer its MT = 1 kernels allocated 78 / 76 VGPRs for 82 / 80
__device__ __forceinline__ uint2 ldw8(const void* p) { return *(const uint2*)p; }
// word i < 4 of a 16-B piece (i compile-time or not).  By reference, as the skinny GEMM's own helper
// took it: with the pieces its dequant reads passed by value 31 of its kernels spilled
// (profiles/qblock/README.md)
__device__ __forceinline__ uint32_t word_of(const uint4& v, int i) {
  return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// ---------------------------------------------------------------- Q4_K / Q5_K
// ggml's d1 = d * sc_s and m1 = dmin * m_s of sub-block s: get_scale_min_k4 on the 12 scale bytes
// (header words y, z, w), four sub-blocks per word operation
__device__ __forceinline__ void kq_scale_min(const uint4& h, int s, float& d1, float& m1) {
  const uint32_t scw = s < 4 ? (h.y & 0x3F3F3F3Fu) : ((h.w & 0x0F0F0F0Fu) | ((h.y >> 2) & 0x30303030u));
  const uint32_t mw = s < 4 ? (h.z & 0x3F3F3F3Fu) : (((h.w >> 4) & 0x0F0F0F0Fu) | ((h.z >> 2) & 0x30303030u));
  const int sh = 8 * (s & 3);
  d1 = __fmul_rn(h2f_lo(h.x), (float)((scw >> sh) & 0xFFu));
  m1 = __fmul_rn(h2f_lo(h.x >> 16), (float)((mw >> sh) & 0xFFu));
}

struct KqRegs {  // one packed block of this lane's row: header, sub-blocks 0-3, 4-7 of lane group g
  uint4 h, q0, q1;
};
struct Q5Regs {  // the same and qh[8g .. 8g + 7], the fifth bits of the lane group's weights
  uint4 h, q0, q1;
  uint2 qh;
};
__device__ __forceinline__ void kq_fetch(KqRegs& r, const uint8_t* bp, int g) {
  r.h = ldw16(bp + kKqHdr);
  r.q0 = ldw16(bp + kKqNib0 + 16 * g);
  r.q1 = ldw16(bp + kKqNib1 + 16 * g);
}
__device__ __forceinline__ void kq_fetch(Q5Regs& r, const uint8_t* bp, int g) {
  r.h = ldw16(bp + kKqHdr);
  r.q0 = ldw16(bp + kKqNib0 + 16 * g);
  r.q1 = ldw16(bp + kKqNib1 + 16 * g);
  r.qh = ldw8(bp + kQ5Qh + 8 * g);
}
// the 4-bit codes of weights k .. k + 3 (lo) and k + 4 .. k + 7 (hi), k = 32 s + 8 g, one per byte
__device__ __forceinline__ void kq_codes(const uint4& q0, const uint4& q1, int s, uint32_t& lo, uint32_t& hi) {
  const uint32_t qw = word_of(s < 4 ? q0 : q1, s & 3);  // byte i = q[k_i] | q[k_{i+4}] << 4
  lo = qw & 0x0F0F0F0Fu;
  hi = (qw >> 4) & 0x0F0F0F0Fu;
}
// bytes [q, 0, q', 0] = the fp16 subnormals q 2^-24, q' 2^-24 (exact; gfx950 MFMA keeps fp16 denormal
// operands): weights k .. k + 7 in order (perm selector 0x0C is the constant byte 0)
__device__ __forceinline__ f16x8 subnormal_frag(uint32_t lo, uint32_t hi) {
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  const u4v pk = {__builtin_amdgcn_perm(0u, lo, 0x0C010C00u), __builtin_amdgcn_perm(0u, lo, 0x0C030C02u),
                  __builtin_amdgcn_perm(0u, hi, 0x0C010C00u), __builtin_amdgcn_perm(0u, hi, 0x0C030C02u)};
  return __builtin_bit_cast(f16x8, pk);
}

// ---------------------------------------------------------------- codes -> fp16 weights
// four codes held as the bytes of q4 -> two packed fp16 pairs of fma(a, q, b): each byte converted
// straight to fp32 (v_cvt_f32_ubyte*), two weights per v_pk_fma_f32, rounded to fp16 by
// v_cvt_pk_f16_f32 (RNE) -- ~3 VALU per weight
__device__ __forceinline__ void deq4(uint32_t q4, float a, float b, uint32_t& p0, uint32_t& p1) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 a2 = {a, a}, b2 = {b, b};
  const f2 y01 = __builtin_elementwise_fma(a2, f2{(float)(q4 & 0xFFu), (float)((q4 >> 8) & 0xFFu)}, b2);
  const f2 y23 = __builtin_elementwise_fma(a2, f2{(float)((q4 >> 16) & 0xFFu), (float)(q4 >> 24)}, b2);
  p0 = pack2h(y01.x, y01.y);
  p1 = pack2h(y23.x, y23.y);
}
__device__ __forceinline__ f16x8 deq_frag(uint32_t c0, uint32_t c1, float a, float b) {
  uint32_t pk[4];
  deq4(c0, a, b, pk[0], pk[1]);
  deq4(c1, a, b, pk[2], pk[3]);
  return __builtin_bit_cast(f16x8, pk);
}
// the fp16 weights k = 32 c + 8 g .. + 7 of a Q4_K / Q5_K block: fma(d1, q, -m1) (the products are exact
// in fp32 -- 11 + 6 + 5 bits at most -- so this is ggml's d1 q - m1 with its single rounding)
__device__ __forceinline__ f16x8 kq_dequant(const KqRegs& r, int c) {
  float d1, m1;
  kq_scale_min(r.h, c, d1, m1);
  uint32_t lo, hi;
  kq_codes(r.q0, r.q1, c, lo, hi);
  return deq_frag(lo, hi, d1, -m1);
}
// Q5_K: bit c of qh[8g + i] is the fifth bit of weight 32 c + 8 g + i
__device__ __forceinline__ f16x8 kq_dequant(const Q5Regs& r, int c) {
  float d1, m1;
  kq_scale_min(r.h, c, d1, m1);
  const uint32_t qw = word_of(c < 4 ? r.q0 : r.q1, c & 3);
  uint32_t pk[4];
  deq4((qw & 0x0F0F0F0Fu) | (((r.qh.x >> c) & 0x01010101u) << 4), d1, -m1, pk[0], pk[1]);
  deq4(((qw >> 4) & 0x0F0F0F0Fu) | (((r.qh.y >> c) & 0x01010101u) << 4), d1, -m1, pk[2], pk[3]);
  return __builtin_bit_cast(f16x8, pk);
}

// ---------------------------------------------------------------- Q6_K
// the 6-bit codes of 4 weights as the bytes of one word: nibble | 2 high bits << 4.  aw: 4 ql bytes,
// hw: the 4 qh bytes of the same positions; k4 (compile-time): which of the weights {0, 32, 64, 96} + l
__device__ __forceinline__ uint32_t q6_codes(uint32_t aw, uint32_t hw, int k4) {
  return ((aw >> (4 * (k4 >> 1))) & 0x0F0F0F0Fu) | (((hw >> (2 * k4)) & 0x03030303u) << 4);
}
// The GEMV and the skinny GEMM split a block across the lane groups differently, so Q6_K has two
// register images.  The GEMV is free to permute k (it reads X by the same permutation), so lane group
// g = 2 hh + p takes 16-B pieces -- 16 positions l of half hh, all four k4 -- and MFMA t of the block
// multiplies k = 128 hh + 32 (t >> 1) + 16 p + 8 (t & 1) .. + 7: four loads and d.
struct Q6Regs {
  uint4 qa, qb, qh, sc;  // ql low / high half, qh, the 16 scales
  uint32_t dw;
};
__device__ __forceinline__ void q6_fetch(Q6Regs& r, const uint8_t* bp, int g) {
  r.qa = ldw16(bp + kQ6Ql0 + 16 * g);
  r.qb = ldw16(bp + kQ6Ql1 + 16 * g);
  r.qh = ldw16(bp + kQ6Qh + 16 * g);
  r.sc = ldw16(bp + kQ6Sc);
  r.dw = *(const uint32_t*)(bp + kQ6D);
}
// MFMA t's fp16 weights: fma(ds, q, -32 ds) = ds (q - 32) with the single rounding of ggml's product
// (only the sign of an exact zero can differ), ds = d sc; -32 ds is exact (a power-of-two multiple of
// an fp16 x int8 product).  d = h2f_lo(r.dw), converted once per block by the caller
// SEL64: the same scale byte picked from the half's 8 scales as one 64-bit word (the caller says when)
template <bool SEL64 = false>
__device__ __forceinline__ f16x8 q6_frag(const uint4& qa, const uint4& qb, const uint4& qh, const uint4& sc, float d,
                                          int t, int hh, int p) {
  const int k4 = t >> 1, wi = 2 * (t & 1);  // weights l = 16 p + 4 wi .. + 7
  uint32_t sb;  // scale byte 8 hh + p + 2 k4 of the 16
  if constexpr (SEL64) {
    const uint64_t sw = hh ? (sc.z | (uint64_t)sc.w << 32) : (sc.x | (uint64_t)sc.y << 32);
    sb = (uint32_t)(sw >> (8 * (p + 2 * k4))) & 0xFFu;
  } else {  // word 2 hh + (k4 >> 1), byte p + 2 (k4 & 1): one select and one shift
    const uint32_t sw = hh ? ((k4 >> 1) ? sc.w : sc.z) : ((k4 >> 1) ? sc.y : sc.x);
    sb = (sw >> (8 * (p + 2 * (k4 & 1)))) & 0xFFu;
  }
  const float ds = __fmul_rn(d, (float)(int)(int8_t)sb);
  const uint4& a = (k4 & 1) ? qb : qa;
  return deq_frag(q6_codes(word_of(a, wi), word_of(qh, wi), k4), q6_codes(word_of(a, wi + 1), word_of(qh, wi + 1), k4),
                  ds, -32.0f * ds);
}
__device__ __forceinline__ f16x8 q6_frag(const Q6Regs& r, float d, int t, int hh, int p) {
  return q6_frag(r.qa, r.qb, r.qh, r.sc, d, t, hh, p);
}
// The skinny GEMM reads X from an LDS image in natural k order, so MFMA column c = 4 n + k4 of the
// block must hold k = 32 c + 8 g .. + 7: lane group g takes the 8 positions l = 8 g + i of both halves n
// -- 8-B pieces: raw ql[64 n + 32 half + l] sits at 64 half + 32 n + l of the packed block (the GEMV's
// regrouping, 64 half + 16 (2 n + p) + j for l = 16 p + j, is that).  Six 8-B loads, the scales and d.
struct Q6ColRegs {
  uint2 ql[2][2], qh[2];  // ql [k4 & 1][n], qh [n]
  uint4 sc;
  uint32_t d;
};
__device__ __forceinline__ void q6_fetch(Q6ColRegs& r, const uint8_t* bp, int g) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int n = 0; n < 2; ++n) r.ql[h][n] = *(const uint2*)(bp + kQ6Ql0 + h * 64 + 32 * n + 8 * g);
#pragma unroll
  for (int n = 0; n < 2; ++n) r.qh[n] = *(const uint2*)(bp + kQ6Qh + 32 * n + 8 * g);
  r.sc = ldw16(bp + kQ6Sc);
  r.d = *(const uint32_t*)(bp + kQ6D);
}
__device__ __forceinline__ f16x8 q6_dequant(const Q6ColRegs& r, int c, int g) {
  const int n = c >> 2, k4 = c & 3;  // weights n*128 + k4*32 + l, l = 8g + i
  const float ds = __fmul_rn(h2f_lo(r.d), (float)(int)(int8_t)((word_of(r.sc, 2 * n + (k4 >> 1)) >> (8 * ((g >> 1) + 2 * (k4 & 1)))) & 0xFFu));
  const uint2 a = r.ql[k4 & 1][n], hq = r.qh[n];
  uint32_t pk[4];  // (deq_frag's statements in place: through it two MT = 16 kernels moved by 2 AGPRs)
  deq4(q6_codes(a.x, hq.x, k4), ds, -32.0f * ds, pk[0], pk[1]);
  deq4(q6_codes(a.y, hq.y, k4), ds, -32.0f * ds, pk[2], pk[3]);
  return __builtin_bit_cast(f16x8, pk);
}

// ---------------------------------------------------------------- Q8_0
struct Q8Regs {  // one packed unit of this lane's row: the 8 scales and lane group g's four 16-B quant pieces
  uint4 sc, q[4];
};
// tile: the block-uniform address of the tile's first row (a scalar base for the loads); row, sb:
// this lane's row in the tile and unit in the row (a 32-bit lane offset)
__device__ __forceinline__ void q8_fetch(Q8Regs& r, const uint8_t* tile, int row_bytes, int row, int sb, int g) {
  const uint32_t o = (uint32_t)(row * row_bytes + sb * kQ8Bytes);
  const uint8_t* qp = tile + (o + (uint32_t)kQ8Q + 16u * (uint32_t)g);  // one 32-bit lane offset per address
  r.sc = ldw16(tile + o);
#pragma unroll
  for (int c = 0; c < 4; ++c) r.q[c] = ldw16(qp + 64 * c);
}
// the same in two halves (the grid-stride loop's prefetch): the scales and blocks 0-3, blocks 4-7.
// Here the tile is a 32-bit byte offset from the matrix base (the launcher checks the matrix is
// < 4 GiB): scalar base + 32-bit lane offsets, where 64-bit lane addresses carried across the
// loop (4 VGPRs) spilled
template <int HALF>
__device__ __forceinline__ void q8_fetch_half(Q8Regs& r, const uint8_t* base, uint32_t tile, int row_bytes, int row, int sb,
                                              int g) {
  const uint32_t o = tile + (uint32_t)(row * row_bytes + sb * kQ8Bytes);
  const uint8_t* qp = base + (o + (uint32_t)kQ8Q + 16u * (uint32_t)g);
  if constexpr (HALF == 0) r.sc = ldw16(base + o);
#pragma unroll
  for (int c = 2 * HALF; c < 2 * HALF + 2; ++c) r.q[c] = ldw16(qp + 64 * c);
}
__device__ __forceinline__ float q8_scale(const Q8Regs& r, int s) {  // s compile-time
  // (the words picked from the members: through word_of's reference two instantiations lost a wave)
  const uint32_t w = (s >> 1) == 0 ? r.sc.x : (s >> 1) == 1 ? r.sc.y : (s >> 1) == 2 ? r.sc.z : r.sc.w;
  return h2f_lo(w >> (16 * (s & 1)));
}
// block s's 8 int8 weights of this lane group as the exact fp16 integers: byte ^ 0x80 under the
// exponent byte 0x64 is the fp16 1024 + (q + 128) (perm selector 4 = byte 0 of the constant),
// and 1024 + (q + 128) - 1152 = q with no rounding (q = -128: 1024 - 1152)
__device__ __forceinline__ f16x8 q8_frag(const Q8Regs& r, int s) {  // s compile-time
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  const uint4 v = r.q[s >> 1];
  const uint32_t w0 = ((s & 1) ? v.z : v.x) ^ 0x80808080u, w1 = ((s & 1) ? v.w : v.y) ^ 0x80808080u;
  const h2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
  auto cv = [&](uint32_t w, uint32_t sel) {
    const h2 u = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, w, sel));
    return __builtin_bit_cast(uint32_t, u - bias);
  };
  const u4v pk = {cv(w0, 0x04010400u), cv(w0, 0x04030402u), cv(w1, 0x04010400u), cv(w1, 0x04030402u)};
  return __builtin_bit_cast(f16x8, pk);
}

}  // namespace ms
