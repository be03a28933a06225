// kvq8.h -- the q8_0 KV cache format, stated once: the pool layout with its byte offsets, the row
// quantiser every writer calls, and decode attention's fetches and code -> MFMA-fragment functions.
// k_misc.hip / k_qknorm.hip (writers), k_attn.hip (the q8_0 decode attention form) and the op-level
// store include it; nothing else knows a byte offset.  DESIGN.md §2 "q8_0 KV cache" is the contract,
// tests/kv_q8_0_ref.py its numpy restatement.
//
// A cached row is the 128 fp16 values t of one (token, kv head), exactly as the fp16 pool would hold
// them, cut into 4 blocks of 32 consecutive stored elements.  Per block, in fp32, one IEEE operation
// per step (ggml's quantize_row_q8_0_ref):
//   amax = max |t_i|;  d = amax / 127;  id = d != 0 ? 1 / d : 0;  c_i = roundf(t_i * id) (half away
//   from zero, -127..127);  stored scale f16_rne(d);  dequantised value (float)f16(d) * c_i.
// A block whose amax is not finite stores the scale 0x7E00 (NaN) and codes 0.
//
// Pool, per (layer, page, kv head) -- kKvq8Slab = 8704 B:
//   bytes 0..8191     codes  int8 [64 tokens][128]
//   bytes 8192..8703  scales fp16 [64 tokens][4 blocks]
// Pages, block table, slot-major rule and 64-token pages are the fp16 pool's (kernels.h KVView).
#pragma once
#include "kernels.h"

namespace ms {

constexpr int kKvq8Block = 32, kKvq8Blocks = kHeadDim / kKvq8Block;       // 4 blocks per row
constexpr int kKvq8Codes = 0, kKvq8CodeBytes = kPage * kHeadDim;          // 8192
constexpr int kKvq8Scales = kKvq8CodeBytes, kKvq8ScaleBytes = kPage * kKvq8Blocks * 2;  // 512
constexpr int kKvq8Slab = kKvq8CodeBytes + kKvq8ScaleBytes;               // 8704

// Where the q8_0 K/V of one layer live: pool[page][kv_head] slabs of kKvq8Slab bytes.
struct KVQ8View {
  uint8_t* k;
  uint8_t* v;
  const int32_t* block_table;  // [slots][max_pages]
  int32_t max_pages;
  int32_t n_kv_heads;
  int32_t slot_major;  // as KVView's
};

__host__ __device__ inline size_t kvq8_slab(int page, int n_kv_heads, int kvh) {
  return ((size_t)page * n_kv_heads + kvh) * kKvq8Slab;
}

// launch_rope_kv with the K / V rows quantised into the q8_0 pools; stage: the fp16 staging pool of a
// prefill (receives the fp16 rows too), or stage.k == nullptr
void launch_rope_kv_q8(f16_t* qkv, int T, int Hq, int Hk, const int32_t* tok_pos, const int32_t* tok_slot,
                       const float* cos_tab, const float* sin_tab, KVQ8View q8, KVView stage, hipStream_t s,
                       bool rope_q = true);
// fp16 K and V rows [T][Hk][128], as the fp16 pool would hold them, quantised into the pools
void launch_kv_store_q8(const f16_t* k, const f16_t* v, int T, int Hk, const int32_t* tok_pos,
                        const int32_t* tok_slot, KVQ8View q8, hipStream_t s);
// launch_attn_decode's rows route (Q already rotated in qkv) over the q8_0 pools: the same split grid,
// ppw rule, workspace and combine
void launch_attn_decode_q8(const f16_t* qkv, f16_t* out, int Hq, int Hk, KVQ8View kv, DecodeAttnArgs a, float* ws,
                           hipStream_t s);

#if defined(__HIPCC__)
// THE quantiser.  A whole wave stores one row: lane l passes the row's stored elements 2l and 2l + 1
// (fp16 values as floats; block l / 16), `slab` is the (page, kv head) slab of the K or the V pool and
// `off` the token's offset in the page.  amax over the block's 16 lanes by an xor tree (max is exact in
// any order); every lane of the wave must be active.
__device__ __forceinline__ void kvq8_store_row(uint8_t* slab, int off, float e0, float e1, int lane) {
  float amax = fmaxf(fabsf(e0), fabsf(e1));
  // fmaxf drops a NaN: the block's "not finite" flag travels beside the maximum
  int bad = !(fabsf(e0) < INFINITY) || !(fabsf(e1) < INFINITY);
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) {
    amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    bad |= __shfl_xor(bad, o, 64);
  }
  const float d = __fdiv_rn(amax, 127.0f);
  const float id = d != 0.0f ? __fdiv_rn(1.0f, d) : 0.0f;
  const int c0 = bad ? 0 : (int)roundf(__fmul_rn(e0, id));
  const int c1 = bad ? 0 : (int)roundf(__fmul_rn(e1, id));
  *(uint16_t*)(slab + kKvq8Codes + off * kHeadDim + 2 * lane) = (uint16_t)((c0 & 0xFF) | ((c1 & 0xFF) << 8));
  if ((lane & 15) == 0)
    *(f16_t*)(slab + kKvq8Scales + (off * kKvq8Blocks + (lane >> 4)) * 2) = bad ? (f16_t)0x7E00 : f2h(d);
}

// ---- decode attention's register image of one page (lane = 16 g + r)
typedef uint32_t kvq8_u2 __attribute__((ext_vector_type(2)));
typedef uint32_t kvq8_u4 __attribute__((ext_vector_type(4)));
// K codes of key row `row`, block b: this lane group's 8 codes (stored elements 32 b + 8 g .. + 7)
__device__ __forceinline__ kvq8_u2 kvq8_fetch_codes8(const uint8_t* slab, int row, int b, int g) {
  return *(const kvq8_u2*)(slab + kKvq8Codes + row * kHeadDim + kKvq8Block * b + 8 * g);
}
// V codes of row `row`, 16-B chunk ch (stored elements 8 ch .. + 7; block ch / 4)
__device__ __forceinline__ kvq8_u2 kvq8_fetch_chunk(const uint8_t* slab, int row, int ch) {
  return *(const kvq8_u2*)(slab + kKvq8Codes + row * kHeadDim + 8 * ch);
}
// the 16 scales of the 4 consecutive tokens tok0 .. tok0 + 3 (tok0 % 4 == 0): [token][block], 32 B
struct Kvq8Scales4 {
  kvq8_u4 lo, hi;  // tokens tok0, tok0 + 1 | tok0 + 2, tok0 + 3
};
// One page's scales as decode attention stages them in LDS (kKvq8ScaleImg bytes: the K slab's 512 B of
// scales, then the V slab's): lane l's 16-B source piece of the single LDS DMA that fills it ...
constexpr int kKvq8ScaleImg = 2 * kKvq8ScaleBytes;
__device__ __forceinline__ const uint8_t* kvq8_scales_src(const uint8_t* kslab, const uint8_t* vslab, int lane) {
  return (lane < 32 ? kslab : vslab) + kKvq8Scales + 16 * (lane & 31);
}
// ... and the 16 scales of tokens tok0 .. tok0 + 3 read back from the image
__device__ __forceinline__ Kvq8Scales4 kvq8_lds_scales4(const char* img, bool v, int tok0) {
  const char* p = img + (v ? kKvq8ScaleBytes : 0) + tok0 * kKvq8Blocks * 2;
  return Kvq8Scales4{*(const kvq8_u4*)p, *(const kvq8_u4*)(p + 16)};
}
// scale of token tok0 + j, block b (j, b compile-time)
__device__ __forceinline__ float kvq8_scale(const Kvq8Scales4& s, int j, int b) {
  const kvq8_u4& v = j < 2 ? s.lo : s.hi;
  const uint32_t w = v[2 * (j & 1) + (b >> 1)];
  return (float)__builtin_bit_cast(f16x2, w)[b & 1];
}
// 8 int8 codes -> the exact fp16 integers, in order: byte ^ 0x80 under the exponent byte 0x64 is the
// fp16 1024 + (c + 128), and subtracting 1152 leaves c with no rounding -- qblock.h's Q8_0 trick
// (v_perm + v_pk_add_f16)
__device__ __forceinline__ kvq8_u4 kvq8_codes_f16(kvq8_u2 c) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const uint32_t w0 = c[0] ^ 0x80808080u, w1 = c[1] ^ 0x80808080u;
  const h2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
  auto cv = [&](uint32_t w, uint32_t sel) {
    const h2 u = __builtin_bit_cast(h2, __builtin_amdgcn_perm(0x64646464u, w, sel));
    return __builtin_bit_cast(uint32_t, u - bias);
  };
  return kvq8_u4{cv(w0, 0x04010400u), cv(w0, 0x04030402u), cv(w1, 0x04010400u), cv(w1, 0x04030402u)};
}
#endif

}  // namespace ms
