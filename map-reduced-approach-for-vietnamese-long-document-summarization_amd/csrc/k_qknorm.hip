// k_qknorm.hip -- per-head Q/K RMSNorm + RoPE + paged-KV scatter of a QK-norm model (Qwen3).
//
// Numerics contract ("QK-norm engines"; tests/qwen3_ref.py restates it): a head's
// 128 fp16 values t -- f16(r * acc), the projection's usual rounding point -- are normalised
// in fp32, rho = rsq(sum(t^2) / 128 + eps), n = (t * rho) * w with the layer's fp16 gain w
// indexed by the LOGICAL head dimension (the rows arrive rope-permuted), rotated in fp32
// (rotate-half pairs (i, i + 64)) and rounded to fp16 ONCE.  The sum of squares has one order:
// lane i of the head's wave adds t[i]^2 + t[i + 64]^2, then the wave's xor tree -- it depends on
// the head's 128 values only, never on the token count, the slot, the regime or the input form.
//
// One wave per (token, head), 4 waves per block.  Two input forms share qk_head():
//   rows : fp16 qkv [T][(Hq + 2 Hk) * 128] (the QKV GEMM / GEMV output), as rope_kv_kernel takes it;
//   slabs: S fp32 split-K slabs [S][rows][(Hq + 2 Hk) * 128] + the row's deferred-norm statistics,
//          folded in slab order and rounded f16(rinv * sum) as decode attention's slab prologue does.
// Both leave Q rotated in natural dim order in its qkv row and K / V at the page and offset of the
// token's position (V copied as is); the slabs form also leaves the folded fp16 K / V in the row.
//
// Q8 (a q8_0-KV engine, kvq8.h), both forms: the K and V rows go through kvq8_store_row into the q8_0
// pools; kv is then a prefill's fp16 staging pool (it also receives the fp16 rows) or has kv.k null.
#include "kernels.h"
#include "kvq8.h"

namespace ms {

// lane i of a head's wave: (lo, hi) = the head's fp16 values at logical dims (i, i + 64) ->
// the normalised, rotated pair, still fp32 (the caller rounds once)
__device__ __forceinline__ void qk_head(float lo, float hi, const f16_t* __restrict__ gain, float cs, float sn,
                                        float eps, int lane, float& ra, float& rb) {
  const float ss = wave_sum(__fadd_rn(__fmul_rn(lo, lo), __fmul_rn(hi, hi)));
  const float rho = __builtin_amdgcn_rsqf(__fmaf_rn(ss, 1.0f / (float)kHeadDim, eps));
  const float nl = __fmul_rn(__fmul_rn(lo, rho), h2f(gain[lane]));
  const float nh = __fmul_rn(__fmul_rn(hi, rho), h2f(gain[64 + lane]));
  ra = __fsub_rn(__fmul_rn(nl, cs), __fmul_rn(nh, sn));
  rb = __fadd_rn(__fmul_rn(nh, cs), __fmul_rn(nl, sn));
}

template <bool FROM_SLABS, bool Q8>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(f16_t* __restrict__ qkv, const float* __restrict__ slabs,
                                                           int S, int slab_rows, RowScale rs, int T, int Hq, int Hk,
                                                           const int32_t* __restrict__ tok_pos,
                                                           const int32_t* __restrict__ tok_slot,
                                                           const float* __restrict__ cos_tab,
                                                           const float* __restrict__ sin_tab,
                                                           const f16_t* __restrict__ q_gain,
                                                           const f16_t* __restrict__ k_gain, float eps, KVView kv,
                                                           KVQ8View q8) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = blockIdx.x;
  const int head = blockIdx.y * 4 + wave;
  const int NH = Hq + 2 * Hk;
  if (t >= T || head >= NH) return;  // wave-uniform; no barrier below
  const int row_elems = NH * kHeadDim;
  f16_t* row = qkv + (size_t)t * row_elems + head * kHeadDim;
  const int pos = tok_pos[t];
  const int slot = tok_slot[t];
  const bool is_q = head < Hq, is_k = !is_q && head < Hq + Hk;

  // the head's values as fp16-valued floats: Q / K lanes hold logical dims (lane, lane + 64),
  // V lanes the consecutive pair (2 lane, 2 lane + 1)
  const int e0 = is_q || is_k ? rope_perm(lane) : 2 * lane;
  const int e1 = is_q || is_k ? rope_perm(64 + lane) : 2 * lane + 1;
  float lo, hi;
  if constexpr (FROM_SLABS) {
    float rrow = 1.0f;
    if (rs.ssq) {  // the row's factor: tiles lane + 64 i in i order, then the wave tree (RowScale)
      float rv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int tl = lane + 64 * i;
        rv[i] = tl < rs.tiles ? rs.ssq[(size_t)tl * slab_rows + t] : 0.f;
      }
      rrow = rs_rinv(wave_sum(((rv[0] + rv[1]) + rv[2]) + rv[3]), rs);
    }
    const size_t sstride = (size_t)slab_rows * row_elems;
    const float* src = slabs + (size_t)t * row_elems + head * kHeadDim;
    float a0 = src[e0], a1 = src[e1];
    for (int q = 1; q < S; ++q) {
      a0 += src[q * sstride + e0];
      a1 += src[q * sstride + e1];
    }
    lo = h2f(f2h(a0 * rrow));
    hi = h2f(f2h(a1 * rrow));
  } else {
    lo = h2f(row[e0]);
    hi = h2f(row[e1]);
  }

  const bool f16_kv = !Q8 || kv.k;  // the fp16 pool (a q8_0-KV engine: its prefill staging pool)
  const int page = f16_kv ? kv.block_table[(size_t)slot * kv.max_pages + pos / kPage] : 0;
  const int off = pos % kPage;
  int qpage = 0;
  if constexpr (Q8) qpage = is_q ? 0 : q8.block_table[(size_t)slot * q8.max_pages + pos / kPage];
  if (!is_q && !is_k) {  // V: copied as is
    const int kh = head - Hq - Hk;
    const uint32_t pr = pack2h(lo, hi);  // exact: both are fp16 values
    if (f16_kv) {
      f16_t* dst = kv.v + (((size_t)page * kv.n_kv_heads + kh) * kPage + off) * kHeadDim;
      *(uint32_t*)(dst + 2 * lane) = pr;
    }
    if constexpr (Q8) kvq8_store_row(q8.v + kvq8_slab(qpage, q8.n_kv_heads, kh), off, lo, hi, lane);
    if constexpr (FROM_SLABS) *(uint32_t*)(row + 2 * lane) = pr;
    return;
  }
  if constexpr (FROM_SLABS) {
    if (is_k) {  // the folded, un-normalised K stays in the row (what the rows form was given)
      row[e0] = f2h(lo);
      row[e1] = f2h(hi);
    }
  }
  const float cs = cos_tab[(size_t)pos * 64 + lane], sn = sin_tab[(size_t)pos * 64 + lane];
  float ra, rb;
  qk_head(lo, hi, is_q ? q_gain : k_gain, cs, sn, eps, lane, ra, rb);
  // (every lane's result depends on all 128 loads through the reduction, so the in-place Q
  // stores below cannot pass another lane's load of the same row)
  const f16_t ha = f2h(ra), hb = f2h(rb);
  if (is_q || f16_kv) {
    f16_t* dst = is_q ? row
                      : kv.k + (((size_t)page * kv.n_kv_heads + (head - Hq)) * kPage + off) * kHeadDim;
    dst[lane] = ha;
    dst[64 + lane] = hb;
  }
  if constexpr (Q8) {
    if (is_k) {  // wave-uniform.  Stored element e sits in lane e % 64 (ha below 64, hb above): lane l
                 // gathers elements 2l and 2l + 1, the quantiser's order
      const float fa = h2f(ha), fb = h2f(hb);
      const int s0 = (2 * lane) & 63;
      const float a0 = __shfl(fa, s0, 64), a1 = __shfl(fa, s0 + 1, 64);
      const float b0 = __shfl(fb, s0, 64), b1 = __shfl(fb, s0 + 1, 64);
      kvq8_store_row(q8.k + kvq8_slab(qpage, q8.n_kv_heads, head - Hq), off, lane < 32 ? a0 : b0,
                     lane < 32 ? a1 : b1, lane);
    }
  }
}

void launch_qk_norm_rope(f16_t* qkv, const float* slabs, int S, int slab_rows, const RowScale& rs, int T, int Hq,
                         int Hk, const int32_t* tok_pos, const int32_t* tok_slot, const float* cos_tab,
                         const float* sin_tab, const f16_t* q_gain, const f16_t* k_gain, float eps, KVView kv,
                         hipStream_t s, const KVQ8View* q8) {
  if (T <= 0) return;
  const dim3 grid(T, (Hq + 2 * Hk + 3) / 4);
#define QN(SL_, Q8_, S_, R_, RS_)                                                                                  \
  MS_LAUNCH((qk_norm_rope_kernel<SL_, Q8_>), grid, dim3(256), 0, s, qkv, slabs, S_, R_, RS_, T, Hq, Hk, tok_pos, \
            tok_slot, cos_tab, sin_tab, q_gain, k_gain, eps, kv, Q8_ ? *q8 : KVQ8View{})
  if (q8) {
    if (slabs) QN(true, true, S, slab_rows, rs);
    else QN(false, true, 0, 0, RowScale{});
  } else {
    if (slabs) QN(true, false, S, slab_rows, rs);
    else QN(false, false, 0, 0, RowScale{});
  }
#undef QN
}

}  // namespace ms
