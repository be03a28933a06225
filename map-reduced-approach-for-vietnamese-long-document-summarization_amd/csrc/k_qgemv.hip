// k_qgemv.hip -- ggml K-quant and Q8_0 weights on gfx950: bit-exact dequantisation, the loader's
// packing kernel and the dequant-fused decode GEMV (BASELINE.json config 5).
//
// Ollama's default llama3.2:3b is Q4_K_M: Q4_K (144 B / 256 weights) for most matrices,
// Q6_K (210 B / 256 weights) for some (EXT: llama.cpp); the q5_K_M / q5_K_S / q4_K_S mixes add Q5_K,
// llama3.2:3b-instruct-q8_0 is Q8_0 throughout.  The dequantisers restate llama.cpp's
// dequantize_row_q4_K / _q5_K / _q6_K / _q8_0 (oracle/ggml_quants.c) with the non-contracted float
// forms  y = d1*q - m1,  y = (d*sc)*q  and  y = d*q  (__fmul_rn/__fsub_rn), so the fp32 result is
// bit-identical to the C restatement.
//
// Storage (engine.cpp): every quantised matrix keeps both
//   * a fp16 copy = f16(dequant(blocks)) in the fused row layout, for prefill GEMMs
//     and the embedding gather (compute-bound; fp16 is what MFMA consumes), and
//   * the quantised rows for decode, which is HBM-bound: 4.5 / 5.5 / 6.56 / 8.5 bits per weight
//     instead of 16, repacked by quant_rows_kernel so that one wave load instruction reads 64
//     contiguous bytes of each row.  The packed layouts, the per-lane register images and the
//     fragment arithmetic are stated once, in qblock.h.
// The fused GEMV streams the blocks HBM -> VGPR (one super-block of 256 weights per row
// per wave-step) and feeds v_mfma_f32_16x16x32_f16:
//   * Q4_K, one MFMA per 32-weight sub-block: the nibbles become the fp16 subnormals q 2^-24
//     by a byte permute, the MFMA gives A_s = 2^-24 sum_k x_k q_k, and sum_k x_k y_k =
//     (2^24 d_s) A_s - m_s X_s with ggml's fp32 d1 / m1 and X_s = sum of the sub-block's x (one
//     more MFMA, against ones, shared by the weight tiles of the block) -- 2 FMAs per output
//     element per sub-block instead of dequantising every weight: the decode GEMV uses the
//     exact fp32 dequantised weights (no fp16 rounding of them, and no cancellation: a
//     1024 + q bias form cost ~7e-6 relative against fp64);
//   * Q5_K: Q4_K's, sum order included -- a 5-bit code is still an exact fp16 subnormal q 2^-24;
//   * Q6_K, dequantised in registers to the fp16 values of the fp16 copy;
//   * Q8_0, one MFMA per 32-weight block on q held as the exact fp16 integers -128 .. 127,
//     A_b = sum_k x_k q_k, then acc = fma(d_b, A_b, acc) in fp32: the weights are never rounded
//     to fp16, out = sum_b d_b (sum_k x_k q_k).
#include <algorithm>
#include <cstdlib>

#include "qblock.h"

namespace ms {

// ---------------------------------------------------------------- dequantisers
// one 256-thread block per super-block, thread t -> weight t (the C loop order)
// raw Q4_K {d, dmin, scales[12], qs[128]} / Q5_K {.., qh[32], qs[128]}: weight t = 32 s + l of sub-block s
__device__ __forceinline__ float deq_kq_one(const uint8_t* b, int t, bool q5) {
  const int s = t >> 5, l = t & 31;
  float d1, m1;
  kq_scale_min(*(const uint4*)b, s, d1, m1);
  const uint32_t qb = b[(q5 ? kQ5RawQs : kQ4RawQs) + (t >> 6) * 32 + l];
  uint32_t q = (s & 1) ? (qb >> 4) : (qb & 0xF);
  if (q5) q += (((uint32_t)b[kQ5RawQh + l] >> s) & 1u) << 4;
  return __fsub_rn(__fmul_rn(d1, (float)q), m1);
}

// raw ggml Q6_K block: ql[128] qh[64] scales[16] d
__device__ __forceinline__ float deq_q6k_one(const uint8_t* b, int t) {
  const int n = t >> 7, r = t & 127, k4 = r >> 5, l = r & 31;
  const uint32_t a = b[n * 64 + l + ((k4 & 1) ? 32 : 0)];
  const uint32_t hb = b[kQ6Qh + n * 32 + l];
  const int q = (int)(((k4 >> 1) ? (a >> 4) : (a & 0xF)) | (((hb >> (2 * k4)) & 3) << 4)) - 32;
  const int sc = (int)(int8_t)b[kQ6Sc + n * 8 + (l >> 4) + 2 * k4];
  const float d = h2f_lo((uint32_t)b[kQ6D] | ((uint32_t)b[kQ6D + 1] << 8));
  return __fmul_rn(__fmul_rn(d, (float)sc), (float)q);
}

// raw unit of 8 ggml Q8_0 blocks {fp16 d; int8 qs[32]}: weight t is element t & 31 of block t >> 5
__device__ __forceinline__ float deq_q8_one(const uint8_t* b, int t) {
  const uint8_t* blk = b + kQ8RawBlock * (t >> 5);
  const float d = h2f_lo((uint32_t)blk[0] | ((uint32_t)blk[1] << 8));
  return __fmul_rn(d, (float)(int)(int8_t)blk[2 + (t & 31)]);
}

__device__ __forceinline__ float deq_one(int type, const uint8_t* b, int t) {
  return type == MS_QT_Q4_K || type == MS_QT_Q5_K ? deq_kq_one(b, t, type == MS_QT_Q5_K)
         : type == MS_QT_Q8_0                     ? deq_q8_one(b, t)
                                                  : deq_q6k_one(b, t);
}

__global__ __launch_bounds__(256) void dequant_f32_kernel(int type, const uint8_t* __restrict__ blocks,
                                                          float* __restrict__ out) {
  const size_t sb = blockIdx.x;
  const int t = threadIdx.x;
  out[sb * 256 + t] = deq_one(type, blocks + sb * qblock_bytes(type, false), t);
}

void launch_dequant_f32(int type, const uint8_t* blocks, int64_t n_blocks, float* out, hipStream_t s) {
  if (n_blocks <= 0) return;
  MS_LAUNCH(dequant_f32_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, type, blocks, out);
}

// rows of raw blocks -> (a) fp16 rows of the fused matrix, (b) packed quantised rows (qblock.h's layouts)
__global__ __launch_bounds__(256) void quant_rows_kernel(int type, const uint8_t* __restrict__ blocks,
                                                         int K, f16_t* __restrict__ dst_f16,
                                                         int map_mul, int map_add,
                                                         uint8_t* __restrict__ dst_q, int q_row_base) {
  const int r = blockIdx.y, sb = blockIdx.x, t = threadIdx.x;
  const int nsb = K / 256;
  const int braw = qblock_bytes(type, false);
  const uint8_t* b = blocks + ((size_t)r * nsb + sb) * braw;
  const float y = deq_one(type, b, t);
  const size_t drow = map_row(r, map_mul, map_add);
  dst_f16[drow * K + (size_t)sb * 256 + t] = f2h(y);
  if (dst_q) {
    const int bp = qblock_bytes(type, true);
    uint8_t* q = dst_q + ((drow - q_row_base) * nsb + sb) * bp;
    if (type == MS_QT_Q8_0) {
      if (t < 16) q[kQ8Sc + t] = b[kQ8RawBlock * (t >> 1) + (t & 1)];
      const int s_ = t >> 5, g = (t >> 3) & 3, i = t & 7;
      q[kQ8Q + 64 * (s_ >> 1) + 16 * g + 8 * (s_ & 1) + i] = b[kQ8RawBlock * s_ + 2 + (t & 31)];
    } else if (type == MS_QT_Q4_K || type == MS_QT_Q5_K) {
      // header as is; the nibbles from the raw qs (Q5_K's sit behind its qh); Q5_K's qh unmoved in value
      const int qs = type == MS_QT_Q5_K ? kQ5RawQs : kQ4RawQs;
      if (t < 16) q[kKqHdr + t] = b[t];
      if (t < 128) {
        const int g = t >> 5, s_ = (t >> 2) & 7, i = t & 3;
        auto nib = [&](int k) {
          const uint32_t qb = b[qs + (k >> 6) * 32 + (k & 31)];
          return ((k & 63) >> 5) ? (qb >> 4) : (qb & 0xF);
        };
        const int k = 32 * s_ + 8 * g + i;
        q[(s_ < 4 ? kKqNib0 : kKqNib1) + 16 * g + 4 * (s_ & 3) + i] = (uint8_t)(nib(k) | (nib(k + 4) << 4));
      } else if (type == MS_QT_Q5_K && t < 160) {
        q[kQ5Qh + (t - 128)] = b[kQ5RawQh + (t - 128)];
      }
    } else {
      // Q6_K: ql regrouped by the GEMV's lane group g = 2 hh + p, the other fields where they were,
      // the tail zeroed
      if (t < 128) {
        const int hh = t >> 6, half = (t >> 5) & 1, p = (t >> 4) & 1, i = t & 15;
        q[(half ? kQ6Ql1 : kQ6Ql0) + 16 * (2 * hh + p) + i] = b[t];
      } else if (t < braw) {
        q[t] = b[t];
      }
      if (t >= braw && t < kQ6KPacked) q[t] = 0;
    }
  }
}

void launch_quant_rows(int type, const uint8_t* blocks, int rows, int K, f16_t* dst_f16, int map_mul,
                       int map_add, uint8_t* dst_q, int q_row_base, hipStream_t s) {
  if (rows <= 0) return;
  MS_LAUNCH(quant_rows_kernel, dim3(K / 256, rows), dim3(256), 0, s, type, blocks, K, dst_f16,
            map_mul, map_add, dst_q, q_row_base);
}

// seeded random blocks (bench / config 5 synthetic weights): every byte from a counter
// hash, then the fp16 scale fields set so dequantised weights have std ~ `scale`
__device__ __forceinline__ uint64_t smix(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ void put_f16(uint8_t* p, _Float16 v) {
  const uint16_t u = __builtin_bit_cast(uint16_t, v);
  p[0] = u & 0xFF;
  p[1] = u >> 8;
}
// the K-quant header's d and dmin = ratio * d (of the rounded d)
__device__ __forceinline__ void put_d_dmin(uint8_t* b, float d, float ratio) {
  const _Float16 dh = (_Float16)d;
  put_f16(b, dh);
  put_f16(b + 2, (_Float16)((float)dh * ratio));
}

__global__ void synth_qblocks_kernel(int type, uint8_t* __restrict__ blocks, int64_t n_blocks,
                                     uint64_t seed_h, float scale) {
  const int braw = qblock_bytes(type, false);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_blocks;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t* b = blocks + i * braw;
    uint64_t h = smix((uint64_t)i ^ seed_h);
    for (int k = 0; k < braw; k += 8) {
      h = smix(h);
      for (int q = 0; q < 8 && k + q < braw; ++q) b[k + q] = (uint8_t)(h >> (8 * q));
    }
    const float u = 0.5f + (float)(smix(h) >> 40) * (1.0f / 16777216.0f);
    if (type == MS_QT_Q4_K) {
      put_d_dmin(b, u * scale / 270.f, 7.5f);
    } else if (type == MS_QT_Q5_K) {
      // sc, m uniform on 0..63 and q on 0..31: dmin = 15.5 d centres y / d = sc q - 15.5 m, whose
      // variance is E[sc^2] E[q^2] - (E[sc] E[q])^2 + 15.5^2 Var(m) = 434054 - 238388 + 81985, std 527;
      // with u on [0.5, 1.5) (rms 1.041) the weights have std ~ scale for d = u scale / 548
      put_d_dmin(b, u * scale / 548.f, 15.5f);
    } else if (type == MS_QT_Q8_0) {
      // uniform int8 quants have std 73.9; the 8 blocks' scales spread over [0.5, 1.5) scale / 74
      // (std of the weights 1.04 scale), positive normal fp16 for any scale >= 5e-3
      uint64_t hs = smix(h ^ 0x51ull);
      for (int k = 0; k < 8; ++k) {
        const float uk = 0.5f + (float)((hs >> (8 * k)) & 0xFF) * (1.0f / 256.0f);
        put_f16(b + kQ8RawBlock * k, (_Float16)(uk * scale / 74.f));
      }
    } else {
      for (int k = 0; k < 16; ++k) b[kQ6Sc + k] = (uint8_t)((int)(b[kQ6Sc + k] & 0x7F) - 64);
      put_f16(b + kQ6D, (_Float16)(u * scale / 680.f));
    }
  }
}

void launch_synth_qblocks(int type, uint8_t* blocks, int64_t n_blocks, uint64_t seed, float scale,
                          hipStream_t s) {
  MS_LAUNCH(synth_qblocks_kernel, dim3(2048), dim3(256), 0, s, type, blocks, n_blocks,
            (uint64_t)smix_host(seed), scale);
}

// ---------------------------------------------------------------- dequant-fused GEMV
// What qgemv_kernel and the grid-stride kernels share: each format's register image, fetch and
// code -> fragment functions (qblock.h), so a Q6_K tile is q6_frag in both.  The Q4_K / Q5_K and the
// Q8_0 multiply-accumulate are stated twice: kq_mac below serves the grid-stride gate/up kernel, and
// qgemv_kernel's two branches and the Q8_0 grid-stride loop write the same statements inline, because
// any shared function in those loop bodies moved the register allocation of spilling SwiGLU
// instantiations (the branches say which; profiles/qblock/README.md).  tests/test_gpu_qkernel_pins.py
// holds the copies to the same bits with the grid-stride forms on and off.
//
// Q4_K / Q5_K sub-block s (compile-time after unrolling): A = 2^-24 sum_k x_k q_k on the subnormal
// codes, then acc = fma(-m1, X_s, fma(2^24 d1, A, acc)); xs = kq_xsum(xf), shared by the weight tiles
__device__ __forceinline__ f32x4 kq_xsum(f16x8 xf) {
  // X_s = the sub-block's sum of each row's x: one more MFMA against ones (no separate pass over
  // X, no barrier)
  typedef uint32_t u4v __attribute__((ext_vector_type(4)));
  const f16x8 ones = __builtin_bit_cast(f16x8, u4v{0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u});
  return mfma16(xf, ones, f32x4{0.f, 0.f, 0.f, 0.f});
}
__device__ __forceinline__ f32x4 kq_mac(f32x4 acc, uint4 h, uint4 q0, uint4 q1, int s, f16x8 xf, f32x4 xs) {
  float d1, m1;
  kq_scale_min(h, s, d1, m1);
  const float d1s = d1 * 16777216.0f;  // d1 * 2^24 (exact)
  uint32_t lo, hi;
  kq_codes(q0, q1, s, lo, hi);
  const f32x4 A = mfma16(xf, subnormal_frag(lo, hi), f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = __fmaf_rn(-m1, xs[i], __fmaf_rn(d1s, A[i], acc[i]));
  return acc;
}

// X by LDS DMA has landed once at most the N weight loads issued after it are pending (vmcnt
// retires in issue order); no fence at the barrier: a fence would wait for the weight loads too
template <int N>
__device__ __forceinline__ void x_landed() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(vmcnt_imm(N));
  __builtin_amdgcn_s_barrier();
}

// One block per 16*NT rows, waves split the K/256 super-blocks (SBW per wave).  Lane group
// g = lane>>4 owns 64 weights of each super-block (qblock.h): k = 32s + 8g .. +7 of every sub-block s
// (Q4_K, Q5_K, Q8_0), or half hh = g>>1, positions [16p, 16p+16), p = g&1 (Q6_K).
// MFMA t of a super-block takes 8 of those weights per lane and the X elements of the
// same k -- a k permutation applied to both operands, so every dot product is unchanged.
// XM: the X source (gemv_common.h kXGlobal / kXLds / kXRegs, as in k_gemv.hip)
// QF: 0 = K-quant regions (Q4_K / Q6_K chosen per region at run time), MS_QT_Q8_0 = a Q8_0 matrix
// (its own instantiations: as a third run-time branch it raised the registers and the scratch of
// every K-quant instantiation, the kernel's allocation being the largest branch's), MS_QT_Q5_K = a
// K-quant matrix with a Q5_K region (regions Q4_K / Q5_K / Q6_K at run time; own instantiations for
// the same reason; matrices without one keep the QF = 0 instantiations).  There the Q4_K body
// serves both 4- and 5-bit regions: a fourth load per block fetches lane group g's qh bytes -- for
// a Q4_K region the header's first bytes, masked to zero -- so the load count, and with it the
// counted X wait, does not depend on the region's type
template <int QF, int MT, int NT, int EPI, int SBW, int XM, bool RS>
__global__ __launch_bounds__(1024) void qgemv_kernel(const f16_t* __restrict__ X, QMat qm,
                                                     void* __restrict__ out, int M, int N, int K,
                                                     int ldo, int rinv_off, GemvArgs ga) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float rsd = 0.f;  // the rows' deferred-norm statistics, ahead of every load
  if constexpr (RS) rsd = rs_begin<true>(smem, rinv_off, ga.rs, M);
  // split-K (fp32 slab epilogue only): block row y owns super-blocks [y*K/256, (y+1)*K/256)
  // of the full row, where K is the per-split length; X and out shift to that slab.
  const int ldx = K * gridDim.y, sbk = blockIdx.y * (K / 256);
  if constexpr (EPI == MS_GEMV_EPI_STORE_F32) {
    X += (size_t)blockIdx.y * K;
    out = (float*)out + (size_t)blockIdx.y * (ga.slab_rows > 0 ? ga.slab_rows : M) * ldo;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  // RESID_SSQ: ga.rt weight rows per tile (lanes fr >= rt load the last row again, never stored)
  constexpr bool RESID = EPI == MS_GEMV_EPI_RESID_SSQ;
  const int rt = RESID && ga.rt > 0 ? ga.rt : 16;
  const int n0 = RESID ? blockIdx.x * rt : blockIdx.x * 16 * NT;
  const int frw = RESID ? min(fr, rt - 1) : fr;  // this lane's weight row in the tile
  const ResidPre pre = resid_prefetch<EPI>(M, N, ldo, out, n0, ga);
  // the region holding this tile (regions are 16-row aligned; block-uniform)
  int type = qm.type0, row_bytes = qm.row_bytes0, rbase = n0 - qm.row0_0;
  const uint8_t* base = qm.base0;
  if (qm.n > 1 && n0 >= qm.row0_1) { type = qm.type1; row_bytes = qm.row_bytes1; rbase = n0 - qm.row0_1; base = qm.base1; }
  if (qm.n > 2 && n0 >= qm.row0_2) { type = qm.type2; row_bytes = qm.row_bytes2; rbase = n0 - qm.row0_2; base = qm.base2; }
  const int sb0 = wave * SBW;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr bool XL = XM == kXLds, XR = XM == kXRegs;
  // X first (LDS DMA of the block's rows, or this wave's super-blocks into registers), then
  // the weight stream: vmcnt retires in issue order
  if constexpr (XL) gemv_dma_x(smem, X, M, K, ldx);
  // Q4_K sub-block s of super-block j: lane group g's 8 weights at k = (j*8 + s)*32 + 8g;
  // Q6_K MFMA t: k = j*256 + hh*128 + (t>>1)*32 + 16p + 8(t&1)
  f16x8 xr[XR ? SBW : 1][XR ? 8 : 1][XR ? MT : 1];
  if constexpr (XR) {
    // Q8_0 and Q5_K blocks take Q4_K's k order
    const bool q6 = QF == MS_QT_Q5_K ? type == MS_QT_Q6_K : (QF != MS_QT_Q8_0 && type != MS_QT_Q4_K);
#pragma unroll
    for (int j = 0; j < SBW; ++j)
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const int k = q6 ? (sb0 + j) * 256 + (g >> 1) * 128 + (t >> 1) * 32 + 16 * (g & 1) + 8 * (t & 1)
                           : ((sb0 + j) * 8 + t) * 32 + 8 * g;
          xr[j][t][m] = as_f16x8(ldg16(X + (size_t)min(m * 16 + fr, M - 1) * ldx + k));
        }
  }
  // m-tile m's X fragment for MFMA t of this wave's super-block j (its 8 elements from k)
  auto xfrag = [&](int j, int t, int m, int k) -> f16x8 {
    const int xrow = min(m * 16 + fr, M - 1);
    return XR ? xr[XR ? j : 0][XR ? t : 0][XR ? m : 0]
           : XL ? *(const f16x8*)(smem + x_lds(xrow, k, K))
                : *(const f16x8*)(X + (size_t)xrow * ldx + k);
  };
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (QF == MS_QT_Q8_0) {
    // (the multiply-accumulate inline: through a shared function <Q8_0,2,2,SWIGLU,2,kXLds,false> went
    // from 460 to 488 B of scratch and <Q8_0,3,2,SWIGLU,2,kXLds,true> from 736 to 780 B)
    Q8Regs w[SBW][NT];
#pragma unroll
    for (int j = 0; j < SBW; ++j)
#pragma unroll
      for (int n = 0; n < NT; ++n)
        q8_fetch(w[j][n], base + (size_t)(rbase + n * 16) * row_bytes + (size_t)sbk * kQ8Bytes, row_bytes, frw,
                 sb0 + j, g);
    if constexpr (XL) {  // the X image has landed once at most the weight loads are pending
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_waitcnt(vmcnt_imm(5 * SBW * NT));
      __builtin_amdgcn_s_barrier();  // no fence: a fence would wait for the weight loads too
    }
#pragma unroll
    for (int j = 0; j < SBW; ++j)
#pragma unroll
      for (int s_ = 0; s_ < 8; ++s_) {
        const int k = ((sb0 + j) * 8 + s_) * 32 + 8 * g;  // as Q4_K: block s_, this lane group's 8 weights
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const float d = q8_scale(w[j][n], s_);
          const f16x8 wf = q8_frag(w[j][n], s_);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const int xrow = min(m * 16 + fr, M - 1);
            const f16x8 xf = XR ? xr[XR ? j : 0][XR ? s_ : 0][XR ? m : 0]
                            : XL ? *(const f16x8*)(smem + x_lds(xrow, k, K))
                                 : *(const f16x8*)(X + (size_t)xrow * ldx + k);
            // A_b = sum_k x_k q_k on the exact integers, then one fp32 FMA per output element
            const f32x4 A = mfma16(xf, wf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[m][n][i] = __fmaf_rn(d, A[i], acc[m][n][i]);
          }
        }
      }
  } else if (type == MS_QT_Q4_K || (QF == MS_QT_Q5_K && type == MS_QT_Q5_K)) {
    // kq_mac's arithmetic, statement for statement, but written out on loose arrays: with any shared
    // function in this loop body (kq_mac, or only kq_scale_min or kq_codes / subnormal_frag; by
    // reference, by value, as a struct image) the SwiGLU instantiations <0, 1, 2, SWIGLU, 2, kXLds, *>
    // went from 352 to 548-600 B of scratch (profiles/qblock/README.md).  tests/test_gpu_qkernel_pins.py
    // holds the two statements of it to the same bits (grid-stride on and off).
    constexpr bool Q5F = QF == MS_QT_Q5_K;
    const bool q5 = Q5F && type == MS_QT_Q5_K;  // block-uniform
    const int bbytes = q5 ? kQ5KBytes : kQ4KBytes;
    uint4 hq[SBW][NT], q0[SBW][NT], q1[SBW][NT];
    uint2 q5h[Q5F ? SBW : 1][Q5F ? NT : 1];  // Q5_K: qh[8g .. 8g + 7], the fifth bits of this lane group's weights
#pragma unroll
    for (int j = 0; j < SBW; ++j)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const uint8_t* bp = base + (size_t)(rbase + n * 16 + frw) * row_bytes + (size_t)(sbk + sb0 + j) * bbytes;
        hq[j][n] = ldw16(bp + kKqHdr);
        q0[j][n] = ldw16(bp + kKqNib0 + 16 * g);  // sub-blocks 0-3
        q1[j][n] = ldw16(bp + kKqNib1 + 16 * g);  // sub-blocks 4-7
        if constexpr (Q5F) q5h[j][n] = *(const uint2*)(bp + (q5 ? kQ5Qh + 8 * g : 0));
      }
    if constexpr (XL) x_landed<(Q5F ? 4 : 3) * SBW * NT>();
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    const f16x8 ones = __builtin_bit_cast(f16x8, u4v{0x3C003C00u, 0x3C003C00u, 0x3C003C00u, 0x3C003C00u});
#pragma unroll
    for (int j = 0; j < SBW; ++j)
#pragma unroll
      for (int s_ = 0; s_ < 8; ++s_) {
        const int k = ((sb0 + j) * 8 + s_) * 32 + 8 * g;  // this lane group's 8 weights
        const int sh = 8 * (s_ & 3);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const f16x8 xf = xfrag(j, s_, m, k);
          // X_s = the sub-block's sum of each row's x: one more MFMA against ones, shared by
          // the NT weight tiles (no separate pass over X, no barrier)
          const f32x4 xs = mfma16(xf, ones, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            // get_scale_min_k4 of sub-block s_ from the 12 scale bytes (header words y, z, w)
            const uint4 h = hq[j][n];
            const uint32_t scw = s_ < 4 ? (h.y & 0x3F3F3F3Fu) : ((h.w & 0x0F0F0F0Fu) | ((h.y >> 2) & 0x30303030u));
            const uint32_t mw = s_ < 4 ? (h.z & 0x3F3F3F3Fu) : (((h.w >> 4) & 0x0F0F0F0Fu) | ((h.z >> 2) & 0x30303030u));
            const float d1 = __fmul_rn(h2f_lo(h.x), (float)((scw >> sh) & 0xFFu));        // ggml d1 = d * sc
            const float m1 = __fmul_rn(h2f_lo(h.x >> 16), (float)((mw >> sh) & 0xFFu));   // ggml m1 = dmin * m
            const float d1s = d1 * 16777216.0f;                                  // d1 * 2^24 (exact)
            const uint4 qq = s_ < 4 ? q0[j][n] : q1[j][n];
            const int si = s_ & 3;
            const uint32_t qw = si == 0 ? qq.x : si == 1 ? qq.y : si == 2 ? qq.z : qq.w;
            uint32_t lo = qw & 0x0F0F0F0Fu, hi = (qw >> 4) & 0x0F0F0F0Fu;
            if constexpr (Q5F) {  // bit s_ of qh[8g + i] is weight k + i's fifth bit (none in a Q4_K region)
              const uint32_t hm = q5 ? 0x01010101u : 0u;
              lo |= ((q5h[j][n].x >> s_) & hm) << 4;
              hi |= ((q5h[j][n].y >> s_) & hm) << 4;
            }
            // bytes [q, 0, q', 0] = the fp16 subnormals q * 2^-24, q' * 2^-24 (exact): weights
            // k .. k+7 in order (perm selector 0x0C is the constant byte 0)
            const u4v pk = {__builtin_amdgcn_perm(0u, lo, 0x0C010C00u), __builtin_amdgcn_perm(0u, lo, 0x0C030C02u),
                            __builtin_amdgcn_perm(0u, hi, 0x0C010C00u), __builtin_amdgcn_perm(0u, hi, 0x0C030C02u)};
            const f32x4 A = mfma16(xf, __builtin_bit_cast(f16x8, pk), f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[m][n][i] = __fmaf_rn(-m1, xs[i], __fmaf_rn(d1s, A[i], acc[m][n][i]));
          }
        }
      }
  } else {  // Q6_K, packed 224-B blocks
    const int hh = g >> 1, p = g & 1;
    // one instantiation picks its scale byte by q6_frag's 64-bit form: with the 32-bit select, which every
    // other kernel keeps (it took 48 B of scratch off the SBW = 2 ones), <0,2,2,SWIGLU,1,kXLds,false>
    // spilled 424 B for the parent's 416; the 64-bit form everywhere cost nine kernels a wave
    // (profiles/qblock/README.md).  Same byte, same bits.
    constexpr bool kSel64 = QF == 0 && MT == 2 && NT == 2 && SBW == 1 && XL && !RS;
    uint4 qa[SBW][NT], qb[SBW][NT], qh[SBW][NT], sc[SBW][NT];
    uint32_t dw[SBW][NT];
#pragma unroll
    for (int j = 0; j < SBW; ++j)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const uint8_t* bp = base + (size_t)(rbase + n * 16 + frw) * row_bytes + (size_t)(sbk + sb0 + j) * kQ6KPacked;
        qa[j][n] = ldw16(bp + kQ6Ql0 + 16 * g);
        qb[j][n] = ldw16(bp + kQ6Ql1 + 16 * g);
        qh[j][n] = ldw16(bp + kQ6Qh + hh * 32 + 16 * p);
        sc[j][n] = ldw16(bp + kQ6Sc);
        dw[j][n] = *(const uint32_t*)(bp + kQ6D);
      }
    if constexpr (XL) x_landed<5 * SBW * NT>();
#pragma unroll
    for (int j = 0; j < SBW; ++j)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float d = h2f_lo(dw[j][n]);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const int k4 = t >> 1, sub = t & 1;
          const f16x8 wf = q6_frag<kSel64>(qa[j][n], qb[j][n], qh[j][n], sc[j][n], d, t, hh, p);
          const int k = (sb0 + j) * 256 + hh * 128 + k4 * 32 + 16 * p + 8 * sub;
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][n] = mfma16(xfrag(j, t, m, k), wf, acc[m][n]);
        }
      }
  }
  gemv_finish<MT, NT, EPI, RS>(acc, smem, rinv_off, M, N, ldo, out, n0, ga, pre, rsd);
}

// ---- grid-stride forms.  One-tile blocks (qgemv_kernel) each stage the whole X and pay one exposed
// weight latency per tile; here resident blocks stage X and the rows' norm factors once, then walk
// tiles b, b + G, ... with the next tile's weight loads in flight under the current tile's
// multiply, and the per-tile cross-wave reduction uses LDS-only barriers so those loads stay in
// flight.  Wave w owns super-block w (SBW = 1), MT = 1.
//
// once the first tile's LOADS weight loads are issued: X and the statistics (issued first) landed
template <int LOADS>
__device__ __forceinline__ void gs_staged(char* smem, int rinv_off, const GemvArgs& ga, int M, bool rs_on) {
  x_landed<LOADS>();
  if (rs_on) rs_finish<false>(smem, rinv_off, ga.rs, M, 0.f);
  lds_sync();
}
// the argmax kernels' first steps: row statistics and X once per block, ahead of the first tile's weights
__device__ __forceinline__ bool gs_argmax_begin(char* smem, const f16_t* X, int M, int K, int rinv_off,
                                                const GemvArgs& ga) {
  const bool rs_on = ga.rs.ssq != nullptr;
  if (rs_on) rs_begin<false>(smem, rinv_off, ga.rs, M);
  gemv_dma_x(smem, X, M, K, K);
  __builtin_amdgcn_sched_barrier(0);
  return rs_on;
}
// tile t's cross-wave reduction and argmax partials (gemv_epilogue's order; LDS-only barriers: the
// next tile's loads stay in flight)
__device__ __forceinline__ void gs_argmax_tile(f32x4 acc, float* red, const float* rinv, bool rs_on, int t, int M,
                                               int N, int ldo, float2* out) {
  constexpr int ELEMS = 256;  // MT = NT = 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  *(f32x4*)&red[wave * ELEMS + lane * 4] = acc;
  lds_sync();
  if ((int)threadIdx.x < ELEMS) {
    const int e = threadIdx.x, l = (e >> 2) & 63, j = e & 3;
    const int row = 4 * (l >> 4) + j, col = t * 16 + (l & 15);
    float v = -INFINITY;
    if (row < M && col < N) {
      float sum = 0.f;
      for (int q = 0; q < nw; ++q) sum += red[q * ELEMS + e];
      v = sum * (rs_on ? rinv[row] : 1.0f);
    }
    if (!(v == v)) v = -INFINITY;
    int idx = col;
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) amax_merge_dev(v, idx, __shfl_xor(v, o, 64), __shfl_xor(idx, o, 64));
    // (a 32-bit offset from the scalar base: a 64-bit lane address held across the loop spilled)
    if ((l & 15) == 0 && row < M)
      *(float2*)((char*)out + (uint32_t)(row * ldo + t) * 8u) = make_float2(v, __int_as_float(idx));
  }
  lds_sync();  // red is rewritten by the next tile
}

// ---- the Q6_K lm_head (greedy argmax partials).  One-tile blocks each DMA the whole X image
// (M x K fp16: 48 KiB at M = 8 -- 385 MB over the vocabulary's 8016 tiles, more than the weights'
// 323 MB); here 2 x 256 resident blocks stage it once, and each wave issues the NEXT tile's weight
// loads (17 VGPRs) before it dequantises and multiplies the current one.  Per tile the arithmetic is
// qgemv_kernel<0, 1, 1, ARGMAX, 1, LDS, false>'s (same K split over waves, same MFMA order, same
// reduction order and epilogue): bit-identical partials.  launch_qgemv clears the row scale for the
// argmax (a row's positive scale never moves its argmax), as qgemv_go does for the one-tile kernels:
// rs_on is false in every launch today, and the rinv path is kept for a caller that wants scaled maxima.
__global__ __launch_bounds__(768) __attribute__((amdgpu_waves_per_eu(6, 8))) void qgemv_q6_argmax_gs_kernel(const f16_t* __restrict__ X, QMat qm,
                                                                float2* __restrict__ out, int M, int N, int K,
                                                                int ldo, int red_off, int rinv_off, GemvArgs ga) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4, hh = g >> 1, p = g & 1;
  const int tiles = N / 16, G = gridDim.x;
  const uint8_t* base = qm.base0;
  const int row_bytes = qm.row_bytes0;
  // this lane's block of tile t: row 16 t + fr, super-block `wave`
  auto block = [&](int t) { return base + (size_t)(t * 16 + fr) * row_bytes + (size_t)wave * kQ6KPacked; };
  const bool rs_on = gs_argmax_begin(smem, X, M, K, rinv_off, ga);
  Q6Regs cur, nxt;
  int t = blockIdx.x;
  q6_fetch(cur, block(t), g);
  gs_staged<5>(smem, rinv_off, ga, M, rs_on);
  const float* rinv = (const float*)(smem + rinv_off);
  float* red = (float*)(smem + red_off);
  for (; t < tiles; t += G) {
    const bool more = t + G < tiles;
    if (more) q6_fetch(nxt, block(t + G), g);
    __builtin_amdgcn_sched_barrier(0);
    if (more) __builtin_amdgcn_s_waitcnt(vmcnt_imm(5));
    else __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float d = h2f_lo(cur.dw);
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
      const int k = wave * 256 + hh * 128 + (tt >> 1) * 32 + 16 * p + 8 * (tt & 1);
      acc = mfma16(*(const f16x8*)(smem + x_lds(min(fr, M - 1), k, K)), q6_frag(cur, d, tt, hh, p), acc);
    }
    gs_argmax_tile(acc, red, rinv, rs_on, t, M, N, ldo, out);
    cur = nxt;
  }
}

// ---- the Q8_0 lm_head (418 MB, the largest stream of a Q8_0 step) in the same form, the next
// tile's 5 loads in flight under the current tile's 8 MFMAs -- issued in two halves, the second once
// blocks 0-3 are multiplied and their 8 VGPRs free (both tiles whole, 40 VGPRs, spilled under
// the 80-VGPR cap of two resident 12-wave blocks per CU).  Per tile the arithmetic is
// qgemv_kernel<Q8_0, 1, 1, ARGMAX, 1, LDS, false>'s: bit-identical partials.
__global__ __launch_bounds__(768) __attribute__((amdgpu_waves_per_eu(6, 8))) void qgemv_q8_argmax_gs_kernel(const f16_t* __restrict__ X, QMat qm,
                                                                float2* __restrict__ out, int M, int N, int K,
                                                                int ldo, int red_off, int rinv_off, GemvArgs ga) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int tiles = N / 16, G = gridDim.x;
  const uint8_t* base = qm.base0;
  const int row_bytes = qm.row_bytes0;
  const bool rs_on = gs_argmax_begin(smem, X, M, K, rinv_off, ga);
  Q8Regs cur, nxt;
  int t = blockIdx.x;
  q8_fetch(cur, base + (size_t)t * 16 * row_bytes, row_bytes, fr, wave, g);
  gs_staged<5>(smem, rinv_off, ga, M, rs_on);
  const float* rinv = (const float*)(smem + rinv_off);
  float* red = (float*)(smem + red_off);
  // this lane's X fragment of block s_: chunk (wave * 32 + 4 s_ + g) ^ (row & 7) of its row; the
  // swizzle touches chunk bits 0-2 only, so block s_ sits 128 (s_ >> 1) bytes behind block s_ & 1
  // (two addresses live across the tile loop instead of eight)
  const int xrow = min(fr, M - 1);
  const char* xs0 = smem + x_lds(xrow, wave * 256 + 8 * g, K);
  const char* xs1 = smem + x_lds(xrow, wave * 256 + 32 + 8 * g, K);
  for (; t < tiles; t += G) {
    const bool more = t + G < tiles;
    const uint32_t ntile = (uint32_t)(t + G) * 16u * (uint32_t)row_bytes;
    if (more) q8_fetch_half<0>(nxt, base, ntile, row_bytes, fr, wave, g);
    __builtin_amdgcn_sched_barrier(0);
    // the waits for `cur` are the compiler's own (register dependencies: no DMA is in flight here)
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s_ = 0; s_ < 8; ++s_) {
      if (s_ == 4) {
        if (more) q8_fetch_half<1>(nxt, base, ntile, row_bytes, fr, wave, g);
        __builtin_amdgcn_sched_barrier(0);
      }
      const float d = q8_scale(cur, s_);
      const f16x8 xf = *(const f16x8*)(((s_ & 1) ? xs1 : xs0) + 128 * (s_ >> 1));
      const f32x4 A = mfma16(xf, q8_frag(cur, s_), f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = __fmaf_rn(d, A[i], acc[i]);
      // two blocks' products in flight at most: all eight cost 32 VGPRs and spilled the prefetch
      if (s_ & 1) __builtin_amdgcn_sched_barrier(0);
    }
    gs_argmax_tile(acc, red, rinv, rs_on, t, M, N, ldo, out);
    cur = nxt;
  }
}

// ---- the Q4_K gate/up projection (SwiGLU epilogue): 256 blocks of 12 waves (wave w = super-block
// w of the 3072-long rows) take X into registers ONCE (the one-tile kernel's 512 blocks each re-read
// the 8 x 3072 X -- 49 MB of L2 traffic against 28 MB of weights), then walk 32-row tiles (16 gate
// + 16 up rows) with the next tile's 6 weight loads per lane in flight under the current tile's
// dequant.  Per tile the arithmetic is qgemv_kernel<0, 1, 2, SWIGLU, 1, REGS, RS>'s: bit-identical
// outputs.
__global__ __launch_bounds__(768) void qgemv_q4_swiglu_gs_kernel(const f16_t* __restrict__ X, QMat qm,
                                                                 f16_t* __restrict__ out, int M, int N, int K,
                                                                 int ldo, int rinv_off, GemvArgs ga) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = 2, ELEMS = NT * 256;  // MT = 1
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int fr = lane & 15, g = lane >> 4;
  const int tiles = N / 32, G = gridDim.x;
  const uint8_t* base = qm.base0;
  const int row_bytes = qm.row_bytes0, row0 = qm.row0_0;
  const bool rs_on = ga.rs.ssq != nullptr;
  if (rs_on) rs_begin<false>(smem, rinv_off, ga.rs, M);
  // this wave's super-block of X (qgemv_kernel's kXRegs load, SBW = 1, MT = 1)
  f16x8 xr[8];
  const f16_t* xrow = X + (size_t)min(fr, M - 1) * K;
#pragma unroll
  for (int t = 0; t < 8; ++t) xr[t] = as_f16x8(ldg16(xrow + (wave * 8 + t) * 32 + 8 * g));
  __builtin_amdgcn_sched_barrier(0);
  // tile t's weight tile n: this lane's row 32 t - row0 + 16 n + fr, super-block `wave`
  auto fetch = [&](KqRegs (&r)[NT], int t) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
      kq_fetch(r[n], base + (size_t)(t * 32 - row0 + n * 16 + fr) * row_bytes + (size_t)wave * kQ4KBytes, g);
  };
  KqRegs cur[NT], nxt[NT];
  int t = blockIdx.x;
  fetch(cur, t);
  gs_staged<3 * NT>(smem, rinv_off, ga, M, rs_on);
  const float* rinv = (const float*)(smem + rinv_off);
  float* red = (float*)smem;
  for (; t < tiles; t += G) {
    const bool more = t + G < tiles;
    if (more) fetch(nxt, t + G);
    __builtin_amdgcn_sched_barrier(0);
    if (more) __builtin_amdgcn_s_waitcnt(vmcnt_imm(3 * NT));
    else __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s_ = 0; s_ < 8; ++s_) {
      const f32x4 xs = kq_xsum(xr[s_]);
#pragma unroll
      for (int n = 0; n < NT; ++n) acc[n] = kq_mac(acc[n], cur[n].h, cur[n].q0, cur[n].q1, s_, xr[s_], xs);
    }
    // cross-wave reduction and the SwiGLU epilogue (gemv_epilogue's order), LDS-only barriers
#pragma unroll
    for (int n = 0; n < NT; ++n) *(f32x4*)&red[wave * ELEMS + (n * 64 + lane) * 4] = acc[n];
    lds_sync();
    if ((int)threadIdx.x < 256) {
      const int e = threadIdx.x, l = (e >> 2) & 63, j = e & 3;
      const int row = 4 * (l >> 4) + j;
      if (row < M) {
        const float rv = rs_on ? rinv[row] : 1.0f;
        float gs = 0.f, us = 0.f;
        for (int q = 0; q < nw; ++q) gs += red[q * ELEMS + (0 * 64 + l) * 4 + j];
        for (int q = 0; q < nw; ++q) us += red[q * ELEMS + (1 * 64 + l) * 4 + j];
        const float gv = gs * rv, uv = us * rv;
        out[(size_t)row * ldo + t * 16 + (l & 15)] = f2h(gv / (1.0f + __expf(-gv)) * uv);
      }
    }
    lds_sync();  // red is rewritten by the next tile
#pragma unroll
    for (int n = 0; n < NT; ++n) cur[n] = nxt[n];
  }
}

// which quantised GEMVs take the grid-stride form: MS_QGEMV_GS bit 0 the Q6_K lm_head argmax,
// bit 1 the Q4_K gate/up, bit 2 the Q8_0 lm_head argmax (default 3: the two K-quant forms;
// ms_set_qgemv_gs(1): all three, (0): one-tile blocks everywhere).  The Q8_0 form is off by
// default: it measured slower than the one-tile blocks, 99.4 vs 86.3 us per lm_head launch at 8
// slots (profiles/q8_0/) -- a tile is 8 MFMAs per wave, too little work to cover the two block
// barriers and the prefetch wait each tile costs, where Q6_K's dequantisation covers them.  The
// same form for the single-type split-K slab projections (O, down: X slice staged once per
// block) measured slower -- O 5.10 -> 6.04 us, down 8.89 -> 9.4-10.7 us, decode 1.806 -> 1.871
// ms per Q4_K_M step (profiles/r04/v25_*): those launches are one latency each, and fewer
// blocks leave fewer weight bytes in flight.
static int g_q_gs = -1;
void set_qgemv_gs(bool on) { g_q_gs = on ? 7 : 0; }
static int q_gs_mask() {
  if (g_q_gs < 0) {
    const char* e = getenv("MS_QGEMV_GS");
    g_q_gs = e ? atoi(e) : 3;
  }
  return g_q_gs;
}
static bool q6_gs_on() { return (q_gs_mask() & 1) != 0; }
static bool q4_gs_on() { return (q_gs_mask() & 2) != 0; }
static bool q8_gs_on() { return (q_gs_mask() & 4) != 0; }


struct QPlan {
  int MT, NT, SBW, waves, tiles;
};

static QPlan qplan(int M, int N, int K, int epi, int rt = 0) {  // K: per-split length
  QPlan p{};
  p.MT = (M + 15) / 16;
  p.NT = (epi == MS_GEMV_EPI_SWIGLU) ? 2 : 1;
  const int rows = epi == MS_GEMV_EPI_RESID_SSQ && rt > 0 ? rt : 16 * p.NT;
  p.tiles = (N + rows - 1) / rows;
  const int nsb = K / 256;
  p.SBW = nsb > 16 ? 2 : 1;
  p.waves = (nsb % p.SBW == 0) ? nsb / p.SBW : 0;
  if (p.waves > 16) p.waves = 0;
  return p;
}

static constexpr size_t kLdsCap = 160 * 1024;

// the X image is staged in LDS only when the whole block's LDS -- the image, the deferred-norm
// factors and the staged statistics (gemv_lds_total) -- fits; a shape whose image alone fits
// (M = 40 at K = 2048: exactly 160 KiB) takes the global-X path instead of being refused
// (a refused split once made one row group of a K-quant batch fall back to an unsplit slab
// while the others split 4 ways, and the residual fold then dropped slabs of every row)
static bool qx_in_lds(int M, int K, const RowScale& rs = RowScale{}) {
  return gemv_lds_total(gemv_x_lds_bytes(M, K), rs, M) <= kLdsCap;
}

static bool qx_in_regs(const QPlan& p) {
  const int m = qgemv_x_mode();
  const bool want = m == 0 || (m == 2 && p.NT == 2) || (m == 3 && p.NT != 2);
  return want && p.MT * p.SBW == 1;
}

static size_t qlds_main(const QPlan& p, int M, int K, const RowScale& rs = RowScale{}) {
  // X image (when it fits and X is not taken into registers)
  const size_t xs = (!qx_in_regs(p) && qx_in_lds(M, K, rs)) ? gemv_x_lds_bytes(M, K) : 0;
  const size_t red = (size_t)p.waves * p.MT * p.NT * 256 * 4;
  return xs > red ? xs : red;
}
static size_t qlds(const QPlan& p, int M, int K, const RowScale& rs = RowScale{}) {
  return gemv_lds_total(qlds_main(p, M, K, rs), rs, M);
}

bool qgemv_supported(int M, int N, int K, int epi, int rs_tiles) {
  if (M < 1 || M > 64 || K % 256 || N % 16) return false;
  if ((epi == MS_GEMV_EPI_ROPE_KV || epi == MS_GEMV_EPI_RESID_SSQ) && M > 16) return false;
  const QPlan p = qplan(M, N, K, epi);
  // the residual epilogue's prefetch covers one element per thread of a >= 256-thread block
  if (epi == MS_GEMV_EPI_RESID_SSQ && p.waves < 4) return false;
  RowScale rs{};
  if (rs_tiles > 0 && epi != MS_GEMV_EPI_ARGMAX && epi != MS_GEMV_EPI_ADD_F32) {  // qgemv_go drops it there
    if (!gemv_rs_supported(M, rs_tiles)) return false;
    rs = make_row_scale(reinterpret_cast<const float*>(16), rs_tiles, 1, 0.f);
  }
  return p.waves > 0 && qlds(p, M, K, rs) <= kLdsCap;
}

template <int MT, int NT, int EPI>
static void qgemv_go(const f16_t* X, const QMat& q, void* out, int M, int N, int K, int ldo,
                     const QPlan& p, const GemvArgs& ga_in, hipStream_t s, int S = 1) {
  GemvArgs ga = ga_in;
  if (EPI == MS_GEMV_EPI_ARGMAX || EPI == MS_GEMV_EPI_ADD_F32) ga.rs = RowScale{};  // r > 0 keeps the order
  if (ga.rs.ssq && rs_stage_floats(ga.rs, M) == 0) return;  // callers check gemv_rs_supported
  const size_t lds = qlds(p, M, K, ga.rs);
  const int ro = (int)gemv_rinv_offset(qlds_main(p, M, K, ga.rs));
  const dim3 grid(p.tiles, S), blk(64 * p.waves);
  if constexpr ((EPI == MS_GEMV_EPI_ROPE_KV || EPI == MS_GEMV_EPI_RESID_SSQ) && MT != 1) {
    return;
  } else {
    const bool xl = qx_in_lds(M, K, ga.rs);
    constexpr bool kRsEpi = gemv_rs_epi<EPI>();
    const bool rs = kRsEpi && ga.rs.ssq != nullptr;
    const bool q8 = q.type0 == MS_QT_Q8_0;  // an engine's matrices are all Q8_0 or all K-quant
    // a K-quant matrix with a Q5_K region: the instantiations whose run-time branches include it
    const bool q5 = q.type0 == MS_QT_Q5_K || (q.n > 1 && q.type1 == MS_QT_Q5_K) || (q.n > 2 && q.type2 == MS_QT_Q5_K);
#define QLF(SBW_, XM_, RS_)                                                                                   \
    do {                                                                                                      \
      if (q8)                                                                                                 \
        MS_LAUNCH((qgemv_kernel<MS_QT_Q8_0, MT, NT, EPI, SBW_, XM_, RS_>), grid, blk, lds, s, X, q, out, M, N, K, \
                  ldo, ro, ga);                                                                               \
      else if (q5)                                                                                            \
        MS_LAUNCH((qgemv_kernel<MS_QT_Q5_K, MT, NT, EPI, SBW_, XM_, RS_>), grid, blk, lds, s, X, q, out, M, N, K, \
                  ldo, ro, ga);                                                                               \
      else                                                                                                    \
        MS_LAUNCH((qgemv_kernel<0, MT, NT, EPI, SBW_, XM_, RS_>), grid, blk, lds, s, X, q, out, M, N, K, ldo, ro, \
                  ga);                                                                                        \
    } while (0)
#define QL(SBW_, XM_)                                                                                         \
    do {                                                                                                      \
      if constexpr (kRsEpi) {                                                                                 \
        if (rs) {                                                                                             \
          QLF(SBW_, XM_, true);                                                                               \
          break;                                                                                              \
        }                                                                                                     \
      }                                                                                                       \
      QLF(SBW_, XM_, false);                                                                                  \
    } while (0)
    if (p.SBW == 2 && xl) QL(2, kXLds);
    else if (p.SBW == 2) QL(2, kXGlobal);
    else if (xl && !qx_in_regs(p)) QL(1, kXLds);
    else if (!qx_in_regs(p)) QL(1, kXGlobal);
    else if constexpr (MT == 1) QL(1, kXRegs);
#undef QL
#undef QLF
  }
}

template <int MT>
static void qgemv_go_mt(const f16_t* X, const QMat& q, void* out, int M, int N, int K, int ldo, int epi,
                        const QPlan& p, const GemvArgs& ga, hipStream_t s) {
  switch (epi) {
    case MS_GEMV_EPI_STORE_F16: qgemv_go<MT, 1, MS_GEMV_EPI_STORE_F16>(X, q, out, M, N, K, ldo, p, ga, s); break;
    case MS_GEMV_EPI_ADD_F32: qgemv_go<MT, 1, MS_GEMV_EPI_ADD_F32>(X, q, out, M, N, K, ldo, p, ga, s); break;
    case MS_GEMV_EPI_SWIGLU: qgemv_go<MT, 2, MS_GEMV_EPI_SWIGLU>(X, q, out, M, N, K, ldo, p, ga, s); break;
    case MS_GEMV_EPI_ROPE_KV: qgemv_go<MT, 1, MS_GEMV_EPI_ROPE_KV>(X, q, out, M, N, K, ldo, p, ga, s); break;
    case MS_GEMV_EPI_ARGMAX: qgemv_go<MT, 1, MS_GEMV_EPI_ARGMAX>(X, q, out, M, N, K, ldo, p, ga, s); break;
    case MS_GEMV_EPI_RESID_SSQ: qgemv_go<MT, 1, MS_GEMV_EPI_RESID_SSQ>(X, q, out, M, N, K, ldo, p, ga, s); break;
    default: qgemv_go<MT, 1, MS_GEMV_EPI_STORE_F32>(X, q, out, M, N, K, ldo, p, ga, s); break;
  }
}

void launch_qgemv(const f16_t* X, const QMat& q, void* out, int M, int N, int K, int ldo, int epi,
                  const GemvArgs* ga_in, hipStream_t s) {
  if (M <= 0) return;
  const QPlan p = qplan(M, N, K, epi, ga_in ? ga_in->rt : 0);
  if (p.waves == 0) return;  // callers check qgemv_supported()
  GemvArgs ga{};
  if (ga_in) ga = *ga_in;
  // (both grid-stride kernels finish a tile with one thread per element: >= 4 waves)
  const bool lm_q6 = q6_gs_on() && q.type0 == MS_QT_Q6_K, lm_q8 = q8_gs_on() && q.type0 == MS_QT_Q8_0;
  if (epi == MS_GEMV_EPI_ARGMAX && (lm_q6 || lm_q8) && q.n == 1 && p.MT == 1 && p.SBW == 1 &&
      p.waves >= 4 && p.waves <= 12 && N % 16 == 0 &&  // (the kernels' launch bounds: 12 waves)
      (!lm_q8 || (uint64_t)N * (uint64_t)q.row_bytes0 < (1ull << 32))) {  // (its 32-bit tile offsets)
    ga.rs = RowScale{};  // as qgemv_go: a row's positive scale never moves its argmax
    // LDS: [X image][per-wave partials][rinv][staged statistics]
    const int red_off = (int)((gemv_x_lds_bytes(M, K) + 15) / 16 * 16);
    const size_t main_bytes = (size_t)red_off + (size_t)p.waves * 256 * 4;
    const int ro = (int)gemv_rinv_offset(main_bytes);
    const size_t lds = gemv_lds_total(main_bytes, ga.rs, M);
    if (lds <= kLdsCap) {
      const int grid = std::min(N / 16, 512);  // two resident blocks per CU
      if (lm_q8)
        MS_LAUNCH(qgemv_q8_argmax_gs_kernel, dim3(grid), dim3(64 * p.waves), lds, s, X, q, (float2*)out, M, N, K,
                  ldo, red_off, ro, ga);
      else
        MS_LAUNCH(qgemv_q6_argmax_gs_kernel, dim3(grid), dim3(64 * p.waves), lds, s, X, q, (float2*)out, M, N, K,
                  ldo, red_off, ro, ga);
      return;
    }
  }
  if (epi == MS_GEMV_EPI_SWIGLU && q4_gs_on() && q.n == 1 && q.type0 == MS_QT_Q4_K && p.MT == 1 && p.SBW == 1 &&
      p.NT == 2 && p.waves >= 4 && qx_in_regs(p) && N % 32 == 0) {
    if (ga.rs.ssq && rs_stage_floats(ga.rs, M) == 0) return;  // callers check gemv_rs_supported
    const size_t main_bytes = (size_t)p.waves * 2 * 256 * 4;  // the per-wave partials
    const int ro = (int)gemv_rinv_offset(main_bytes);
    const size_t lds = gemv_lds_total(main_bytes, ga.rs, M);
    if (lds <= kLdsCap) {
      const int grid = std::min(N / 32, 256);  // one 12-wave block per CU
      MS_LAUNCH(qgemv_q4_swiglu_gs_kernel, dim3(grid), dim3(64 * p.waves), lds, s, X, q, (f16_t*)out, M, N, K,
                ldo, ro, ga);
      return;
    }
  }
  switch (p.MT) {
    case 1: qgemv_go_mt<1>(X, q, out, M, N, K, ldo, epi, p, ga, s); break;
    case 2: qgemv_go_mt<2>(X, q, out, M, N, K, ldo, epi, p, ga, s); break;
    case 3: qgemv_go_mt<3>(X, q, out, M, N, K, ldo, epi, p, ga, s); break;
    default: qgemv_go_mt<4>(X, q, out, M, N, K, ldo, epi, p, ga, s); break;
  }
}

bool qgemv_split_supported(int M, int N, int K, int S, int rs_tiles) {
  if (S < 1 || K % (256 * S)) return false;
  return qgemv_supported(M, N, K / S, MS_GEMV_EPI_STORE_F32, rs_tiles);
}

// fp32 partial slabs [S][M][N] over S equal K ranges (super-block aligned); the caller
// folds them (residual_rmsnorm_kernel / the decode attention prologue)
void launch_qgemv_split(const f16_t* X, const QMat& q, float* slabs, int M, int N, int K, int S,
                        hipStream_t s, const GemvArgs* ga_in) {
  if (M <= 0) return;
  const int Ks = K / S;
  const QPlan p = qplan(M, N, Ks, MS_GEMV_EPI_STORE_F32);
  if (p.waves == 0) return;  // callers check qgemv_split_supported()
  GemvArgs ga{};
  if (ga_in) ga = *ga_in;
  switch (p.MT) {
    case 1: qgemv_go<1, 1, MS_GEMV_EPI_STORE_F32>(X, q, slabs, M, N, Ks, N, p, ga, s, S); break;
    case 2: qgemv_go<2, 1, MS_GEMV_EPI_STORE_F32>(X, q, slabs, M, N, Ks, N, p, ga, s, S); break;
    case 3: qgemv_go<3, 1, MS_GEMV_EPI_STORE_F32>(X, q, slabs, M, N, Ks, N, p, ga, s, S); break;
    default: qgemv_go<4, 1, MS_GEMV_EPI_STORE_F32>(X, q, slabs, M, N, Ks, N, p, ga, s, S); break;
  }
}

}  // namespace ms
