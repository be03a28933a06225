// k_gemv.hip -- decode projections of the map call: weight-streaming skinny GEMM.
//
// Replaces ggml mul_mat at decode time: every decode step
// multiplies the B <= 64 in-flight sequences' rows by every weight matrix once, so the
// step is HBM-bound on the 6.4 GB of fp16 weights.  Design for that:
//  * one block per 16*NT weight rows, the whole K range split over the block's waves
//    (reduced through LDS) -- no cross-block split-K, so no fences or tickets;
//  * every wave issues the loads of its whole K slice (U steps of 64) before its
//    first MFMA: W straight HBM -> VGPR (no LDS round trip, cdna_hip_programming.md
//    §5 'GEMV / M <= 16'), 32 contiguous bytes per lane per step, so a wave-instruction
//    pair covers 16 full 128-B lines (pair form: each instruction reads half of every line;
//    line-exact form: each instruction reads eight whole lines, non-temporal where that measured
//    ahead, and a half-row swap between lanes restores the pair form's registers, gemv_common.h
//    lx_exchange); X (tiny, L2-resident) is staged into LDS by DMA (chunk
//    swizzle on the source address), the block's whole image or each wave's own k-slice.
//    The DMA requests are queued AHEAD of the weight stream (all of it in the parent order,
//    all but its first step in the weight-first orders, gemv_order below): vmcnt retires in
//    issue order, so X behind the weights would land only with the last weight byte;
//  * v_mfma_f32_16x16x32_f16 with the sequences as MFMA rows (M padded to 16*MT);
//    both operands use the same permuted k order (lane group g holds k0+16g..+15),
//    which leaves every dot product unchanged.
// Fusions that remove whole launches from the decode step:
//  * the deferred RMSNorm (kernels.h RowScale): X is already f16(x * g), written by the
//    producer of x (RESID_SSQ epilogue or a norm kernel) with per-tile sums of x^2; the block
//    loads its rows' partial sums ahead of everything else and scales its output rows by
//    rinv in the epilogue -- no norm launch between the residual update and the projection
//    (recomputing the norm from the fp32 residual in each block measured slower: every block
//    re-read x before its weight stream, GU 19 -> 27 us, profiles/r03/v1_norm_fused_ab.txt);
//  * EPI_ROPE_KV (QKV): Q/K rows are uploaded rope-permuted (dims i and i+64 in one
//    16-row tile), so the epilogue applies RoPE, writes Q for attention and scatters
//    K/V into the paged cache;
//  * fp16 store, fp32 residual add (O, down), SwiGLU on 16-row-interleaved gate/up,
//    fp32 store (lm_head logits).
// Results are deterministic and independent of the batch composition: a row's sum
// order depends only on (N, K), never on M or on the other rows.
#include "gemv_common.h"

namespace ms {

struct GemvPlan {
  int MT, NT, waves, U, tiles;
};

static GemvPlan gemv_plan(int M, int N, int K, int epi, int force_waves = 0, int rt = 0) {
  GemvPlan p;
  p.MT = (M + 15) / 16;
  p.NT = (epi == MS_GEMV_EPI_SWIGLU) ? 2 : 1;
  const int rows = p.NT == 1 && rt > 0 ? rt : 16 * p.NT;
  p.tiles = (N + rows - 1) / rows;
  const int steps = K / 64;
  int best_w = 0;
  if (force_waves > 0 && steps % force_waves == 0 && steps / force_waves <= 8) {
    best_w = force_waves;
  } else {
    // most waves (<= 16) that split K evenly with U <= 8 steps each: measured on MI355X
    // (tools/bench_kernels.py gemv) 16 waves beat 6-12 on every Llama-3.2-3B shape
    for (int w = 16; w >= 1; --w)
      if (steps % w == 0 && steps / w <= 8) { best_w = w; break; }
  }
  p.waves = best_w;
  p.U = best_w ? steps / best_w : 0;
  return p;
}

size_t gemv_workspace_bytes(int, int, int) { return 256; }

constexpr size_t kMaxLds = 160 * 1024;

// LDS: the X image (gemv_x_lds_bytes, when staged) or the per-wave partials, whichever is
// larger, then the deferred-norm factors (gemv_lds_total)
static size_t gemv_lds_main(const GemvPlan& p, int M, int K, int xm) {
  size_t xs = xm == kXLds ? gemv_x_lds_bytes(M, K) : xm == kXWave ? gemv_xw_lds_bytes(M, K) : 0;
  const size_t red = (size_t)p.waves * p.MT * p.NT * 256 * 4;  // per-wave partials
  return xs > red ? xs : red;
}
static size_t gemv_lds_bytes(const GemvPlan& p, int M, int K, int xm, const RowScale& rs = RowScale{}) {
  return gemv_lds_total(gemv_lds_main(p, M, K, xm), rs, M);
}

// In-kernel timeline stamps (diagnostic instantiations only, MS_GEMV_STAMPS=1, tools/gemv_stamps.py):
// per block of the latest launch, s_memrealtime (100 MHz) of wave 0 in [0..15] and of the last wave
// in [16..31]: [0] entry, [1] XCC_ID << 32 | HW_ID, [2] first weight pair issued, [3] X and
// statistics issued, [4] all weight loads issued, [5] the wave's own wait for X passed, [6] the X
// barrier passed (= [5] where there is none), [7] first weight step landed, [8] last weight step
// landed, [9] MFMAs issued, [10] partials written, [11] epilogue stores issued.  The stamps stay in
// scalar registers until the end of the kernel (a store in between would count on vmcnt and move
// the counted waits); [7] / [8] add a wait of their own in front of the first / last MFMA step.
constexpr int kGvStampBlocks = 1024, kGvStamps = 32;
__device__ unsigned long long g_gemv_stamps[kGvStampBlocks * kGvStamps];
#define GV_STAMP(k)                                     \
  do {                                                  \
    if constexpr (STAMP) {                              \
      __builtin_amdgcn_sched_barrier(0);                \
      ts[k] = __builtin_amdgcn_s_memrealtime();         \
      __builtin_amdgcn_sched_barrier(0);                \
    }                                                   \
  } while (0)

// Split-K (gridDim.y = S > 1, STORE_F32 only): block (x, y) covers k in [y*K, (y+1)*K) of
// rows of length ldk and writes its fp32 partial to slab y = out + y*M*ldo; the consumer
// (residual_rmsnorm_kernel) adds the S slabs in slab order -- deterministic, no atomics.
// XM = where the MFMA's X fragments come from:
//   kXGlobal: global loads inside the MFMA loop (large M*K: no room in LDS or registers);
//   kXLds:    the block's LDS image, copied by DMA (gemv_dma_x), all waves meet at a barrier;
//   kXWave:   each wave copies its OWN k-slice (the only part it multiplies) by DMA into an LDS
//             region of its own (gemv_dma_x_wave) and waits on its own vmcnt: no registers, and
//             no block barrier unless the row factors are folded there (RS, one-tile plans);
//   kXRegs:   each wave loads its own k-slice straight into registers ahead of its weight
//             loads -- no LDS image, no block barrier, but MT x U x 8 VGPRs.
// WF = issue order (gemv_order below): false = statistics DMA, residual prefetch and X DMA,
// then the weight stream; true = the first weight step (u = 0) ahead of all of those, the other
// steps behind them.  vmcnt retires in issue order, so either way "at most the weight loads
// issued after the DMA are pending" means X has landed.  The sum order is the same in every
// form: per wave MFMAs in u order, then the waves in wave order (gemv_epilogue).
// rinv_off: LDS byte offset of the deferred-norm factors (gemv_rinv_offset).  (Two
// 1024-thread gate/up blocks share a CU at <= 64 VGPRs: 58 / 60 without / with the row scale.)
template <int MT, int NT, int EPI, int U, int XM, bool RS, bool WF, bool STAMP, int LX = 0>
__device__ __forceinline__ void gemv_body(const f16_t* __restrict__ X, const f16_t* __restrict__ W,
                                          void* __restrict__ out, int M, int N, int K, int ldk, int ldo,
                                          int rinv_off, const GemvArgs& ga) {
  static_assert(!WF || XM == kXLds || XM == kXWave, "weight-first applies to the DMA-staged forms");
  static_assert(XM != kXWave || WF, "per-wave slices come with the weight-first order");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  unsigned long long ts[STAMP ? 12 : 1] = {};
  GV_STAMP(0);
  // NT = 1: ga.rt weight rows per tile (lanes fr >= rt duplicate the last row; never stored)
  const int rt = NT == 1 && ga.rt > 0 ? ga.rt : 16;
  const int n0 = blockIdx.x * (NT == 1 ? rt : 16 * NT);
  const int kbeg = wave * U * 64;
  if constexpr (EPI == MS_GEMV_EPI_STORE_F32) {
    X += (size_t)blockIdx.y * K;
    W += (size_t)blockIdx.y * K;
    out = (float*)out + (size_t)blockIdx.y * (ga.slab_rows > 0 ? ga.slab_rows : M) * ldo;
  }
  constexpr bool kXL = XM == kXLds || XM == kXWave;  // fragments come from LDS
  constexpr bool kRsEarly = kXL && NT == 1;          // row factors folded right after the X barrier
  constexpr bool kBar = XM == kXLds || (RS && NT == 1);
  constexpr int kAfterX = WF ? (U - 1) * NT * 2 : U * NT * 2;  // weight loads issued behind the X DMA

  uint4 w[U][NT][2];
  // line-exact forms (LX, gemv_common.h lx_exchange): instruction A / B of a pair reads tile rows
  // (fr & 7) + 0 / 8, chunk 2 fg + (fr >> 3) of the step's 128 bytes; the row clamps apply to the
  // row each instruction loads.  LX = 2: non-temporal, every line having this one reader
  auto wrow_lx = [&](int n, int half) {
    const int r = (fr & 7) + half;
    const int wrow = NT == 1 ? n0 + min(r, rt - 1) : n0 + n * 16 + r;
    // the block's 64-bit tile base plus a 32-bit lane offset (< 32 rows): one VGPR per row
    // pointer, where the form holds twice as many row pointers as the pair form
    const unsigned off = (unsigned)((min(wrow, N - 1) - n0) * ldk + kbeg + 16 * fg + 8 * (fr >> 3)) * 2u;
    return (const f16_t*)((const char*)(W + (size_t)n0 * ldk) + off);
  };
  auto ldw = [](const f16_t* p) { return LX == 2 ? ldw16_nt(p) : ldw16(p); };
  // weight-first: step u = 0 of every tile leaves ahead of the statistics / residual / X requests
  if constexpr (WF) {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      if constexpr (LX) {
        w[0][n][0] = ldw(wrow_lx(n, 0));
        w[0][n][1] = ldw(wrow_lx(n, 8));
      } else {
        const int wrow = NT == 1 ? n0 + min(fr, rt - 1) : n0 + n * 16 + fr;
        const f16_t* wp = W + (size_t)min(wrow, N - 1) * ldk + kbeg + 16 * fg;
        w[0][n][0] = ldw16(wp);
        w[0][n][1] = ldw16(wp + 8);
      }
    }
    GV_STAMP(2);
    __builtin_amdgcn_sched_barrier(0);
  }
  // the output rows' deferred-norm partial sums, the residual element, then X (LDS DMA of the
  // block's rows or of this wave's slice, or this wave's slice into registers)
  // (row statistics always staged here: gemv_common.h rs_begin HOLD)
  if constexpr (RS) rs_begin<false>(smem, rinv_off, ga.rs, M);
  // (weight-first: the gain stays raw until the MFMAs are issued, so no wave waits here)
  ResidPre pre = resid_prefetch<EPI, WF>(M, N, ldo, out, n0, ga);
  if constexpr (XM == kXLds) gemv_dma_x(smem, X, M, K, ldk);
  if constexpr (XM == kXWave) gemv_dma_x_wave<U>(smem, X, M, ldk, kbeg);
  uint4 xr[XM == kXRegs ? U : 1][XM == kXRegs ? MT : 1][2];
  if constexpr (XM == kXRegs) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const f16_t* xg = X + (size_t)min(m * 16 + fr, M - 1) * ldk + kbeg + u * 64 + 16 * fg;
        xr[u][m][0] = ldg16(xg);
        xr[u][m][1] = ldg16(xg + 8);
      }
  }
  GV_STAMP(3);
  __builtin_amdgcn_sched_barrier(0);
  // the (rest of the) weight stream: parent order tile by tile, weight-first in MFMA (u) order
  if constexpr (WF) {
#pragma unroll
    for (int u = 1; u < U; ++u)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        if constexpr (LX) {
          w[u][n][0] = ldw(wrow_lx(n, 0) + u * 64);
          w[u][n][1] = ldw(wrow_lx(n, 8) + u * 64);
        } else {
          const int wrow = NT == 1 ? n0 + min(fr, rt - 1) : n0 + n * 16 + fr;
          const f16_t* wp = W + (size_t)min(wrow, N - 1) * ldk + kbeg + 16 * fg;
          w[u][n][0] = ldw16(wp + u * 64);
          w[u][n][1] = ldw16(wp + u * 64 + 8);
        }
      }
  } else {
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int wrow = NT == 1 ? n0 + min(fr, rt - 1) : n0 + n * 16 + fr;
      const f16_t* wp = LX ? wrow_lx(n, 0) : W + (size_t)min(wrow, N - 1) * ldk + kbeg + 16 * fg;
      const f16_t* wq = LX ? wrow_lx(n, 8) : wp + 8;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        w[u][n][0] = ldw(wp + u * 64);
        w[u][n][1] = ldw(wq + u * 64);
        if (n == 0 && u == 0) GV_STAMP(2);
      }
    }
  }
  GV_STAMP(4);
  // X (and the staged row statistics, issued before it) has landed once at most the weight loads
  // issued behind it are pending; the row factors are folded now, under the weight stream
  if constexpr (kXL) {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(kAfterX));
    GV_STAMP(5);
    // (no fence: a fence would wait for the W loads too; per-wave slices without early row
    // factors need no barrier at all: the wave reads only what its own DMA wrote)
    if constexpr (kBar) __builtin_amdgcn_s_barrier();
    GV_STAMP(6);
    // (two-tile plans fold them at the end: their 6 weight stages fill the 64 VGPRs)
    if constexpr (RS && NT == 1) rs_finish<false>(smem, rinv_off, ga.rs, M, 0.f);
    // (the exchange of step 0 stays behind the counted wait: hoisted above it, it made the compiler
    // wait for the whole stream, vmcnt(0), in front of the first MFMA)
    if constexpr (LX) __builtin_amdgcn_sched_barrier(0);
  }

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int mp = (M + 7) >> 3;
  const char* xw = smem + (size_t)wave * U * mp * 1024;  // kXWave: this wave's region
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if constexpr (STAMP) {  // step 0 / the last step landed (the parent order issues tile 0 whole, then tile 1)
      if (u == 0) {
        __builtin_amdgcn_s_waitcnt(vmcnt_imm(WF ? (U - 1) * NT * 2 : (U - 1) * 2));
        GV_STAMP(7);
      }
      if (u == U - 1) {
        __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
        GV_STAMP(8);
      }
    }
    if constexpr (LX) {  // back to the pair form's registers (waits for this step's loads only)
#pragma unroll
      for (int n = 0; n < NT; ++n) lx_exchange(w[u][n][0], w[u][n][1], fr >> 3);
      // two-tile plans: the exchange's temporaries are dead before the X fragments are read (the
      // six weight stages leave the gate/up GEMV no room for both at once)
      if constexpr (NT == 2) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int xrow = min(m * 16 + fr, M - 1);
      f16x8 x0, x1;
      if constexpr (XM == kXRegs) {
        x0 = as_f16x8(xr[u][m][0]);
        x1 = as_f16x8(xr[u][m][1]);
      } else if constexpr (XM == kXLds) {
        const int k0 = kbeg + u * 64 + 16 * fg;
        x0 = *(const f16x8*)(smem + x_lds(xrow, k0, K));
        x1 = *(const f16x8*)(smem + x_lds(xrow, k0 + 8, K));
      } else if constexpr (XM == kXWave) {
        x0 = *(const f16x8*)(xw + xw_lds(xrow, u, 2 * fg, mp));
        x1 = *(const f16x8*)(xw + xw_lds(xrow, u, 2 * fg + 1, mp));
      } else {
        const f16_t* xg = X + (size_t)xrow * ldk + kbeg + u * 64 + 16 * fg;
        x0 = as_f16x8(ldg16(xg));
        x1 = as_f16x8(ldg16(xg + 8));
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        acc[m][n] = mfma16(x0, as_f16x8(w[u][n][0]), acc[m][n]);
        acc[m][n] = mfma16(x1, as_f16x8(w[u][n][1]), acc[m][n]);
      }
    }
  }
  if constexpr (WF && EPI == MS_GEMV_EPI_RESID_SSQ) resid_gain(pre);
  GV_STAMP(9);
  unsigned long long* t_red = nullptr;
  if constexpr (STAMP) t_red = &ts[10];
  gemv_finish<MT, NT, EPI, RS, kRsEarly, false>(acc, smem, rinv_off, M, N, ldo, out, n0, ga, pre, 0.f, t_red);
  if constexpr (STAMP) {
    GV_STAMP(11);
    const int nw = blockDim.x >> 6, blk = blockIdx.y * gridDim.x + blockIdx.x;
    if (lane == 0 && (wave == 0 || wave == nw - 1) && blk < kGvStampBlocks) {
      unsigned hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      ts[1] = ((unsigned long long)xcc << 32) | hw;
      unsigned long long* dst = g_gemv_stamps + (size_t)blk * kGvStamps + (wave == 0 ? 0 : 16);
#pragma unroll
      for (int k = 0; k < 12; ++k) dst[k] = ts[k];
    }
  }
}

// The parent order (X requests first), every X mode but kXWave: gemv_body<.., WF = false> spelled out
// on its own.  The gate/up instance sits at the 64-VGPR edge that lets two blocks share a CU
// (tests/test_register_budget.py), and routing it through the shared body moved its register
// allocation (60 -> 66 VGPRs), so the measured kernel keeps its text.
template <int MT, int NT, int EPI, int U, int XM, bool RS>
__global__ __launch_bounds__(1024) void gemv_kernel(const f16_t* __restrict__ X,
                                                    const f16_t* __restrict__ W,
                                                    void* __restrict__ out, int M, int N, int K,
                                                    int ldk, int ldo, int rinv_off, GemvArgs ga) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  // NT = 1: ga.rt weight rows per tile (lanes fr >= rt duplicate the last row; never stored)
  const int rt = NT == 1 && ga.rt > 0 ? ga.rt : 16;
  const int n0 = blockIdx.x * (NT == 1 ? rt : 16 * NT);
  const int kbeg = wave * U * 64;
  if constexpr (EPI == MS_GEMV_EPI_STORE_F32) {
    X += (size_t)blockIdx.y * K;
    W += (size_t)blockIdx.y * K;
    out = (float*)out + (size_t)blockIdx.y * (ga.slab_rows > 0 ? ga.slab_rows : M) * ldo;
  }

  // 0. the output rows' deferred-norm partial sums, 1. X (LDS DMA of the block's rows or this
  // wave's slice into registers), then this wave's whole W stream: vmcnt retires in issue order
  // (row statistics always staged here: gemv_common.h rs_begin HOLD)
  constexpr bool kRsEarly = XM == kXLds && NT == 1;  // folds right after the X barrier
  if constexpr (RS) rs_begin<false>(smem, rinv_off, ga.rs, M);
  const ResidPre pre = resid_prefetch<EPI>(M, N, ldo, out, n0, ga);
  if constexpr (XM == kXLds) gemv_dma_x(smem, X, M, K, ldk);
  uint4 xr[XM == kXRegs ? U : 1][XM == kXRegs ? MT : 1][2];
  if constexpr (XM == kXRegs) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const f16_t* xg = X + (size_t)min(m * 16 + fr, M - 1) * ldk + kbeg + u * 64 + 16 * fg;
        xr[u][m][0] = ldg16(xg);
        xr[u][m][1] = ldg16(xg + 8);
      }
  }
  __builtin_amdgcn_sched_barrier(0);
  uint4 w[U][NT][2];
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int wrow = NT == 1 ? n0 + min(fr, rt - 1) : n0 + n * 16 + fr;
    const f16_t* wp = W + (size_t)min(wrow, N - 1) * ldk + kbeg + 16 * fg;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      w[u][n][0] = ldw16(wp + u * 64);
      w[u][n][1] = ldw16(wp + u * 64 + 8);
    }
  }
  // 2. the X image (and the staged row statistics, issued before it) has landed once at most
  // the W loads are pending; the row factors are folded now, under the weight stream
  if constexpr (XM == kXLds) {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(vmcnt_imm(U * NT * 2));
    __builtin_amdgcn_s_barrier();  // no fence: a fence would wait for the W loads too
    // (two-tile plans fold them at the end: their 6 weight stages fill the 64 VGPRs)
    if constexpr (RS && NT == 1) rs_finish<false>(smem, rinv_off, ga.rs, M, 0.f);
  }

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int xrow = min(m * 16 + fr, M - 1);
      f16x8 x0, x1;
      if constexpr (XM == kXRegs) {
        x0 = as_f16x8(xr[u][m][0]);
        x1 = as_f16x8(xr[u][m][1]);
      } else if constexpr (XM == kXLds) {
        const int k0 = kbeg + u * 64 + 16 * fg;
        x0 = *(const f16x8*)(smem + x_lds(xrow, k0, K));
        x1 = *(const f16x8*)(smem + x_lds(xrow, k0 + 8, K));
      } else {
        const f16_t* xg = X + (size_t)xrow * ldk + kbeg + u * 64 + 16 * fg;
        x0 = as_f16x8(ldg16(xg));
        x1 = as_f16x8(ldg16(xg + 8));
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        acc[m][n] = mfma16(x0, as_f16x8(w[u][n][0]), acc[m][n]);
        acc[m][n] = mfma16(x1, as_f16x8(w[u][n][1]), acc[m][n]);
      }
    }
  }
  gemv_finish<MT, NT, EPI, RS, kRsEarly, false>(acc, smem, rinv_off, M, N, ldo, out, n0, ga, pre);
}

// weight-first order: XM = kXLds (the block's image) or kXWave (per-wave slices)
template <int MT, int NT, int EPI, int U, int XM, bool RS>
__global__ __launch_bounds__(1024) void gemv_wf_kernel(const f16_t* __restrict__ X,
                                                       const f16_t* __restrict__ W,
                                                       void* __restrict__ out, int M, int N, int K,
                                                       int ldk, int ldo, int rinv_off, GemvArgs ga) {
  gemv_body<MT, NT, EPI, U, XM, RS, true, false>(X, W, out, M, N, K, ldk, ldo, rinv_off, ga);
}

// line-exact weight loads (gemv_body LX: 1 default cache policy, 2 non-temporal) under each issue
// order of the DMA-staged forms; WF = false is the parent order through the shared body
template <int MT, int NT, int EPI, int U, int XM, bool RS, bool WF, int LX>
__global__ __launch_bounds__(1024) void gemv_lx_kernel(const f16_t* __restrict__ X,
                                                       const f16_t* __restrict__ W,
                                                       void* __restrict__ out, int M, int N, int K,
                                                       int ldk, int ldo, int rinv_off, GemvArgs ga) {
  gemv_body<MT, NT, EPI, U, XM, RS, WF, false, LX>(X, W, out, M, N, K, ldk, ldo, rinv_off, ga);
}

// the stamped twins of both (M <= 16; never launched unless MS_GEMV_STAMPS=1)
template <int NT, int EPI, int U, int XM, bool RS, bool WF>
__global__ __launch_bounds__(1024) void gemv_stamp_kernel(const f16_t* __restrict__ X,
                                                          const f16_t* __restrict__ W,
                                                          void* __restrict__ out, int M, int N, int K,
                                                          int ldk, int ldo, int rinv_off, GemvArgs ga) {
  gemv_body<1, NT, EPI, U, XM, RS, WF, true>(X, W, out, M, N, K, ldk, ldo, rinv_off, ga);
}

void gemv_stamps(unsigned long long* host, int n) {
  n = std::min(n, kGvStampBlocks * kGvStamps);
  (void)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_gemv_stamps), (size_t)n * sizeof(unsigned long long));
  // read and clear: a later launch of fewer blocks must not show this one's
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_gemv_stamps)) == hipSuccess)
    (void)hipMemset(p, 0, sizeof(unsigned long long) * kGvStampBlocks * kGvStamps);
}

static bool gemv_stamps_on() {
  static const bool on = [] { const char* e = getenv("MS_GEMV_STAMPS"); return e && atoi(e); }();
  return on;
}

// Issue order of the DMA-staged decode GEMVs (ms_set_gemv_order / MS_GEMV_ORDER): 0 = X requests
// first (the parent order), 1 = first weight step first, 2 = that with per-wave X slices; every
// order gives the same bits.  The weight load form composes with it: order = issue order + 3 x
// form, form 0 = the pair form (each instruction of a pair reads half of every line of the tile),
// 1 = line-exact (gemv_common.h lx_exchange), 2 = line-exact with non-temporal loads; so 3..5 and
// 6..8 are the three issue orders on the line-exact forms.  The library starts on the per-shape
// table below (-1); a forced order applies to every launch.  MS_GEMV_ORDER is one digit (forced)
// or one digit per class in the order of the enum (A/B tuning).
constexpr int kGemvOrders = 9;
enum { kGcQkv = 0, kGcO, kGcGateUp, kGcDown, kGcLmHead, kGcCount };
// Measured per shape at M = 8, weights from HBM (tools/gemv_stamps.py --time, us per launch, orders
// 0 / 1 / 2; profiles/gemv_order/time_ab.txt): O 9.01 / 8.72 / 8.47 and down 15.33 / 14.81 / 14.51
// take order 2; QKV split-6 12.20 / 13.11 / 12.89 and the lm_head 128.1 / 130.9 / 131.0 lose with
// their weights ahead of X and stay on the parent order.  Gate/up 22.73 / 22.55 / 22.67 moves
// inside its own op-level spread; inside the decode step order 1 was ahead in 3 of 3 paired
// bench rounds (2.0635 vs 2.0694 ms per step, profiles/gemv_order/bench_env_ab.txt), so it takes 1.
// Load form, same method (profiles/gemv_lines/time_ab.txt, median (min-max) us; a class moves only
// when its range stays clear of its current default's): the line-exact non-temporal form on per-wave
// slices (8) takes O 8.16 (8.09-8.42) -> 6.63 (6.52-7.43), down 14.01 (13.90-14.58) -> 12.73
// (12.58-13.14) and the lm_head 128.45 (128.04-134.10) -> 123.30 (122.59-123.91); gate/up 21.41 ->
// 19.50 overlaps at op level and was ahead in 3 of 3 in-step pairs (2.0289 vs 2.0453 ms per decode
// step, bench_env_ab.txt; 63 VGPRs, tests/test_gemv_lines_budget.py).  QKV split-6 reads 12.02
// (11.82-13.36) -> 10.96 (10.75-12.15) on order 6: the ranges overlap, so it stays on 0.  Line-exact
// loads under the default policy (3..5) are level with or behind the pair form everywhere.
static int g_gemv_class_order[kGcCount] = {0, 8, 8, 8, 8};
static int g_gemv_order = [] {
  const char* e = getenv("MS_GEMV_ORDER");
  if (!e || !e[0]) return -1;
  auto dig = [](char c) { return c >= '0' && c < '0' + kGemvOrders ? c - '0' : 0; };
  if (!e[1]) return dig(e[0]);
  for (int i = 0; i < kGcCount && e[i]; ++i) g_gemv_class_order[i] = dig(e[i]);
  return -1;
}();
void set_gemv_order(int v) { g_gemv_order = v; }
// the launch's class: the bench's five decode projections by what tells them apart structurally
// (epilogue, loads in flight per wave, width); anything else keeps the parent order
static int gemv_order_for(int epi, int N, int U) {
  if (g_gemv_order >= 0) return g_gemv_order;
  if (epi == MS_GEMV_EPI_SWIGLU) return g_gemv_class_order[kGcGateUp];
  if (epi == MS_GEMV_EPI_RESID_SSQ) return g_gemv_class_order[U <= 4 ? kGcO : kGcDown];
  if (epi == MS_GEMV_EPI_ARGMAX || (epi == MS_GEMV_EPI_STORE_F32 && N >= 65536)) return g_gemv_class_order[kGcLmHead];
  if (epi == MS_GEMV_EPI_STORE_F32) return g_gemv_class_order[kGcQkv];
  return 0;
}

// sel: the order (issue order + 3 x load form); the issue order is 0 parent order or weight-first
// (xm = kXLds or kXWave), the line-exact forms exist for the DMA-staged X modes
template <int MT, int NT, int EPI, int U, bool RS>
static void gemv_go_rs(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldk,
                       const dim3& grid, const dim3& blk, size_t lds, int ro, int ldo, int xm, int sel,
                       const GemvArgs& ga, hipStream_t s) {
  const int ord = sel % 3, lx = sel / 3;
#define GL(...) MS_LAUNCH((__VA_ARGS__), grid, blk, lds, s, X, W, out, M, N, K, ldk, ldo, ro, ga)
  // (built for M <= 16, the batches the decode step runs through these kernels; wider batches
  // and the stamped twins keep the pair form, which gives the same bits)
  if constexpr (MT == 1)
  if (lx && !gemv_stamps_on() && (xm == kXLds || xm == kXWave)) {
#define GLX(LX_)                                                                     \
  do {                                                                                 \
    if (xm == kXWave) GL(gemv_lx_kernel<MT, NT, EPI, U, kXWave, RS, true, LX_>);        \
    else if (ord) GL(gemv_lx_kernel<MT, NT, EPI, U, kXLds, RS, true, LX_>);             \
    else GL(gemv_lx_kernel<MT, NT, EPI, U, kXLds, RS, false, LX_>);                     \
  } while (0)
    if (lx == 1) GLX(1);
    else GLX(2);
#undef GLX
    return;
  }
  if constexpr (MT * U <= kXRegsMaxFrags) {
    if (xm == kXRegs) {
      GL(gemv_kernel<MT, NT, EPI, U, kXRegs, RS>);
      return;
    }
  }
  // the stamped twins exist for the bench's decode shapes (512-, 3072- and 8192-wide k ranges)
  constexpr bool kStampEpi = EPI == MS_GEMV_EPI_STORE_F32 || EPI == MS_GEMV_EPI_SWIGLU ||
                             EPI == MS_GEMV_EPI_RESID_SSQ || EPI == MS_GEMV_EPI_ARGMAX;
  if constexpr (MT == 1 && (U == 1 || U == 3 || U == 8) && kStampEpi) {
    if (gemv_stamps_on() && (xm == kXLds || xm == kXWave)) {
      if (xm == kXWave) GL(gemv_stamp_kernel<NT, EPI, U, kXWave, RS, true>);
      else if (ord) GL(gemv_stamp_kernel<NT, EPI, U, kXLds, RS, true>);
      else GL(gemv_stamp_kernel<NT, EPI, U, kXLds, RS, false>);
      return;
    }
  }
  if (xm == kXWave) GL(gemv_wf_kernel<MT, NT, EPI, U, kXWave, RS>);
  else if (xm == kXLds && ord) GL(gemv_wf_kernel<MT, NT, EPI, U, kXLds, RS>);
  else if (xm == kXLds) GL(gemv_kernel<MT, NT, EPI, U, kXLds, RS>);
  else GL(gemv_kernel<MT, NT, EPI, U, kXGlobal, RS>);
#undef GL
}

template <int MT, int NT, int EPI, int U>
static void gemv_go(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldk,
                    int S, int ldo, const GemvPlan& p, size_t lds, int xm, int ord, const GemvArgs& ga,
                    hipStream_t s) {
  const dim3 grid(p.tiles, S), blk(64 * p.waves);
  const int ro = (int)gemv_rinv_offset(gemv_lds_main(p, M, K, xm));
  if constexpr (EPI == MS_GEMV_EPI_ROPE_KV && MT != 1) {
    return;  // rope epilogue works on M <= 16 (checked by gemv_supported)
  } else if constexpr (gemv_rs_epi<EPI>()) {
    if (ga.rs.ssq) gemv_go_rs<MT, NT, EPI, U, true>(X, W, out, M, N, K, ldk, grid, blk, lds, ro, ldo, xm, ord, ga, s);
    else gemv_go_rs<MT, NT, EPI, U, false>(X, W, out, M, N, K, ldk, grid, blk, lds, ro, ldo, xm, ord, ga, s);
  } else {
    gemv_go_rs<MT, NT, EPI, U, false>(X, W, out, M, N, K, ldk, grid, blk, lds, ro, ldo, xm, ord, ga, s);
  }
}

template <int MT, int NT, int EPI>
static void gemv_go_u(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldk,
                      int S, int ldo, const GemvPlan& p, size_t lds, int xm, int ord, const GemvArgs& ga,
                      hipStream_t s) {
#define GU(U_) gemv_go<MT, NT, EPI, U_>(X, W, out, M, N, K, ldk, S, ldo, p, lds, xm, ord, ga, s)
  switch (p.U) {
    case 1: GU(1); break;
    case 2: GU(2); break;
    case 3: GU(3); break;
    case 4: GU(4); break;
    case 5: GU(5); break;
    case 6: GU(6); break;
    case 7: GU(7); break;
    default: GU(8); break;
  }
#undef GU
}

template <int MT>
static void gemv_go_mt(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldk,
                       int S, int ldo, int epi, const GemvPlan& p, size_t lds, int xm, int ord,
                       const GemvArgs& ga, hipStream_t s) {
#define GE(NT_, E_) gemv_go_u<MT, NT_, E_>(X, W, out, M, N, K, ldk, S, ldo, p, lds, xm, ord, ga, s)
  switch (epi) {
    case MS_GEMV_EPI_STORE_F16: GE(1, MS_GEMV_EPI_STORE_F16); break;
    case MS_GEMV_EPI_ADD_F32: GE(1, MS_GEMV_EPI_ADD_F32); break;
    case MS_GEMV_EPI_SWIGLU: GE(2, MS_GEMV_EPI_SWIGLU); break;
    case MS_GEMV_EPI_ROPE_KV: GE(1, MS_GEMV_EPI_ROPE_KV); break;
    case MS_GEMV_EPI_ARGMAX: GE(1, MS_GEMV_EPI_ARGMAX); break;
    case MS_GEMV_EPI_RESID_SSQ: GE(1, MS_GEMV_EPI_RESID_SSQ); break;
    default: GE(1, MS_GEMV_EPI_STORE_F32); break;
  }
#undef GE
}

bool gemv_supported(int M, int N, int K, int epi, int rs_tiles) {
  if (M < 1 || M > 64 || K % 64) return false;
  if (epi == MS_GEMV_EPI_ROPE_KV && M > 16) return false;
  if (epi == MS_GEMV_EPI_ARGMAX && N % 16) return false;
  const GemvPlan p = gemv_plan(M, N, K, epi);
  if (p.waves == 0) return false;
  // the residual epilogue's prefetch covers one element per thread of a >= 256-thread block
  if (epi == MS_GEMV_EPI_RESID_SSQ && p.waves < 4) return false;
  if (epi == MS_GEMV_EPI_ROPE_KV && gemv_lds_bytes(p, M, K, kXLds) > kMaxLds) return false;
  RowScale rs{};
  const bool takes_rs = epi != MS_GEMV_EPI_ARGMAX && epi != MS_GEMV_EPI_ADD_F32 && epi != MS_GEMV_EPI_RESID_SSQ;
  if (rs_tiles > 0 && takes_rs) {  // gemv_dispatch drops the scale for the other epilogues
    if (!gemv_rs_supported(M, rs_tiles)) return false;
    rs = make_row_scale(reinterpret_cast<const float*>(16), rs_tiles, 1, 0.f);
  }
  return gemv_lds_bytes(p, M, K, kXGlobal, rs) <= kMaxLds;
}

static void gemv_dispatch(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldk,
                          int S, int ldo, int epi, const GemvArgs* ga_in, int force_waves,
                          hipStream_t s) {
  if (M <= 0) return;
  const int rt = ga_in ? ga_in->rt : 0;
  const GemvPlan p = gemv_plan(M, N, K, epi, force_waves, rt);
  if (p.waves == 0) return;  // callers check gemv_supported()
  GemvArgs ga{};
  if (ga_in) ga = *ga_in;
  if (epi == MS_GEMV_EPI_ARGMAX || epi == MS_GEMV_EPI_ADD_F32 || epi == MS_GEMV_EPI_RESID_SSQ)
    ga.rs = RowScale{};  // argmax: r > 0 keeps every row's order; the others take unnormalised X
  // the X image only when the block's whole LDS (image + factors + staged statistics) fits
  const bool xl = gemv_lds_bytes(p, M, K, kXLds, ga.rs) <= kMaxLds;
  int xm = xl ? kXLds : kXGlobal;
  // the issue order applies to the DMA-staged forms; per-wave slices (whole 8-row pieces) where
  // they fit as well, else the block's image in weight-first order
  const int ord = xl ? gemv_order_for(epi, N, p.U) : 0;
  if (ord % 3 == 2 && gemv_lds_bytes(p, M, K, kXWave, ga.rs) <= kMaxLds) xm = kXWave;
  if (gemv_x_regs_for(epi) && p.MT * p.U <= kXRegsMaxFrags) xm = kXRegs;
  if (ga.rs.ssq && rs_stage_floats(ga.rs, M) == 0) return;  // callers check gemv_rs_supported
  const size_t lds = gemv_lds_bytes(p, M, K, xm, ga.rs);
  if (lds > kMaxLds) return;
  switch (p.MT) {
    case 1: gemv_go_mt<1>(X, W, out, M, N, K, ldk, S, ldo, epi, p, lds, xm, ord, ga, s); break;
    case 2: gemv_go_mt<2>(X, W, out, M, N, K, ldk, S, ldo, epi, p, lds, xm, ord, ga, s); break;
    case 3: gemv_go_mt<3>(X, W, out, M, N, K, ldk, S, ldo, epi, p, lds, xm, ord, ga, s); break;
    default: gemv_go_mt<4>(X, W, out, M, N, K, ldk, S, ldo, epi, p, lds, xm, ord, ga, s); break;
  }
}

void launch_gemv_ex(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldo,
                    int epi, const GemvArgs* ga_in, int force_waves, hipStream_t s) {
  gemv_dispatch(X, W, out, M, N, K, K, 1, ldo, epi, ga_in, force_waves, s);
}

// tuning hook: W rows of stride ldk >= K elements (padded layouts: HBM channel spread)
void launch_gemv_strided(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldk,
                         int ldo, int epi, hipStream_t s) {
  gemv_dispatch(X, W, out, M, N, K, ldk, 1, ldo, epi, nullptr, 0, s);
}

bool gemv_rs_supported(int M, int tiles) { return M >= 1 && tiles >= 1 && tiles * M <= kRsStage; }

bool gemv_split_supported(int M, int N, int K, int S, int rs_tiles) {
  if (S < 1 || K % S) return false;
  return gemv_supported(M, N, K / S, MS_GEMV_EPI_STORE_F32, rs_tiles);
}

void launch_gemv_split(const f16_t* X, const f16_t* W, float* slabs, int M, int N, int K, int S,
                       int force_waves, hipStream_t s, const GemvArgs* ga) {
  gemv_dispatch(X, W, slabs, M, N, K / S, K, S, N, MS_GEMV_EPI_STORE_F32, ga, force_waves, s);
}

// ---------------------------------------------------------------- argmax of partials
// rows of {max, id} float2 partials (MS_GEMV_EPI_ARGMAX) -> greedy ids; ties -> lowest id
// whatever the merge order; -1 when the row has no finite maximum (a failed chunk)
__global__ __launch_bounds__(1024) void argmax_partials_kernel(const float2* __restrict__ part, int tiles,
                                                               int32_t* __restrict__ out) {
  __shared__ float sv[16];
  __shared__ int si[16];
  const float2* p = part + (size_t)blockIdx.x * tiles;
  float v = -INFINITY;
  int idx = 0x7FFFFFFF;
  for (int t0 = 0; t0 < tiles; t0 += 8 * 1024) {  // 8 loads in flight per thread
    float2 q[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int t = t0 + i * 1024 + threadIdx.x;
      q[i] = t < tiles ? p[t] : make_float2(-INFINITY, __int_as_float(0x7FFFFFFF));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) amax_merge_dev(v, idx, q[i].x, __float_as_int(q[i].y));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax_merge_dev(v, idx, __shfl_xor(v, o, 64), __shfl_xor(idx, o, 64));
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = idx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w) amax_merge_dev(v, idx, sv[w], si[w]);
    out[blockIdx.x] = (idx == 0x7FFFFFFF || !__builtin_isfinite(v)) ? -1 : idx;
  }
}

void launch_argmax_partials(const void* partials, int rows, int tiles, int32_t* out, hipStream_t s) {
  if (rows <= 0) return;
  MS_LAUNCH(argmax_partials_kernel, dim3(rows), dim3(1024), 0, s, (const float2*)partials, tiles, out);
}

void launch_gemv(const f16_t* X, const f16_t* W, void* out, int M, int N, int K, int ldo, int epi,
                 void*, hipStream_t s) {
  launch_gemv_ex(X, W, out, M, N, K, ldo, epi, nullptr, 0, s);
}

}  // namespace ms
