// decode_forms.h -- which kernel family each decode projection launches: plain host data and
// free functions, no device.  DecodeSettings is everything an engine resolves once at ms_create
// (resolve_settings), DecodeMat one decode matrix, pick_form the ONE place that ranks the kernel
// families (engine.cpp launch_form maps its result to the launcher).  tests/native/decode_forms.cpp
// pins the table on the Llama-3.2-3B shapes.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "mapsum.h"

namespace ms {

constexpr int kMaxGemvRows = 64, kMaxSlabRows = 256, kMaxSplit = 8;

// Quantised (ggml K-quant) copy of one fused matrix for the decode GEMV; `need` = the
// logical tensors that must all be loaded quantised before decode uses it.
struct QSlot {
  QMat m{};
  size_t bytes[3] = {0, 0, 0};  // device bytes of each region (weight broadcast)
  uint32_t loaded = 0, need = 0;
  bool ready() const { return need != 0 && loaded == need; }
};
enum { QS_QKV = 0, QS_O = 1, QS_GU = 2, QS_DOWN = 3, QS_LM = 4 };

struct DecodeSettings {
  int max_batch = 0, H = 0, QD = 0, QKVN = 0, F = 0, V = 0;  // QD = n_heads * head_dim
  bool kv_paged = false;  // MS_KV_PAGED: the page-table pool even where slot-major would fit
  // decode attention with one page per wave (k_attn.hip v2, MS_ATTN_V2; engines of <= 16 slots),
  // attn_ppb waves / pages per block; attn_ppw: pages per wave of v1.  Fixed per engine.
  bool attn_v2 = false;
  int attn_ppb = 9, attn_ppw = 2;
  bool attn_ticket = false;  // MS_ATTN_TICKET: v2's splits merged in the launch by each group's last block
  int split_qkv = 6, split_o = 6, split_down = 4;  // small-regime split-K of QKV / O / down (MS_SPLIT_*)
  bool attn_slabs = true;  // decode attention's q/k/v from QKV split slabs (else the GEMV RoPE epilogue, B <= 16)
  // large-batch regime (BASELINE configs[2]): QKV / O / down / gate-up / lm_head on the skinny
  // GEMM (k_dgemm.hip, split 6 / 4 / 8 / 1 / 1).  The regime is chosen per ENGINE, from its
  // max_batch (>= dgemm_min), never from the rows of one step: every step of an engine then
  // runs one arithmetic whatever the number of sequences in flight (admission ramps, tails,
  // a chunk alone), so a chunk's summary never depends on its companions.  The crossover:
  // at M = 16 the GEMV and the skinny GEMM tie over a layer's four projections, at M = 32
  // the skinny GEMM takes 30 % less (profiles/r02/v7_dgemm_lds_sync_ab.txt).
  int dgemm_min = 24, dsplit_qkv = 6, dsplit_o = 4, dsplit_down = 8;
  bool large_engine = false;
  // Engines with K-quant weights keep the exact Q4_K / Q6_K GEMV up to qlarge_min - 1 slots (in
  // row groups of <= kMaxGemvRows above 64: a row's sum order does not depend on its group); from
  // qlarge_min (MS_QLARGE_MIN, default 65: the row groups' weight re-streams cost Q4_K_M 18.2 ms
  // per decode step at 128 slots, profiles/r06/v9_*) they take the large regime too, where every
  // quantised matrix streams its packed blocks once per step through the K-quant skinny GEMM
  // (k_qdgemm.hip, the fp16-copy values).  MS_QDGEMM selects which matrices: 1 (default) the
  // all-Q4_K and the all-Q5_K ones -- a Q6_K matrix (the Q4_K_M lm_head, half of the down / V
  // projections) runs its fp16 copy through k_dgemm.hip, which measured faster there (its dequant
  // is twice the VALU; r06/v11_*), and so does one of mixed types --, 2 every K-quant matrix,
  // 0 none (the fp16 copies everywhere), 3 the all-Q4_K ones only (the A/B of the Q5_K form: a
  // 128-slot Q5_K_M engine decodes 0.33-0.37 ms per step faster with its all-Q5_K matrices on
  // packed rows, in each of four paired rounds, profiles/q5_k/qdgemm_q5_k_ab_128_slots.jsonl)
  int qlarge_min = 65, qdgemm_mode = 1;
  // engines of >= lm_gemm_min slots run the large-regime lm_head (its greedy partials) on the
  // prefill GEMM's 128x128 tile (k_gemm.hip gemm_kernel, ~1000 blocks of 128 vocabulary rows)
  // instead of the skinny GEMM: 169 vs 252 us at 128 rows, 276 vs 429 at 256
  // (profiles/r06/v21_rows_dgemm_vs_gemm128.txt).  MS_LM_GEMM_MIN (0 = never) for A/B.
  int lm_gemm_min = 96;
  // gate/up skinny-GEMM block form (k_dgemm.hip kh): the library setting (2, the default: k split
  // over the two wave groups of an 8-wave block; 41.4 -> 34.9 us at M = 128, profiles/r05/v20_*)
  // for engines of <= 128 slots (the k-half block steps 128 k at a time: hidden % 128 == 0); the
  // split projections and the lm_head keep the 4-wave block (as fast or faster there)
  int dgemm_kh = 1;
  // fp16 engines of >= qdf_min slots (16-row-tile launches of up to 256 rows) run their skinny
  // GEMMs on k_qdgemm.hip's fp16-rows form (activations by LDS DMA three steps ahead) with
  // QKV / down split 3 / 4 instead of 6 / 8: at 256 rows gate/up 57.3 -> 50.4 us, QKV 30.2 ->
  // 22.6, down 43.3 -> 34.5, O 19.8 -> 19.2 (profiles/r06/v22_*).  MS_QDF_MIN, 0 = never: below
  // it the tested 24-128-slot arithmetic is unchanged.  The splits follow for any weights.
  int qdf_min = 192;
  // weight-row groups per skinny-GEMM block (k_dgemm.hip wn) for launches of <= 128 rows: the
  // 128-row block for QKV, down and the lm_head (down 22.3 -> 20.4 us, lm_head 262 -> 241 us at
  // M = 128, profiles/r05/v21_*), 64 rows for O (15.6 vs 12.9 us at its split 4); bit-identical
  int dwn_qkv = 8, dwn_o = 4, dwn_down = 8, dwn_lm = 8;
  // split count of every quantised slab projection (MS_QSPLIT; 0: as fp16): 4 measured best
  // for Q4_K_M at B = 8 -- 1.878 vs 1.900 ms/step with the fp16 splits (6 / 6 / 4), 2 / 3 / 8
  // slower (profiles/r02/v27_qsplit_sweep_q4_k_m.txt)
  int qsplit = 4;
  // Residual-fused decode (small-regime engines of <= 16 slots): O and down run unsplit on
  // resid_rt-row tiles (3072 / 12 = 256 workgroups, one per CU) and their epilogue adds into
  // the fp32 residual and emits the next projection's input itself -- xb = f16(x * g_next)
  // and per-tile sums of x^2 (ssq [256][B]) -- so the decode layer has no residual_rmsnorm
  // launch: the deferred RMSNorm (kernels.h RowScale) scales the rows of the QKV / gate-up /
  // lm_head outputs instead.  MS_RESID_FUSED=0: split-K slabs + norm launches.
  bool resid_fuse = true;
  int resid_rt = 12;
  // K-quant O / down with the same epilogue (MS_QRESID=0: split-K 4 + residual_rmsnorm): 1.785 vs
  // 1.794 ms per Q4_K_M decode step -- O 5.8 vs 4.8 + 4.7 us, down 12.8 vs 8.8 + 4.7 us, the
  // gate/up folding 256 statistics tiles +0.9 us (profiles/r04/v31_*)
  bool qresid = true;
  // the K-quant GEMVs that regime launches support its shapes (RESID_SSQ on O / down, the gate/up
  // SwiGLU folding 256 statistics tiles); the launchers return silently on an unsupported shape,
  // so an engine whose quantised shapes fall outside the Q plan takes split-K + residual_rmsnorm
  bool qresid_ok = true;
  bool tail_fuse = true;  // MS_DECODE_TAIL: greedy ids, argument advance and next embedding in one launch
  // chained decode steps per graph launch (MS_GRAPH_STEPS): 16 measured 12.12 -> 12.20
  // chunks/s on configs[1], unchanged on the ragged level and configs[2]
  // (profiles/r02/v35_graph_steps_ab.txt); a run's remainder uses the one-step graph
  int graph_steps = 16;
  bool use_graphs = true;  // MAPSUM_NO_GRAPHS=1: every decode step launched eagerly
  bool overlap = false;    // MS_OVERLAP=1: prefill and decode on two streams (slower: ms_engine::Ctx)
  bool persist = false;    // MS_PERSIST / ms_set_persist: the persistent decode step, opt-in
  int max_run = 64;        // MS_DECODE_RUN: chained decode steps per host synchronisation (<= 64)
  bool has_quant = false;  // a quantised tensor was loaded or declared (the loaders set it, not ms_create)

  bool large() const { return large_engine && (!has_quant || max_batch >= qlarge_min); }
  bool row_groups(int B) const { return !large() && B > kMaxGemvRows; }
  // O / down of this matrix add into the residual in their epilogue (else slabs + residual_rmsnorm)
  bool resid_fused(const QSlot* q) const {
    if (!resid_fuse || large_engine) return false;
    if (has_quant && !qresid_ok) return false;
    return !(q && q->ready()) || qresid;
  }
};

// The default splits are tuned for K = 3072 / 8192 (Llama-3.2-3B).  At another width (Qwen3-8B:
// 4096 / 12288, where 6 does not divide 4096 in 64-k steps) a large-regime default steps down to
// the largest split whose slabs are whole 64-k steps -- valid, not tuned; the small regime's
// pick_form already falls back to one slab where a GEMV refuses the split.  One value per engine,
// so a row's sum order is the same at every row count.  The MS_* overrides are taken as given.
inline int fit_split(int S, int K) {
  while (S > 1 && K % (64 * S) != 0) --S;
  return S;
}

inline void env_int(const char* name, int& v) { if (const char* s = getenv(name)) v = atoi(s); }
inline void env_flag(const char* name, bool& v) { if (const char* s = getenv(name)) v = atoi(s) != 0; }

// every MS_* / MAPSUM_NO_GRAPHS read of an engine: default -> derived -> override -> clamp
inline DecodeSettings resolve_settings(const ms_config& c) {
  DecodeSettings s;
  s.max_batch = c.max_batch; s.H = c.hidden; s.QD = c.n_heads * c.head_dim; s.F = c.ffn; s.V = c.vocab;
  s.QKVN = (c.n_heads + 2 * c.n_kv_heads) * c.head_dim;
  s.kv_paged = getenv("MS_KV_PAGED") != nullptr;
  s.attn_ppb = attn_decode2_ppb(c.max_batch, c.n_kv_heads, c.max_ctx);
  s.attn_v2 = c.max_batch <= 16;
  env_flag("MS_ATTN_V2", s.attn_v2); env_flag("MS_ATTN_TICKET", s.attn_ticket); env_flag("MS_ATTN_SLABS", s.attn_slabs);
  env_int("MS_SPLIT_QKV", s.split_qkv); env_int("MS_SPLIT_O", s.split_o); env_int("MS_SPLIT_DOWN", s.split_down);
  env_int("MS_DGEMM_MIN", s.dgemm_min);
  s.large_engine = c.max_batch >= s.dgemm_min;
  env_int("MS_QLARGE_MIN", s.qlarge_min); env_int("MS_QDGEMM", s.qdgemm_mode); env_int("MS_LM_GEMM_MIN", s.lm_gemm_min);
  s.dgemm_kh = c.max_batch <= 128 && s.H % 128 == 0 ? dgemm_kh_setting() : 1;
  env_int("MS_QDF_MIN", s.qdf_min);
  if (s.qdf_min > 0 && c.max_batch >= s.qdf_min) {  // splits measured at 256 rows (v22_*), any weights
    s.dsplit_qkv = 3;
    s.dsplit_down = 4;
  }
  s.dsplit_qkv = fit_split(s.dsplit_qkv, s.H); s.dsplit_o = fit_split(s.dsplit_o, s.QD); s.dsplit_down = fit_split(s.dsplit_down, s.F);
  env_int("MS_DSPLIT_QKV", s.dsplit_qkv); env_int("MS_DSPLIT_O", s.dsplit_o); env_int("MS_DSPLIT_DOWN", s.dsplit_down);
  if (const char* v = getenv("MS_DWN")) s.dwn_qkv = s.dwn_o = s.dwn_down = s.dwn_lm = atoi(v) == 8 ? 8 : 4;
  for (int* d : {&s.dsplit_qkv, &s.dsplit_o, &s.dsplit_down}) *d = std::min(std::max(*d, 1), kMaxSplit);
  s.attn_ppw = attn_decode_ppw(c.max_batch, c.n_kv_heads, c.max_ctx);
  env_int("MS_QSPLIT", s.qsplit);
  env_flag("MS_RESID_FUSED", s.resid_fuse); env_flag("MS_DECODE_TAIL", s.tail_fuse); env_flag("MS_QRESID", s.qresid);
  if (s.H % s.resid_rt || s.H / s.resid_rt > 256) s.resid_rt = 16;
  if (s.H % s.resid_rt || s.H / s.resid_rt > 256) s.resid_fuse = false;
  // the consumers stage the 256-tile statistics in LDS: engines of <= 16 slots (per engine,
  // so every step of it runs the same arithmetic)
  if (!gemv_rs_supported(c.max_batch, s.H / s.resid_rt)) s.resid_fuse = false;
  const int Bg = std::min(c.max_batch, kMaxGemvRows);
  // ... and the fp16 GEMV takes O and down with that epilogue (not at Qwen3-8B's K = 12288 down:
  // split-K slabs + residual_rmsnorm there, like the K-quant rule below)
  if (!gemv_supported(Bg, s.H, s.QD, MS_GEMV_EPI_RESID_SSQ) || !gemv_supported(Bg, s.H, s.F, MS_GEMV_EPI_RESID_SSQ))
    s.resid_fuse = false;
  s.qresid_ok = qgemv_supported(Bg, s.H, s.QD, MS_GEMV_EPI_RESID_SSQ) &&
                qgemv_supported(Bg, s.H, s.F, MS_GEMV_EPI_RESID_SSQ) &&
                qgemv_supported(Bg, 2 * s.F, s.H, MS_GEMV_EPI_SWIGLU, s.H / s.resid_rt);
  if (const char* v = getenv("MS_GRAPH_STEPS")) s.graph_steps = std::max(1, std::min(atoi(v), 16));
  env_flag("MS_OVERLAP", s.overlap); env_flag("MS_PERSIST", s.persist);
  if (const char* v = getenv("MS_DECODE_RUN")) s.max_run = std::max(1, std::min(atoi(v), 64));
  if (const char* ng = getenv("MAPSUM_NO_GRAPHS")) s.use_graphs = !(ng[0] == '1');
  return s;
}

// One decode matrix: out[M][N] = X[M][K] . W^T from its K-quant slot (or null) or its fp16 rows.
struct DecodeMat {
  const QSlot* q = nullptr;
  const f16_t* W = nullptr;
  int N = 0, K = 0;
  int split = 1, dsplit = 1;  // split-K slabs in the small / the large regime
  int kh = 1;                 // skinny-GEMM block form (k_dgemm.hip kh)
  int wn = 4;                 // its weight-row groups at <= 128 rows (0: the library's setting)
  bool f16_rows = true;       // a candidate for the fp16-rows skinny GEMM (never the lm_head)
  bool tile128 = false;       // a candidate for the 128x128 GEMM tile (the lm_head from lm_gemm_min)
};

inline DecodeMat decode_mat(const DecodeSettings& s, int which, const QSlot* q, const f16_t* W) {
  DecodeMat m{q, W};
  switch (which) {
    case QS_QKV: m.N = s.QKVN; m.K = s.H; m.split = s.split_qkv; m.dsplit = s.dsplit_qkv; m.wn = s.dwn_qkv; break;
    case QS_O: m.N = s.H; m.K = s.QD; m.split = s.split_o; m.dsplit = s.dsplit_o; m.wn = s.dwn_o; break;
    case QS_GU: m.N = 2 * s.F; m.K = s.H; m.kh = s.dgemm_kh; m.wn = 0; break;
    case QS_DOWN: m.N = s.H; m.K = s.F; m.split = s.split_down; m.dsplit = s.dsplit_down; m.wn = s.dwn_down; break;
    default:  // QS_LM
      m.N = s.V; m.K = s.H; m.wn = s.dwn_lm; m.f16_rows = false;
      m.tile128 = s.lm_gemm_min > 0 && s.max_batch >= s.lm_gemm_min;
  }
  return m;
}

enum Family { F_NONE = 0, F_GEMV, F_QGEMV, F_DGEMM, F_QDGEMM, F_QDGEMM_F16, F_GEMM128 };
inline bool small_family(Family f) { return f == F_GEMV || f == F_QGEMV; }

// one launch (or, with lm_gate, the whole batch a row-group loop will cut into launches)
struct FormCall {
  int M = 0, epi = 0;
  int rs_tiles = 0;    // statistics tiles of the deferred row scale the call asks about (0: none)
  bool slabs = false;  // fp32 split-K slabs [S][M][N] (epi STORE_F32); else one output, S = 1
  // the lm_heads: "none" unless the fp16 GEMV takes a row group of this batch with its statistics
  // (above kMaxGemvRows rows: row groups, one-tile statistics only); the caller's fallback follows
  bool lm_gate = false;
  // the greedy lm_head: the large regime only where the plain skinny GEMM takes the shape, else the
  // small-regime families are ranked; without it a large-regime engine never takes those
  bool dgemm_gate = false;
  bool presupported = false;  // O / down residual epilogue: Q-GEMV support settled per engine (qresid_ok)
};
struct Form {
  Family family = F_NONE;
  int S = 1;  // slabs written, or 1
  bool slabs = false;
};

inline int dgemm_wn(const DecodeMat& m, int M) { return M <= 128 && m.N % 128 == 0 ? m.wn : 4; }
// the K-quant skinny GEMM streams this matrix's packed rows (MS_QDGEMM)
inline bool qdgemm_ok(const DecodeSettings& s, const QSlot* q, int M, int N, int K, int S, int epi) {
  if (!s.qdgemm_mode || !q || !q->ready()) return false;
  const QMat& m = q->m;
  if (m.type0 == MS_QT_Q8_0) return false;  // no packed Q8_0 skinny GEMM: the fp16 copies
  const bool q4 = m.type0 == MS_QT_Q4_K && (m.n < 2 || m.type1 == MS_QT_Q4_K) && (m.n < 3 || m.type2 == MS_QT_Q4_K);
  const bool q5 = m.type0 == MS_QT_Q5_K && (m.n < 2 || m.type1 == MS_QT_Q5_K) && (m.n < 3 || m.type2 == MS_QT_Q5_K);
  return (q4 || s.qdgemm_mode == 2 || (q5 && s.qdgemm_mode == 1)) && qdgemm_supported(M, N, K, S, epi, m);
}

// THE ranking of the decode kernel families.  Large regime: the K-quant skinny GEMM on packed
// rows, then the fp16-rows skinny GEMM or the 128x128 tile, then the plain skinny GEMM on the fp16
// rows (the skinny GEMMs fold one-tile statistics only).  Small regime: the Q-GEMV where the matrix
// is quantised and the Q plan takes the shape, else the fp16 GEMV; for slabs the quantised split
// is qsplit (0: the fp16 one), and an unsupported split falls back to 1.
inline Form pick_form(const DecodeSettings& s, const DecodeMat& m, const FormCall& c) {
  const int M = c.M, N = m.N, K = m.K, epi = c.epi;
  if (s.large()) {
    const int S = c.slabs ? m.dsplit : 1;
    const bool one_tile = c.rs_tiles <= 1;
    const bool dg = one_tile && dgemm_supported(M, N, K, S, epi, m.kh, dgemm_wn(m, M));
    if (dg || !c.dgemm_gate) {
      if (one_tile && qdgemm_ok(s, m.q, M, N, K, S, epi)) return {F_QDGEMM, S, c.slabs};
      const bool qdf = m.f16_rows && !s.has_quant && s.qdf_min > 0 && s.max_batch >= s.qdf_min;
      if (qdf && qdgemm_f16_supported(M, N, K, S, epi)) return {F_QDGEMM_F16, S, c.slabs};
      // argmax partials carry no row scale (r > 0 keeps every row's order)
      if (m.tile128 && K % 64 == 0 && (epi == MS_GEMV_EPI_ARGMAX ? N % 16 == 0 : gemm_rs_tiles_ok(M, N, c.rs_tiles)))
        return {F_GEMM128, 1, false};
      return dg ? Form{F_DGEMM, S, c.slabs} : Form{};
    }
  }
  const int Mg = std::min(M, kMaxGemvRows);
  if (c.lm_gate && !(gemv_supported(Mg, N, K, epi, c.rs_tiles) &&
                     (M <= kMaxGemvRows || (s.row_groups(M) && c.rs_tiles <= 1))))
    return {};
  const bool q = m.q && m.q->ready() && (c.presupported || qgemv_supported(Mg, N, K, epi, c.rs_tiles));
  if (!c.slabs) return {q ? F_QGEMV : F_GEMV, 1, false};
  // Q4_K/Q6_K: split-K like fp16 (a 16-row tile carries 3.6x fewer weight bytes, so the unsplit
  // grid -- 192 blocks for O/down -- is too thin to cover 256 CUs)
  const int S = q && s.qsplit > 0 ? s.qsplit : m.split;
  if (q) return {F_QGEMV, S > 1 && S <= kMaxSplit && qgemv_split_supported(M, N, K, S) ? S : 1, true};
  return {F_GEMV, S >= 1 && S <= kMaxSplit && gemv_split_supported(M, N, K, S) ? S : 1, true};
}

// Decode attention's split grid.  A run of k chained steps launches one grid, set from its longest
// sequence at the run's last step rounded UP to 256 keys, so the grid (and the captured graph) only
// changes at multiples of 256; ms_step bounds k so that a run never crosses one (decode_run_cap).
// When max_ctx is no multiple of 256 the grid passes max_ctx: the v1 / v2 partial workspaces and
// the persistent step's partial stride are sized for attn_ws_ctx(max_ctx), the longest grid an
// engine can launch (tests/native/decode_forms.cpp sweeps every reachable length against them).
inline int attn_ws_ctx(int max_ctx) { return (max_ctx + 255) / 256 * 256; }
inline int decode_grid_len(int max_len, int k) { return ((max_len + k - 1 + 255) / 256) * 256; }
inline int decode_run_cap(int max_len) { return ((max_len + 255) / 256) * 256 - max_len + 1; }
// v2's splits over a grid of grid_len keys (ppb pages per block), as launch_attn_decode2 counts them
inline int attn2_nsplit(int grid_len, int ppb) { return ((grid_len + kPage - 1) / kPage + ppb - 1) / ppb; }

}  // namespace ms
