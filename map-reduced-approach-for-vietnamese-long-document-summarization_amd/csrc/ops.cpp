// ops.cpp -- libmapsum's stateless entry points (include/mapsum.h): the op-level ms_op_* calls (each
// validates its operands and launches on the caller's stream) and the library-wide setters / stamp readers.
#include <cstdint>
#include <functional>

#include "internal.h"
#include "kernels.h"
#include "kvq8.h"

using namespace ms;

static int op_guard(const std::function<void()>& fn) {
  try {
    fn();
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) {
      g_last_error = std::string("kernel launch failed: ") + hipGetErrorString(err);
      return MS_EIO;
    }
    return MS_OK;
  } catch (const MsError& x) {
    g_last_error = x.what();
    return x.code;
  }
}

// a library-wide setter or stamp reader: validate, then apply
template <class Fn>
static int checked(bool ok, Fn&& fn) {
  if (!ok) return MS_EINVAL;
  fn();
  return MS_OK;
}

// the deferred RMSNorm scale the next op calls of this thread apply (ms_op_set_row_scale)
static thread_local RowScale g_op_rs{};
static int op_rs_tiles() { return g_op_rs.ssq ? g_op_rs.tiles : 0; }

static const GemvArgs* op_gemv_args(GemvArgs& ga) {
  ga = GemvArgs{};
  ga.rs = g_op_rs;
  return g_op_rs.ssq ? &ga : nullptr;
}

// the residual epilogue's arguments (RESID_SSQ)
static GemvArgs op_resid_args(int rt, float* ssq_out, const void* gamma, void* xg_out) {
  GemvArgs ga{};
  ga.rt = rt;
  ga.ssq_out = ssq_out;
  ga.gamma = (const f16_t*)gamma;
  ga.xg_out = (f16_t*)xg_out;
  return ga;
}

// packed rows [N][K / 256 blocks] of one quant type as a one-region matrix
static QMat op_qmat(int type, const void* packed, int K) {
  QMat q{};
  q.n = 1;
  q.base0 = (const uint8_t*)packed;
  q.row0_0 = 0;
  q.type0 = type;
  q.row_bytes0 = (K / 256) * qblock_bytes(type, true);
  return q;
}

extern "C" {

int ms_op_set_row_scale(const float* ssq, int32_t tiles, int32_t hidden, float eps) {
  if (ssq && (tiles < 1 || hidden < 1)) return MS_EINVAL;
  g_op_rs = ssq ? make_row_scale(ssq, tiles, hidden, eps) : RowScale{};
  return MS_OK;
}

int ms_op_gemm(const void* A, const void* W, void* out, int32_t M, int32_t N, int32_t K, int32_t ldo,
               int32_t epi, void* stream) {
  return op_guard([&] {
    REQUIRE(A && W && out && M >= 1 && N >= 16 && K >= 64 && K % 64 == 0, MS_EINVAL, "bad gemm shape");
    REQUIRE(((epi >= 0 && epi <= 3) || epi == MS_EPI_ARGMAX) && (epi != MS_EPI_SWIGLU || N % 32 == 0), MS_EINVAL,
            "bad epilogue");
    REQUIRE(epi != MS_EPI_ADD_F32 || (N % 4 == 0 && ldo % 4 == 0), MS_EINVAL,
            "residual gemm: N and ldo multiples of 4 (16-B x rows)");
    // argmax: {max, id} float2 partials [M][ldo >= N / 16], the 128x128 tile, no row scale
    REQUIRE(epi != MS_EPI_ARGMAX || (N % 16 == 0 && ldo >= N / 16), MS_EINVAL, "gemm argmax: N % 16, ldo >= N / 16");
    // the epilogues store 4 consecutive columns per lane (8 B fp16, 16 B fp32)
    REQUIRE(((uintptr_t)out & ((epi == MS_EPI_ADD_F32 || epi == MS_EPI_STORE_F32) ? 15 : 7)) == 0, MS_EINVAL,
            "gemm: out must be 16-B (fp32) / 8-B (fp16) aligned");
    REQUIRE(!g_op_rs.ssq || gemm_rs_tiles_ok(M, N, g_op_rs.tiles), MS_EINVAL,
            "gemm row scale: at most 24 tiles of statistics (kGemmRsTiles, both GEMM tiles)");
    launch_gemm((const f16_t*)A, (const f16_t*)W, out, M, N, K, ldo, epi == MS_EPI_ARGMAX ? MS_GEMV_EPI_ARGMAX : epi,
                (hipStream_t)stream, &g_op_rs);
  });
}

int ms_op_gemm_resid(const void* A, const void* W, float* x, void* xg_out, const void* gamma, float* ssq_out,
                     int32_t M, int32_t N, int32_t K, void* stream) {
  return op_guard([&] {
    REQUIRE(A && W && x && xg_out && gamma && ssq_out && M >= 1 && N >= 16 && K >= 64 && K % 64 == 0, MS_EINVAL,
            "bad gemm_resid operands (K % 64 == 0)");
    REQUIRE(gemm_resid_tiles(M, N) <= kGemmRsTiles, MS_EINVAL, "gemm_resid: N over 24 column tiles");
    REQUIRE(N % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)xg_out & 7) == 0, MS_EINVAL,
            "gemm_resid: N a multiple of 4, x 16-B and xg 8-B aligned (vector rows)");
    GemmResid gr{(const f16_t*)gamma, (f16_t*)xg_out, ssq_out};
    launch_gemm((const f16_t*)A, (const f16_t*)W, x, M, N, K, N, MS_EPI_ADD_F32, (hipStream_t)stream, nullptr, &gr);
  });
}

int ms_gemm_resid_tiles(int32_t M, int32_t N) { return gemm_resid_tiles(M, N); }

int ms_set_gemm_variant(int32_t v) { return checked(v >= 0 && v <= 4, [&] { set_gemm_variant(v); }); }
int ms_set_gemv_order(int32_t order) { return checked(order >= -1 && order <= 8, [&] { set_gemv_order(order); }); }
int ms_set_attn_tuning(int32_t combine_grp, int32_t order) {
  return checked(combine_grp >= 0 && combine_grp <= 1 && (order == 0 || order == 3),
                 [&] { set_attn_tuning(combine_grp, order); });
}
int ms_set_dgemm_kh(int32_t kh) { return checked(kh == 1 || kh == 2, [&] { set_dgemm_kh(kh); }); }
int ms_set_dgemm_wn(int32_t wn) { return checked(wn == 4 || wn == 8, [&] { set_dgemm_wn(wn); }); }
int ms_set_qgemv_gs(int32_t on) { return checked(on >= 0 && on <= 1, [&] { set_qgemv_gs(on != 0); }); }

// the kernels' per-block phase stamps of their latest stamped launch (tools/*_stamps.py)
static int stamps(void (*read)(unsigned long long*, int), uint64_t* out, int32_t n) {
  return checked(out && n >= 0, [&] { read(reinterpret_cast<unsigned long long*>(out), n); });
}
int ms_debug_gemv_stamps(uint64_t* out, int32_t n) { return stamps(gemv_stamps, out, n); }
int ms_debug_pk_stamps(uint64_t* out, int32_t n) { return stamps(persist_stamps, out, n); }
int ms_debug_a2_stamps(uint64_t* out, int32_t n) { return stamps(attn2_stamps, out, n); }

int64_t ms_op_gemv_workspace(int32_t M, int32_t N, int32_t K) {
  if (M < 1 || M > 64 || N < 16 || K < 64 || K % 64) return MS_EINVAL;
  return (int64_t)gemv_workspace_bytes(M, N, K);
}

int ms_op_gemv(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K, int32_t ldo,
               int32_t epi, void* ws, void* stream) {
  return ms_op_gemv_tuned(X, W, out, M, N, K, ldo, epi, ws, 0, stream);
}

int ms_op_gemv_tuned(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K,
                     int32_t ldo, int32_t epi, void* ws, int32_t waves, void* stream) {
  return op_guard([&] {
    // (the plain stores take a ragged last tile: its rows are clamped on load and masked in the epilogue)
    const bool ragged_ok = epi == MS_EPI_STORE_F16 || epi == MS_EPI_STORE_F32;
    REQUIRE(X && W && out && ws && N >= 16 && (N % 16 == 0 || ragged_ok), MS_EINVAL, "bad gemv operands");
    REQUIRE(((epi >= 0 && epi <= 3) || epi == MS_EPI_ARGMAX) && (epi != MS_EPI_SWIGLU || N % 32 == 0),
            MS_EINVAL, "bad epilogue");
    REQUIRE(gemv_supported(M, N, K, epi, op_rs_tiles()), MS_EINVAL,
            "gemv shape unsupported (M<=64, K%64==0, K/64 split into <=16 waves of <=8 steps; "
            "row-scale statistics within kRsStage and LDS)");
    GemvArgs ga;
    launch_gemv_ex((const f16_t*)X, (const f16_t*)W, out, M, N, K, ldo, epi, op_gemv_args(ga), waves,
                   (hipStream_t)stream);
  });
}

int ms_op_gemv_strided(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K,
                       int32_t ldk, int32_t ldo, int32_t epi, void* stream) {
  return op_guard([&] {
    REQUIRE(X && W && out && N >= 16 && N % 16 == 0 && ldk >= K && ldk % 8 == 0, MS_EINVAL,
            "bad strided gemv operands");
    REQUIRE(epi >= 0 && epi <= 3 && epi != MS_EPI_SWIGLU, MS_EINVAL, "bad epilogue");
    REQUIRE(gemv_supported(M, N, K, epi), MS_EINVAL, "gemv shape unsupported");
    launch_gemv_strided((const f16_t*)X, (const f16_t*)W, out, M, N, K, ldk, ldo, epi, (hipStream_t)stream);
  });
}

int ms_op_gemv_resid(const void* X, const void* W, float* x, void* xg_out, const void* gamma,
                     float* ssq_out, int32_t M, int32_t N, int32_t K, int32_t rt, void* stream) {
  return op_guard([&] {
    // (a ragged last tile is fine: its rows are clamped on load and masked in the epilogue)
    REQUIRE(X && W && x && xg_out && gamma && ssq_out && rt >= 1 && rt <= 16 && N >= 1, MS_EINVAL,
            "bad gemv_resid operands");
    REQUIRE(gemv_supported(M, N, K, MS_GEMV_EPI_RESID_SSQ), MS_EINVAL, "gemv_resid shape unsupported");
    const GemvArgs ga = op_resid_args(rt, ssq_out, gamma, xg_out);
    launch_gemv_ex((const f16_t*)X, (const f16_t*)W, x, M, N, K, N, MS_GEMV_EPI_RESID_SSQ, &ga, 0,
                   (hipStream_t)stream);
  });
}

int ms_op_dgemm(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K, int32_t S,
                int32_t ldo, int32_t epi, void* stream) {
  return op_guard([&] {
    REQUIRE(X && W && out, MS_EINVAL, "bad dgemm operands");
    REQUIRE(((epi >= 0 && epi <= 3) || epi == MS_EPI_ARGMAX) && dgemm_supported(M, N, K, S, epi), MS_EINVAL,
            "dgemm shape unsupported (M <= 256, N % 64 == 0, K % (64 S) == 0, S > 1 only for fp32 slabs)");
    REQUIRE(!g_op_rs.ssq || g_op_rs.tiles == 1, MS_EINVAL, "dgemm row scale: one-tile statistics only");
    launch_dgemm((const f16_t*)X, (const f16_t*)W, out, M, N, K, S, ldo, epi, (hipStream_t)stream, &g_op_rs);
  });
}

int ms_op_gemv_split(const void* X, const void* W, float* slabs, int32_t M, int32_t N, int32_t K,
                     int32_t S, int32_t waves, void* stream) {
  return op_guard([&] {
    REQUIRE(X && W && slabs && N >= 16 && S >= 1, MS_EINVAL, "bad gemv_split operands");
    REQUIRE(gemv_split_supported(M, N, K, S, op_rs_tiles()), MS_EINVAL,
            "gemv_split shape unsupported (M<=64, (K/S)%64==0, row-scale statistics within kRsStage and LDS)");
    GemvArgs ga;
    launch_gemv_split((const f16_t*)X, (const f16_t*)W, slabs, M, N, K, S, waves, (hipStream_t)stream,
                      op_gemv_args(ga));
  });
}

int ms_op_residual_rmsnorm(float* x, const float* slabs, int32_t S, const void* w, void* y, float* ssq,
                           int32_t rows, int32_t hidden, void* stream) {
  return op_guard([&] {
    REQUIRE(x && w && y && ssq && rows >= 1 && hidden >= 4 && hidden % 4 == 0 && hidden <= 8192, MS_EINVAL,
            "bad residual_rmsnorm shape");
    REQUIRE(S == 0 || slabs, MS_EINVAL, "slabs missing");
    REQUIRE(residual_rmsnorm_supported(S, hidden) || (S == 0 && hidden <= 8192), MS_EINVAL,
            "residual_rmsnorm: S <= 8 and hidden <= 3072 (wider rows: S == 0 only)");
    launch_residual_rmsnorm(x, slabs, S, (const f16_t*)w, (f16_t*)y, ssq, rows, hidden,
                            (hipStream_t)stream);
  });
}

int ms_op_dequant(int32_t type, const void* blocks, int64_t n_blocks, float* out, void* stream) {
  return op_guard([&] {
    REQUIRE(blocks && out && n_blocks >= 1, MS_EINVAL, "bad dequant arguments");
    REQUIRE(qtype_known(type), MS_EINVAL, "ggml type must be Q8_0, Q4_K, Q5_K or Q6_K");
    launch_dequant_f32(type, (const uint8_t*)blocks, n_blocks, out, (hipStream_t)stream);
  });
}

int ms_op_quant_rows(int32_t type, const void* blocks, int32_t rows, int32_t K, void* f16_out,
                     void* packed_out, void* stream) {
  return op_guard([&] {
    REQUIRE(blocks && f16_out && rows >= 1 && K >= 256 && K % 256 == 0, MS_EINVAL, "bad quant_rows arguments");
    REQUIRE(qtype_known(type), MS_EINVAL, "ggml type must be Q8_0, Q4_K, Q5_K or Q6_K");
    launch_quant_rows(type, (const uint8_t*)blocks, rows, K, (f16_t*)f16_out, 16, 0,
                      (uint8_t*)packed_out, 0, (hipStream_t)stream);
  });
}

int ms_op_qgemv(const void* X, int32_t type, const void* packed, void* out, int32_t M, int32_t N,
                int32_t K, int32_t ldo, int32_t epi, void* stream) {
  return op_guard([&] {
    REQUIRE(X && packed && out && N >= 16, MS_EINVAL, "bad qgemv operands");
    REQUIRE(qtype_known(type), MS_EINVAL, "ggml type must be Q8_0, Q4_K, Q5_K or Q6_K");
    REQUIRE(((epi >= 0 && epi <= 3) || epi == MS_EPI_ARGMAX) && (epi != MS_EPI_SWIGLU || N % 32 == 0),
            MS_EINVAL, "bad epilogue");
    REQUIRE(qgemv_supported(M, N, K, epi, op_rs_tiles()), MS_EINVAL,
            "qgemv shape unsupported (M<=64, K%256==0, N%16==0, row-scale statistics within kRsStage and LDS)");
    GemvArgs ga;
    launch_qgemv((const f16_t*)X, op_qmat(type, packed, K), out, M, N, K, ldo, epi, op_gemv_args(ga),
                 (hipStream_t)stream);
  });
}

int ms_op_qgemv_split(const void* X, int32_t type, const void* packed, float* slabs, int32_t M,
                      int32_t N, int32_t K, int32_t S, void* stream) {
  return op_guard([&] {
    REQUIRE(X && packed && slabs && N >= 16 && S >= 1, MS_EINVAL, "bad qgemv_split operands");
    REQUIRE(qtype_known(type), MS_EINVAL, "ggml type must be Q8_0, Q4_K, Q5_K or Q6_K");
    REQUIRE(qgemv_split_supported(M, N, K, S, op_rs_tiles()), MS_EINVAL,
            "qgemv_split shape unsupported (M<=64, K%(256*S)==0, row-scale statistics within kRsStage and LDS)");
    GemvArgs ga;
    launch_qgemv_split((const f16_t*)X, op_qmat(type, packed, K), slabs, M, N, K, S, (hipStream_t)stream,
                       op_gemv_args(ga));
  });
}

int ms_op_qgemv_resid(const void* X, int32_t type, const void* packed, float* x, void* xg_out, const void* gamma,
                      float* ssq_out, int32_t M, int32_t N, int32_t K, int32_t rt, void* stream) {
  return op_guard([&] {
    REQUIRE(X && packed && x && xg_out && gamma && ssq_out && rt >= 1 && rt <= 16 && N % rt == 0, MS_EINVAL,
            "bad qgemv_resid operands");
    REQUIRE(qtype_known(type), MS_EINVAL, "ggml type must be Q8_0, Q4_K, Q5_K or Q6_K");
    REQUIRE(qgemv_supported(M, N, K, MS_GEMV_EPI_RESID_SSQ), MS_EINVAL, "qgemv_resid shape unsupported");
    const GemvArgs ga = op_resid_args(rt, ssq_out, gamma, xg_out);
    launch_qgemv((const f16_t*)X, op_qmat(type, packed, K), x, M, N, K, N, MS_GEMV_EPI_RESID_SSQ, &ga,
                 (hipStream_t)stream);
  });
}

int ms_op_qdgemm(const void* X, int32_t type, const void* packed, void* out, int32_t M, int32_t N, int32_t K,
                 int32_t S, int32_t ldo, int32_t epi, void* stream) {
  return op_guard([&] {
    REQUIRE(X && packed && out && N >= 64 && K >= 256 && S >= 1, MS_EINVAL, "bad qdgemm operands");
    REQUIRE(type != MS_QT_Q8_0, MS_EINVAL,
            "qdgemm has no Q8_0 form (Q8_0 engines run their fp16 copies in the large regime): Q4_K, Q5_K, Q6_K or F16");
    REQUIRE(type == MS_QT_Q4_K || type == MS_QT_Q5_K || type == MS_QT_Q6_K || type == 1, MS_EINVAL,
            "ggml type must be Q4_K, Q5_K, Q6_K or F16");
    REQUIRE(!g_op_rs.ssq || g_op_rs.tiles == 1, MS_EINVAL, "qdgemm row scale: one-tile statistics only");
    const int e = epi == MS_EPI_ARGMAX ? MS_GEMV_EPI_ARGMAX : epi;
    if (type == 1) {  // fp16 rows [N][K] through the same kernel
      REQUIRE(qdgemm_f16_supported(M, N, K, S, e), MS_EINVAL, "qdgemm (fp16 rows) shape unsupported");
      launch_qdgemm_f16((const f16_t*)X, (const f16_t*)packed, out, M, N, K, S, ldo, e, (hipStream_t)stream, &g_op_rs);
      return;
    }
    const QMat q = op_qmat(type, packed, K);
    REQUIRE(qdgemm_supported(M, N, K, S, e, q), MS_EINVAL,
            "qdgemm shape unsupported (M <= 256, N % 64 == 0, K % (256 S) == 0, S > 1 only for fp32 slabs)");
    launch_qdgemm((const f16_t*)X, q, out, M, N, K, S, ldo, e, (hipStream_t)stream, &g_op_rs);
  });
}

int ms_op_rmsnorm(const void* x, const void* w, void* y, float* ssq, int32_t rows, int32_t hidden,
                  const int32_t* row_idx, void* stream) {
  return op_guard([&] {
    REQUIRE(x && w && y && ssq && rows >= 1 && hidden >= 4 && hidden % 4 == 0 && hidden <= 8192, MS_EINVAL,
            "bad rmsnorm shape");
    launch_rmsnorm((const float*)x, (const f16_t*)w, (f16_t*)y, ssq, rows, hidden, row_idx,
                   (hipStream_t)stream);
  });
}

int ms_op_qk_norm_rope(void* qkv, const float* slabs, int32_t S, int32_t T, int32_t n_heads, int32_t n_kv_heads,
                       const int32_t* tok_pos, const int32_t* tok_slot, const float* cos_tab, const float* sin_tab,
                       const void* q_gain, const void* k_gain, float eps, void* k_pool, void* v_pool,
                       const int32_t* block_table, int32_t max_pages, void* stream) {
  return op_guard([&] {
    REQUIRE(qkv && tok_pos && tok_slot && cos_tab && sin_tab && q_gain && k_gain && k_pool && v_pool && block_table,
            MS_EINVAL, "qk_norm_rope: null operand");
    REQUIRE(T >= 1 && n_heads >= 1 && n_kv_heads >= 1 && n_heads + n_kv_heads <= 64 && max_pages >= 1, MS_EINVAL,
            "bad qk_norm_rope shape (at most 64 query+key heads)");
    REQUIRE(!slabs || (S >= 1 && S <= 8), MS_EINVAL, "qk_norm_rope: 1..8 slabs");
    REQUIRE(!slabs || !g_op_rs.ssq || g_op_rs.tiles <= 256, MS_EINVAL, "qk_norm_rope row scale: at most 256 tiles");
    REQUIRE(((uintptr_t)qkv & 3) == 0 && ((uintptr_t)v_pool & 3) == 0, MS_EINVAL, "qk_norm_rope: 4-B aligned rows");
    KVView kv{(f16_t*)k_pool, (f16_t*)v_pool, block_table, max_pages, n_kv_heads, 0};
    launch_qk_norm_rope((f16_t*)qkv, slabs, slabs ? S : 0, T, slabs ? g_op_rs : RowScale{}, T, n_heads, n_kv_heads,
                        tok_pos, tok_slot, cos_tab, sin_tab, (const f16_t*)q_gain, (const f16_t*)k_gain, eps, kv,
                        (hipStream_t)stream);
  });
}

int ms_op_kv_store_q8_0(const void* k_rows, const void* v_rows, int32_t T, int32_t n_kv_heads, const int32_t* tok_pos,
                        const int32_t* tok_slot, void* k_pool, void* v_pool, const int32_t* block_table,
                        int32_t max_pages, void* stream) {
  return op_guard([&] {
    REQUIRE(k_rows && v_rows && tok_pos && tok_slot && k_pool && v_pool && block_table, MS_EINVAL,
            "kv_store_q8_0: null operand");
    REQUIRE(T >= 1 && n_kv_heads >= 1 && max_pages >= 1, MS_EINVAL, "bad kv_store_q8_0 shape");
    REQUIRE((((uintptr_t)k_rows | (uintptr_t)v_rows) & 3) == 0 && (((uintptr_t)k_pool | (uintptr_t)v_pool) & 15) == 0,
            MS_EINVAL, "kv_store_q8_0: 4-B aligned rows, 16-B aligned pools");
    const KVQ8View q8{(uint8_t*)k_pool, (uint8_t*)v_pool, block_table, max_pages, n_kv_heads, 0};
    launch_kv_store_q8((const f16_t*)k_rows, (const f16_t*)v_rows, T, n_kv_heads, tok_pos, tok_slot, q8,
                       (hipStream_t)stream);
  });
}

int64_t ms_op_attn_decode_q8_0_workspace(int32_t B, int32_t n_heads, int32_t max_len, int32_t ppw) {
  if (B < 1 || n_heads < 1 || max_len < 1 || ppw < 1 || ppw > 16) return MS_EINVAL;
  return (int64_t)B * n_heads * attn_decode_nsplit(ppw, max_len) * 132 * (int64_t)sizeof(float);
}

int ms_op_attn_decode_q8_0(const void* qkv, int32_t n_heads, int32_t n_kv_heads, const void* k_pool, const void* v_pool,
                           const int32_t* block_table, int32_t max_pages, int32_t slot_major, const int32_t* seq_len,
                           const int32_t* seq_slot, int32_t B, int32_t max_len, int32_t ppw, float* workspace,
                           void* out, void* stream) {
  return op_guard([&] {
    REQUIRE(qkv && k_pool && v_pool && block_table && seq_len && seq_slot && workspace && out, MS_EINVAL,
            "attn_decode_q8_0: null operand");
    REQUIRE(B >= 1 && max_len >= 1 && max_pages >= (max_len + kPage - 1) / kPage && ppw >= 1 && ppw <= 16, MS_EINVAL,
            "bad attn_decode_q8_0 shape (1 <= ppw <= 16, max_pages covers max_len)");
    REQUIRE(n_kv_heads >= 1 && attn_decode_supported(B, n_heads, n_kv_heads, max_len, ppw), MS_EINVAL,
            "attn_decode_q8_0: group of at most 8 query heads per kv head, at most 127 splits");
    REQUIRE((((uintptr_t)k_pool | (uintptr_t)v_pool | (uintptr_t)qkv) & 15) == 0, MS_EINVAL,
            "attn_decode_q8_0: 16-B aligned pools and rows");
    const KVQ8View kv{(uint8_t*)k_pool, (uint8_t*)v_pool, block_table, max_pages, n_kv_heads, slot_major ? 1 : 0};
    const DecodeAttnArgs a{seq_len, seq_slot, B, max_len, ppw};
    launch_attn_decode_q8((const f16_t*)qkv, (f16_t*)out, n_heads, n_kv_heads, kv, a, workspace, (hipStream_t)stream);
  });
}

int ms_op_argmax_partials(const void* partials, int32_t rows, int32_t tiles, int32_t* ids, void* stream) {
  return op_guard([&] {
    REQUIRE(partials && ids && rows >= 1 && tiles >= 1, MS_EINVAL, "bad argmax_partials shape");
    launch_argmax_partials(partials, rows, tiles, ids, (hipStream_t)stream);
  });
}

int ms_op_sample(const float* logits, int32_t rows, int32_t n, int64_t ldl, const ms_sampling* params,
                 const int32_t* win, const int32_t* win_len, const int32_t* steps, int32_t* ids,
                 int32_t* cand_ids, float* cand_p, int32_t* cand_n, void* stream) {
  return op_guard([&] {
    REQUIRE(logits && params && win && win_len && steps && ids && rows >= 1, MS_EINVAL, "bad sample operands");
    REQUIRE(n >= 1 && n <= kSampleMaxN && ldl >= n, MS_EINVAL,
            "bad sample shape (1 <= n <= " + std::to_string(kSampleMaxN) + ", ldl >= n)");
    REQUIRE((cand_ids && cand_p && cand_n) || (!cand_ids && !cand_p && !cand_n), MS_EINVAL,
            "sample: the candidate outputs come together");
    const SampleArgs a{logits, ldl, n, reinterpret_cast<const SampleParams*>(params), win, win_len, steps,
                       /*slots*/ nullptr, /*row_slot*/ nullptr, ids, cand_ids, cand_p, cand_n};
    launch_sample_rows(a, rows, (hipStream_t)stream);
  });
}

int ms_op_argmax(const void* logits, int32_t rows, int32_t n, int32_t* ids, void* stream) {
  return op_guard([&] {
    REQUIRE(logits && ids && rows >= 1 && n >= 1, MS_EINVAL, "bad argmax shape");
    launch_argmax((const float*)logits, rows, n, ids, (hipStream_t)stream);
  });
}

}  // extern "C"
