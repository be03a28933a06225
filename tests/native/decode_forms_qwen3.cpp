// decode_forms_qwen3.cpp -- the decode regime table at the Qwen3-8B widths, checked on the CPU.
//
// Built by `make -C map-reduced-approach-for-vietnamese-long-document-summarization_amd/csrc forms`
// next to decode_forms.cpp and, like it, linked against the library's objects without making a HIP
// call (tests/test_decode_forms_qwen3.py).  The default splits are tuned for K = 3072 / 8192; here
// K = 4096 / 12288 (hidden 4096, ffn 12288, 32 / 8 heads of 128, vocab 151936), where split 6 does
// not divide 4096 in whole 64-k steps.  For fp16 and Q4_K_M engines of 8 / 20 / 32 / 128 / 256
// slots and EVERY row count 1 .. max_batch, each projection's pick_form result -- asked as the
// engine asks -- must be a real kernel family with a split its launcher accepts, and the family's
// split must be the same at every row count of one engine (a row's sum order, so batch invariance).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>

#include "decode_forms.h"

using namespace ms;

struct Eng {
  DecodeSettings s;
  QSlot q[5];
};

static void region(QSlot& q, int i, int row0, int type, int K) {
  int* r0[3] = {&q.m.row0_0, &q.m.row0_1, &q.m.row0_2};
  int* ty[3] = {&q.m.type0, &q.m.type1, &q.m.type2};
  int* rb[3] = {&q.m.row_bytes0, &q.m.row_bytes1, &q.m.row_bytes2};
  *r0[i] = row0; *ty[i] = type; *rb[i] = (K / 256) * qblock_bytes(type, true);
  q.m.n = i + 1;
  q.need = q.loaded = 1;
}

static Eng make(int slots, bool quant, bool q6_rows) {
  ms_config c;
  std::memset(&c, 0, sizeof c);
  c.abi_version = MS_ABI_VERSION;
  c.n_layers = 36; c.hidden = 4096; c.n_heads = 32; c.n_kv_heads = 8; c.head_dim = 128;
  c.ffn = 12288; c.vocab = 151936; c.max_batch = slots; c.max_ctx = 4096; c.max_prefill_tokens = 4096;
  Eng e;
  e.s = resolve_settings(c);
  if (!quant) return e;
  e.s.has_quant = true;
  const int base = MS_QT_Q4_K, more = q6_rows ? MS_QT_Q6_K : base, H = e.s.H, QD = e.s.QD, KD = 8 * 128;
  region(e.q[QS_QKV], 0, 0, base, H);
  region(e.q[QS_QKV], 1, QD, base, H);
  region(e.q[QS_QKV], 2, QD + KD, more, H);
  region(e.q[QS_O], 0, 0, base, QD);
  region(e.q[QS_GU], 0, 0, base, H);
  region(e.q[QS_DOWN], 0, 0, more, e.s.F);
  region(e.q[QS_LM], 0, 0, MS_QT_Q6_K, H);
  return e;
}

// what the launcher of form f checks before it launches M rows (engine.cpp launch_form)
static bool launcher_takes(const DecodeSettings& s, const DecodeMat& m, const Form& f, const FormCall& c) {
  const int M = c.M, N = m.N, K = m.K;
  switch (f.family) {
    case F_GEMV:
      return f.slabs ? gemv_split_supported(M, N, K, f.S) : gemv_supported(M, N, K, c.epi, c.rs_tiles);
    case F_QGEMV:
      if (f.slabs && f.S > 1) return qgemv_split_supported(M, N, K, f.S);
      return c.presupported ? s.qresid_ok : qgemv_supported(M, N, K, c.epi, c.rs_tiles);
    case F_DGEMM: return dgemm_supported(M, N, K, f.S, c.epi, m.kh, dgemm_wn(m, M));
    case F_QDGEMM: return qdgemm_supported(M, N, K, f.S, c.epi, m.q->m);
    case F_QDGEMM_F16: return qdgemm_f16_supported(M, N, K, f.S, c.epi);
    case F_GEMM128: return K % 64 == 0;
    default: return false;
  }
}

static int fails = 0;

// the engine's calls (engine.cpp proj_split / resid_update / proj / lm_head) at B rows in flight;
// row groups launch at most kMaxGemvRows rows at a time
static void check(const char* what, const Eng& e) {
  const DecodeSettings& s = e.s;
  static const char* fam[] = {"none", "GEMV", "QGEMV", "DGEMM", "QDGEMM", "F16ROWS", "GEMM128"};
  static const char* mat[] = {"QKV", "O", "gate/up", "down", "lm_head", "lm_head(sampling)"};
  std::printf("%-28s", what);
  for (int col = 0; col < 6; ++col) {
    const int which = std::min(col, (int)QS_LM);
    const bool samp = col == 5;
    const DecodeMat m = decode_mat(s, which, &e.q[which], nullptr);
    Form first{};
    bool ok = true;
    for (int B = 1; B <= s.max_batch && ok; ++B) {
      const int Bg = s.row_groups(B) ? std::min(B, kMaxGemvRows) : B;
      FormCall c{Bg, MS_GEMV_EPI_STORE_F32};
      if (which == QS_GU) {
        c.epi = MS_GEMV_EPI_SWIGLU;
      } else if (which == QS_LM) {
        const int tiles = s.resid_fused(&e.q[QS_DOWN]) ? s.H / s.resid_rt : 1;
        c = FormCall{B, samp ? MS_GEMV_EPI_STORE_F32 : MS_GEMV_EPI_ARGMAX, samp ? tiles : 0};
        c.lm_gate = true;
        c.dgemm_gate = !samp;
      } else if (which != QS_QKV && s.resid_fused(m.q)) {
        c.epi = MS_GEMV_EPI_RESID_SSQ;
        c.presupported = true;
      } else {
        c.slabs = true;
      }
      Form f = pick_form(s, m, c);
      FormCall lc = c;
      if (which == QS_LM && small_family(f.family)) {  // engine.cpp lm_head: the row-group loop asks again
        lc = FormCall{std::min(B, kMaxGemvRows), c.epi};  // (proj: no statistics in the question)
        lc.dgemm_gate = c.dgemm_gate;
        DecodeMat lm = m;
        if (samp && f.family != F_QGEMV) lm.q = nullptr;
        f = pick_form(s, lm, lc);
        lc.rs_tiles = c.rs_tiles;  // ... but the launch carries them
      }
      if (B == 1) first = f;
      const bool same = f.family == first.family && f.S == first.S && f.slabs == first.slabs;
      // the lm_heads may change family with the rows (greedy partials / stored logits carry no
      // split); every split projection must keep family and split
      const bool stable = which == QS_LM ? f.S == first.S : same;
      if (f.family == F_NONE || !launcher_takes(s, m, f, lc) || !stable) {
        std::printf(" %s:%s/%d@B=%d(!)", mat[col], fam[f.family], f.S, B);
        ok = false;
      }
    }
    if (ok) std::printf(" %s%s", fam[first.family], first.slabs ? ("/" + std::to_string(first.S)).c_str() : "");
    fails += !ok;
  }
  std::printf("\n");
}

int main() {
  std::printf("%-28s QKV O gate/up down lm_head(greedy) lm_head(sampling)   [at B = 1; every B checked]\n", "engine");
  for (int b : {8, 20, 32, 128, 256}) {
    check(("fp16 " + std::to_string(b)).c_str(), make(b, false, false));
    check(("Q4_K_M " + std::to_string(b)).c_str(), make(b, true, false));
    check(("Q4_K_M " + std::to_string(b) + ", Q6_K V / down").c_str(), make(b, true, true));
  }
  // the check has teeth: the untouched default split 6 is not a whole number of 64-k steps of 4096
  const bool teeth = !gemv_split_supported(8, 6144, 4096, 6) && !dgemm_supported(32, 6144, 4096, 6, MS_GEMV_EPI_STORE_F32, 1);
  fails += !teeth;
  std::printf("%s: %d failure(s)%s\n", fails ? "QWEN3_FORMS_FAIL" : "QWEN3_FORMS_OK", fails,
              teeth ? "" : " (split 6 at K = 4096 was expected to be refused)");
  return fails ? 1 : 0;
}
