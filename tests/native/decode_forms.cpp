// decode_forms.cpp -- the decode regime table, pinned on the CPU.
//
// Built by `make -C map-reduced-approach-for-vietnamese-long-document-summarization_amd/csrc forms`
// and linked against the library's objects; it makes no HIP call, so it runs on a machine without
// a GPU (tests/test_decode_forms.py).  For the Llama-3.2-3B shapes (hidden 3072, ffn 8192, vocab
// 128256, 24 / 8 heads of 128) it asks pick_form (csrc/decode_forms.h) -- with the calls the
// engine makes -- for the kernel family and split of QKV, O, gate/up, down and the lm_head (greedy
// and sampling) of every regime DESIGN.md §5 lists, and compares them with the table below.
// Quantised engines are QMat type fields filled by hand: no device pointers.
//
// It also sweeps the decode-attention workspaces (sweep_workspaces below): for every engine shape,
// MS_ATTN_PPB / MS_ATTN_PPW setting, reachable context length and run length, the split grid that
// decode_run launches (decode_forms.h decode_grid_len) must fit what ms_create allocates
// (attn_ws_ctx) -- the grid is rounded up to 256 keys and passes max_ctx when max_ctx is not a
// multiple of 256.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "decode_forms.h"

using namespace ms;

enum Weights { F16, Q4KM, Q4KM_Q6, Q5KM, Q8 };  // Q4KM_Q6: a layer whose V / down rows are Q6_K

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

static Eng make(int slots, Weights w) {
  ms_config c;
  std::memset(&c, 0, sizeof c);
  c.abi_version = MS_ABI_VERSION;
  c.n_layers = 28; c.hidden = 3072; c.n_heads = 24; c.n_kv_heads = 8; c.head_dim = 128;
  c.ffn = 8192; c.vocab = 128256; c.max_batch = slots; c.max_ctx = 4096; c.max_prefill_tokens = 4096;
  Eng e;
  e.s = resolve_settings(c);
  if (w == F16) return e;
  e.s.has_quant = true;
  const int base = w == Q8 ? MS_QT_Q8_0 : w == Q5KM ? MS_QT_Q5_K : MS_QT_Q4_K;
  const int more = w == Q4KM_Q6 ? MS_QT_Q6_K : base, H = e.s.H, QD = e.s.QD, KD = 8 * 128;
  region(e.q[QS_QKV], 0, 0, base, H);
  region(e.q[QS_QKV], 1, QD, base, H);
  region(e.q[QS_QKV], 2, QD + KD, more, H);
  region(e.q[QS_O], 0, 0, base, QD);
  region(e.q[QS_GU], 0, 0, base, H);
  region(e.q[QS_DOWN], 0, 0, more, e.s.F);
  region(e.q[QS_LM], 0, 0, w == Q8 ? MS_QT_Q8_0 : MS_QT_Q6_K, H);
  return e;
}

static std::string name(const Form& f, bool resid = false) {
  static const char* fam[] = {"none", "GEMV", "QGEMV", "DGEMM", "QDGEMM", "F16ROWS", "GEMM128"};
  std::string s = fam[f.family];
  if (f.slabs) s += "/" + std::to_string(f.S);
  return resid ? s + "+resid" : s;
}

// the engine's calls (engine.cpp proj_split / resid_update / proj / lm_head) at a full batch; row
// groups launch kMaxGemvRows rows at a time
static std::string form(const Eng& e, int which, bool samp = false) {
  const DecodeSettings& s = e.s;
  const DecodeMat m = decode_mat(s, which, &e.q[which], nullptr);
  const int B = s.max_batch, Bg = s.row_groups(B) ? kMaxGemvRows : B;
  FormCall c{Bg, MS_GEMV_EPI_STORE_F32};
  if (which == QS_GU) {
    c.epi = MS_GEMV_EPI_SWIGLU;
  } else if (which == QS_LM) {
    const int tiles = s.resid_fused(&e.q[QS_DOWN]) ? s.H / s.resid_rt : 1;  // the last down's statistics
    c = FormCall{B, samp ? MS_GEMV_EPI_STORE_F32 : MS_GEMV_EPI_ARGMAX, samp ? tiles : 0};
    c.lm_gate = true;
    c.dgemm_gate = !samp;
  } else if (which != QS_QKV && s.resid_fused(m.q)) {
    c.epi = MS_GEMV_EPI_RESID_SSQ;
    c.presupported = true;
    return name(pick_form(s, m, c), true);
  } else {
    c.slabs = true;
  }
  return name(pick_form(s, m, c));
}

static int fails = 0;
// expected: QKV, O, gate/up, down, lm_head greedy, lm_head sampling ("-": not pinned)
static void expect(const char* what, const Eng& e, const char* const (&want)[6]) {
  const std::string got[6] = {form(e, QS_QKV), form(e, QS_O),  form(e, QS_GU),
                              form(e, QS_DOWN), form(e, QS_LM), form(e, QS_LM, true)};
  std::printf("%-34s", what);
  for (int i = 0; i < 6; ++i) {
    const bool ok = !std::strcmp(want[i], "-") || got[i] == want[i];
    std::printf(" %s%s", got[i].c_str(), ok ? "" : (std::string("(!= ") + want[i] + ")").c_str());
    fails += !ok;
  }
  std::printf("\n");
}

// the partials of one launch: (row, q head, split) x 132 floats (k_attn.hip)
static size_t partial_bytes(int B, int Hq, int nsplit) { return (size_t)B * Hq * nsplit * 132 * sizeof(float); }

static void env_or_unset(const char* name, int v) {
  if (v > 0) setenv(name, std::to_string(v).c_str(), 1);
  else unsetenv(name);
}

// Every launch of decode attention an engine can make, against the engine's allocation.  ms_create
// sizes one workspace, max(v1, v2) bytes at attn_ws_ctx(max_ctx), and the persistent step's
// partial stride nsplit_ws; decode_run launches a grid of decode_grid_len(max_len, k) keys, where
// max_len = the longest sequence + its new token (2 .. max_ctx) and k <= min(64, decode_run_cap)
// steps that stay inside max_ctx.  ppb / ppw: the engine's own choice and every pinned value.
static void sweep_workspaces() {
  const int Hq = 24, Hk = 8;
  long checked = 0, bad = 0;
  for (int ppw_env = 0; ppw_env <= 16; ++ppw_env) {
    env_or_unset("MS_ATTN_PPW", ppw_env);
    for (int ppb_env : {0, 4, 5, 6, 7, 8, 9}) {
      env_or_unset("MS_ATTN_PPB", ppb_env);
      for (int mb : {1, 6, 8, 16, 24, 128, 256})
        for (int ctx : {64, 100, 1000, 1600, 2304, 4100}) {
          const int ppw = attn_decode_ppw(mb, Hk, ctx), ppb = attn_decode2_ppb(mb, Hk, ctx);
          const int ws_ctx = attn_ws_ctx(ctx), nsplit_ws = attn2_nsplit(ws_ctx, ppb);
          const size_t ws = std::max(attn_decode_workspace_bytes(mb, Hq, ws_ctx),
                                     attn_decode2_workspace_bytes(mb, Hq, ws_ctx, ppb));
          bool ok = (ppw_env == 0 || ppw == ppw_env) && (ppb_env == 0 || ppb == ppb_env) &&
                    partial_bytes(mb, Hq, nsplit_ws) <= ws;  // the persistent step's stride
          for (int len = 2; len <= ctx; ++len) {
            const int kmax = std::min({64, decode_run_cap(len), ctx - len + 1});
            for (int k = 1; k <= kmax; ++k, ++checked) {
              const int grid = decode_grid_len(len, k);
              const int n2 = attn2_nsplit(grid, ppb), n1 = attn_decode_nsplit(ppw, grid);
              ok = ok && grid >= len + k - 1 && n2 <= nsplit_ws && partial_bytes(mb, Hq, n2) <= ws &&
                   partial_bytes(mb, Hq, n1) <= ws;
            }
          }
          if (!ok) {
            ++bad;
            std::printf("workspace too small: max_batch %d max_ctx %d ppb %d ppw %d\n", mb, ctx, ppb, ppw);
          }
        }
    }
  }
  unsetenv("MS_ATTN_PPW");
  unsetenv("MS_ATTN_PPB");
  // the sweep can fail: sized for max_ctx itself (as before the rounding fix), a 1600-key engine at
  // 9 pages per block has 3 splits' room and launches 4 (the grid is 1792 keys)
  const bool teeth = attn2_nsplit(decode_grid_len(1591, 1), 9) > attn2_nsplit(1600, 9);
  fails += (int)bad + !teeth;
  std::printf("workspace sweep: %ld launches checked, %ld engine shapes too small%s\n", checked, bad,
              teeth ? "" : ", and the un-rounded sizing passes (it must not)");
}

int main() {
  std::printf("%-34s QKV O gate/up down lm_head(greedy) lm_head(sampling)\n", "engine");
  // fp16: GEMV with the residual epilogue up to 16 slots, split-K + residual_rmsnorm above; the
  // skinny GEMM from 24 slots, the 128x128 lm_head tile from 96, the fp16-rows form from 192
  for (int b : {8, 16}) expect(("fp16 " + std::to_string(b)).c_str(), make(b, F16),
                               {"GEMV/6", "GEMV+resid", "GEMV", "GEMV+resid", "GEMV", "GEMV"});
  expect("fp16 20", make(20, F16), {"GEMV/6", "GEMV/6", "GEMV", "GEMV/4", "GEMV", "GEMV"});
  expect("fp16 64", make(64, F16), {"DGEMM/6", "DGEMM/4", "DGEMM", "DGEMM/8", "DGEMM", "DGEMM"});
  expect("fp16 128", make(128, F16), {"DGEMM/6", "DGEMM/4", "DGEMM", "DGEMM/8", "GEMM128", "GEMM128"});
  expect("fp16 256", make(256, F16), {"F16ROWS/3", "F16ROWS/4", "F16ROWS", "F16ROWS/4", "GEMM128", "GEMM128"});
  // Q4_K_M: the Q-GEMV up to 64 slots (qsplit 4 replaces the fp16 splits), from 65 the K-quant
  // skinny GEMM for all-Q4_K matrices and the fp16 copies for Q6_K / mixed ones
  expect("Q4_K_M 8", make(8, Q4KM), {"QGEMV/4", "QGEMV+resid", "QGEMV", "QGEMV+resid", "QGEMV", "QGEMV"});
  for (int b : {20, 64}) expect(("Q4_K_M " + std::to_string(b)).c_str(), make(b, Q4KM),
                                {"QGEMV/4", "QGEMV/4", "QGEMV", "QGEMV/4", "QGEMV", "QGEMV"});
  expect("Q4_K_M 128", make(128, Q4KM), {"QDGEMM/6", "QDGEMM/4", "QDGEMM", "QDGEMM/8", "GEMM128", "GEMM128"});
  expect("Q4_K_M 128, Q6_K V / down", make(128, Q4KM_Q6),
         {"DGEMM/6", "QDGEMM/4", "QDGEMM", "DGEMM/8", "GEMM128", "GEMM128"});
  // 192 slots and more take the 3 / 4 / 4 splits with any weights (no test ran this before)
  expect("Q4_K_M 256", make(256, Q4KM), {"QDGEMM/3", "QDGEMM/4", "QDGEMM", "QDGEMM/4", "GEMM128", "GEMM128"});
  expect("Q4_K_M 256, Q6_K V / down", make(256, Q4KM_Q6),
         {"DGEMM/3", "QDGEMM/4", "QDGEMM", "DGEMM/4", "GEMM128", "GEMM128"});
  expect("Q5_K_M 128", make(128, Q5KM), {"QDGEMM/6", "QDGEMM/4", "QDGEMM", "QDGEMM/8", "-", "-"});
  Eng e = make(128, Q5KM);
  e.s.qdgemm_mode = 3;  // MS_QDGEMM=3: the all-Q5_K matrices on their fp16 copies
  expect("Q5_K_M 128, MS_QDGEMM=3", e, {"DGEMM/6", "DGEMM/4", "DGEMM", "DGEMM/8", "-", "-"});
  expect("Q8_0 8", make(8, Q8), {"QGEMV/4", "QGEMV+resid", "QGEMV", "QGEMV+resid", "QGEMV", "QGEMV"});
  expect("Q8_0 128", make(128, Q8), {"DGEMM/6", "DGEMM/4", "DGEMM", "DGEMM/8", "GEMM128", "GEMM128"});
  // qlarge_min above the slots: row groups of 64 on the Q-GEMV with split-K O / down
  e = make(128, Q4KM);
  e.s.qlarge_min = 129;
  fails += !(e.s.row_groups(128) && !e.s.large());
  expect("Q4_K_M 128, MS_QLARGE_MIN=129", e, {"QGEMV/4", "QGEMV/4", "QGEMV", "QGEMV/4", "QGEMV", "QGEMV"});
  sweep_workspaces();
  std::printf("%s: %d mismatch(es)\n", fails ? "DECODE_FORMS_FAIL" : "DECODE_FORMS_OK", fails);
  return fails ? 1 : 0;
}
