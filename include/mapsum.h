/*
 * mapsum.h -- C-ABI of libmapsum.so, the MI355X-native map-phase engine.
 *
 * What this replaces.  The reference has no native boundary: its
 * map call is one HTTP request per chunk,
 *     OllamaLLM._call(prompt) -> requests.post(f"{url}/api/generate",
 *         json={"model", "prompt", "stream": False, "options": {"num_predict": N}})
 *         -> resp.json()["response"]
 * (run_full_evaluation_pipeline.py:80-106; runner copies
 *  runners/run_summarization_ollama_mapreduce.py:37-49,
 *  runners/run_summarization_ollama_mapreduce_critique.py:63-79,
 *  runners/run_summarization_ollama_mapreduce_hierarchical.py:56-68).
 * Everything behind that request (template -> tokenize -> prefill -> decode ->
 * detokenize) happens inside Ollama.  libmapsum takes over the
 * prefill/decode part on ids: the Python host (mapsum/compat.py OllamaLLM) keeps
 * the prompt-in/summary-out contract and calls
 *     ms_submit (one per chunk)  ~ the body of one /api/generate request
 *     ms_step                    ~ one scheduler iteration (admit+prefill, decode)
 *     ms_poll                    ~ resp.json()["response"] (as ids)
 * Errors: every entry point returns an int status (0 = OK, < 0 errno-like) and
 * never throws across the ABI; ms_last_error() gives the text.  The Python
 * wrapper raises RuntimeError, mirroring resp.raise_for_status()
 * (run_full_evaluation_pipeline.py:91).
 * Ownership: input ids are copied at submit; result id buffers are owned by the
 * engine and stay valid until the next ms_poll / ms_destroy.  One engine per GPU
 * per process; an engine is not thread-safe.
 */
#ifndef MAPSUM_H
#define MAPSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS_ABI_VERSION 3  /* 3: the 16-bit type is IEEE fp16 (weights, KV cache, activations) */

/* status codes */
#define MS_OK 0
#define MS_EIO -5       /* device / runtime failure                  */
#define MS_ENOMEM -12   /* device allocation failed                  */
#define MS_EBUSY -16    /* operation not allowed while work pending  */
#define MS_EINVAL -22   /* bad argument                              */
#define MS_ENOSPC -28   /* request can never fit (ctx / KV pages)    */

/* finish reasons (ms_result.finish_reason) -- Ollama's done_reason "stop"/"length" */
#define MS_FINISH_EOS 1
#define MS_FINISH_LENGTH 2
#define MS_FINISH_ERROR 3 /* this chunk only: no finite logit (NaN/Inf in its activations);
                             the other chunks of the batch are unaffected.  The reference has
                             no retry (run_full_evaluation_pipeline.py:627-638 marks the whole
                             model failed); the Python host re-queues such a chunk once. */

/* ms_submit flags */
#define MS_FLAG_IGNORE_EOS 1u /* bench mode: always generate num_predict tokens */

/* logical weight tensors for ms_load_weight ([rows][cols] row-major fp16, HF
 * nn.Linear layout [out][in]); the engine fuses Q|K|V and interleaves gate/up
 * on upload. */
enum ms_tensor {
  MS_T_EMBED = 0,      /* [vocab][hidden]          */
  MS_T_ATTN_NORM = 1,  /* [hidden]                 */
  MS_T_WQ = 2,         /* [n_heads*head_dim][hidden] */
  MS_T_WK = 3,         /* [n_kv*head_dim][hidden]  */
  MS_T_WV = 4,         /* [n_kv*head_dim][hidden]  */
  MS_T_WO = 5,         /* [hidden][n_heads*head_dim] */
  MS_T_FFN_NORM = 6,   /* [hidden]                 */
  MS_T_WGATE = 7,      /* [ffn][hidden]            */
  MS_T_WUP = 8,        /* [ffn][hidden]            */
  MS_T_WDOWN = 9,      /* [hidden][ffn]            */
  MS_T_FINAL_NORM = 10,/* [hidden]                 */
  MS_T_LM_HEAD = 11,   /* [vocab][hidden]; only when tie_embeddings == 0 */
  MS_T_Q_NORM = 12,    /* [head_dim]; QK-norm engines only (ms_enable_qk_norm) */
  MS_T_K_NORM = 13     /* [head_dim]; QK-norm engines only */
};

typedef struct ms_config {
  int32_t abi_version;          /* = MS_ABI_VERSION */
  /* model (Llama-3.2 family; head_dim must be 128) */
  int32_t n_layers, hidden, n_heads, n_kv_heads, head_dim, ffn, vocab;
  float rope_theta, rope_factor, rope_low_freq_factor, rope_high_freq_factor;
  int32_t rope_orig_ctx;
  float norm_eps;
  int32_t tie_embeddings;
  /* engine */
  int32_t device;               /* HIP device ordinal                         */
  int32_t max_batch;            /* sequences in flight (<= 1024).  Also fixes the
                                   engine's decode arithmetic, ranked in ONE place,
                                   pick_form of csrc/decode_forms.h (the table:
                                   DESIGN.md section 5, pinned on the CPU by
                                   tests/native/decode_forms.cpp).  fp16 weights:
                                   1-16 residual-fused GEMV, 17-23 split GEMV +
                                   residual_rmsnorm, 24-95 skinny GEMM, 96-191
                                   + the lm_head on the 128x128 GEMM tile,
                                   >= 192 the skinny GEMM's fp16-rows form with
                                   QKV / down split 3 / 4;
                                   K-quant: 1-16 residual-fused Q-GEMV, 17-64
                                   split-4 Q-GEMV + residual_rmsnorm, >= 65 the
                                   K-quant skinny GEMM (all-Q4_K and all-Q5_K
                                   matrices; Q6_K and mixed ones their fp16
                                   copies on the skinny GEMM), lm_head tile from
                                   96, the 3 / 4 splits from 192;
                                   Q8_0: as K-quant up to 64 (the exact d*q
                                   weights), >= 65 every matrix's fp16 copy on
                                   the skinny GEMM, lm_head tile from 96.
                                   Results are batch-invariant inside one engine,
                                   not across these boundaries                   */
  int32_t max_ctx;              /* prompt + generated tokens per sequence     */
  int32_t max_prefill_tokens;   /* packed prompt tokens per prefill pass      */
  int32_t n_pages;              /* KV pages of 64 tokens; 0 = enough for all  */
  int32_t n_eos;                /* end-of-turn ids (<|eot_id|> etc.)          */
  int32_t eos_ids[8];
} ms_config;

typedef struct ms_result {
  uint64_t tag;          /* the caller's tag from ms_submit                    */
  const int32_t* ids;    /* generated ids (EOS excluded); engine-owned          */
  int32_t n_ids;
  int32_t finish_reason; /* MS_FINISH_*                                         */
  int32_t n_prompt;
  int32_t _pad;
} ms_result;

typedef struct ms_stats {
  int64_t prefill_tokens;     /* prompt tokens processed                       */
  int64_t decode_tokens;      /* tokens produced by decode steps               */
  int64_t prefill_passes, decode_steps;
  int64_t finished;
  double prefill_ms, decode_ms; /* device time (events) when profiling is on   */
  double kernel_ms[8];          /* per kernel class, when profiling is on:
                                   0 gemm(prefill) 1 attn_prefill 2 gemv(decode)
                                   3 attn_decode 4 lm_head 5 norm/rope/misc
                                   6 persist (the decode step's layers as one
                                   persistent launch, <= 8-slot engines)        */
  int64_t kernel_launches[8];
  int64_t decode_kv_tokens;     /* sum over decode steps and rows of the keys attended
                                   (the KV-read term of SURVEY.md §8d's decode bytes)  */
  int64_t graphs_built;         /* decode hipGraphs captured + instantiated (the cache keeps
                                   at most 64, least recently used evicted)            */
  int64_t persist_fallbacks;    /* decode runs recomputed with the per-layer launches after a
                                   hand-off of the persistent step timed out (expected 0)  */
  int64_t persist_steps;        /* decode steps that ran the persistent launch             */
} ms_stats;

typedef struct ms_engine ms_engine;

/* ---- engine lifecycle ------------------------------------------------------ */
int ms_create(const ms_config* cfg, ms_engine** out);
int ms_destroy(ms_engine* e);
/* e == NULL returns the last error of a failed ms_create / op call */
const char* ms_last_error(const ms_engine* e);

/* QK-norm models (Qwen3): every layer normalises each Q head and each K head (RMSNorm over the
   head's 128 values, fp16 gains MS_T_Q_NORM / MS_T_K_NORM shared by the heads) between the QKV
   projection and RoPE, in prefill and decode alike.  Call after ms_create and before any weight
   load or request; afterwards it returns MS_EBUSY.  It allocates the gains (1.0 until loaded;
   ms_init_synthetic* leaves them there) and lists them in ms_weight_regions after every other
   region.  Such an engine never runs the persistent decode step (ms_set_persist returns 0). */
int ms_enable_qk_norm(ms_engine* e);

/* q8_0 KV cache (Ollama's OLLAMA_KV_CACHE_TYPE=q8_0): the engine's K/V pools hold ggml Q8_0 blocks -- per
   (token, kv head) row of 128 fp16 values, 4 blocks of 32 consecutive stored elements, each int8 codes
   c_i = roundf(t_i / d) with d = amax / 127 in fp32 and the scale stored as fp16 (quantize_row_q8_0_ref;
   a block with a non-finite value stores the scale NaN and codes 0) -- 60,928 instead of 114,688 bytes
   per Llama-3.2-3B token.  Pool per (layer, page, kv head): 8192 B of codes int8 [64 tokens][128], then
   512 B of scales fp16 [64 tokens][4] (8704 B; MS_DBG_KPOOL / MS_DBG_VPOOL return these bytes).
   Prefill attends over the fp16 K/V of its own pass, so prefill logits and first tokens are those of the
   fp16-cache engine bit for bit; decode writes the new token quantised and attends over the dequantised
   cache.  Call after ms_create and before any weight load or request; afterwards it
   returns MS_EBUSY.  Either order with ms_enable_qk_norm.  Such an engine decodes on the rows route in
   every regime and never runs the v2 attention, the slab prologue or the persistent decode step
   (ms_set_persist returns 0).  ms_config and the ABI version are unchanged. */
int ms_enable_kv_q8_0(ms_engine* e);

/* ---- weights ---------------------------------------------------------------- */
int ms_load_weight(ms_engine* e, int32_t tensor, int32_t layer, const uint16_t* host_f16,
                   int64_t n_elems);
/* device-side counter-based N(0,std)-like init; restated in oracle/synth.py */
int ms_init_synthetic(ms_engine* e, uint64_t seed, float std, float norm_jitter);

/* ggml quantised weights: the K-quants Q4_K / Q5_K / Q6_K (Q4_K_M files: BASELINE.json config 5;
 * the q5_K_M, q5_K_S and q4_K_S mixes) and Q8_0 (llama3.2:3b-instruct-q8_0).  `blocks` are the
 * tensor's rows as raw ggml blocks (Q4_K = 144 B, Q5_K = 176 B, Q6_K = 210 B per 256 weights;
 * Q8_0 = 34 B per 32 weights, so rows * (cols / 32) * 34 bytes).  The engine keeps f16(dequant) for prefill and the blocks for the dequant-fused
 * decode GEMV.  RMSNorm weights stay fp16 (ms_load_weight).  An engine's quantised matrices
 * are all Q8_0 or all K-quant: the other family is refused with MS_EINVAL. */
#define MS_GGML_Q8_0 8
#define MS_GGML_Q4_K 12
#define MS_GGML_Q5_K 13
#define MS_GGML_Q6_K 14
int ms_load_weight_q(ms_engine* e, int32_t tensor, int32_t layer, int32_t ggml_type,
                     const void* host_blocks, int64_t n_bytes);
/* random Q4_K/Q6_K blocks with the Q4_K_M per-tensor type mix (bench) */
int ms_init_synthetic_q(ms_engine* e, uint64_t seed, float scale, float norm_jitter);
/* random Q8_0 blocks for every matrix, dequantised weights of std ~ scale (bench) */
int ms_init_synthetic_q8_0(ms_engine* e, uint64_t seed, float scale, float norm_jitter);
/* random Q5_K/Q6_K blocks in the Q5_K_M mix: Q4_K_M's per-tensor types with Q5_K for Q4_K (bench) */
int ms_init_synthetic_q5_k_m(ms_engine* e, uint64_t seed, float scale, float norm_jitter);

/* ---- weight broadcast (one process per GPU: rank 0 loads, the others receive over RCCL) -- */
/* every device weight buffer in a fixed order (fp16 matrices and norms, then K-quant
   regions); returns the count, fills up to cap (ptr, bytes) pairs */
int ms_weight_regions(const ms_engine* e, void** ptrs, int64_t* bytes, int32_t cap);
/* the (tensor, layer, ggml_type) triples of the K-quant tensors loaded so far; returns the count */
int ms_quant_manifest(const ms_engine* e, int32_t* triples, int32_t cap);
/* lay out a K-quant tensor as ms_load_weight_q would, without its bytes (a broadcast fills
   the regions afterwards) */
int ms_declare_weight_q(ms_engine* e, int32_t tensor, int32_t layer, int32_t ggml_type);

/* ---- request path (replaces one /api/generate per chunk) -------------------- */
int ms_submit(ms_engine* e, const int32_t* ids, int32_t n, int32_t num_predict,
              uint32_t flags, uint64_t tag);
/* Sampled decoding (Ollama's `options`; DESIGN.md "Sampler").  Per generated token, on the row's
 * fp32 logits: repeat penalty over the distinct ids among the last repeat_last_n of prompt +
 * generated tokens (l > 0 ? l / rp : l * rp) -> the top_k largest (ties to the lowest id) ->
 * top_p (the shortest prefix of softmax at T = 1 reaching it; >= 1 off) -> min_p (l >= l_max +
 * ln(min_p); <= 0 off) -> softmax(l / temperature) -> the first candidate, in (logit desc, id asc)
 * order, whose cumulative probability exceeds
 *     u(seed, step) = (mix64(mix64(seed) + 0x9E3779B97F4A7C15 * (step + 1)) >> 40) * 2^-24,
 * step = the index of the generated token.  The ids depend on nothing else: not on the slot, the
 * other chunks of the batch or how ms_step chunks the decode runs.  The order is llama.cpp's
 * sampler chain; the random numbers are this engine's own, not Ollama's generator.
 * temperature <= 0: greedy, every other field ignored. */
#define MS_SAMPLE_MAX_TOPK 256
#define MS_SAMPLE_MAX_WINDOW 256
typedef struct ms_sampling {
  float temperature;      /* <= 0: greedy                                         */
  int32_t top_k;          /* 1 .. MS_SAMPLE_MAX_TOPK (<= 0, "whole vocabulary", is refused) */
  float top_p;            /* > 0                                                  */
  float min_p;            /* 0 <= min_p < 1                                       */
  float repeat_penalty;   /* > 0; 1 = off                                         */
  int32_t repeat_last_n;  /* 0 .. MS_SAMPLE_MAX_WINDOW; 0 = off                   */
  uint64_t seed;
} ms_sampling;
/* ms_submit with sampling; sp == NULL or sp->temperature <= 0 is exactly ms_submit.  A field out
   of range is MS_EINVAL with a message that names it. */
int ms_submit_sampled(ms_engine* e, const int32_t* ids, int32_t n, int32_t num_predict,
                      uint32_t flags, uint64_t tag, const ms_sampling* sp);
/* replace the config's end-of-turn ids by a larger stop set (0 <= ids < vocab; n = 0 restores
   cfg.eos_ids).  Ollama's `stop` option; bench.py --eos uses a synthetic set so that random-init
   weights finish chunks at natural, varied lengths (slot turnover). */
int ms_set_eos_ids(ms_engine* e, const int32_t* ids, int32_t n);
/* one scheduler iteration: admit + prefill, then a decode run of up to 64 chained
   steps (greedy, or sampled on the device when a chunk of the run samples) with one host synchronisation (fewer when a chunk reaches num_predict, the
   attention split grid changes, or admissible work waits for a slot); a chunk that meets
   EOS mid-run stops there.  Returns sequences still waiting or running (>= 0).
   MS_DECODE_RUN=1 in the environment restores one decode step per call. */
int ms_step(ms_engine* e);
/* copies up to cap finished results; returns the number copied */
int ms_poll(ms_engine* e, ms_result* out, int32_t cap);
int ms_pending(const ms_engine* e);
int ms_get_stats(const ms_engine* e, ms_stats* out);
int ms_reset_stats(ms_engine* e);
/* bit mask of kernel classes to bracket with HIP events (0 = off) */
int ms_set_profiling(ms_engine* e, uint32_t class_mask);
/* roctx ranges (rocprofv3 --marker-trace).  ms_step brackets itself ("mapsum.step") and its
   phases ("mapsum.prefill", "mapsum.decode_run"); these let the host mark its own phases
   (dist.gather_summaries: "mapsum.gather").  Nest; no-ops unless a profiler is attached. */
int ms_trace_push(const char* name);
int ms_trace_pop(void);
int ms_synchronize(ms_engine* e);
/* the decode step's layers as ONE persistent launch (k_persist.hip; engines of <= 8 slots on
   fp16 Llama-3.2-3B weights, bit-identical to the per-layer launches).  Opt-in: an engine starts
   with it off (0) unless MS_PERSIST=1 is set at ms_create; 1 turns it on (it measured slower than
   the launches).  Returns 1 when this engine supports it, 0 when it never runs it. */
int ms_set_persist(ms_engine* e, int32_t on);
/* test hook: copy `bytes` from byte `offset` of an engine buffer to host memory (after the
   engine's streams are idle) */
#define MS_DBG_KPOOL 0          /* K cache [layer][page][kv_head][64][head_dim] fp16; a q8_0-KV engine:
                                   [layer][page][kv_head] slabs of 8704 B (ms_enable_kv_q8_0) */
#define MS_DBG_VPOOL 1          /* V cache, same layout */
#define MS_DBG_DECODE_LOGITS 2  /* the decode lm_head output (argmax partials {max, id} per 16 columns;
                                   after a sampling run: the scaled fp32 logits [rows][vocab]) */
#define MS_DBG_DECODE_X 3       /* the decode residual [max_batch][hidden] fp32 */
#define MS_DBG_PREFILL_LOGITS 4 /* the scaled fp32 logits [prompts][vocab] behind the latest prefill's first tokens */
int ms_debug_read(ms_engine* e, int32_t which, int64_t offset, void* host, int64_t bytes);
/* diagnostic: the persistent step's in-kernel timeline of its latest launch, [256][28][16]
   s_memrealtime ticks (100 MHz), recorded only under MS_PK_STAMPS=1 (tools/pk_stamps.py) */
int ms_debug_pk_stamps(uint64_t* out, int32_t n);
/* diagnostic: decode attention v2's per-block phase stamps of its latest launch, [1024][32]
   (entry, XCC / HW id, prologue, per-wave S and P.V done, partial stored), recorded only under
   MS_A2_STAMPS=1 (tools/a2_stamps.py) */
int ms_debug_a2_stamps(uint64_t* out, int32_t n);
/* diagnostic: the fp16 decode GEMV's per-block phase stamps of its latest stamped launch,
   [1024][32] (k_gemv.hip lists the slots), recorded only under MS_GEMV_STAMPS=1
   (tools/gemv_stamps.py) */
int ms_debug_gemv_stamps(uint64_t* out, int32_t n);

/* ---- parity probe (tests): one prompt through the prefill path -------------- */
/* hidden_out: [n][hidden] fp32 residual after `n_layers_run` layers (or NULL);
   logits_out: [n][vocab] fp32 logits of every position (or NULL; needs
   n_layers_run == n_layers). */
int ms_forward(ms_engine* e, const int32_t* ids, int32_t n, int32_t n_layers_run,
               float* hidden_out, float* logits_out);
/* the same over n_seqs prompts packed into ONE varlen prefill pass (the ragged batches of
   the hierarchical runner, runners/run_summarization_ollama_mapreduce_hierarchical.py:242-274):
   ids = the prompts back to back, lens[i] = length of prompt i; hidden_out / logits_out rows
   follow the packed order ([sum lens][hidden], [sum lens][vocab]). */
int ms_forward_packed(ms_engine* e, const int32_t* ids, const int32_t* lens, int32_t n_seqs,
                      int32_t n_layers_run, float* hidden_out, float* logits_out);
/* teacher forcing through the DECODE path (parity tests): as ms_submit, but decode step j
   (j >= 1) is fed forced[j-1] instead of the engine's own previous choice, so the result ids
   are the engine's greedy choices after a context the caller fixes (e.g. the oracle's own
   greedy tokens).  n_forced >= num_predict - 1.  Such a sequence decodes one step per run. */
int ms_submit_forced(ms_engine* e, const int32_t* ids, int32_t n, const int32_t* forced,
                     int32_t n_forced, int32_t num_predict, uint32_t flags, uint64_t tag);

/* ---- op-level entry points (device pointers; stream = hipStream_t or NULL) -- */
#define MS_EPI_STORE_F16 0  /* out fp16 [M][ldo]                              */
#define MS_EPI_ADD_F32 1     /* out fp32 [M][ldo] += acc  (residual add)       */
#define MS_EPI_SWIGLU 2      /* W rows interleaved gate/up per 16; out fp16 [M][N/2] */
#define MS_EPI_STORE_F32 3   /* out fp32 [M][ldo]                              */
#define MS_EPI_ARGMAX 5      /* decode GEMV only: out {max, id} float2 [M][ldo = N/16], one per
                                16-column tile (ties -> lowest id; NaN never wins); finish the
                                rows with ms_op_argmax_partials                          */
/* prefill GEMM: out[M][N] (op) A[M][K] . W[N][K]^T ; K % 64 == 0.  MS_EPI_ARGMAX (the large
   decode regime's lm_head): {max, id} float2 partials [M][ldo >= N/16] per 16-column tile on the
   128x128 tile, no row scale, N % 16 == 0 */
int ms_op_gemm(const void* A, const void* W, void* out, int32_t M, int32_t N, int32_t K,
               int32_t ldo, int32_t epilogue, void* stream);
/* prefill O / down with the residual update fused (the engine's prefill layer): x fp32 [M][N] +=
   A . W^T, and the input of the next normalised projection: xg_out fp16 [M][N] = f16(x * gamma * 2^-4),
   ssq_out fp32 [tiles][M] = per-128-column sums of the new x^2 (tiles = ms_gemm_resid_tiles(M, N) = N / 128),
   the deferred RMSNorm statistics the next ms_op_gemm takes through ms_op_set_row_scale */
int ms_op_gemm_resid(const void* A, const void* W, float* x, void* xg_out, const void* gamma, float* ssq_out,
                     int32_t M, int32_t N, int32_t K, void* stream);
int ms_gemm_resid_tiles(int32_t M, int32_t N);
/* tuning/test hook: prefill GEMM tile (0 heuristic, 1 = 128x128, 2 = 256x256 8-phase,
   3 = 256x256 on 4 waves, 4 = 3 for the stored epilogues and 2 for the residual one; every
   variant gives the same bits) */
int ms_set_gemm_variant(int32_t variant);
/* tuning/test hook: issue order of the fp16 decode GEMVs that stage X by LDS DMA: 0 = the X
   requests ahead of the weight stream, 1 = the first weight step ahead of them, 2 = that with
   per-wave X slices (no X barrier), -1 = the library's per-shape choice (MS_GEMV_ORDER_DEFAULT,
   what it starts with).  Adding 3 loads the weights line-exact (each load instruction reads whole
   128-byte lines that no other instruction reads), adding 6 does so with non-temporal loads: 3..8
   are the three issue orders on those two load forms.  Every order gives the same bits.  An engine
   launches whatever is set when it captures its decode graphs. */
#define MS_GEMV_ORDER_DEFAULT (-1)
int ms_set_gemv_order(int32_t order);
/* tuning/test hook: the quantised GEMVs that have a grid-stride two-stage form (the Q6_K and the
   Q8_0 lm_head argmax, the Q4_K gate/up SwiGLU) all take it (1) or all run one-tile blocks (0);
   the two give bit-identical outputs.  The library starts with the two K-quant forms on and the
   Q8_0 one off (it measured slower); MS_QGEMV_GS is the mask (bit 0 Q6_K
   lm_head, 1 Q4_K gate/up, 2 Q8_0 lm_head) */
int ms_set_qgemv_gs(int32_t on);
/* tuning/test hook: decode attention's split combine on the XCD-matched grid (1, default) or the
   (B, Hq) grid (0), and the v2 prologue form (0 default, 3 a dedicated prologue wave); every
   setting gives the same bits.  Engines capture their decode graphs with the current setting. */
int ms_set_attn_tuning(int32_t combine_grp, int32_t order);
/* tuning/test hook: the large-batch decode skinny GEMM on 4-wave blocks (1) or on 8-wave
   blocks that split each 128-k step in two k halves (2, the default); the two sum in
   different orders, each independent of the batch rows.  Engines of <= 128 slots take the
   setting for their gate/up launch at creation (set it before ms_engine_create);
   ms_op_dgemm takes it where it applies (M <= 128, K % (128 S) == 0). */
int ms_set_dgemm_kh(int32_t kh);
/* tuning/test hook: ms_op_dgemm's weight rows per block, 64 (4 row groups, the default) or 128
   (8; 4-wave-group blocks only, M <= 128, N % 128 == 0, else 64) -- the same bits either way.
   Engines choose per projection (128 for QKV, down and the lm_head at <= 128 rows). */
int ms_set_dgemm_wn(int32_t wn);
/* decode skinny GEMM (M <= 64): same contract; workspace >= ms_op_gemv_workspace() bytes */
int64_t ms_op_gemv_workspace(int32_t M, int32_t N, int32_t K);
int ms_op_gemv(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K,
               int32_t ldo, int32_t epilogue, void* workspace, void* stream);
/* tuning hook: as ms_op_gemv with the K-splitting wave count forced (0 = heuristic) */
int ms_op_gemv_tuned(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K,
                     int32_t ldo, int32_t epilogue, void* workspace, int32_t waves, void* stream);
/* tuning hook: ms_op_gemv over X [M][ldk] and W [N][ldk] (row stride ldk >= K elements) */
int ms_op_gemv_strided(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K,
                       int32_t ldk, int32_t ldo, int32_t epilogue, void* stream);
/* decode O / down with the residual update fused (the engine's small-regime layer): x fp32
   [M][N] += X . W^T on rt-row tiles (tiles = ceil(N / rt) <= 256; the last may be ragged), and the input of the
   next normalised projection: xg_out fp16 [M][N] = f16(x * gamma * 2^-4), ssq_out fp32 [tiles][M] =
   per-tile sums of the new x^2 (its deferred RMSNorm statistics, see ms_op_set_row_scale) */
int ms_op_gemv_resid(const void* X, const void* W, float* x, void* xg_out, const void* gamma,
                     float* ssq_out, int32_t M, int32_t N, int32_t K, int32_t rt, void* stream);
/* the deferred RMSNorm of the numerics contract: the next ms_op_gemm /
   ms_op_gemv / ms_op_gemv_split / ms_op_dgemm / ms_op_qgemv / ms_op_qgemv_split calls of the
   calling thread scale output row r by 16/sqrt(sum_t ssq[t][r] / hidden + eps) -- 16 undoes the
   2^-4 the producers pre-scale their fp16 output by (ssq [tiles][M];
   gemm / dgemm: tiles == 1); ssq = NULL turns the scale off.  Test hook: the engine passes the
   scale with each launch. */
int ms_op_set_row_scale(const float* ssq, int32_t tiles, int32_t hidden, float eps);
/* large-batch decode GEMM (M <= 256 rows; 64 weight rows per block, X shared via LDS): the
   ms_op_gemv epilogues (plus MS_EPI_ARGMAX); S > 1: split-K fp32 slabs [S][M][N] with
   epilogue MS_EPI_STORE_F32; N % 64 == 0, K % (64 S) == 0 */
int ms_op_dgemm(const void* X, const void* W, void* out, int32_t M, int32_t N, int32_t K, int32_t S,
                int32_t ldo, int32_t epilogue, void* stream);
/* decode split-K: slabs fp32 [S][M][N], slab s = X[:, sK/S:(s+1)K/S] . W[:, same]^T;
   waves = 0 picks the heuristic (tuning hook otherwise) */
int ms_op_gemv_split(const void* X, const void* W, float* slabs, int32_t M, int32_t N, int32_t K,
                     int32_t S, int32_t waves, void* stream);
/* x fp32 [rows][hidden] += slab_0 + ... + slab_{S-1} (slab order); then the input of the
   normalised projection that follows: y fp16 = f16(x * w * 2^-4), ssq[r] = sum of x[r]^2 (one tile) */
int ms_op_residual_rmsnorm(float* x, const float* slabs, int32_t S, const void* w, void* y, float* ssq,
                           int32_t rows, int32_t hidden, void* stream);
/* quantised-weight ops (Q4_K, Q5_K, Q6_K, Q8_0): raw ggml blocks -> fp32 (bit-exact restatement of
   llama.cpp's dequantize_row_q4_K/q5_K/q6_K/q8_0; n_blocks counts 256-weight units, for Q8_0 8 ggml
   blocks = 272 B each); raw rows -> fp16 rows + packed rows (Q6_K repacked to 224 B, Q8_0 to
   272 B units: 8 scales, then the regrouped quants, Q5_K to header | Q4_K-order nibbles | qh);
   dequant-fused GEMV over packed rows (same epilogues as ms_op_gemv) */
int ms_op_dequant(int32_t ggml_type, const void* blocks, int64_t n_blocks, float* out, void* stream);
int ms_op_quant_rows(int32_t ggml_type, const void* blocks, int32_t rows, int32_t K, void* f16_out,
                     void* packed_out, void* stream);
int ms_op_qgemv(const void* X, int32_t ggml_type, const void* packed_rows, void* out, int32_t M,
                int32_t N, int32_t K, int32_t ldo, int32_t epilogue, void* stream);
/* dequant-fused split-K: slabs fp32 [S][M][N] over S equal, super-block aligned K ranges
   (the quantised counterpart of ms_op_gemv_split; K % (256*S) == 0) */
int ms_op_qgemv_split(const void* X, int32_t ggml_type, const void* packed_rows, float* slabs,
                      int32_t M, int32_t N, int32_t K, int32_t S, void* stream);
/* ms_op_gemv_resid over packed quantised rows (the residual-fused O / down of quantised engines of
   <= 16 slots): same outputs, M <= 16 */
int ms_op_qgemv_resid(const void* X, int32_t ggml_type, const void* packed_rows, float* x, void* xg_out,
                      const void* gamma, float* ssq_out, int32_t M, int32_t N, int32_t K, int32_t rt,
                      void* stream);
/* large-batch K-quant decode GEMM (M <= 256 rows): ms_op_dgemm over the packed rows, each weight
   dequantised in registers to its fp16-copy value f16(ggml dequant); epilogues MS_EPI_STORE_F32
   (S > 1: split-K slabs [S][M][N]), MS_EPI_SWIGLU, MS_EPI_ARGMAX; N % 64 == 0, K % (256 S) == 0
   with K / (256 S) even or a multiple of 3 (the engine's K-quant decode projections in engines
   of >= 65 slots).  Q4_K, Q5_K, Q6_K or F16 (1) rows: Q8_0 has no form here (MS_EINVAL) */
int ms_op_qdgemm(const void* X, int32_t ggml_type, const void* packed_rows, void* out, int32_t M,
                 int32_t N, int32_t K, int32_t S, int32_t ldo, int32_t epilogue, void* stream);
/* the input of a normalised projection: y fp16 [rows][hidden] = f16(x * w * 2^-4) and ssq[r] = sum
   of x[r]^2 over x fp32 [.][hidden] rows (row_idx optional gather); the projection then scales
   its output rows by 16/sqrt(ssq / hidden + eps) (ms_op_set_row_scale).  The 2^-4 pre-scale
   (exact) keeps un-normalised residual rows up to ~1e6 inside fp16 (kernels.h kXgScale). */
int ms_op_rmsnorm(const void* x, const void* w, void* y, float* ssq, int32_t rows, int32_t hidden,
                  const int32_t* row_idx, void* stream);
/* The QK-norm kernel (k_qknorm.hip) on device operands.  qkv: fp16 [T][(n_heads + 2 n_kv_heads) * 128]
   rows with rope-permuted Q / K heads.  slabs == NULL: the rows form, reading qkv.  Else the slabs
   form: S (1..8) fp32 split-K slabs [S][T][row] folded in slab order, scaled by the row scale set
   with ms_op_set_row_scale (statistics [tiles][T], tiles <= 256; none set: no scale) and rounded to
   fp16, which also writes the K / V parts of the qkv rows.  Per Q / K head: RMSNorm with the fp16
   gains q_gain / k_gain [128] (logical dim order), RoPE with the caller's cos / sin tables
   [positions][64] at tok_pos[t], one rounding.  Q is written rotated, natural dim order, into its
   qkv row; K and V go to page block_table[tok_slot[t]][tok_pos[t] / 64], offset tok_pos[t] % 64 of
   the pools [page][n_kv_heads][64][128].  The caller keeps every position inside its tables. */
int ms_op_qk_norm_rope(void* qkv, const float* slabs, int32_t S, int32_t T, int32_t n_heads, int32_t n_kv_heads,
                       const int32_t* tok_pos, const int32_t* tok_slot, const float* cos_tab, const float* sin_tab,
                       const void* q_gain, const void* k_gain, float eps, void* k_pool, void* v_pool,
                       const int32_t* block_table, int32_t max_pages, void* stream);
/* The q8_0 KV cache's writer on device operands: fp16 K and V rows [T][n_kv_heads][128], exactly as the
   fp16 pools would hold them (K after RoPE's rounding), quantised by the engine's own device function into
   the caller's pools [page][n_kv_heads] x 8704 B (ms_enable_kv_q8_0's layout) at page
   block_table[tok_slot[t]][tok_pos[t] / 64], offset tok_pos[t] % 64.  Pools 16-B aligned. */
int ms_op_kv_store_q8_0(const void* k_rows, const void* v_rows, int32_t T, int32_t n_kv_heads, const int32_t* tok_pos,
                        const int32_t* tok_slot, void* k_pool, void* v_pool, const int32_t* block_table,
                        int32_t max_pages, void* stream);
/* Decode attention over q8_0 pools (the engine's rows route): qkv fp16 [B][(n_heads + 2 n_kv_heads) * 128]
   rows whose Q heads are rotated, natural dim order; seq_len[b] keys (the newest included, already in the
   pools) of block-table row seq_slot[b] (slot_major != 0: page p of slot s is page s * max_pages + p, no
   table lookup); max_len >= every seq_len sets the split grid with ppw pages per wave (1..16); workspace of
   ms_op_attn_decode_q8_0_workspace bytes; out fp16 [B][n_heads * 128].  Runs the attention launch and
   the split combine.  Scores sum d_K * (q . c) per block in fp32, softmax in fp32, P.V with
   f16(p * d_V) against the integer codes. */
int64_t ms_op_attn_decode_q8_0_workspace(int32_t B, int32_t n_heads, int32_t max_len, int32_t ppw);
int ms_op_attn_decode_q8_0(const void* qkv, int32_t n_heads, int32_t n_kv_heads, const void* k_pool, const void* v_pool,
                           const int32_t* block_table, int32_t max_pages, int32_t slot_major, const int32_t* seq_len,
                           const int32_t* seq_slot, int32_t B, int32_t max_len, int32_t ppw, float* workspace,
                           void* out, void* stream);
/* ids[r] = argmax_j logits[r][j] (ties -> lowest j; -1 when no logit of the row is finite) */
int ms_op_argmax(const void* logits, int32_t rows, int32_t n, int32_t* ids, void* stream);
/* ids[r] = the lowest id of the largest {max, id} partial of row r (MS_EPI_ARGMAX output) */
int ms_op_argmax_partials(const void* partials, int32_t rows, int32_t tiles, int32_t* ids, void* stream);
/* the row sampler (ms_sampling above) over device logits [rows][ldl] fp32, n <= 131072 columns:
   params [rows]; win [rows][MS_SAMPLE_MAX_WINDOW] with win_len[r] <= 256 ids of row r's history,
   oldest first (the penalty window is the last repeat_last_n of them); steps [rows]; ids [rows]
   (-1: the row's largest non-NaN logit is not finite).  Optional, all three or none: the final
   candidates cand_ids / cand_p [rows][MS_SAMPLE_MAX_TOPK] in (logit desc, id asc) order with
   their probabilities, and their counts cand_n [rows].  Every pointer is a device pointer. */
int ms_op_sample(const float* logits, int32_t rows, int32_t n, int64_t ldl, const ms_sampling* params,
                 const int32_t* win, const int32_t* win_len, const int32_t* steps, int32_t* ids,
                 int32_t* cand_ids, float* cand_p, int32_t* cand_n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAPSUM_H */
