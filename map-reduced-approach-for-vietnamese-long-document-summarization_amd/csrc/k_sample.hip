// k_sample.hip -- sampled decoding on the device: repeat penalty -> top-k -> top-p -> min-p ->
// temperature -> one counter-based draw, per row of stored fp32 logits (DESIGN.md "Sampler").
//
// Reference semantics (EXT, inside Ollama for one /api/generate): llama.cpp's sampler chain in
// its published order with Ollama's defaults (temperature 0.8, top_k 40, top_p 0.9, min_p 0,
// repeat_penalty 1.1 over the last 64 tokens).  The order is restated here and in
// tests/sampling_ref.py; the random numbers are this project's own (mix64 below), so the ids are
// not Ollama's generator's.
//
// One 1024-thread block per row (decode_tail_kernel's geometry).  The row (513 KB at the real
// vocabulary) does not fit LDS and is RE-READ from L2 by every pass (4-byte loads, striped by
// thread, so n needs no alignment; sixteen loads in flight per thread):
//   0  the penalty window as a bitmap over the vocabulary in LDS (a duplicated id sets one bit:
//      penalised once); each load applies the penalty, so no pass ever stores a logit
//   1  per-thread maxima -> the row's argmax (greedy rows and top_k = 1 stop here) and, sorted,
//      a lower bound t0 of the k-th largest value: the k-th largest of the 1024 thread maxima
//   2  every value >= t0 (with its id) into LDS: k to 2k of them on an ordinary row; when at
//      most 1024, an LDS bitonic sort by (value desc, id asc) finishes the selection, boundary
//      ties included -- two reads of the row in all
//   3  otherwise (a row full of ties, or large values all in one thread's stripe): an exact
//      radix select (4 x 8 bits on the order-preserving integer image of the float, LDS
//      histogram of the values >= t0), compaction of the survivors, ties at the boundary taken
//      in id order (lowest first) by a blocked ballot scan, and the sort of the <= 256
//   4  top-p / min-p / temperature / the draw on the <= 256 sorted candidates (threads 0-255)
#include "gemv_common.h"

namespace ms {

namespace {

struct SampleShared {
  uint32_t bitmap[kSampleMaxN / 32];          // penalty window over the vocabulary
  unsigned long long sortbuf[1024];           // thread maxima, then the candidates
  unsigned hist[256];
  unsigned long long red64[16];
  unsigned redu[16];
  float redf[16];
  unsigned wave_cnt[4][16];
  unsigned sel_digit, sel_kk, sel_cnt, ccount;
  int result;
};

__device__ __forceinline__ uint32_t fkey(float v) {  // larger float <-> larger key; never 0
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ float sample_u(uint64_t seed, uint32_t step) {
  const uint64_t h = mix64(mix64(seed) + 0x9E3779B97F4A7C15ull * ((uint64_t)step + 1));
  return (float)(uint32_t)(h >> 40) * 5.9604644775390625e-08f;  // 24 bits * 2^-24: exact
}

// the penalised logit l of column c as its integer image; 0 = NaN (never a candidate)
__device__ __forceinline__ uint32_t key_of(float l, int c, bool pen, float rp, const uint32_t* bitmap) {
  if (pen && ((bitmap[c >> 5] >> (c & 31)) & 1u)) l = l > 0.f ? __fdiv_rn(l, rp) : __fmul_rn(l, rp);
  if (l != l) return 0u;
  if (l == 0.f) l = 0.f;  // -0 ties with +0
  return fkey(l);
}
__device__ __forceinline__ uint32_t load_key(const float* __restrict__ row, int c, bool pen, float rp,
                                             const uint32_t* bitmap) {
  return key_of(row[c], c, pen, rp, bitmap);
}

// f(c, key) for every column c = tid, tid + 1024, ... of the row, in ascending c per thread.
// A pass is latency-bound (one block per row, every load an L2 round trip), so kRowBatch loads
// are issued before the first is used (clamped, never predicated).
constexpr int kRowBatch = 16;
template <class F>
__device__ __forceinline__ void for_each_key(const float* __restrict__ row, int n, bool pen, float rp,
                                             const uint32_t* bitmap, F&& f) {
  const int tid = threadIdx.x;
#pragma unroll 1
  for (int base = 0; base < n; base += kRowBatch * 1024) {
    float v[kRowBatch];
#pragma unroll
    for (int i = 0; i < kRowBatch; ++i) v[i] = row[min(base + i * 1024 + tid, n - 1)];
#pragma unroll
    for (int i = 0; i < kRowBatch; ++i) {
      const int c = base + i * 1024 + tid;
      if (c < n) f(c, key_of(v[i], c, pen, rp, bitmap));
    }
  }
}

// descending bitonic sort of buf[0, N) (N a power of two <= 1024) by the whole block
__device__ __forceinline__ void bitonic_desc(unsigned long long* buf, int N) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= N; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (tid < N) {
        const int o = tid ^ j;
        if (o > tid) {
          const unsigned long long a = buf[tid], b = buf[o];
          const bool desc = (tid & k) == 0;
          if (desc ? a < b : a > b) { buf[tid] = b; buf[o] = a; }
        }
      }
      __syncthreads();
    }
}

// sum over the block (every thread calls; the result is uniform)
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // red free again
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int w = 0; w < 16; ++w) t += red[w];
  return t;
}
__device__ __forceinline__ unsigned block_sum_u(unsigned v, unsigned* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned t = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) t += red[w];
  return t;
}
// inclusive prefix sum in thread order (every thread calls)
__device__ __forceinline__ float block_scan(float v, float* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  __syncthreads();
  if (lane == 63) red[w] = v;
  __syncthreads();
  float base = 0.f;
  for (int i = 0; i < w; ++i) base += red[i];
  return base + v;
}

// The id of one row (uniform over the block); every thread of the 1024-thread block calls.
// ring / wcount: the last min(repeat_last_n, wcount, 256) ids, newest at ring[(wcount - 1) & 255].
__device__ __forceinline__ int sample_row(const float* __restrict__ row, int n, const SampleParams p, const int32_t* ring,
                          int wcount, uint32_t step, SampleShared& sh, int32_t* cand_ids, float* cand_p,
                          int32_t* cand_n) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool greedy = !(p.temperature > 0.f);
  int k = greedy ? 1 : min(min(p.top_k, n), kSampleMaxTopK);
  if (k < 1) k = 1;
  int w = greedy ? 0 : min(min(p.repeat_last_n, wcount), kSampleMaxWindow);
  const float rp = p.repeat_penalty;
  const bool pen = w > 0 && rp != 1.0f;
  __syncthreads();  // the shared state of a previous call is no longer read
  if (pen) {
    for (int i = tid; i < (n + 31) / 32; i += 1024) sh.bitmap[i] = 0u;
    __syncthreads();
    if (tid < w) {
      const int id = ring[(wcount - 1 - tid) & (kSampleMaxWindow - 1)];
      if (id >= 0 && id < n) atomicOr(&sh.bitmap[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
  }
  // ---- pass 1: thread maxima (ascending c: the first maximum is the lowest id), valid count
  uint32_t bk = 0u;
  int bi = 0;
  unsigned nv = 0;
  for_each_key(row, n, pen, rp, sh.bitmap, [&](int c, uint32_t key) {
    nv += key != 0u;
    if (key > bk) { bk = key; bi = c; }
  });
  sh.sortbuf[tid] = (unsigned long long)bk;
  unsigned long long best = ((unsigned long long)bk << 32) | (0xFFFFFFFFu - (uint32_t)bi);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(best, o, 64);
    best = t > best ? t : best;
  }
  if (lane == 0) sh.red64[wave] = best;
  const unsigned n_valid = block_sum_u(nv, sh.redu);  // (its barriers also publish red64 / sortbuf)
  for (int i = 0; i < 16; ++i) best = sh.red64[i] > best ? sh.red64[i] : best;
  const uint32_t maxkey = (uint32_t)(best >> 32);
  const int argmax = (int)(0xFFFFFFFFu - (uint32_t)best);
  // the largest non-NaN logit must be finite, as in the greedy tail
  if (maxkey == 0u || !__builtin_isfinite(fkey_inv(maxkey))) {
    if (tid == 0 && cand_n) *cand_n = 0;
    return -1;
  }
  if (k == 1) {
    if (tid == 0 && cand_n) { *cand_n = 1; cand_ids[0] = argmax; cand_p[0] = 1.0f; }
    return argmax;
  }
  const unsigned ktot = min((unsigned)k, n_valid);
  // ---- t0: the ktot-th largest thread maximum, a lower bound of the ktot-th largest value
  bitonic_desc(sh.sortbuf, 1024);
  const uint32_t t0 = (uint32_t)sh.sortbuf[ktot - 1];
  // ---- pass 2: every key >= t0 (at least ktot of them) into LDS.  When they fit -- k to 2k of
  // them on an ordinary row -- one sort by (value desc, id asc) finishes the selection, boundary
  // ties included, and the row is read only twice.
  __syncthreads();  // every thread has read t0
  sh.sortbuf[tid] = 0ull;
  if (tid == 0) sh.ccount = 0u;
  __syncthreads();
  for_each_key(row, n, pen, rp, sh.bitmap, [&](int c, uint32_t key) {
    if (key != 0u && key >= t0) {
      const unsigned pos = atomicAdd(&sh.ccount, 1u);
      if (pos < 1024u) sh.sortbuf[pos] = ((unsigned long long)key << 32) | (0xFFFFFFFFu - (uint32_t)c);
    }
  });
  __syncthreads();
  const unsigned n_ge = sh.ccount;
  if (n_ge <= 1024u) {  // block-uniform
    int N = 256;
    while ((unsigned)N < n_ge) N <<= 1;
    bitonic_desc(sh.sortbuf, N);
  } else {
  // ---- otherwise (a row full of ties, or its large values all in one thread's stripe): an exact
  // radix select of the ktot-th largest key among the keys >= t0, re-reading the row
  uint32_t prefix = 0u;
  unsigned kk = ktot, eq = 0;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    __syncthreads();
    if (tid < 256) sh.hist[tid] = 0u;
    __syncthreads();
    for_each_key(row, n, pen, rp, sh.bitmap, [&](int, uint32_t key) {
      const bool in = shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8));
      if (key != 0u && key >= t0 && in) atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
    });
    __syncthreads();
    if (wave == 0) {  // lane L owns digits 255 - 4L .. 252 - 4L, scanned from the top
      unsigned h[4], tot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = sh.hist[255 - 4 * lane - j]; tot += h[j]; }
      unsigned inc = tot;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
      }
      unsigned before = inc - tot;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (before < kk && kk <= before + h[j]) {
          sh.sel_digit = 255u - 4u * lane - j;
          sh.sel_kk = kk - before;
          sh.sel_cnt = h[j];
        }
        before += h[j];
      }
    }
    __syncthreads();
    prefix |= sh.sel_digit << shift;
    kk = sh.sel_kk;
    eq = sh.sel_cnt;
  }
  // ---- pass 3: the candidates.  kstar = the ktot-th largest key, held by `eq` columns of which
  // kk are wanted: all of them (eq == kk), or the kk lowest ids (ties at the boundary)
  const uint32_t kstar = prefix;
  const unsigned g = ktot - kk;  // keys above kstar
  const bool ties = eq > kk;
  __syncthreads();
  if (tid < 256) sh.sortbuf[tid] = 0ull;
  if (tid == 0) sh.ccount = 0u;
  __syncthreads();
  for_each_key(row, n, pen, rp, sh.bitmap, [&](int c, uint32_t key) {
    if (key > kstar || (key == kstar && !ties)) {
      const unsigned pos = atomicAdd(&sh.ccount, 1u);
      if (pos < 256u) sh.sortbuf[pos] = ((unsigned long long)key << 32) | (0xFFFFFFFFu - (uint32_t)c);
    }
  });
  if (ties) {  // block-uniform
    unsigned running = 0;
#pragma unroll 1
    for (int base = 0; base < n && running < kk; base += 4096) {
      bool f[4];
      unsigned lp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = base + j * 1024 + tid;
        f[j] = c < n && load_key(row, c, pen, rp, sh.bitmap) == kstar;
        const unsigned long long m = __ballot(f[j]);
        lp[j] = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) sh.wave_cnt[j][wave] = (unsigned)__popcll(m);
      }
      __syncthreads();
      unsigned off = running;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned mine = off;
        for (int ww = 0; ww < 16; ++ww) {
          const unsigned cw = sh.wave_cnt[j][ww];
          if (ww < wave) mine += cw;
          off += cw;
        }
        const unsigned rank = mine + lp[j];
        if (f[j] && rank < kk && g + rank < 256u)
          sh.sortbuf[g + rank] =
              ((unsigned long long)kstar << 32) | (0xFFFFFFFFu - (uint32_t)(base + j * 1024 + tid));
      }
      running = off;
      __syncthreads();
    }
  }
  __syncthreads();
  bitonic_desc(sh.sortbuf, 256);
  }
  // ---- pass 4: top-p, min-p, temperature and the draw on the sorted candidates
  const int m = (int)ktot;
  const unsigned long long ent = tid < 256 ? sh.sortbuf[tid] : 0ull;
  const float l = fkey_inv((uint32_t)(ent >> 32));
  const int cid = (int)(0xFFFFFFFFu - (uint32_t)ent);
  const float lmax = fkey_inv(maxkey);
  int m2 = m;
  if (p.top_p < 1.0f) {
    const float e = tid < m ? expf(l - lmax) : 0.f;
    const float S = block_sum(e, sh.redf);
    const float inc = block_scan(e, sh.redf);
    // the shortest prefix whose cumulative probability reaches top_p: every candidate whose
    // exclusive cumulative sum is still below it (at least the first one)
    m2 = (int)block_sum_u(tid < m && (tid == 0 || (inc - e) < p.top_p * S) ? 1u : 0u, sh.redu);
  }
  int m3 = m2;
  if (p.min_p > 0.f) {
    const float thr = logf(p.min_p);
    m3 = (int)block_sum_u(tid < m2 && (tid == 0 || (l - lmax) >= thr) ? 1u : 0u, sh.redu);
  }
  const float e = tid < m3 ? expf((l - lmax) / p.temperature) : 0.f;
  const float S = block_sum(e, sh.redf);
  const float inc = block_scan(e, sh.redf);
  const float u = sample_u(p.seed, step);
  // the first candidate whose cumulative probability exceeds u; none (rounding): the last one
  int pick = (int)block_sum_u(tid < m3 && !(inc / S > u) ? 1u : 0u, sh.redu);
  if (pick > m3 - 1) pick = m3 - 1;
  if (tid == pick) sh.result = cid;
  if (cand_n) {
    if (tid < m3) { cand_ids[tid] = cid; cand_p[tid] = e / S; }
    if (tid == 0) *cand_n = m3;
  }
  __syncthreads();
  return sh.result;
}

}  // namespace

// ---------------------------------------------------------------- row sampler
// ids_out[r] of logits row r.  slots == nullptr (ms_op_sample): parameters, window and step of
// row r from the per-row arrays.  slots != nullptr (the engine's first token): the state of
// slot row_slot[r], advanced after the draw as the fused tail does.
__global__ __launch_bounds__(1024) void sample_rows_kernel(SampleArgs a) {
  __shared__ SampleShared sh;
  const int r = blockIdx.x;
  const float* row = a.logits + (size_t)r * a.ldl;
  SampleSlot* st = a.slots ? a.slots + a.row_slot[r] : nullptr;
  const SampleParams p = st ? st->p : a.params[r];
  const int32_t* ring = st ? st->ring : a.win + (size_t)r * kSampleMaxWindow;
  const int wcount = st ? st->wcount : min(max(a.win_len[r], 0), kSampleMaxWindow);
  const uint32_t step = (uint32_t)(st ? st->step : a.steps[r]);
  const int id = sample_row(row, a.n, p, ring, wcount, step, sh,
                            a.cand_n ? a.cand_ids + (size_t)r * kSampleMaxTopK : nullptr,
                            a.cand_n ? a.cand_p + (size_t)r * kSampleMaxTopK : nullptr,
                            a.cand_n ? a.cand_n + r : nullptr);
  if (threadIdx.x == 0) {
    a.ids_out[r] = id;
    if (st && p.temperature > 0.f) {
      st->ring[wcount & (kSampleMaxWindow - 1)] = (id >= 0 && id < a.n) ? id : 0;
      st->wcount = wcount + 1;
      st->step = (int32_t)(step + 1u);
    }
  }
}

void launch_sample_rows(const SampleArgs& a, int rows, hipStream_t s) {
  if (rows <= 0 || a.n < 1 || a.n > kSampleMaxN) return;
  MS_LAUNCH(sample_rows_kernel, dim3(rows), dim3(1024), 0, s, a);
}

// ---------------------------------------------------------------- fused sampling tail
// decode_tail_kernel's counterpart in a sampling run: block b draws row b's id from the stored,
// scaled logits (a greedy row: their argmax), then does what the greedy tail does with the same
// arithmetic -- the id to ids_out and the run's ring, the arguments advanced, the step counter
// moved by the last block on the ticket, the next input row gathered with embed_kernel's sums
// in the same order -- and advances the row's sampler state (window ring, step).
__global__ __launch_bounds__(1024) void sample_tail_kernel(const float* __restrict__ logits, SampleSlot* slots,
                                                           int32_t* __restrict__ args, int32_t* __restrict__ ids_out,
                                                           int32_t* __restrict__ ring, int B, int V,
                                                           const f16_t* __restrict__ emb, int H, float* __restrict__ x,
                                                           const f16_t* __restrict__ gamma, f16_t* __restrict__ xg,
                                                           float* __restrict__ ssq) {
  __shared__ SampleShared sh;
  __shared__ int next_id;
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  SampleSlot* st = slots + args[2 * B + b];
  const SampleParams p = st->p;
  const int wcount = st->wcount;
  const uint32_t sstep = (uint32_t)st->step;
  const int id = sample_row(logits + (size_t)b * V, V, p, st->ring, wcount, sstep, sh, nullptr, nullptr, nullptr);
  if (tid == 0) {
    ids_out[b] = id;
    const int step = args[4 * B];
    ring[(size_t)step * B + b] = id;
    const int in = (id >= 0 && id < V) ? id : 0;
    args[b] = in;
    args[B + b] += 1;
    args[3 * B + b] += 1;
    next_id = in;
    if (p.temperature > 0.f) {
      st->ring[wcount & (kSampleMaxWindow - 1)] = in;
      st->wcount = wcount + 1;
      st->step = (int32_t)(sstep + 1u);
    }
    __threadfence();  // this block's read of the step counter precedes its ticket
    typedef __attribute__((address_space(1))) unsigned gu32_t;
    const unsigned arrived =
        __hip_atomic_fetch_add((gu32_t*)&args[4 * B + 1], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived == (unsigned)B - 1) {
      args[4 * B + 1] = 0;
      args[4 * B] = step + 1;
    }
  }
  __syncthreads();
  if (tid < 256) {
    const f16_t* row = emb + (size_t)next_id * H;
    float* xo = x + (size_t)b * H;
    float ss = 0.f;
    for (int c = tid; c < H / 8; c += 256) {
      uint4 e = *(const uint4*)(row + c * 8);
      const uint32_t w[4] = {e.x, e.y, e.z, e.w};
      float4 a, bb;
      a.x = h_lo(w[0]); a.y = h_hi(w[0]);
      a.z = h_lo(w[1]); a.w = h_hi(w[1]);
      bb.x = h_lo(w[2]); bb.y = h_hi(w[2]);
      bb.z = h_lo(w[3]); bb.w = h_hi(w[3]);
      *(float4*)(xo + c * 8) = a;
      *(float4*)(xo + c * 8 + 4) = bb;
      const uint4 gv = *(const uint4*)(gamma + c * 8);
      const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w};
      uint4 o;
      o.x = pack2h(a.x * h_lo(gw[0]) * kXgScale, a.y * h_hi(gw[0]) * kXgScale);
      o.y = pack2h(a.z * h_lo(gw[1]) * kXgScale, a.w * h_hi(gw[1]) * kXgScale);
      o.z = pack2h(bb.x * h_lo(gw[2]) * kXgScale, bb.y * h_hi(gw[2]) * kXgScale);
      o.w = pack2h(bb.z * h_lo(gw[3]) * kXgScale, bb.w * h_hi(gw[3]) * kXgScale);
      *(uint4*)(xg + (size_t)b * H + c * 8) = o;
      ss += (a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w) + (bb.x * bb.x + bb.y * bb.y + bb.z * bb.z + bb.w * bb.w);
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
  }
  __syncthreads();
  if (tid == 0) ssq[b] = ((red[0] + red[1]) + red[2]) + red[3];
}

void launch_sample_tail(const float* logits, SampleSlot* slots, int32_t* args, int32_t* ids_out, int32_t* ring,
                        int B, int V, const f16_t* emb, int H, float* x, const f16_t* gamma, f16_t* xg, float* ssq,
                        hipStream_t s) {
  if (B <= 0 || V < 1 || V > kSampleMaxN) return;
  MS_LAUNCH(sample_tail_kernel, dim3(B), dim3(1024), 0, s, logits, slots, args, ids_out, ring, B, V, emb, H, x,
            gamma, xg, ssq);
}

}  // namespace ms
