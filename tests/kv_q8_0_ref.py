"""TEST INFRASTRUCTURE ONLY -- the q8_0 KV cache contract (csrc/kvq8.h) in numpy.

  quantize_rows / dequantize   ggml's quantize_row_q8_0_ref on rows of 128 fp16 values, float32, one
                               IEEE operation per step; a block with a non-finite value -> scale NaN, codes 0;
  pack_rows / unpack_pool      the pool layout: per (page, kv head) 8192 B of codes int8 [64][128], then 512 B
                               of scales fp16 [64][4];
  attend_f64 / attend_emul     decode attention of one (sequence, q head) over dequantised K^ = d c, V^ = d c
                               in float64, and the engine's arithmetic in float32 with its fp16 roundings
                               (scores sum_b d_K[b] (q . c)_b, fp32 softmax, P.V with f16(p d_V[b]) against
                               the integer codes -- the V scale folded into P --, fp16 output);
  mirror_hook                  OracleLlama.forward's mut["attend"] quantising K and V: the model mirror of a
                               q8_0-KV engine's decode steps (its prefill calls take no hook);
  OpCase                       the op-level test's inputs: decisive keys, pools, the float64 reference and the
                               mutants that show what the 2e-3 bar can see.
"""
from __future__ import annotations

import math

import numpy as np

D, BLOCK, NB, PAGE = 128, 32, 4, 64
CODE_BYTES, SCALE_BYTES = PAGE * D, PAGE * NB * 2
SLAB = CODE_BYTES + SCALE_BYTES  # 8704
NAN_SCALE = 0x7E00
# norm-wise per output row: at most four fp16 roundings of <= 2^-11 each (P d, the output, and the rounded q
# and scales being given) -- derived, not measured
BAR = 2e-3
MUTANT_FACTOR = 10.0


def quantize_rows(t16):
    """t16 [..., 128] fp16 (or uint16 bit patterns) -> (codes int8 [..., 128], scales uint16 [..., 4])."""
    t16 = np.asarray(t16)
    if t16.dtype == np.uint16:
        t16 = t16.view(np.float16)
    assert t16.dtype == np.float16 and t16.shape[-1] == D
    t = t16.astype(np.float32).reshape(t16.shape[:-1] + (NB, BLOCK))
    bad = ~np.isfinite(t).all(axis=-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        amax = np.abs(t).max(axis=-1)
        d = (amax / np.float32(127.0)).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        x = (t * inv[..., None]).astype(np.float32).astype(np.float64)  # the fp32 product, exactly
        c = np.sign(x) * np.floor(np.abs(x) + 0.5)  # roundf: half away from zero
        scales = d.astype(np.float16).view(np.uint16)
    c = np.where(bad[..., None], 0.0, c)
    scales = np.where(bad, np.uint16(NAN_SCALE), scales).astype(np.uint16)
    return c.astype(np.int8).reshape(t16.shape), scales


def dequantize(codes, scales, dtype=np.float32):
    """(float)f16(d) * c: exact in fp32."""
    d = np.asarray(scales, np.uint16).view(np.float16).astype(dtype)
    c = np.asarray(codes, np.int8).astype(dtype).reshape(codes.shape[:-1] + (NB, BLOCK))
    with np.errstate(invalid="ignore"):
        return (d[..., None] * c).reshape(codes.shape)


def pack_rows(pool, page, kvh, off, codes, scales):
    """Write one row (codes [128], scales [4]) into pool uint8 [pages][kv heads][8704]."""
    slab = pool[page, kvh]
    slab[off * D:(off + 1) * D] = np.asarray(codes, np.int8).view(np.uint8)
    slab[CODE_BYTES + off * NB * 2:CODE_BYTES + (off + 1) * NB * 2] = np.asarray(scales, np.uint16).view(np.uint8)


def unpack_pool(pool):
    """pool uint8 [..., 8704] -> (codes int8 [..., 64, 128], scales uint16 [..., 64, 4])."""
    pool = np.ascontiguousarray(pool)
    codes = pool[..., :CODE_BYTES].reshape(pool.shape[:-1] + (PAGE, D)).view(np.int8)
    scales = np.ascontiguousarray(pool[..., CODE_BYTES:]).view(np.uint16).reshape(pool.shape[:-1] + (PAGE, NB))
    return codes, scales


def mirror_hook(layer, k, v):
    """mut["attend"] of a decode call: the cache as a q8_0-KV engine's attention sees it."""
    kq = dequantize(*quantize_rows(k.astype(np.float16)))
    vq = dequantize(*quantize_rows(v.astype(np.float16)))
    return kq.astype(k.dtype), vq.astype(v.dtype)


# ------------------------------------------------------------------ attention of one (sequence, q head)
def attend_f64(q16, kc, ks, vc, vs):
    """q16 [128] fp16; kc / vc int8 [n][128]; ks / vs uint16 [n][4] -> float64 [128]."""
    K = dequantize(kc, ks, np.float64)
    V = dequantize(vc, vs, np.float64)
    s = K @ q16.astype(np.float64) / math.sqrt(D)
    p = np.exp(s - s.max())
    return (p / p.sum()) @ V


def attend_emul(q16, kc, ks, vc, vs):
    """The contract in float32 with its fp16 roundings -> fp16 [128] (as float32)."""
    f32 = np.float32
    q = q16.astype(f32).reshape(NB, BLOCK)
    c = kc.astype(f32).reshape(-1, NB, BLOCK)
    t = np.einsum("nbk,bk->nb", c, q).astype(f32)  # exact integers x fp16: fp32 block sums
    dk = ks.view(np.float16).astype(f32)
    s = np.zeros(len(kc), f32)
    for b in range(NB):
        s = (s + dk[:, b] * t[:, b]).astype(f32)
    s = (s * f32(1.4426950408889634 / math.sqrt(D))).astype(f32)
    p = np.exp2(s - s.max()).astype(f32)
    den = p.sum(dtype=f32)
    dv = vs.view(np.float16).astype(f32)
    pd = (p[:, None] * dv).astype(f32).astype(np.float16).astype(f32)  # f16(p d_V[b]) [n][4]
    o = np.einsum("nb,nbk->bk", pd, vc.astype(f32).reshape(-1, NB, BLOCK)).astype(f32).reshape(D)
    return (o / den).astype(f32).astype(np.float16).astype(f32)


def row_rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ------------------------------------------------------------------ the op-level case
LENS = (1, 63, 64, 65, 512, 513, 1590)  # one batch, the longest last
MAX_PAGES = (max(LENS) + PAGE - 1) // PAGE
HK = 2
KINDS = ("first", "page_first", "page_last", "split_first", "newest")
BLOCK_AMPS = np.array([1.0, 0.5, 1.5, 0.75], np.float32)


def decisive_pos(kind: str, n: int, split_keys: int) -> int:
    mid = ((n - 1) // PAGE) // 2 * PAGE  # a page in the middle of the sequence
    return {"first": 0, "page_first": mid, "page_last": min(mid + PAGE - 1, n - 1),
            "split_first": (n - 1) // split_keys * split_keys, "newest": n - 1}[kind]


class OpCase:
    """Group size G (Hq = G * 2 kv heads), split boundary every ``split_keys`` keys (256 ppw keys).
    Every (sequence, q head) has its own decisive key: its K row is a multiple of that head's q (score
    ln(n) + 1 above the crowd, so the key takes about half the weight and neither it nor the crowd can go
    missing unseen) and its V^ row a draw three times the crowd's.  The kinds rotate over the heads of a
    group and over the sequences; q and every row carry per-block amplitudes 1 / 0.5 / 1.5 / 0.75, so a
    block's scale is not its neighbour's."""

    def __init__(self, G: int, split_keys: int, seed: int = 811):
        self.G, self.Hq, self.split_keys = G, G * HK, split_keys
        rng = np.random.default_rng(seed + 31 * G + split_keys)
        amps = np.repeat(BLOCK_AMPS, BLOCK)
        self.q = (rng.standard_normal((len(LENS), self.Hq, D)).astype(np.float32) * amps).astype(np.float16)
        self.k, self.v, self.pos = [], [], np.zeros((len(LENS), self.Hq), np.int64)
        for i, n in enumerate(LENS):
            k = rng.standard_normal((n, HK, D)).astype(np.float32) * 0.5 * amps
            v = rng.standard_normal((n, HK, D)).astype(np.float32) * amps
            hit = {}
            for h in range(self.Hq):
                kind = KINDS[(h % G + i) % len(KINDS)]
                p = decisive_pos(kind, n, split_keys)
                self.pos[i, h] = p
                hit.setdefault((p, h // G), []).append(h)
            for (p, kvh), heads in hit.items():
                qs = self.q[i, heads].astype(np.float32)
                gamma = (math.log(n) + 1.0) * math.sqrt(D) / float((qs[0] ** 2).sum())
                k[p, kvh] = gamma * qs.sum(axis=0)
                v[p, kvh] = 3.0 * rng.standard_normal(D).astype(np.float32) * amps
            self.k.append(k.astype(np.float16))
            self.v.append(v.astype(np.float16))
        self.kq = [quantize_rows(k) for k in self.k]  # (codes [n][HK][128], scales [n][HK][4])
        self.vq = [quantize_rows(v) for v in self.v]

    def pools(self, table):
        """table int32 [slots][MAX_PAGES] -> (k pool, v pool) uint8 [pages][HK][8704]; slot i = sequence i."""
        n_pages = int(table.max()) + 1
        kp = np.zeros((n_pages, HK, SLAB), np.uint8)
        vp = np.zeros((n_pages, HK, SLAB), np.uint8)
        for i, n in enumerate(LENS):
            for pos in range(n):
                page = int(table[i, pos // PAGE])
                for h in range(HK):
                    pack_rows(kp, page, h, pos % PAGE, self.kq[i][0][pos, h], self.kq[i][1][pos, h])
                    pack_rows(vp, page, h, pos % PAGE, self.vq[i][0][pos, h], self.vq[i][1][pos, h])
        return kp, vp

    def operands(self, i, h, mutant=None):
        """(q, kc, ks, vc, vs) of sequence i, q head h; ``mutant`` one of MUTANTS (None where it cannot occur)."""
        kvh, p = h // self.G, int(self.pos[i, h])
        kc, ks = self.kq[i][0][:, kvh], self.kq[i][1][:, kvh]
        vc, vs = self.vq[i][0][:, kvh], self.vq[i][1][:, kvh]
        n = LENS[i]
        if mutant == "drop_decisive":
            if n < 2:
                return None
            keep = np.arange(n) != p
            kc, ks, vc, vs = kc[keep], ks[keep], vc[keep], vs[keep]
        elif mutant == "swap_v":
            if n < 2:
                return None
            o = p + 1 if p + 1 < n else p - 1
            vc, vs = vc.copy(), vs.copy()
            vc[[p, o]], vs[[p, o]] = vc[[o, p]], vs[[o, p]]
        elif mutant == "k_scale_neighbour":
            if n < 2:  # one key: its score cancels in the softmax
                return None
            ks = np.roll(ks, 1, axis=-1)
        elif mutant == "v_scale_neighbour":
            vs = np.roll(vs, 1, axis=-1)
        elif mutant == "other_kv_head":
            o = (kvh + 1) % HK
            kc, ks, vc, vs = self.kq[i][0][:, o], self.kq[i][1][:, o], self.vq[i][0][:, o], self.vq[i][1][:, o]
        return self.q[i, h], kc, ks, vc, vs

    def reference(self):
        """float64 [sequences][Hq][128]."""
        return np.stack([np.stack([attend_f64(*self.operands(i, h)) for h in range(self.Hq)])
                         for i in range(len(LENS))])

    def emulation(self):
        return np.stack([np.stack([attend_emul(*self.operands(i, h)) for h in range(self.Hq)])
                         for i in range(len(LENS))])


MUTANTS = ("drop_decisive", "swap_v", "k_scale_neighbour", "v_scale_neighbour", "other_kv_head")


def mutant_ratios(case: OpCase, ref) -> dict:
    """kind -> the smallest distance / BAR over every (sequence, q head) the mutant can occur in."""
    out = {}
    for kind in MUTANTS:
        worst = np.inf
        for i in range(len(LENS)):
            for h in range(case.Hq):
                ops = case.operands(i, h, kind)
                if ops is not None:
                    worst = min(worst, row_rel(attend_f64(*ops), ref[i, h]) / BAR)
        out[kind] = float(worst)
    return out


_CASES = {}


def op_case(G: int, split_keys: int) -> dict:
    """The case, its float64 reference and its emulation, computed once per (G, split_keys)."""
    key = (G, split_keys)
    if key not in _CASES:
        c = OpCase(G, split_keys)
        _CASES[key] = {"case": c, "ref": c.reference(), "emul": c.emulation()}
    return _CASES[key]


# ------------------------------------------------------------------ the QK-norm model's mirror
def qwen3_mirror_forward(o, ids, cache, quantise: bool):
    """tests/qwen3_ref.py's OracleQwen3.forward in mode "engine" with fp32 accumulation, restated with the
    one edit OracleLlama's mut["attend"] makes (OracleQwen3 takes no mutations): with ``quantise`` the call
    attends over the dequantised q8_0 K and V; the cache keeps the fp16 rows.  -> the last token's logits."""
    from oracle.llama_ref import _f16, apply_rope, rms_rinv, rope_tables, silu
    cfg, w = o.cfg, o.w
    assert o.mode == "engine" and o.acc == np.float32
    ids = np.asarray(ids, dtype=np.int64)
    T, p0 = ids.shape[0], cache["len"]
    cos, sin = rope_tables(cfg, np.arange(p0, p0 + T))
    Dh, Hq, Hk = cfg.head_dim, cfg.n_heads, cfg.n_kv_heads
    G, eps = Hq // Hk, cfg.norm_eps
    scale = np.float32(1.0 / math.sqrt(Dh))

    def normed(x, g):
        return _f16((x * g).astype(np.float32) * np.float32(0.0625)), rms_rinv(x, eps) * np.float32(16.0)

    def head_norm(t, g):
        return ((t * rms_rinv(t, eps)).astype(np.float32) * _f16(g)).astype(np.float32)

    x = w["embed"][ids].astype(np.float32)
    for l, L in enumerate(w["layers"]):
        xg, r = normed(x, L["attn_norm"])
        q = _f16(r * np.matmul(xg, L["wq"].T)).reshape(T, Hq, Dh)
        k = _f16(r * np.matmul(xg, L["wk"].T)).reshape(T, Hk, Dh)
        v = _f16(r * np.matmul(xg, L["wv"].T)).reshape(T, Hk, Dh)
        q = apply_rope(head_norm(q, L["q_norm"]), cos, sin, _f16)
        k = apply_rope(head_norm(k, L["k_norm"]), cos, sin, _f16)
        if cache["k"][l] is not None:
            k = np.concatenate([cache["k"][l], k], axis=0)
            v = np.concatenate([cache["v"][l], v], axis=0)
        cache["k"][l], cache["v"][l] = k, v
        if quantise:
            k, v = mirror_hook(l, k, v)
        S = k.shape[0]
        kq, vq = np.repeat(k, G, axis=1), np.repeat(v, G, axis=1)
        s = np.matmul(q.transpose(1, 0, 2), kq.transpose(1, 2, 0)) * scale
        mask = (np.arange(S)[None, :] > (p0 + np.arange(T))[:, None])
        s = np.where(mask[None], np.float32(-np.inf), s)
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        den = p.sum(axis=-1, keepdims=True, dtype=np.float32)
        o_ = _f16((np.matmul(_f16(p), vq.transpose(1, 0, 2)) / den).transpose(1, 0, 2))
        x = x + np.matmul(o_.reshape(T, Hq * Dh), L["wo"].T)
        xg, r = normed(x, L["ffn_norm"])
        h = _f16(silu(r * np.matmul(xg, L["w_gate"].T)) * (r * np.matmul(xg, L["w_up"].T)))
        x = x + np.matmul(h, L["w_down"].T)
    cache["len"] = p0 + T
    xg, r = normed(x[-1:], w["final_norm"])
    o.last_rinv = r
    return (r * np.matmul(xg, w["lm_head"].T))[0]
