"""CPU side of tests/test_gpu_attn_keys.py: a model in which ONE chosen key decides each attention
row, the prefill and decode cases built on it, their references, noise floors, bounds, the
deliberately wrong references ("mutants") and the count of the prefill kernel's lazy-max branches
the cases reach.  Plain helper, no test in here; method and constants (MARGIN, MUTANT_RATIO, the
decode observables) are tests/decode_edges_ref.py's.

Model (weights): make_weights(cfg, 1234, std 0.05, jitter 0.1), then three edits in numpy, so the
oracle and load_logical get the same tensors:
  token classes   E[v, :A] = E[v % C, :A] (C = 1000, A = 256; tied lm_head = the same array): tokens v
                  and v + 1000 k share the first A hidden channels, the rest differ;
  keys            every layer's wk has its columns >= A zeroed: a key reads only the class;
  queries         wq[head h] = fp16(gamma * wk[kv head of h]) on the output rows 36..63 and 100..127 of
                  the head (the rotate-half pairs 36..63, whose llama3-scaled wavelengths exceed 3e5
                  tokens: cos >= 0.9999 over 700 positions), zero elsewhere.
q(m) . k(n) is therefore large exactly when tokens m and n share a class, wherever they sit; wv, wo and
the MLP stay random, so two members of one class have equal keys but different values and losing
either changes the output row completely.  That holds in layer 0; layer 1 reads the residual after
layer 0 (see "Mutants" below).  These queries are blind to the rotation by construction: RoPE itself is
tested pair by pair in tests/rope_pairs_ref.py, on a model whose scores depend on relative position.

Prompts: position i draws class order[(i + rot) % C] (one fixed permutation, rotated per sequence of
a pack so that another sequence's K/V hold this row's class at a nearby position) and a random member
k < 4 of it (token = class + 1000 k < 4000), so a row's only same-class key is itself.  Then plants:
  pairs (m, n < m)   token m becomes another member of token n's class: row m splits its weight
                     between keys n and m.  Rows: one before, on and after every multiple of 16 (so of
                     64 and 128 too) the prompt has room for; partners in turn at key 0, key 63, key 64,
                     the first key of the row's tile, the last key of the previous tile, the previous
                     position and a key 6 tiles back -- the first of these still free, else the
                     nearest free key below the previous position ("near");
  successors m       token m + 1 becomes another member of token m's class: the key just after row m
                     would win if row m could see it.  Rows 63, 127, 128, 191, 255, 575 and n - 2.
No position is in two plants, but where the case list itself claims one twice; then three positions
share a class (plants()): successors 127 and 128 form a chain (row 128 is a successor row that also
sees 127), and a row whose partner is key 63, key 64, the first key of its tile or the last of the
previous one joins the plant that key is already in (key 64 is successor 63's token; the keys at a tile's
edges are edge rows with partners of their own).  Such a row has two earlier class-mates, each hidden in turn ("partner",
"copartner").  Kinds of row: "successor", "planted" (the later row of a pair or of a successor), "diagonal".

Mutants (mut["mask"] of the oracle): a fault is present in every layer, as a faulty kernel's would be,
and is scored on the rows it targets, each read after layer 1 and after layer 2 as the GPU test reads
them.  The rows of one layer are independent given its input and no targeted row attends decisively to
another targeted row (plants are disjoint), so hiding every planted partner at once is, after layer 1
row for row exactly and after layer 2 up to background keys, the one-at-a-time fault.  The read after
layer 1 alone carries the condition (>= 125 x the bound); after layer 2 a row shows the same fault
through its residual (>= 117 x; prefill_mutants records both).  A fault in layer 1's attention ALONE is weaker:
its keys read the residual after layer 0, where the attention and MLP outputs outweigh the class
embedding about 40 : 1, so class-mates no longer have equal keys there (a hidden partner moves such a
row by 5 x the bound in the median, 0.1 x at the least) -- layer 1 checks the kernel on other data and
reaches the same lazy-max branches, layer 0 is where one key decides.
"""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np

import decode_edges_ref as R
from mapsum.config import TINY
from oracle.llama_ref import OracleLlama, _f16, apply_rope, rms_rinv, rope_inv_freq, rope_tables
from oracle.synth import make_weights

MARGIN, MUTANT_RATIO, PAGE = R.MARGIN, R.MUTANT_RATIO, R.PAGE
SEED, STD, JITTER = 1234, 0.05, 0.1
C, A = 1000, 256
MEMBERS = 4  # class + 1000 k < 4000 for k < 4: below TINY's bos / eos ids
STILL = np.r_[36:64, 100:128]  # head dims of the RoPE pairs that do not rotate over these lengths
WAVE, TILE, LAZY = 16, 64, 8.0  # csrc/k_attn.hip attn_prefill_kernel (a 128-row q-block is 8 whole waves)

CONFIGS = {
    "g3": TINY.with_(name="keys-g3", n_heads=6, n_kv_heads=2, hidden=768),
    "g8": TINY.with_(name="keys-g8", n_heads=8, n_kv_heads=1, hidden=1024),
    "g5": TINY.with_(name="keys-g5", n_heads=10, n_kv_heads=2, hidden=1280),
    "g1": TINY.with_(name="keys-g1", n_heads=4, n_kv_heads=4, hidden=512),
}
GB = {"g3": 3, "g8": 2, "g5": 1, "g1": 1}  # launch_attn_prefill: 3 | group, else 2 | group, else 1
# one constant per config, chosen from the oracle alone (survey_gamma, on the 700-token prompt, per
# layer): at gamma 1 a class-mate peaks 4.6 log2 units over a background of std 0.6 and no config has a
# single late grow; at 2 there are 240 - 750, from the tail of the peaks only; at 3 the typical peak
# (13.8 units, background std 1.8) clears the 8-unit threshold: 1,500 - 4,100 late grows, 6,000 - 16,800
# tiles above the reference that keep it (excess up to 7.99), 90 - 570 mixed waves, |q| <= 12; 4 adds a
# third more grows and nothing new.  tests/test_attn_keys_ref.py asserts what gamma must deliver.
GAMMA = {"g3": 3.0, "g8": 3.0, "g5": 3.0, "g1": 3.0}

P1_LENS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193, 257, 700)
P2_LENS = (1, 17, 64, 129, 65, 1, 320, 128)
P3_LENS = (1, 1, 2, 16, 33, 64, 65, 130)
SUCCESSORS = (63, 127, 128, 191, 255, 575)
PARTNER_KINDS = ("key0", "key63", "key64", "tile_first", "prev_tile_last", "prev", "far")
PREFILL_MUTANTS = ("diagonal", "partner", "copartner", "successor", "column")
COLUMN_T = 1  # the whole-column mutant hides key 64 from every later row

DEC_LENS = (1, 63, 64, 300)
NPRED = 6  # the prefill's token + 5 decode steps
DEC_KINDS = ("key0", "key63", "page_first", "self", "prev")  # the partner of decode step j = 1..5
DEC_MUTANTS = ("drop_partner", "drop_new")
DEC_MAX_CTX, DEC_PPB = 320, 4  # 5 pages; splits of 256 keys: the 300-key row's new token sits in the second

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_keys_bounds.json")
_GOLDEN = {}


def golden() -> dict:
    if not _GOLDEN:
        with open(GOLDEN) as f:
            _GOLDEN.update(json.load(f))
    return _GOLDEN


# ------------------------------------------------------------------ model
_WEIGHTS, _ORACLES = {}, {}


def weights(name: str, gamma: float | None = None) -> dict:
    gamma = GAMMA[name] if gamma is None else gamma
    if (name, gamma) in _WEIGHTS:
        return _WEIGHTS[name, gamma]
    cfg = CONFIGS[name]
    w = make_weights(cfg, SEED, std=STD, jitter=JITTER)
    D, Hq, Hk, H = cfg.head_dim, cfg.n_heads, cfg.n_kv_heads, cfg.hidden
    emb = w["embed"]
    emb[:, :A] = emb[np.arange(cfg.vocab) % C, :A]
    assert w["lm_head"] is emb
    for ly in w["layers"]:
        ly["wk"][:, A:] = 0.0
        wk = ly["wk"].reshape(Hk, D, H)
        wq = np.zeros((Hq, D, H), np.float32)
        for h in range(Hq):
            wq[h, STILL] = np.float32(gamma) * wk[h // (Hq // Hk), STILL]
        ly["wq"] = _f16(wq.reshape(Hq * D, H))
    _WEIGHTS[name, gamma] = w
    return w


def oracle(name: str, acc=np.float32, gamma: float | None = None) -> OracleLlama:
    key = (name, np.dtype(acc).name, GAMMA[name] if gamma is None else gamma)
    if key not in _ORACLES:
        _ORACLES[key] = OracleLlama(CONFIGS[name], weights(name, gamma), acc=acc)
    return _ORACLES[key]


def still_cos_min(n: int = 700) -> float:
    """The smallest cos over positions < n of the RoPE pairs the queries read."""
    ang = np.arange(n)[:, None] * rope_inv_freq(TINY)[None, 36:64]
    return float(np.cos(ang).min())


# ------------------------------------------------------------------ prompts and plants
_ORDER = np.random.default_rng(8100).permutation(C)


CHAIN_KINDS = ("key63", "key64", "tile_first", "prev_tile_last")  # keys that rows or successors of the list also claim


def plants(n: int) -> dict:
    """{"pairs": [(row, partner key, kind)], "succ": [row], "co": {row: [further earlier class-mates]}}
    of a prompt of n tokens.  A group is the positions that share one class: two, or three where the
    case list claims one position twice -- successors 127 and 128 (127, 128, 129), and a partner of
    CHAIN_KINDS that is already in a plant (key 64 is successor 63's token, so one row takes keys 63
    and 64 as partners; the first key of a tile and the last of the previous one are themselves edge
    rows with partners)."""
    used, succ, grp, size = set(), [], {}, {}

    def join(m, k):
        root = grp.setdefault(k, k)
        size[root] = size.get(root, 1) + 1
        grp[m] = root
        used.update((m, k))

    def free(k, kind):
        return k not in used or (kind in CHAIN_KINDS and size[grp[k]] < 3)

    for s in SUCCESSORS + (n - 2,):
        if s < 0 or s + 1 > n - 1 or s in succ or s + 1 in used:
            continue
        if s in used and s - 1 not in succ:
            continue  # only the chain 127 -> 128 may share a position
        succ.append(s)
        join(s + 1, s)
    # ascending: an edge row that a later row wants as its partner already has its own plant
    rows = [m for x in range(WAVE, n + 1, WAVE) for m in (x - 1, x, x + 1) if 1 <= m <= n - 1]
    pairs = []
    for i, m in enumerate(rows):
        if m in used:
            continue
        t0 = TILE * (m // TILE)
        far = next((k for k in range(m - 6 * TILE, m - 6 * TILE - 8, -1) if k not in used), -1)
        where = {"key0": 0, "key63": 63, "key64": 64, "tile_first": t0, "prev_tile_last": t0 - 1, "prev": m - 1,
                 "far": far, "near": next((k for k in range(m - 2, -1, -1) if k not in used), -1)}
        for j in range(len(PARTNER_KINDS) + 1):
            kind = PARTNER_KINDS[(i + j) % len(PARTNER_KINDS)] if j < len(PARTNER_KINDS) else "near"
            k = where[kind]
            if 0 <= k < m and free(k, kind):
                pairs.append((m, k, kind))
                join(m, k)
                break
    nominal = dict([(m, k) for m, k, _ in pairs] + [(s + 1, s) for s in succ])
    co = {m: sorted(x for x in grp if grp[x] == grp[m] and x < m and x != k) for m, k in nominal.items()}
    return {"pairs": pairs, "succ": sorted(succ), "co": {m: v for m, v in co.items() if v}}


def _member(tok, cls: int) -> int:
    """The first member of a class that no token of the prompt is yet."""
    held = {int(t) // 1000 for t in tok if int(t) % 1000 == cls}
    return cls + 1000 * min(set(range(MEMBERS)) - held)


def build_prompt(n: int, rot: int, seed: int, planted: bool = True) -> np.ndarray:
    rng = np.random.default_rng(seed)
    cls = _ORDER[(np.arange(n) + rot) % C]
    tok = cls + 1000 * rng.integers(0, MEMBERS, size=n)
    if planted:
        pl = plants(n)
        # in the order the plants were made: a partner that is itself planted holds its final token
        for m, k in [(s + 1, s) for s in pl["succ"]] + [(m, k) for m, k, _ in pl["pairs"]]:
            tok[m] = _member(tok, int(tok[k]) % 1000)
    return tok.astype(np.int32)


def row_kinds(n: int) -> list:
    pl = plants(n)
    kinds = ["diagonal"] * n
    for m, _, _ in pl["pairs"]:
        kinds[m] = "planted"
    for s in pl["succ"]:
        kinds[s + 1] = "planted"
    for s in pl["succ"]:
        kinds[s] = "successor"
    return kinds


PREFILL_CASES = {"P1": P1_LENS, "P2": P2_LENS, "P3": P3_LENS}
_CASE_SEED = {"P1": 8200, "P2": 8300, "P3": 8400}


def prefill_prompts(case: str) -> list:
    """P1: 13 prompts probed one per call; P2 / P3: the sequences of one pack, the class order rotated
    by 5 per sequence."""
    return [build_prompt(n, 0 if case == "P1" else 5 * i, _CASE_SEED[case] + 17 * i)
            for i, n in enumerate(PREFILL_CASES[case])]


# ------------------------------------------------------------------ prefill references, floors, mutants
_PROBES = {}


def probes(name: str, prompt, acc=np.float32, mut=None, tag=None) -> list:
    """Hidden rows after each layer, [n_layers][n][H] (cached by tokens; a mutant by ``tag``)."""
    key = (name, np.dtype(acc).name, tuple(int(t) for t in prompt), tag)
    if key not in _PROBES:
        _PROBES[key] = oracle(name, acc).forward(prompt, collect=True, mut=mut)[1]
    return _PROBES[key]


def prefill_floors(name: str) -> list:
    """Per layer: the largest fp32-vs-fp64 row distance over every sequence of every prefill case."""
    out = [0.0, 0.0]
    for case in PREFILL_CASES:
        for p in prefill_prompts(case):
            a, b = probes(name, p), probes(name, p, np.float64)
            for l in range(2):
                out[l] = max(out[l], float(R.row_rel(a[l], b[l]).max()))
    return out


def _mask_mutant(kind: str, n: int):
    """(mut, targeted rows) of one prefill mutant of an n-token prompt."""
    pl = plants(n)
    hide, show = [], []  # (row, key)
    if kind == "diagonal":
        hide = [(m, m) for m in range(1, n)]
    elif kind == "partner":
        hide = [(m, k) for m, k, _ in pl["pairs"]] + [(s + 1, s) for s in pl["succ"]]
    elif kind == "copartner":  # rows of a group of three: the earliest class-mate instead of the nominal one
        hide = [(m, v[0]) for m, v in pl["co"].items()]
    elif kind == "successor":
        show = [(s, s + 1) for s in pl["succ"]]
    elif kind == "column":
        hide = [(m, TILE * COLUMN_T) for m in range(TILE * COLUMN_T + 1, n)]
    rows = sorted({m for m, _ in hide + show})

    def f(l, mask):
        mask = mask.copy()
        for m, k in hide:
            mask[m, k] = True
        for m, k in show:
            mask[m, k] = False
        return mask
    return {"mask": f}, rows


def prefill_mutants(name: str, bound: list) -> dict:
    """kind -> {"ratio": the smallest ratio over every targeted row of every sequence, "layer0" /
    "layer1": the same of each read alone, "rows": how many rows}.  A row's ratio is the larger of
    its two distances / bounds: the GPU test reads it after layer 1 and after layer 2 and asserts
    both.  For the whole-column mutant the exempt form: "moved" = the rows it moves beyond a bound,
    "ratio" = the largest."""
    out = {}
    for kind in PREFILL_MUTANTS:
        per_layer = [[], []]
        for case in PREFILL_CASES:
            for p in prefill_prompts(case):
                mut, rows = _mask_mutant(kind, len(p))
                if not rows:
                    continue
                base, got = probes(name, p), probes(name, p, mut=mut, tag=kind)
                for l in range(2):
                    per_layer[l].append(R.row_rel(got[l][rows], base[l][rows]) / bound[l])
        d = np.stack([np.concatenate(x) for x in per_layer])  # [layer][targeted row]
        both = d.max(axis=0)
        if kind == "column":
            out[kind] = {"ratio": float(both.max()), "moved": int((both > 1.0).sum()), "rows": int(both.size)}
        else:
            out[kind] = {"ratio": float(both.min()), "layer0": float(d[0].min()), "layer1": float(d[1].min()),
                         "rows": int(both.size)}
    return out


def swapped_ratio(name: str, bound: list) -> float:
    """The smallest distance / bound between the reference rows of two different sequences of one
    pack at the same (sequence-relative) position, over every pair of P2 and of P3, every common row
    and both layers -- the equal-length pair (the two one-token sequences) included: what a row that
    was computed from, or written into, another sequence's place would be off by."""
    worst = np.inf
    for case in ("P2", "P3"):
        ps = prefill_prompts(case)
        for i in range(len(ps)):
            for j in range(i):
                m = min(len(ps[i]), len(ps[j]))
                a, b = probes(name, ps[i]), probes(name, ps[j])
                for l in range(2):
                    worst = min(worst, float((R.row_rel(a[l][:m], b[l][:m]) / bound[l]).min()))
    return worst


# ------------------------------------------------------------------ the lazy-max rule on the oracle's scores
def scores_log2(name: str, prompt, layer: int) -> tuple:
    """([Hq][n][n] the fp32 oracle's attention scores of one layer in log2 units (what the kernel's
    exponent sees: q . k * log2(e) / sqrt(d)), -inf above the diagonal, and the largest |q|)."""
    cfg, o = CONFIGS[name], oracle(name)
    n, D, Hq, Hk = len(prompt), cfg.head_dim, cfg.n_heads, cfg.n_kv_heads
    cache = o.new_cache()
    pr = o.forward(prompt, cache, collect=True)[1]
    x = o.w["embed"][np.asarray(prompt)].astype(np.float32) if layer == 0 else pr[layer - 1]
    ly = o.w["layers"][layer]
    xg = _f16((x * ly["attn_norm"]).astype(np.float32) * np.float32(0.0625))  # OracleLlama.forward normed()
    r = rms_rinv(x, cfg.norm_eps) * np.float32(16.0)
    cos, sin = rope_tables(cfg, np.arange(n))
    q = apply_rope(_f16(r * (xg @ ly["wq"].T)).reshape(n, Hq, D), cos, sin, _f16)
    k = np.repeat(cache["k"][layer], Hq // Hk, axis=1)
    s = np.einsum("mhd,nhd->hmn", q.astype(np.float64), k.astype(np.float64)) * (math.log2(math.e) / math.sqrt(D))
    s[:, np.triu(np.ones((n, n), bool), 1)] = -np.inf
    return s, float(np.abs(q).max())


def branch_counts(name: str, prompt, layer: int) -> dict:
    """attn_prefill_kernel's rule restated: 64-key tiles; the running reference of a (row, head) grows
    only when a tile's maximum exceeds it by more than 8 log2 units; a wave is 16 consecutive rows of
    one 128-row q-block times the GB heads of one block and skips the tiles wholly after its last row.
      late_grows   grows at a tile t > 0, per (row, head, tile);
      above        tiles whose maximum lies above the reference without moving it; excess = the largest;
      mixed        (wave, head block, tile) in which a growing (row, head) meets one that sees keys of
                   the tile and keeps its reference (alpha = 1)."""
    s, qmax = scores_log2(name, prompt, layer)
    Hq, n, _ = s.shape
    nt = (n + TILE - 1) // TILE
    pad = np.full((Hq, n, nt * TILE), -np.inf)
    pad[:, :, :n] = s
    tm = pad.reshape(Hq, n, nt, TILE).max(axis=-1)  # [Hq][n][tile], -inf where the row sees none of it
    ref = np.full((Hq, n), -np.inf)
    grow = np.zeros((Hq, n, nt), bool)
    above = np.zeros((Hq, n, nt), bool)
    excess = 0.0
    for t in range(nt):
        mx = tm[:, :, t]
        new = np.maximum(ref, mx)
        with np.errstate(invalid="ignore"):
            g = (new != ref) & ~((new - ref) <= LAZY)
        ab = (new != ref) & ~g
        if ab.any():
            excess = max(excess, float((new - ref)[ab].max()))
        grow[:, :, t], above[:, :, t] = g, ab
        ref = np.where(g, new, ref)
    gb = GB[name]
    mixed = 0
    for w0 in range(0, n, WAVE):
        rows = slice(w0, min(w0 + WAVE, n))
        last = min(w0 + WAVE, n) - 1
        for h0 in range(0, Hq, gb):
            for t in range(1, last // TILE + 1):
                g = grow[h0:h0 + gb, rows, t]
                seen = np.isfinite(tm[h0:h0 + gb, rows, t])
                mixed += bool(g.any() and (seen & ~g).any())
    return {"late_grows": int(grow[:, :, 1:].sum()), "above": int(above.sum()), "excess": excess, "mixed": mixed,
            "qmax": qmax}


def branches(name: str) -> dict:
    """The three counts per layer over every sequence of every prefill case, and the largest |q|."""
    out = {}
    for l in range(2):
        tot = {"late_grows": 0, "above": 0, "excess": 0.0, "mixed": 0, "qmax": 0.0}
        for case in PREFILL_CASES:
            for p in prefill_prompts(case):
                b = branch_counts(name, p, l)
                for k in ("late_grows", "above", "mixed"):
                    tot[k] += b[k]
                for k in ("excess", "qmax"):
                    tot[k] = max(tot[k], b[k])
        out[f"layer{l}"] = tot
    return out


# ------------------------------------------------------------------ decode
def decode_prompts() -> list:
    return [build_prompt(n, 5 * i, 8500 + 17 * i, planted=False) for i, n in enumerate(DEC_LENS)]


def forced_ids(prompt) -> tuple:
    """(ids fed to decode steps 1..5, the partner key of each step or None).  Step j's token sits at
    position P = n + j - 1; its partner is, in turn, key 0, key 63, the first key of the last page
    holding cached keys, nothing but itself (a class the sequence has not seen) and the previous
    position -- clamped to the keys that exist (P - 1), each forced token being the first member of the
    partner's class that the sequence does not hold yet."""
    toks, fed, partners = [int(t) for t in prompt], [], []
    n = len(toks)
    for j in range(1, NPRED):
        P = n + j - 1
        kind = DEC_KINDS[j - 1]
        if kind == "self":
            seen = {t % 1000 for t in toks}
            cls, target = next(int(c) for c in _ORDER[::-1] if int(c) not in seen), None
        else:
            target = min({"key0": 0, "key63": 63, "page_first": (P - 1) // PAGE * PAGE, "prev": P - 1}[kind], P - 1)
            cls = toks[target] % 1000
        held = {t // 1000 for t in toks if t % 1000 == cls}
        tok = cls + 1000 * min(set(range(MEMBERS)) - held)
        toks.append(tok)
        fed.append(tok)
        partners.append(target)
    return fed, partners


_DEC = {}


def decode_reference(name: str, acc=np.float32) -> list:
    """Per sequence: decode_edges_ref.run_sequence fed the forced ids."""
    key = (name, np.dtype(acc).name)
    if key not in _DEC:
        _DEC[key] = [R.run_sequence(oracle(name, acc), p, feed=forced_ids(p)[0], steps=NPRED) for p in decode_prompts()]
    return _DEC[key]


def decode_floors(name: str) -> dict:
    out = {f: 0.0 for f in R.FAMILIES}
    for a, b in zip(decode_reference(name), decode_reference(name, np.float64)):
        for f, d in R.distances(a, b).items():
            out[f] = max(out[f], d)
    return out


def decode_mutants(name: str, bound: dict) -> dict:
    """kind -> the smallest ratio over (sequence, step): one key dropped from what that step attends to
    (its partner; the new token), scored on what the GPU test reads of that step -- its tile maxima
    and the new position's K / V rows."""
    o = oracle(name)
    out = {k: np.inf for k in DEC_MUTANTS}
    for p, ref in zip(decode_prompts(), decode_reference(name)):
        n = len(p)
        partners = forced_ids(p)[1]
        for j in range(1, NPRED):
            P = n + j - 1
            prior = {"k": [k[:P] for k in ref["k"]], "v": [v[:P] for v in ref["v"]], "len": P}
            base = {"unscaled": ref["unscaled"][j:j + 1], "logits": ref["logits"][j:j + 1],
                    "k": [k[P:P + 1] for k in ref["k"]], "v": [v[P:P + 1] for v in ref["v"]]}
            for kind, idx in (("drop_partner", partners[j - 1]), ("drop_new", P)):
                if idx is None:
                    continue
                cache = dict(prior, k=list(prior["k"]), v=list(prior["v"]))
                mut = {"attend": lambda l, k, v, idx=idx: (np.delete(k, idx, axis=0), np.delete(v, idx, axis=0))}
                lg, _ = o.forward([ref["fed"][j - 1]], cache, mut=mut)
                got = {"unscaled": R._unscaled(o, lg)[None], "logits": lg[None],
                       "k": [k[P:P + 1] for k in cache["k"]], "v": [v[P:P + 1] for v in cache["v"]]}
                d = R.distances(got, base)
                out[kind] = min(out[kind], max(d[f] / bound[f] for f in ("tilemax", "k", "v")))
    return {k: float(v) for k, v in out.items()}


# ------------------------------------------------------------------ the recorded numbers
def config_numbers(name: str) -> dict:
    """What tests/golden/attn_keys_bounds.json records for one config."""
    fl = prefill_floors(name)
    bnd = [MARGIN * f for f in fl]
    dfl = decode_floors(name)
    dbnd = {f: MARGIN * dfl[f] for f in R.FAMILIES}
    return {"gamma": GAMMA[name],
            "prefill": {"floor": fl, "bound": bnd, "mutants": prefill_mutants(name, bnd),
                        "swapped_ratio": swapped_ratio(name, bnd), "branches": branches(name)},
            "decode": {"floor": dfl, "bound": dbnd, "mutant_ratio": decode_mutants(name, dbnd),
                       "forced": [forced_ids(p)[0] for p in decode_prompts()]}}


def write_golden() -> None:
    """Regenerate the file, by hand after a deliberate change of the model, the cases or the oracle
    (with the repository root, the package directory and tests/ on sys.path:
    python tests/attn_keys_ref.py --record)."""
    out = {"configs": {name: config_numbers(name) for name in CONFIGS}}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    _GOLDEN.clear()


def survey_gamma(gammas=(1.0, 2.0, 3.0, 4.0)) -> None:
    """How GAMMA was chosen: the branch counts of the 700-token prompt per config and gamma."""
    p = prefill_prompts("P1")[-1]
    for name in CONFIGS:
        for g in gammas:
            saved = GAMMA[name]
            GAMMA[name] = g
            try:
                print(name, g, [branch_counts(name, p, l) for l in range(2)], flush=True)
            finally:
                GAMMA[name] = saved


if __name__ == "__main__":
    if "--survey" in sys.argv:
        survey_gamma()
    elif "--record" in sys.argv:
        write_golden()
