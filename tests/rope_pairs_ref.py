"""CPU side of tests/test_gpu_rope_pairs.py: a model whose attention weights depend on RELATIVE
POSITION only, pair by pair of the rotation, the prefill and decode cases built on it, their
references, noise floors, bounds and the deliberately wrong rotations ("mutants").  Plain helper, no
test in here; method and constants (MARGIN, MUTANT_RATIO, the decode observables) are
tests/decode_edges_ref.py's, the layout is tests/attn_keys_ref.py's.

Why: Q is rotated by hand in six places (attn_prefill_kernel's staging, the v1 and v2 decode slab
prologues, the GEMV ROPE_KV epilogue, rope_kv_kernel with rope_q, k_qknorm.hip), each with its own
indexing of the rope-permuted head and of the cos / sin table.  tests/attn_keys_ref.py's queries live
on pairs that do not rotate, every other model of the suite is random (one pair is 1/64 of a
near-uniform row) and uses the llama3-scaled base 500000, under which pairs >= ~32 turn < 0.1 rad over
any context the suite runs.  The kernels only see the tables, so a config may use a small unscaled
base: then every pair turns many radians within 300 tokens.

Model (weights): make_weights(cfg, 1234, std 0.05, jitter 0.1), then edits in numpy, so the oracle and
load_logical get the same tensors:
  constant carrier   E[v, :A] = E[0, :A] for every v (A = 256; tied lm_head = the same array) and every
                     layer's wk has its columns >= A zeroed: up to the row's norm factor every token
                     has the same un-rotated key z in layer 0;
  phase-shifted q    pair i (head dims i, i + 64 in the logical order) is owned by head h = i % n_heads,
                     which has the offset d_h = OFFSETS[h].  With (a, b) = the rows i, i + 64 of the
                     head's kv head in wk, t = d_h theta_i and the gain g_i,
                         wq[h] rows (i, i + 64) = g_i (a cos t + b sin t, b cos t - a sin t)
                     in fp64, rounded to fp16; every other wq row is zero.  The un-rotated query is the
                     key turned back by d_h positions, so
                         q(m) . k(n) = sum_i g_i |z_i|^2 cos((m - n - d_h) theta_i):
                     a function of m - n in which every owned pair carries its share;
  pair gains         g_i = gamma min(CAP, mean_i |z_i|^2 / |z_i|^2), z = layer 0's key of the carrier:
                     every pair's score amplitude is equal (but a pair whose |z_i|^2 is below 1/CAP of
                     the mean);
  l3 only            pairs >= 24 get a quarter turn more (t = d_h theta_i + pi / 2: their angle over a
                     prompt is small, and the score is then first order in it, not second) and SLOW x
                     the gain.
wv, wo and the MLP stay random, so which keys a row weights decides its output.  The construction is
exact in layer 0; layer 1 reads the residual after layer 0 and checks the kernels on other data.

Configs (TINY's layers, ffn and vocab):
  r3  6 / 2 heads (prefill GB 3)                                 rope_theta = BASE (64), rope_factor 0
  r8  8 / 1 heads, hidden 1024 (GB 2; the decode kernels' kMaxGroup)   the same base
  r1  4 / 4 heads, hidden 512 (GB 1)                                   the same base
  l3  TINY unchanged (theta 500000, factor 32): the only config that checks engine.cpp rope_tables'
      scaled and smoothed branches against rope_inv_freq through attention.

Prompts: random ids < 4000 from fixed seeds.  Prefill: P1 = single prompts, P2 = one pack, L = l3's
2048-token prompt.  Decode: six sequences of (1, 63, 64, 300, 200, 230) keys -- the last two are added
positions, see the survey below -- and 5 forced steps (the forced ids are random ids from a fixed
seed too: teacher forcing needs no greedy choice, so no near-tie of the oracle can change the run).

Mutants, all through the oracle's "rope_q" hook (K side: "new_kv"), present in every layer:
  q_pos_minus / q_pos_plus   Q rotated at position - 1 / + 1;
  q_unrotated                Q not rotated;
  q_block_relative           position mod 128 (a q-block-relative row index);
  q_pack_row                 P2 only: the packed row index qstart + i as the position;
  q_freq(i)                  pair i reads table column i ^ 8;
  q_conj(i)                  sin negated for pair i;
  k_freq(i) / k_conj(i)      the same two in the K writer, scored on the K rows it writes.
A mutant's ratio is the largest distance / bound over what the GPU test asserts, taken twice:
  prefill   over the hidden rows after layer 1 and after layer 2 of the 300-token prompt of P1 (l3:
            pairs 24..35 on the 2048-token prompt, after layer 1 only; q_pack_row: over the sequences
            of P2) -- a part of what the test asserts, so a lower bound of the ratio;
  decode    over the tile maxima of the 5 forced steps of the six sequences, the fault being present
            in the decode steps ALONE (each step from the reference's cache, as
            decode_edges_ref._mutant_distances does): what a fault in one decode rotation site shows.
            The prefill logits, which the GPU test asserts too, are left out: a decode site does not
            compute them.  Again a lower bound.
The K-side twins are scored on the rows a faulty writer would write from the reference's own
un-rotated keys (both layers, the 305 positions of the longest decode sequence) against the K bound.

How the constants were chosen (survey(), the oracle alone; the smallest ratio over the 64 pairs,
q_freq / q_conj; every whole-row mutant was >= 45 x throughout):
  BASE 100, gamma 3, CAP 6, the four sequences (1, 63, 64, 300)
      prefill  r3 17.3 / 11.3   r8 13.0 / 7.5   r1 12.6 / 5.4
      decode   r3  5.5 / 3.0    r8  2.8 / 2.6   r1  2.3 / 1.55 (pair 63): short of 2.  A negated sin turns
               the pair by 2 p theta_i too far, and 2 * 300 * theta_63 = 6.45 is one whole turn: at the
               only long sequence the mutant is nearly the identity.
  gamma 6 (r3)                prefill 26 / 28, decode 15.8 / 2.6: gain does not help a pair that aliases.
  BASE 100 and a fifth or sixth sequence of 100 .. 260 keys: r1 reaches 2.5 at the most.
  BASE 64, the four sequences
      prefill  r3 26.9 / 22.3   r8 26.2 / 23.2  r1 19.5 / 19.7: the slow pairs turn 1.6 x further;
      decode   r3  5.8 / 4.8    r8  4.3 / 2.2   r1  2.5 / 0.9 (pair 49: 2 * 302 * theta_49 = 25.0, four
               turns).  Some pair aliases at any base while one sequence alone is long;
  BASE 64 and the sequences of 200 and 230 keys (in force): other positions, other aliases --
      decode   r3  7.5 / 7.8    r8  7.4 / 6.5   r1  6.9 / 5.1; of the pairs (100, 150, 200, 230, 260) tried
               as additions this one is the best for r1 (>= 4.6 in every config before the two
               sequences joined the floors).
  l3 (gamma 3, SLOW 4): whole-row mutants >= 54 x, pairs 0..23 >= 4.6 x on the 300-token prompt, pairs
      24..31 >= 8.4 x on the 2048-token prompt (29: 18.2 / 20.7, 30: 16.5 / 18.3), 32 0.5 / 3.3, 33..35
      0.2 .. 0.7: nothing needed tuning.
The values in force and their figures are in tests/golden/rope_pairs_bounds.json;
tests/test_rope_pairs_ref.py asserts the conditions.
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
A = 256
HALF = 64  # pairs of a head
BASE = 64.0
OFFSETS = (1, 2, 5, 17, 64, 130, 3, 33)  # d_h; the first n_heads of them
GAMMA = {"r3": 3.0, "r8": 3.0, "r1": 3.0, "l3": 3.0}
CAP = 6.0
L3_QUARTER, L3_SLOW = 24, 4.0  # l3: pairs >= 24 get the quarter turn and SLOW x the gain
L3_LONG_PAIRS = tuple(range(24, 36))  # the pairs whose mutants run on the 2048-token prompt
L3_BANDS = {"unscaled": tuple(range(0, 24)), "smoothed": (29, 30)}  # pairs the l3 condition names

CONFIGS = {
    "r3": TINY.with_(name="rope-r3", rope_theta=BASE, rope_factor=0.0),
    "r8": TINY.with_(name="rope-r8", n_heads=8, n_kv_heads=1, hidden=1024, rope_theta=BASE, rope_factor=0.0),
    "r1": TINY.with_(name="rope-r1", n_heads=4, n_kv_heads=4, hidden=512, rope_theta=BASE, rope_factor=0.0),
    "l3": TINY.with_(name="rope-l3"),
}
RNAMES = ("r1", "r3", "r8")
GB = {"r3": 3, "r8": 2, "r1": 1, "l3": 3}  # launch_attn_prefill: 3 | group, else 2 | group, else 1

P1_LENS = (1, 17, 64, 129, 300, 700)
P2_LENS = (1, 17, 64, 129, 65, 1, 320, 128)
L3_P1_LENS = (300, 700)
L3_LONG = 2048
BLOCK = 128  # attn_prefill_kernel's q-block

DEC_LENS = (1, 63, 64, 300, 200, 230)  # the last two: see the survey in the docstring
NPRED = 6  # the prefill's token + 5 decode steps
DEC_MAX_CTX = 320

ROW_MUTANTS = ("q_pos_minus", "q_pos_plus", "q_unrotated", "q_block_relative")
PAIR_MUTANTS = ("q_freq", "q_conj")
K_MUTANTS = ("k_freq", "k_conj")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rope_pairs_bounds.json")
_GOLDEN = {}


def golden() -> dict:
    if not _GOLDEN:
        with open(GOLDEN) as f:
            _GOLDEN.update(json.load(f))
    return _GOLDEN


# ------------------------------------------------------------------ model
_WEIGHTS, _ORACLES = {}, {}


def owner(name: str, i: int) -> int:
    return i % CONFIGS[name].n_heads


def carrier_key(cfg, w: dict) -> np.ndarray:
    """[Hk][D] fp64: layer 0's un-rotated key of token 0 (every token's, up to its norm factor)."""
    ly = w["layers"][0]
    x = _f16(w["embed"][0])
    xg = _f16((x * ly["attn_norm"]).astype(np.float32) * np.float32(0.0625))  # OracleLlama.forward normed()
    r = float(rms_rinv(x[None], cfg.norm_eps)[0, 0]) * 16.0
    return (r * (xg.astype(np.float64) @ _f16(ly["wk"]).astype(np.float64).T)).reshape(cfg.n_kv_heads, cfg.head_dim)


def pair_gains(name: str, w: dict, gamma: float, cap: float) -> np.ndarray:
    """[64] g_i of the owning head, from its kv head's carrier key."""
    cfg = CONFIGS[name]
    z = carrier_key(cfg, w)
    zz = z[:, :HALF] ** 2 + z[:, HALF:] ** 2  # [Hk][pair]
    G = cfg.n_heads // cfg.n_kv_heads
    g = np.empty(HALF)
    for i in range(HALF):
        kv = owner(name, i) // G
        g[i] = gamma * min(cap, zz[kv].mean() / zz[kv, i])
        if name == "l3" and i >= L3_QUARTER:
            g[i] *= L3_SLOW
    return g


def weights(name: str, gamma: float | None = None, cap: float | None = None) -> dict:
    gamma = GAMMA[name] if gamma is None else gamma
    cap = CAP if cap is None else cap
    if (name, gamma, cap) in _WEIGHTS:
        return _WEIGHTS[name, gamma, cap]
    cfg = CONFIGS[name]
    w = make_weights(cfg, SEED, std=STD, jitter=JITTER)
    D, Hq, Hk, H = cfg.head_dim, cfg.n_heads, cfg.n_kv_heads, cfg.hidden
    emb = w["embed"]
    emb[:, :A] = emb[0, :A]
    assert w["lm_head"] is emb
    for ly in w["layers"]:
        ly["wk"][:, A:] = 0.0
    g = pair_gains(name, w, gamma, cap)
    theta = rope_inv_freq(cfg)
    for ly in w["layers"]:
        wk = ly["wk"].reshape(Hk, D, H).astype(np.float64)
        wq = np.zeros((Hq, D, H), np.float64)
        for i in range(HALF):
            h = owner(name, i)
            t = OFFSETS[h] * theta[i] + (math.pi / 2 if name == "l3" and i >= L3_QUARTER else 0.0)
            a, b = wk[h // (Hq // Hk), i], wk[h // (Hq // Hk), i + HALF]
            wq[h, i] = g[i] * (a * math.cos(t) + b * math.sin(t))
            wq[h, i + HALF] = g[i] * (b * math.cos(t) - a * math.sin(t))
        ly["wq"] = _f16(wq.reshape(Hq * D, H))
    _WEIGHTS[name, gamma, cap] = w
    return w


def oracle(name: str, acc=np.float32, layers: int | None = None) -> OracleLlama:
    """``layers``: an oracle of the first layers only (the hidden rows after layer 1 need no layer 2)."""
    key = (name, np.dtype(acc).name, layers, GAMMA[name], CAP)
    if key not in _ORACLES:
        cfg, w = CONFIGS[name], weights(name)
        if layers is not None:
            cfg, w = cfg.with_(n_layers=layers), dict(w, layers=w["layers"][:layers])
        _ORACLES[key] = OracleLlama(cfg, w, acc=acc)
    return _ORACLES[key]


# ------------------------------------------------------------------ prompts
PREFILL_CASES = {n: {"P1": P1_LENS, "P2": P2_LENS} for n in RNAMES}
PREFILL_CASES["l3"] = {"P1": L3_P1_LENS, "L": (L3_LONG,)}
_CASE_SEED = {"P1": 9200, "P2": 9300, "L": 9400, "D": 9500, "F": 9600}


def _ids(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 4000, size=n).astype(np.int32)


def prefill_prompts(name: str, case: str) -> list:
    return [_ids(_CASE_SEED[case] + 17 * i + n, n) for i, n in enumerate(PREFILL_CASES[name][case])]


def decode_prompts() -> list:
    return [_ids(_CASE_SEED["D"] + 17 * i + n, n) for i, n in enumerate(DEC_LENS)]


def forced_ids() -> list:
    """The ids fed to decode steps 1..5 of each sequence."""
    return [[int(t) for t in _ids(_CASE_SEED["F"] + 17 * i, NPRED - 1)] for i in range(len(DEC_LENS))]


# ------------------------------------------------------------------ mutants
def _tables(cfg, pos, kind: str, i):
    """The cos / sin tables of a pair mutant over the positions ``pos``."""
    cos, sin = rope_tables(cfg, pos)
    cos, sin = cos.copy(), sin.copy()
    if kind.endswith("_freq"):
        cos[:, i], sin[:, i] = cos[:, i ^ 8].copy(), sin[:, i ^ 8].copy()
    else:
        sin[:, i] = -sin[:, i]
    return cos, sin


def q_mutant(name: str, kind: str, pos, i: int | None = None, qstart: int = 0) -> dict:
    """The ``mut`` of one Q-side mutant for a call whose new tokens sit at the positions ``pos``."""
    cfg, pos = CONFIGS[name], np.asarray(pos)
    if kind == "q_unrotated":
        return {"rope_q": lambda l, q, cos, sin: q}
    if kind in PAIR_MUTANTS:
        c, s = _tables(cfg, pos, kind, i)
    else:
        at = {"q_pos_minus": pos - 1, "q_pos_plus": pos + 1, "q_block_relative": pos % BLOCK,
              "q_pack_row": pos + qstart}[kind]
        c, s = rope_tables(cfg, at)
    return {"rope_q": lambda l, q, cos, sin: apply_rope(q, c, s, _f16)}


# ------------------------------------------------------------------ prefill references, floors, mutants
_PROBES = {}


def probes(name: str, prompt, acc=np.float32, mut=None, tag=None, layers=None) -> list:
    """Hidden rows after each layer, [n_layers][n][H] (cached by tokens; a mutant by ``tag``: not kept)."""
    key = (name, np.dtype(acc).name, tuple(int(t) for t in prompt), layers)
    if mut is not None:
        return oracle(name, acc, layers).forward(prompt, collect=True, mut=mut)[1]
    if key not in _PROBES:
        _PROBES[key] = oracle(name, acc, layers).forward(prompt, collect=True)[1]
    return _PROBES[key]


def prefill_floors(name: str) -> list:
    """Per layer: the largest fp32-vs-fp64 row distance over every sequence of every prefill case."""
    out = [0.0, 0.0]
    for case in PREFILL_CASES[name]:
        for p in prefill_prompts(name, case):
            a, b = probes(name, p), probes(name, p, np.float64)
            for l in range(2):
                out[l] = max(out[l], float(R.row_rel(a[l], b[l]).max()))
    return out


def _prefill_ratio(name: str, prompt, mut, bound, layers=None) -> float:
    base, got = probes(name, prompt, layers=layers), probes(name, prompt, mut=mut, layers=layers)
    return max(float(R.row_rel(got[l], base[l]).max()) / bound[l] for l in range(len(got)))


def main_prompt(name: str) -> np.ndarray:
    """The 300-token prompt of P1: the one the prefill mutants are scored on."""
    lens = PREFILL_CASES[name]["P1"]
    return prefill_prompts(name, "P1")[lens.index(300)]


def prefill_row_mutants(name: str, bound) -> dict:
    p = main_prompt(name)
    out = {k: _prefill_ratio(name, p, q_mutant(name, k, np.arange(len(p))), bound) for k in ROW_MUTANTS}
    if "P2" in PREFILL_CASES[name]:
        qs, best = 0, 0.0
        for s in prefill_prompts(name, "P2"):
            if qs:
                best = max(best, _prefill_ratio(name, s, q_mutant(name, "q_pack_row", np.arange(len(s)), qstart=qs), bound))
            qs += len(s)
        out["q_pack_row"] = best
    return out


def prefill_pair_mutants(name: str, bound, pairs=range(HALF), long: bool = False) -> dict:
    """kind -> {pair: ratio}.  ``long``: l3's 2048-token prompt, read after layer 1 only."""
    p = prefill_prompts(name, "L")[0] if long else main_prompt(name)
    layers = 1 if long else None
    return {k: {int(i): _prefill_ratio(name, p, q_mutant(name, k, np.arange(len(p)), i), bound, layers) for i in pairs}
            for k in PAIR_MUTANTS}


# ------------------------------------------------------------------ decode
_DEC = {}


def decode_reference(name: str, acc=np.float32) -> list:
    """Per sequence: decode_edges_ref.run_sequence fed the forced ids."""
    key = (name, np.dtype(acc).name)
    if key not in _DEC:
        _DEC[key] = [R.run_sequence(oracle(name, acc), p, feed=f, steps=NPRED) for p, f in zip(decode_prompts(), forced_ids())]
    return _DEC[key]


def decode_floors(name: str) -> dict:
    out = {f: 0.0 for f in R.FAMILIES}
    for a, b in zip(decode_reference(name), decode_reference(name, np.float64)):
        for f, d in R.distances(a, b).items():
            out[f] = max(out[f], d)
    return out


def _decode_ratio(name: str, kind: str, i, bound: dict) -> float:
    """The largest tile-maxima distance / bound over (sequence, step) with the fault in that step alone."""
    o = oracle(name)
    best = 0.0
    for p, ref in zip(decode_prompts(), decode_reference(name)):
        for j in range(1, NPRED):
            P = len(p) + j - 1
            cache = {"k": [k[:P] for k in ref["k"]], "v": [v[:P] for v in ref["v"]], "len": P}
            lg, _ = o.forward([ref["fed"][j - 1]], cache, mut=q_mutant(name, kind, [P], i))
            d = R.rel(R.tile_max(R._unscaled(o, lg)), R.tile_max(ref["unscaled"][j]))
            best = max(best, d / bound["tilemax"])
    return best


def decode_mutants(name: str, bound: dict) -> dict:
    out = {k: _decode_ratio(name, k, None, bound) for k in ROW_MUTANTS}
    for k in PAIR_MUTANTS:
        out[k] = {i: _decode_ratio(name, k, i, bound) for i in range(HALF)}
    return out


def k_mutants(name: str, bound: dict) -> dict:
    """kind -> {pair: ratio}: the K rows a faulty writer writes from the reference's un-rotated keys (both
    layers, every position of the longest decode sequence) against the reference's, / the K bound."""
    cfg = CONFIGS[name]
    at = int(np.argmax(DEC_LENS))
    p, fed = decode_prompts()[at], forced_ids()[at]
    ids = np.concatenate([p, np.asarray(fed, np.int32)])
    raw = {}

    def grab(l, k, v):
        raw[l] = k
        return apply_rope(k, *rope_tables(cfg, np.arange(len(ids))), _f16), v
    oracle(name).forward(ids, mut={"new_kv": grab})
    base = [apply_rope(raw[l], *rope_tables(cfg, np.arange(len(ids))), _f16) for l in range(cfg.n_layers)]
    out = {}
    for kind in K_MUTANTS:
        out[kind] = {}
        for i in range(HALF):
            c, s = _tables(cfg, np.arange(len(ids)), kind, i)
            out[kind][i] = max(float(R.row_rel(apply_rope(raw[l], c, s, _f16), base[l]).max())
                               for l in range(cfg.n_layers)) / bound["k"]
    return out


# ------------------------------------------------------------------ the recorded numbers
def config_numbers(name: str) -> dict:
    """What tests/golden/rope_pairs_bounds.json records for one config."""
    cfg = CONFIGS[name]
    fl = prefill_floors(name)
    bnd = [MARGIN * f for f in fl]
    pre = {"floor": fl, "bound": bnd, "row_mutants": prefill_row_mutants(name, bnd)}
    out = {"gamma": GAMMA[name], "cap": CAP, "rope_theta": cfg.rope_theta, "rope_factor": cfg.rope_factor,
           "offsets": list(OFFSETS[:cfg.n_heads]), "prefill": pre}
    lst = lambda d: {k: [v[i] for i in sorted(v)] for k, v in d.items()}  # noqa: E731
    if name == "l3":
        short = prefill_pair_mutants(name, bnd, L3_BANDS["unscaled"])
        long = prefill_pair_mutants(name, bnd, L3_LONG_PAIRS, long=True)
        pre["pair_mutants"] = {k: {str(i): r for i, r in {**short[k], **long[k]}.items()} for k in PAIR_MUTANTS}
        pre["reached"] = {k: [int(i) for i, r in pre["pair_mutants"][k].items() if r >= MUTANT_RATIO] for k in PAIR_MUTANTS}
        return out
    pre["pair_mutants"] = lst(prefill_pair_mutants(name, bnd))
    dfl = decode_floors(name)
    dbnd = {f: MARGIN * dfl[f] for f in R.FAMILIES}
    dm = decode_mutants(name, dbnd)
    out["decode"] = {"floor": dfl, "bound": dbnd, "forced": forced_ids(),
                     "row_mutants": {k: dm[k] for k in ROW_MUTANTS}, "pair_mutants": lst({k: dm[k] for k in PAIR_MUTANTS}),
                     "k_mutants": lst(k_mutants(name, dbnd))}
    return out


def write_golden() -> None:
    """Regenerate the file, by hand after a deliberate change of the model, the cases or the oracle
    (with the repository root, the package directory and tests/ on sys.path:
    python tests/rope_pairs_ref.py --record)."""
    out = {"configs": {name: config_numbers(name) for name in CONFIGS}}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    _GOLDEN.clear()


def survey(names=RNAMES, gammas=(3.0, 6.0), caps=(6.0,)) -> None:
    """How the constants were chosen: per config, gamma and cap the floors and the smallest pair ratios."""
    global CAP
    for name in names:
        for g in gammas:
            for c in caps:
                saved = GAMMA[name], CAP
                GAMMA[name], CAP = g, c
                _PROBES.clear(), _DEC.clear()
                try:
                    p = main_prompt(name)
                    a, b = probes(name, p), probes(name, p, np.float64)
                    bnd = [MARGIN * float(R.row_rel(a[l], b[l]).max()) for l in range(2)]
                    pm = prefill_pair_mutants(name, bnd, range(0, HALF, 1) if name != "l3" else L3_BANDS["unscaled"])
                    line = f"{name} gamma {g} cap {c}: prefill bound {bnd[0]:.2e} {bnd[1]:.2e} rows " + \
                           " ".join(f"{k} {v:.1f}" for k, v in prefill_row_mutants(name, bnd).items())
                    for k, v in pm.items():
                        i = min(v, key=v.get)
                        line += f" | {k} min {v[i]:.2f} (pair {i}) median {np.median(list(v.values())):.1f}"
                    if name != "l3":
                        dfl = decode_floors(name)
                        dbnd = {f: MARGIN * dfl[f] for f in R.FAMILIES}
                        dm = decode_mutants(name, dbnd)
                        line += f" || decode bound {dbnd['tilemax']:.2e} " + " ".join(f"{k} {dm[k]:.1f}" for k in ROW_MUTANTS)
                        for k in PAIR_MUTANTS:
                            i = min(dm[k], key=dm[k].get)
                            line += f" | {k} min {dm[k][i]:.2f} (pair {i})"
                        km = k_mutants(name, dbnd)
                        line += " | k " + " ".join(f"{k} {min(v.values()):.1f}" for k, v in km.items())
                    print(line, flush=True)
                finally:
                    GAMMA[name], CAP = saved
                    _PROBES.clear(), _DEC.clear()


if __name__ == "__main__":
    if "--survey" in sys.argv:
        survey()
    elif "--record" in sys.argv:
        write_golden()
