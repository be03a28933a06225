"""CPU side of tests/test_gpu_decode_edges.py: the cases, their references, noise floors,
bounds and the deliberately wrong references ("mutants") that show the bounds can tell a
faulty decode kernel from a correct one.  Plain helper, no test in here.

Reference: OracleLlama in mode "engine" (the engine's rounding points) over the case's prompts,
decoding one token per call exactly as the engine's decode steps do: step 0 is the prefill's
first token, step j >= 1 feeds token j-1 at position n + j - 1 and attends to n + j keys.

Noise floor of an observable: the distance between the oracle accumulating in fp32 and the same
oracle accumulating in fp64 (same tokens, same rounding points).  Nothing here comes from a GPU.
Bound = MARGIN (4) x the largest floor of the observable's family; a family is one observable
kind (tile maxima, full logits, K rows, V rows) of one case, over all its sequences and steps.
The GPU sums in a third order (MFMA blocks, split-K slabs, online softmax per page), independent
of both references: about sqrt(2) x the floor is expected, with a heavy tail from fp16 rounding
flips, hence 4.

Model: TINY with tests/test_gpu_parity.py's seed and norm jitter but synthetic std 0.03, not
its 0.05.  The floor is set by the fp16 rounding points (a flip of one q / k / v element moves a
score by ~1e-4, and every later rounding multiplies the flips), ~4e-4 on the tile maxima whatever
the std or the length.  One key of 1,600 must move the logits by 8x that.  Measured on the CPU
with the oracle alone: at std 0.05 the 1,590-key rows of cases a / h reach only 1.8x the bound
for a dropped split-first key; a LARGER std sharpens attention and a random key then weighs
nothing (ratio 0.0 at std 0.1); a flatter attention (std 0.02) weighs every key 1/n but makes
two swapped V rows invisible (0.25).  Between them, 0.03 leaves every mutant >= 6.6x where the
pools are read and 2.5x in f, and every dropped key >= 2.1x at every single step.  Also tried at
std 0.05, on case a: other prompt seeds (its smallest ratio is 1.8 with the seed used here, 3.5 /
3.2 / 4.5 with three others) and n_layers=1 (4.1).  So 0.05 can meet the condition too, by the
draw of a seed, at about half of 0.03's margin and with single steps below 1x.

Observables
  tilemax   the 256 per-16-column maxima of the un-scaled lm_head sums of one row (what the greedy
            lm_head leaves in the decode logits buffer), relative L2 over the row;
  logits    the full scaled fp32 logits row (a sampling run, and the prefill's first token);
  k, v      one cached row (layer, position, kv head), relative L2 over head_dim.

Mutants (every sequence of every case; MUTANT_KINDS): one key dropped from what the step
attends to -- the first key, the first key of every split of the case's kernels, the first key
of the last page, the last cached key, the new token itself --, two adjacent V rows swapped, the
new token roped at pos - 1 / pos + 1, its K/V taken from the other kv head, its K row read
un-permuted (kernels.h rope_perm skipped).  A mutant is one such fault in one sequence, present at
every decode step; its ratio is the largest distance / bound over what the case asserts for that
sequence and nothing else (mutant_ratios: f reads no pool, g reads the partials after every third
step); every ratio must be >= MUTANT_RATIO (2).  With every single step a mutant of its own the
condition still holds but for the swapped V rows and, in f, the wrongly written rows (per_step).
"""
from __future__ import annotations

import json
import os

import numpy as np

from mapsum.config import TINY
from oracle.llama_ref import OracleLlama, _f16, apply_rope, rope_tables
from oracle.synth import make_weights

SEED, STD, JITTER = 1234, 0.03, 0.1  # tests/test_gpu_parity.py's model but for STD (module docstring)
NPRED = 10
PAGE = 64
MARGIN = 4.0
MUTANT_RATIO = 2.0
FAMILIES = ("tilemax", "logits", "k", "v")
MUTANT_KINDS = ("drop_first", "drop_split_first", "drop_page_first", "drop_last_cached", "drop_new",
                "swap_v", "rope_pos_minus", "rope_pos_plus", "other_kv_head", "unpermuted")

_LENS_A = (1, 60, 64, 250, 570, 1590)
_LENS_E = (1, 5, 17, 33, 50, 55, 56, 58, 60, 62, 63, 64, 65, 70, 90, 110, 118, 120, 122, 126, 127, 128, 130, 1590)

# name -> engine shape, prompt lengths (the longest last, one per slot), the prompt set's key
# (cases that share it share one reference), the keys per split of every kernel variant the case
# runs (v2: ppb pages, v1: 4 * ppw pages) and what it asserts: the logits observable, the decode
# steps after which the test reads it (default: every step) and whether it reads the K / V pools
ALL_STEPS = tuple(range(1, NPRED))
CASES = {
    "a": dict(max_batch=6, max_ctx=1600, n_pages=0, lens=_LENS_A, pset="A", split_keys=(256, 576), obs="tilemax"),
    "b": dict(max_batch=6, max_ctx=1600, n_pages=0, lens=(1, 60, 250, 506, 1019, 1590), pset="B",
              split_keys=(512, 256), obs="tilemax"),
    "c": dict(max_batch=6, max_ctx=1600, n_pages=0, lens=_LENS_A, pset="A", split_keys=(256,), obs="tilemax"),
    "d": dict(max_batch=4, max_ctx=1000, n_pages=0, lens=(3, 120, 500, 990), pset="D", split_keys=(256, 512),
              obs="tilemax"),
    "e": dict(max_batch=24, max_ctx=1600, n_pages=0, lens=_LENS_E, pset="E", split_keys=(512,), obs="tilemax"),
    "f": dict(max_batch=6, max_ctx=512, n_pages=20, lens=(3, 61, 64, 65, 300, 440), pset="F", split_keys=(512,),
              obs="tilemax", pools=False),
    "g": dict(max_batch=6, max_ctx=1600, n_pages=0, lens=_LENS_A, pset="A", split_keys=(576,), obs="tilemax",
              steps=(3, 6, 9)),
    "h": dict(max_batch=6, max_ctx=1600, n_pages=0, lens=_LENS_A, pset="A", split_keys=(256,), obs="logits"),
}
for _c in CASES.values():
    _c.setdefault("steps", ALL_STEPS)
    _c.setdefault("pools", True)
WRITE_KINDS = ("rope_pos_minus", "rope_pos_plus", "other_kv_head", "unpermuted")  # faults in the new token's K/V row
_PSET_SEED = {"A": 7100, "B": 7200, "D": 7300, "E": 7400, "F": 7500}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_edges_bounds.json")
_GOLDEN = {}


def golden() -> dict:
    """tests/golden/decode_edges_bounds.json: per case the floors, bounds and smallest mutant ratios,
    per prompt set the forced ids (the fp32 oracle's greedy tokens where the file was written: a
    near-tie must not turn into other tokens, and other numbers, under another BLAS)."""
    if not _GOLDEN:
        with open(GOLDEN) as f:
            _GOLDEN.update(json.load(f))
    return _GOLDEN


def rel(a, b) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def row_rel(a, b) -> np.ndarray:
    """Relative L2 over the last axis, per row."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.maximum(np.linalg.norm(b, axis=-1), 1e-30)


def tile_max(row) -> np.ndarray:
    return np.asarray(row).reshape(-1, 16).max(axis=1)


def prompts(case: str) -> list:
    c = CASES[case]
    return [np.random.default_rng(_PSET_SEED[c["pset"]] + 13 * i + n).integers(0, 4000, size=n).astype(np.int32)
            for i, n in enumerate(c["lens"])]


_ORACLES = {}


def oracle(acc=np.float32) -> OracleLlama:
    key = np.dtype(acc).name
    if key not in _ORACLES:
        _ORACLES[key] = OracleLlama(TINY, make_weights(TINY, SEED, std=STD, jitter=JITTER), acc=acc)
    return _ORACLES[key]


def _unscaled(o: OracleLlama, logits) -> np.ndarray:
    return (logits / o.last_rinv.reshape(())).astype(np.float32)


def run_sequence(o: OracleLlama, prompt, feed=None, steps: int = NPRED) -> dict:
    """Prefill + steps - 1 decode steps.  ``feed``: the ids fed to the decode steps (feed[j-1]
    at step j), default the oracle's own greedy choices.  Returns tokens [steps] (the argmax of
    every step), logits / unscaled [steps][V], and the cache (k / v: per layer [n+steps-1, Hk, D])."""
    cache = o.new_cache()
    lg, _ = o.forward(prompt, cache)
    logits, unscaled, toks = [lg], [_unscaled(o, lg)], [int(np.argmax(lg))]
    for j in range(1, steps):
        t = toks[j - 1] if feed is None else int(feed[j - 1])
        lg, _ = o.forward([t], cache)
        logits.append(lg)
        unscaled.append(_unscaled(o, lg))
        toks.append(int(np.argmax(lg)))
    return {"tokens": toks, "fed": [toks[j] if feed is None else int(feed[j]) for j in range(steps - 1)],
            "logits": np.stack(logits), "unscaled": np.stack(unscaled), "k": cache["k"], "v": cache["v"]}


_REFS = {}


def reference(case: str, acc=np.float32, fresh: bool = False) -> list:
    """Per sequence of the case: run_sequence fed the recorded forced ids (``fresh``: the fp32
    oracle's own greedy tokens, for writing the file)."""
    pset = CASES[case]["pset"]
    key = (pset, np.dtype(acc).name)
    if key not in _REFS:
        ps = prompts(case)
        if fresh and np.dtype(acc) == np.float32:
            _REFS[key] = [run_sequence(oracle(), p) for p in ps]
        else:
            fed = [b["fed"] for b in _REFS[pset, "float32"]] if fresh else golden()["forced"][pset]
            _REFS[key] = [run_sequence(oracle(acc), p, feed=f) for p, f in zip(ps, fed)]
    return _REFS[key]


def distances(got: dict, ref: dict) -> dict:
    """The largest distance of each family between two run_sequence results of one sequence."""
    return {"tilemax": max(rel(tile_max(g), tile_max(r)) for g, r in zip(got["unscaled"], ref["unscaled"])),
            "logits": max(rel(g, r) for g, r in zip(got["logits"], ref["logits"])),
            "k": max(float(row_rel(g, r).max()) for g, r in zip(got["k"], ref["k"])),
            "v": max(float(row_rel(g, r).max()) for g, r in zip(got["v"], ref["v"]))}


def floors(case: str) -> dict:
    """family -> the largest fp32-vs-fp64 oracle distance over the case's sequences and steps;
    plus "k_layer0" / "v_layer0", the same over layer 0's rows alone (recorded, not a bound)."""
    r32, r64 = reference(case), reference(case, np.float64)
    out = {f: 0.0 for f in FAMILIES}
    for a, b in zip(r32, r64):
        for f, d in distances(a, b).items():
            out[f] = max(out[f], d)
    for kv in ("k", "v"):
        out[kv + "_layer0"] = max(float(row_rel(a[kv][0], b[kv][0]).max()) for a, b in zip(r32, r64))
    return out


def bounds(fl: dict) -> dict:
    return {f: MARGIN * fl[f] for f in FAMILIES}


# ------------------------------------------------------------------ mutants
def _inv_rope_perm() -> np.ndarray:
    """raw[rope_perm(d)] holds logical dim d (kernels.h rope_perm), so reading raw[i] in place
    of raw[rope_perm(i)] returns logical dim rope_perm^-1(i)."""
    i = np.arange(128)
    perm = np.where(i < 64, 16 * (i >> 3) + (i & 7), 16 * ((i - 64) >> 3) + 8 + ((i - 64) & 7))
    return np.argsort(perm)


def _mutations(P: int, split_keys) -> list:
    """(kind, boundary, mut) for a decode step whose new token sits at position P >= 1; boundary
    is the dropped key of a split-first mutant (one mutant per split boundary), else 0."""
    cfg = TINY

    def drop(idx):
        return {"attend": lambda l, k, v: (np.delete(k, idx, axis=0), np.delete(v, idx, axis=0))}

    def swap(i):
        def f(l, k, v):
            v = v.copy()
            v[[i, i + 1]] = v[[i + 1, i]]
            return k, v
        return {"attend": f}

    def rope_at(pos):
        cos, sin = rope_tables(cfg, [pos])
        return {"new_kv": lambda l, k, v: (apply_rope(k, cos, sin, _f16), v)}

    cos, sin = rope_tables(cfg, [P])
    perm = _inv_rope_perm()
    out = [("drop_first", 0, drop(0)), ("drop_last_cached", 0, drop(P - 1)), ("drop_new", 0, drop(P)),
           ("swap_v", 0, swap(min(P // 2, P - 1))), ("rope_pos_minus", 0, rope_at(P - 1)),
           ("rope_pos_plus", 0, rope_at(P + 1)),
           ("other_kv_head", 0, {"new_kv": lambda l, k, v: (apply_rope(k[:, ::-1], cos, sin, _f16), v[:, ::-1])}),
           ("unpermuted", 0, {"new_kv": lambda l, k, v: (apply_rope(k[..., perm], cos, sin, _f16), v)})]
    firsts = sorted({m for s in split_keys for m in range(s, P, s)})
    out += [("drop_split_first", m, drop(m)) for m in firsts]
    page = (P - 1) // PAGE * PAGE  # of the last cached key; the new token's own page starts at itself or there
    if page:
        out.append(("drop_page_first", 0, drop(page)))
    return out


_MUTANTS = {}


def _mutant_distances(pset: str) -> list:
    """(sequence, kind, boundary, step, {family: distance}) of every mutant instance of a prompt set, at
    every decode step, over the split boundaries of all the cases that share the set."""
    if pset in _MUTANTS:
        return _MUTANTS[pset]
    o = oracle()
    case = next(c for c in CASES if CASES[c]["pset"] == pset)
    split_keys = sorted({s for c in CASES.values() if c["pset"] == pset for s in c["split_keys"]})
    out = []
    for i, ref in enumerate(reference(case)):
        n = ref["k"][0].shape[0] - (NPRED - 1)
        for j in range(1, NPRED):
            P = n + j - 1
            prior = {"k": [k[:P] for k in ref["k"]], "v": [v[:P] for v in ref["v"]], "len": P}
            base = {"unscaled": ref["unscaled"][j:j + 1], "logits": ref["logits"][j:j + 1],
                    "k": [k[P:P + 1] for k in ref["k"]], "v": [v[P:P + 1] for v in ref["v"]]}
            for kind, where, mut in _mutations(P, split_keys):
                cache = dict(prior, k=list(prior["k"]), v=list(prior["v"]))
                lg, _ = o.forward([ref["fed"][j - 1]], cache, mut=mut)
                got = {"unscaled": _unscaled(o, lg)[None], "logits": lg[None],
                       "k": [k[P:P + 1] for k in cache["k"]], "v": [v[P:P + 1] for v in cache["v"]]}
                out.append((i, kind, where, j, distances(got, base)))
    _MUTANTS[pset] = out
    return out


def mutant_ratios(case: str, bnd: dict, per_step: bool = False) -> dict:
    """kind -> the smallest ratio over the case's mutants of that kind.  One mutant is one fault in
    one sequence (length) of the case -- for a dropped split-first key, at one split boundary of
    the case's kernels -- present at every decode step it can occur at, as a faulty kernel's would
    be; its ratio is the largest distance / bound over what the case asserts for that sequence and
    nothing else: the case's logits observable at the steps after which the test reads it
    (CASES "steps": every step of a forced run, every third of the chained run g), and the K / V
    rows where the test reads the pools (not f).  The test asserts each of these, so one past
    its bound fails it.  Kinds a case has no instance of (no split boundary below its longest
    context) are absent.

    ``per_step``: the stricter figure, every decode step whose logits observable the case reads
    a mutant of its own (the smallest ratio over single steps).  Every kind holds >= MUTANT_RATIO
    that way too, but for: swap_v -- two swapped V rows move the output by (p_i - p_j)(v_j - v_i),
    nothing at a step where the two keys weigh the same, so that fault shows at the steps where
    they do not (the pair moves every other step) --, and the WRITE_KINDS in f, where the wrong row
    cannot be read and shows only through the logits of the steps at which its key weighs enough."""
    c = CASES[case]
    best = {}  # (sequence, kind, boundary[, step]) -> largest ratio
    for i, kind, where, j, d in _mutant_distances(c["pset"]):
        if kind == "drop_split_first" and not any(where % s == 0 for s in c["split_keys"]):
            continue
        if per_step and j not in c["steps"]:
            continue
        fams = ((c["obs"],) if j in c["steps"] else ()) + (("k", "v") if c["pools"] else ())
        ratio = max((d[f] / bnd[f] for f in fams), default=0.0)
        key = (i, kind, where, j) if per_step else (i, kind, where)
        best[key] = max(best.get(key, 0.0), ratio)
    out = {}
    for key, ratio in best.items():
        out[key[1]] = min(out.get(key[1], np.inf), ratio)
    return {k: float(v) for k, v in out.items()}


def case_numbers(case: str) -> dict:
    """What tests/golden/decode_edges_bounds.json records for one case."""
    fl = floors(case)
    bnd = bounds(fl)
    return {"floor": fl, "bound": bnd, "mutant_ratio": mutant_ratios(case, bnd),
            "mutant_ratio_step": mutant_ratios(case, bnd, per_step=True)}


def write_golden() -> None:
    """Regenerate the file, by hand after a deliberate change of the cases or the oracle (with the
    repository root, the package directory and tests/ on sys.path:
    python -c "import decode_edges_ref as R; R.write_golden()")."""
    for c in CASES:
        reference(c, fresh=True)
    forced = {CASES[c]["pset"]: [r["fed"] for r in reference(c)] for c in CASES}
    _GOLDEN.update({"forced": forced})
    out = {"forced": forced, "cases": {c: case_numbers(c) for c in CASES}}
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    _GOLDEN.clear()
