"""CPU restatement of libmapsum's sampler (include/mapsum.h ms_sampling, csrc/k_sample.hip):
repeat penalty -> top-k -> top-p -> min-p -> temperature -> one counter-based draw.

The logits are fp32 values and so is a penalised logit: ``l / rp`` and ``l * rp`` are single
IEEE fp32 operations (numpy float32 here, __fdiv_rn / __fmul_rn on the device), so a penalised
value ties with an unpenalised one in the reference exactly when it does in the kernel.
Everything after the penalty -- the order, the softmaxes, the cumulative sums, the draw -- is
float64.  The random numbers are exact integer arithmetic.

Also the deterministic input generator of the GPU tests (``make_case``): it redraws, on the
CPU, any case whose own top-p / min-p boundary margin is under 1e-4, so no GPU test skips."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

M64 = (1 << 64) - 1
MAX_TOPK, MAX_WINDOW = 256, 256
MARGIN = 1e-4      # a case whose top-p / min-p boundary is closer than this is redrawn
U_EXCUSE = 1e-5    # a draw whose u is this close to a reference CDF boundary is not compared


def mix64(z: int) -> int:
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u(seed: int, step: int) -> float:
    return (mix64((mix64(seed) + 0x9E3779B97F4A7C15 * (step + 1)) & M64) >> 40) * 2.0 ** -24


@dataclass(frozen=True)
class Params:
    temperature: float = 0.8
    top_k: int = 40
    top_p: float = 0.9
    min_p: float = 0.0
    repeat_penalty: float = 1.1
    repeat_last_n: int = 64
    seed: int = 0

    def f32(self):
        """The fields as the device reads them (fp32)."""
        return (np.float32(self.temperature), np.float32(self.top_p), np.float32(self.min_p),
                np.float32(self.repeat_penalty))


@dataclass
class Candidates:
    ids: np.ndarray     # final candidates in (logit desc, id asc) order
    probs: np.ndarray   # softmax(l / T) over them
    cdf: np.ndarray
    margin: float       # distance of the nearest top-p (probability) / min-p (logit) boundary


def _finite_max(l):
    ok = ~np.isnan(l)
    if not ok.any():
        return None
    m = l[ok].max()
    return m if np.isfinite(m) else None


def candidates(logits, p: Params, window) -> Candidates | None:
    """None when the row yields -1 (its largest non-NaN logit is not finite)."""
    l32 = np.array(logits, dtype=np.float32, copy=True)
    n = l32.size
    T, top_p, min_p, rp = p.f32()
    if not T > 0:  # greedy: the plain argmax, ties to the lowest id
        m = _finite_max(l32)
        if m is None:
            return None
        return Candidates(np.array([int(np.flatnonzero(l32 == m)[0])]), np.ones(1), np.ones(1), np.inf)
    w = [int(t) for t in list(window)[-min(p.repeat_last_n, MAX_WINDOW):]] if p.repeat_last_n > 0 else []
    ids = np.unique([t for t in w if 0 <= t < n]).astype(np.int64)
    if ids.size and rp != 1:
        v = l32[ids]
        with np.errstate(all="ignore"):
            l32[ids] = np.where(v > 0, v / rp, v * rp).astype(np.float32)
    m = _finite_max(l32)
    if m is None:
        return None
    l = l32.astype(np.float64) + 0.0  # -0 -> +0
    valid = np.flatnonzero(~np.isnan(l))
    order = valid[np.lexsort((valid, -l[valid]))]  # logit descending, id ascending
    c = order[:min(p.top_k, order.size)]
    lc = l[c]
    margin = np.inf
    with np.errstate(all="ignore"):
        if top_p < 1:
            q = np.exp(lc - m)
            cum = np.cumsum(q / q.sum())
            hit = np.flatnonzero(cum >= float(top_p))
            keep = int(hit[0]) + 1 if hit.size else c.size
            margin = min(margin, float(np.abs(cum[:-1] - float(top_p)).min()) if c.size > 1 else np.inf)
            c, lc = c[:keep], lc[:keep]
        if min_p > 0:
            thr = m + np.log(float(min_p))
            keep = max(1, int((lc >= thr).sum()))
            margin = min(margin, float(np.abs(lc[1:] - thr).min()) if lc.size > 1 else np.inf)
            c, lc = c[:keep], lc[:keep]
        e = np.exp((lc - m) / float(T))
    probs = e / e.sum()
    return Candidates(c, probs, np.cumsum(probs), margin)


def draw(cand: Candidates | None, uu: float) -> int:
    if cand is None:
        return -1
    hit = np.flatnonzero(cand.cdf > uu)
    return int(cand.ids[hit[0] if hit.size else -1])


def excused(cand: Candidates | None, uu: float) -> bool:
    """u within U_EXCUSE of a reference CDF boundary: fp32 cumulative sums may land on either side."""
    return cand is not None and bool((np.abs(cand.cdf - uu) < U_EXCUSE).any())


def sample(logits, p: Params, window, step: int) -> int:
    return draw(candidates(logits, p, window), u(p.seed, step))


# ------------------------------------------------------------------ test inputs
def make_logits(rng, n: int, quantised) -> np.ndarray:
    if quantised == "coarse":  # four values: a quarter of the row ties at the top
        return rng.integers(-1, 3, size=n).astype(np.float32)
    l = (rng.standard_normal(n) * 3.0).astype(np.float32)
    if quantised:  # multiples of 0.25: the k-th boundary is full of ties
        l = (np.round(l * 4.0) / 4.0).astype(np.float32)
    return l


def make_window(rng, logits: np.ndarray, length: int = 300) -> np.ndarray:
    """History ids with duplicates, on both positive and negative logits, among the largest
    logits (where the penalty changes the candidate set) and anywhere else."""
    n = logits.size
    order = np.argsort(-logits, kind="stable")
    top = order[:min(64, n)]
    pos = np.flatnonzero(logits > 0)
    neg = np.flatnonzero(logits < 0)
    parts = [rng.choice(top, size=length // 3), rng.integers(0, n, size=length // 3)]
    if pos.size and neg.size:
        parts += [rng.choice(pos, size=length // 6), rng.choice(neg, size=length // 6)]
    w = np.concatenate(parts)
    w = np.concatenate([w, w[:length - w.size] if w.size < length else w[:0]])[:length]
    rng.shuffle(w)
    w[-1] = w[-3]  # a duplicate inside even the shortest window
    return w.astype(np.int32)


def make_case(seed: int, n: int, psets, quantised: bool, max_redraws: int = 16):
    """rows = len(psets) rows of logits + windows whose reference boundaries all keep MARGIN.
    Returns (logits [rows][n] fp32, windows [rows][300] int32, [Candidates], redraws)."""
    rows = len(psets)
    logits = np.empty((rows, n), np.float32)
    wins = np.empty((rows, 300), np.int32)
    cands, redraws = [], 0
    for r, p in enumerate(psets):
        for attempt in range(max_redraws + 1):
            rng = np.random.default_rng([seed, n, r, 2 if quantised == "coarse" else int(quantised), attempt])
            l = make_logits(rng, n, quantised)
            w = make_window(rng, l)
            c = candidates(l, p, w)
            if c is not None and c.margin >= MARGIN:
                break
            redraws += 1
        else:
            raise AssertionError(f"case {(seed, n, r, quantised)} needs more than {max_redraws} redraws")
        logits[r], wins[r] = l, w
        cands.append(c)
    return logits, wins, cands, redraws


# ------------------------------------------------------------------ the GPU tests' cases
# parameter sets (row r of a case takes PSETS[(r + offset) % 8])
PSETS = [
    Params(0.8, 40, 0.9, 0.0, 1.1, 64),       # Ollama's defaults
    Params(0.7, 1, 0.9, 0.0, 1.0, 64),        # top_k = 1
    Params(1.3, 256, 1.0, 0.0, 1.3, 256),     # the largest k and window, top-p / min-p off
    Params(1.0, 256, 0.95, 0.05, 1.1, 64),    # every stage on
    Params(0.5, 40, 0.5, 0.0, 0.8, 16),       # a penalty below 1 (a reward)
    Params(0.8, 40, 1e-6, 0.0, 1.1, 64),      # top_p small enough for one candidate
    Params(1.0, 100, 1.0, 0.3, 1.1, 0),       # min-p alone, the penalty off by its window
    Params(0.0, 40, 0.9, 0.0, 1.1, 64),       # greedy
]
OP_SHAPES = [(n, rows, q) for n in (1000, 4097, 128256) for rows in (1, 3, 8) for q in (False, True)]
DRAW_CASES = [(pi, q) for pi in (0, 2, 3, 4) for q in (False, True)]
DRAWS = 2048


def with_seed(p: Params, seed: int) -> Params:
    return Params(p.temperature, p.top_k, p.top_p, p.min_p, p.repeat_penalty, p.repeat_last_n, seed)


def op_case(n: int, rows: int, quantised: bool):
    """(psets, logits, windows, candidates, steps, redraws) of one candidate-set case."""
    off = {1000: 0, 4097: 3, 128256: 5}[n] + rows
    psets = [with_seed(PSETS[(r + off) % 8], 1000 * n + r) for r in range(rows)]
    logits, wins, cands, redraws = make_case(11, n, psets, quantised)
    steps = [(7 * r + n) % 97 for r in range(rows)]
    return psets, logits, wins, cands, steps, redraws


# rows full of ties (and far more values at the top than the sampler keeps in LDS): the exact
# radix select and the id-ordered tie scan decide the candidates
TIE_PSETS = [Params(1.3, 256, 1.0, 0.0, 1.3, 256, 31), Params(0.8, 40, 0.93, 0.0, 1.1, 64, 32),
             Params(1.0, 100, 1.0, 0.3, 1.1, 0, 33), Params(0.9, 7, 1.0, 0.0, 0.7, 200, 34)]


def tie_case(n: int):
    logits, wins, cands, redraws = make_case(19, n, TIE_PSETS, "coarse")
    return TIE_PSETS, logits, wins, cands, [3, 0, 9, 1], redraws


def draw_case(pi: int, quantised: bool, n: int = 4097):
    """One logits row and DRAWS (seed, step) pairs for parameter set pi:
    (params, logits [1][n], window, candidates, seeds, steps, redraws)."""
    logits, wins, cands, redraws = make_case(13 + pi, n, [PSETS[pi]], quantised)
    rng = np.random.default_rng([21, pi, int(quantised)])
    seeds = rng.integers(0, 1 << 63, size=DRAWS, dtype=np.int64)
    seeds[:4] = [0, 1, (1 << 63) - 1, 2]
    steps = rng.integers(0, 4096, size=DRAWS)
    steps[:4] = [0, 0, 5, 1]
    return PSETS[pi], logits, wins[0], cands[0], seeds, steps, redraws
