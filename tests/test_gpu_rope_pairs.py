"""RoPE pair by pair: every place that rotates Q (and writes a rotated K row), on a model whose
attention weights depend on relative position only (needs a GPU).

The model, configs, prompts, bounds and mutants are tests/rope_pairs_ref.py's (read its docstring
first): every token has the same un-rotated key, each head's query is that key turned back by the
head's offset on the pairs the head owns, so q(m) . k(n) = sum_i g_i |z_i|^2 cos((m - n - d_h) theta_i)
and one pair rotated with the wrong table column, the wrong sign of sin or the wrong position moves
the rows' outputs.  r3 / r8 / r1 use rope_theta = 64 without scaling, so all 64 pairs turn by radians
within 300 tokens; l3 is TINY's own llama3-scaled table.  Everything goes through hooks the engine
already has: load_logical, ms_forward_packed (hidden rows after 1 and 2 layers), submit_forced +
step, ms_debug_read.  The engine took rope_theta = 64 / rope_factor = 0 as given.

Prefill   (attn_prefill_kernel rotates Q while staging it; rope_kv_kernel writes K) every hidden row
          after layer 1 and after layer 2 within the config's bound of the fp32 oracle's row:
            P1  single prompts of (1, 17, 64, 129, 300, 700) tokens, one per call (l3: 300, 700),
            P2  one pack of lengths (1, 17, 64, 129, 65, 1, 320, 128),
            L   l3's 2048-token prompt.
Decode    per r* config six sequences of (1, 63, 64, 300, 200, 230) keys (the last two were added so
          that every pair meets the mutant condition through the decode steps alone: the survey in
          tests/rope_pairs_ref.py) and 5 forced steps: prefill logits, tile maxima + ids with the
          near-tie rule, K / V rows of both pools and stray writes (the helpers of
          tests/test_gpu_decode_edges.py), on every path that rotates Q differently:
            v2        6 slots, default: the v2 slab prologue;
            v1        MS_ATTN_V2=0: the v1 slab prologue;
            epilogue  MS_ATTN_SLABS=0: the QKV GEMV's ROPE_KV epilogue;
            large     24 slots (the six sequences and 18 idle slots): skinny-GEMM slabs + v1;
            unfused   24 slots and MS_ATTN_SLABS=0: rope_kv_kernel with rope_q.  Confirmed by reading
                      engine.cpp: 24 slots >= dgemm_min makes S.large() true, and fused_decode() then
                      returns "... && S.attn_slabs && ...", false under MS_ATTN_SLABS=0, so run_layer
                      takes the per-kernel branch, whose launch_rope_kv gets rope_q = decode.
          With theta = 64 the K-row assertions are the first that would see a wrong table column in
          pairs 32..63 of a K writer; they run on every path.  The persistent decode kernel cannot run
          at these shapes and is pinned bit-exact to the per-layer launches elsewhere.

The bounds are read from tests/golden/rope_pairs_bounds.json: 4 x the distance between the fp32- and
the fp64-accumulating oracle, none taken from a GPU.  tests/test_rope_pairs_ref.py shows on the CPU
that each mutant -- position +- 1, no rotation, a q-block-relative or packed-row position, and for
each of the 64 pairs the table column i ^ 8 or a negated sin, in Q or in the K writer -- sits at >= 2 x
these bounds.

Measured on an MI355X: the largest distance over all rows of the case / the bound, then the CPU
floor (fp32 vs fp64 oracle) and the config's smallest mutant ratio (the CPU test).  Every case passed
as stated, none is dropped and no kernel had to change.  Prefill distances are 0.9 - 1.5 x their
floors, decode 0.9 - 1.4 x; the largest fraction of a bound is 0.37 in prefill (r8 P1, after layer 1)
and 0.35 in decode (r1 K rows).

  prefill                after layer 1        after layer 2        floors (layer 1, 2)   smallest mutant
  r1  P1 (6 prompts)     7.02e-4 / 2.06e-3    8.32e-4 / 2.50e-3    5.16e-4, 6.25e-4      18.3 x (q_freq, pair 39)
  r1  P2 (pack of 8)     7.22e-4 / 2.06e-3    8.20e-4 / 2.50e-3
  r3  P1                 6.05e-4 / 1.95e-3    7.86e-4 / 2.75e-3    4.87e-4, 6.88e-4      20.5 x (q_conj, pair 59)
  r3  P2                 6.50e-4 / 1.95e-3    7.74e-4 / 2.75e-3
  r8  P1                 6.72e-4 / 1.81e-3    7.98e-4 / 2.78e-3    4.54e-4, 6.96e-4      23.1 x (q_conj, pair 61)
  r8  P2                 6.02e-4 / 1.81e-3    8.16e-4 / 2.78e-3
  l3  P1 (300, 700)      4.94e-4 / 2.00e-3    1.08e-3 / 4.95e-3    5.00e-4, 1.24e-3      4.6 x (q_conj, pairs 22, 23)
  l3  L (2048 tokens)    5.67e-4 / 2.00e-3    1.13e-3 / 4.95e-3                          16.5 x of pairs 29, 30

  decode        tile maxima        logits (prefill)   K rows             V rows             ids excused
  r1  v2        7.54e-4 / 3.52e-3  1.31e-3 / 4.69e-3  1.01e-3 / 2.86e-3  9.03e-4 / 2.72e-3  4 / 7680
  r1  v1        7.54e-4 / 3.52e-3  1.31e-3 / 4.69e-3  1.01e-3 / 2.86e-3  9.03e-4 / 2.72e-3  4 / 7680
  r1  epilogue  7.54e-4 / 3.52e-3  1.31e-3 / 4.69e-3  1.01e-3 / 2.86e-3  9.03e-4 / 2.72e-3  4 / 7680
  r1  large     1.02e-3 / 3.52e-3  1.31e-3 / 4.69e-3  1.01e-3 / 2.86e-3  9.03e-4 / 2.72e-3  3 / 7680
  r1  unfused   7.54e-4 / 3.52e-3  1.31e-3 / 4.69e-3  1.01e-3 / 2.86e-3  9.03e-4 / 2.72e-3  4 / 7680
  r3  v2        4.84e-4 / 1.65e-3  1.20e-3 / 3.58e-3  9.04e-4 / 3.16e-3  8.57e-4 / 2.63e-3  4 / 7680
  r3  v1        4.84e-4 / 1.65e-3  1.20e-3 / 3.58e-3  9.04e-4 / 3.16e-3  8.57e-4 / 2.63e-3  3 / 7680
  r3  epilogue  4.84e-4 / 1.65e-3  1.20e-3 / 3.58e-3  9.04e-4 / 3.16e-3  8.57e-4 / 2.63e-3  6 / 7680
  r3  large     5.32e-4 / 1.65e-3  1.20e-3 / 3.58e-3  9.04e-4 / 3.16e-3  8.57e-4 / 2.63e-3  3 / 7680
  r3  unfused   4.90e-4 / 1.65e-3  1.20e-3 / 3.58e-3  9.04e-4 / 3.16e-3  8.57e-4 / 2.63e-3  5 / 7680
  r8  v2        5.55e-4 / 1.90e-3  8.41e-4 / 3.64e-3  9.00e-4 / 2.84e-3  9.48e-4 / 3.04e-3  4 / 7680
  r8  v1        5.05e-4 / 1.90e-3  8.41e-4 / 3.64e-3  9.00e-4 / 2.84e-3  9.48e-4 / 3.04e-3  3 / 7680
  r8  epilogue  5.55e-4 / 1.90e-3  8.41e-4 / 3.64e-3  9.00e-4 / 2.84e-3  9.48e-4 / 3.04e-3  4 / 7680
  r8  large     4.85e-4 / 1.90e-3  8.41e-4 / 3.64e-3  9.00e-4 / 2.84e-3  9.48e-4 / 3.04e-3  3 / 7680
  r8  unfused   5.05e-4 / 1.90e-3  8.41e-4 / 3.64e-3  9.00e-4 / 2.84e-3  9.48e-4 / 3.04e-3  3 / 7680
  decode floors (tile maxima, logits, K, V) and smallest mutant (fault in the decode steps alone):
  r1  8.80e-4, 1.17e-3, 7.16e-4, 6.81e-4   5.1 x (q_conj, pair 51); K twins >= 99 x
  r3  4.13e-4, 8.94e-4, 7.91e-4, 6.58e-4   7.5 x (q_freq, pair 5);   K twins >= 68 x
  r8  4.76e-4, 9.11e-4, 7.09e-4, 7.61e-4   6.5 x (q_conj, pair 54);  K twins >= 60 x
The logits are the prefill's and so equal on every path, and the largest K / V distances did not
change with the path either; the tile maxima and the excused ids are the decode steps' own.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_edges_ref as R  # noqa: E402
import rope_pairs_ref as K  # noqa: E402
import test_gpu_decode_edges as DE  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from mapsum.engine import Engine  # noqa: E402
from mapsum.weights import load_logical  # noqa: E402

NSEQ = len(K.DEC_LENS)
PATHS = {"v2": (NSEQ, {}), "v1": (NSEQ, {"MS_ATTN_V2": 0}), "epilogue": (NSEQ, {"MS_ATTN_SLABS": 0}), "large": (24, {}),
         "unfused": (24, {"MS_ATTN_SLABS": 0})}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _engine(name, monkeypatch, env=None, max_batch=8, max_ctx=704, max_prefill_tokens=1024):
    for k in DE.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    e = Engine(K.CONFIGS[name], device=0, max_batch=max_batch, max_ctx=max_ctx, max_prefill_tokens=max_prefill_tokens)
    try:
        load_logical(e, K.weights(name))
    except Exception:
        e.close()
        raise
    return e


def _probe(e, prompts):
    """[layer][packed row][H]: the hidden rows after layer 1 and after layer 2."""
    return [e.forward_packed(prompts, n_layers=l + 1)[0] for l in range(2)]


def _check_rows(name, case, prompts, hid, worst):
    bnd = K.golden()["configs"][name]["prefill"]["bound"]
    off = 0
    for i, p in enumerate(prompts):
        n, ref = len(p), K.probes(name, p)
        for l in range(2):
            d = R.row_rel(hid[l][off:off + n], ref[l])
            worst[l] = max(worst[l], float(d.max()))
            print(f"  {name} {case} sequence {i} ({n} rows) layer {l}: {d.max():.2e} / {bnd[l]:.2e}")
            bad = np.argwhere(d > bnd[l]).ravel()
            if bad.size:
                lines = [f"config {name} case {case} sequence {i} row {r} layer {l}: distance {d[r]:.3e} > bound "
                         f"{bnd[l]:.3e}" for r in bad[:12]]
                raise AssertionError(f"{bad.size} rows beyond the bound\n" + "\n".join(lines))
        off += n
    assert off == hid[0].shape[0]


def _report(name, what, worst):
    bnd = K.golden()["configs"][name]["prefill"]["bound"]
    print(f"ROPE {name} {what}: " + " ".join(f"layer{l} {worst[l]:.2e}/{bnd[l]:.2e}" for l in range(2)))


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_p1_single_prompts(monkeypatch, name):
    """One prompt per call: 1 .. 700 tokens (6 q-blocks, the last of 60 rows); l3: 300 and 700."""
    worst = [0.0, 0.0]
    e = _engine(name, monkeypatch)
    try:
        for p in K.prefill_prompts(name, "P1"):
            _check_rows(name, f"P1/{len(p)}", [p], _probe(e, [p]), worst)
    finally:
        e.close()
    _report(name, "P1", worst)


@pytest.mark.parametrize("name", K.RNAMES)
def test_p2_pack(monkeypatch, name):
    """One pack with every qstart unaligned: a row's position is its index in its own sequence."""
    worst = [0.0, 0.0]
    ps = K.prefill_prompts(name, "P2")
    e = _engine(name, monkeypatch)
    try:
        _check_rows(name, "P2", ps, _probe(e, ps), worst)
    finally:
        e.close()
    _report(name, "P2", worst)


def test_l3_long_prompt(monkeypatch):
    """2048 tokens on the llama3-scaled table: the pairs of the smoothed band turn far enough to show."""
    name, worst = "l3", [0.0, 0.0]
    ps = K.prefill_prompts(name, "L")
    e = _engine(name, monkeypatch, max_batch=2, max_ctx=K.L3_LONG, max_prefill_tokens=K.L3_LONG)
    try:
        _check_rows(name, "L", ps, _probe(e, ps), worst)
    finally:
        e.close()
    _report(name, "L", worst)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", K.RNAMES)
def test_decode_paths(monkeypatch, name, path):
    """Forced runs as tests/test_gpu_decode_edges.py's: prefill logits, per-step tile maxima and ids,
    both slot-major pools against the oracle's cache with the stray-write check."""
    cfg = K.CONFIGS[name]
    gold = K.golden()["configs"][name]["decode"]
    bnd, refs, prompts = gold["bound"], K.decode_reference(name), K.decode_prompts()
    slots, env = PATHS[path]
    B, V = len(prompts), cfg.vocab
    c = dict(max_batch=slots, max_ctx=K.DEC_MAX_CTX)
    worst, excused = dict.fromkeys(R.FAMILIES, 0.0), 0
    assert [r["fed"] for r in refs] == gold["forced"]
    e = _engine(name, monkeypatch, env, max_batch=slots, max_ctx=K.DEC_MAX_CTX)
    try:
        before = DE.Pools(e, c, cfg.n_kv_heads)
        tags = [e.submit_forced(p, r["fed"], K.NPRED) for p, r in zip(prompts, refs)]
        lens = [0] * B
        for j in range(1, K.NPRED):  # step() 1 = admission + prefill (token 0) + decode step 1
            pending = e.step()
            assert (pending == 0) == (j == K.NPRED - 1), (j, pending)
            if j == 1:
                first = e.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, B * V * 4).view(np.float32).reshape(B, V)
                DE._check_logits(first, refs, 0, bnd, worst, "prefill")
            pmax, pid = DE._partials(e, B)
            excused += DE._check_partials(pmax, pid, refs, j, bnd, worst)
            new_lens = [len(p) + j for p in prompts]
            after = DE.Pools(e, c, cfg.n_kv_heads)
            if j == 1:
                DE._check_slots(after, refs, new_lens, bnd)
            DE._check_stray(before, after, lens, new_lens)  # the idle slots of a 24-slot engine: no row at all
            DE._check_content(after, refs, new_lens, bnd, worst)
            before, lens = after, new_lens
        e.collect()
        got = e.take(tags)
        for t, p in zip(tags, prompts):
            assert got[t].finish == "length" and len(got[t].ids) == K.NPRED and got[t].n_prompt == len(p)
    finally:
        e.close()
    print(f"ROPE {name} decode {path}: " + " ".join(f"{f} {worst[f]:.2e}/{bnd[f]:.2e}" for f in R.FAMILIES) +
          f", {excused} of {B * DE.TILES * (K.NPRED - 1)} tile ids excused")
