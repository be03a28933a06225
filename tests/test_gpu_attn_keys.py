"""Prefill attention row by row, with one decisive key per row, at tile / q-block / wave edges; and
the decode kernels on the same model at GQA groups 3, 8, 5 and 1 (needs a GPU).

The model, prompts, plants, bounds and mutants are tests/attn_keys_ref.py's (read its docstring
first): q . k is large exactly when two tokens share a class, so a key lost or gained by one row --
its own, a planted partner, the key just after it -- replaces that row's output instead of moving it
by 1/n.  Everything goes through hooks the engine already has: load_logical, ms_forward_packed
(hidden rows after 1 and 2 layers, any packing), submit_forced + step, ms_debug_read.

Prefill   every hidden row after layer 1 and after layer 2 of every sequence of
            P1  13 single prompts of 1 .. 700 tokens, one per call,
            P2  one pack of lengths (1, 17, 64, 129, 65, 1, 320, 128) -- also on the two block-table
                pools (g3), and every sequence probed alone must equal its rows in the pack bit for bit,
            P3  a full batch of 8 sequences (1, 1, 2, 16, 33, 64, 65, 130)
          within the config's bound of the fp32 oracle's row, relative L2 over the hidden size.
Decode    four sequences of (1, 63, 64, 300) keys, 5 forced steps whose partners sit at key 0, key 63,
          the first key of the last page (for the 300-key row the 256-key split boundary at ppb 4,
          across it from the new token), nowhere, and the previous position: prefill logits, tile
          maxima + ids with the near-tie rule, K / V rows and stray writes, with the helpers of
          tests/test_gpu_decode_edges.py.

Configs (TINY's layers, ffn and vocab): g3 6 / 2 heads (prefill GB 3), g8 8 / 1 (GB 2; the decode
kernels' kMaxGroup), g5 10 / 2 (GB 1, kvh = h0 / 5), g1 4 / 4 (GB 1).  The engine accepted all four and
every case as stated: nothing is reduced.

The bounds are read from tests/golden/attn_keys_bounds.json: 4 x the distance between the fp32- and
the fp64-accumulating oracle, none taken from a GPU.  tests/test_attn_keys_ref.py shows on the CPU that
a hidden diagonal, a hidden partner, a visible successor, a dropped decode partner or new token each
move every row they target by >= 2 x these bounds (in fact >= 117 x), that another sequence's row is
>= 143 x away, and that the cases reach the lazy-max branches of attn_prefill_kernel (late grows, tiles
above the reference that do not move it, waves where both meet) thousands of times per config.

Measured on an MI355X: the largest distance over all rows of the case / the bound, then the CPU
floor (fp32 vs fp64 oracle) and the config's smallest mutant ratio (the CPU test; a row's ratio is the
larger of its two reads).  Prefill distances are 1.0 - 1.7 x their floors, decode 1.0 - 2.3 x (each
decode floor is the largest of 24 samples only); the largest fraction of a bound is
0.42 in prefill (g1 P3, after layer 1) and 0.56 in decode (g3 tile maxima).

  prefill                after layer 1        after layer 2        floors (layer 1, 2)   smallest mutant
  g3  P1 (13 prompts)    7.74e-4 / 2.40e-3    1.06e-3 / 3.18e-3    5.99e-4, 7.96e-4      175 x (hidden diagonal)
  g3  P2 (pack of 8)     7.30e-4 / 2.40e-3    1.11e-3 / 3.18e-3
  g3  P2, n_pages 16     7.30e-4 / 2.40e-3    1.11e-3 / 3.18e-3
  g3  P2, MS_KV_PAGED=1  7.30e-4 / 2.40e-3    1.11e-3 / 3.18e-3
  g3  P3 (full batch)    7.53e-4 / 2.40e-3    9.96e-4 / 3.18e-3
  g8  P1                 7.92e-4 / 3.10e-3    1.17e-3 / 3.90e-3    7.75e-4, 9.74e-4      148 x (hidden partner)
  g8  P2                 8.67e-4 / 3.10e-3    1.12e-3 / 3.90e-3
  g8  P3                 7.78e-4 / 3.10e-3    1.02e-3 / 3.90e-3
  g5  P1                 8.70e-4 / 2.40e-3    1.11e-3 / 3.29e-3    5.99e-4, 8.21e-4      173 x (hidden partner)
  g5  P2                 7.55e-4 / 2.40e-3    1.05e-3 / 3.29e-3
  g5  P3                 7.28e-4 / 2.40e-3    1.02e-3 / 3.29e-3
  g1  P1                 7.20e-4 / 1.98e-3    9.65e-4 / 2.95e-3    4.94e-4, 7.39e-4      143 x (another sequence's row;
  g1  P2                 7.26e-4 / 1.98e-3    9.90e-4 / 2.95e-3                          158 x hidden partner)
  g1  P3                 8.35e-4 / 1.98e-3    1.11e-3 / 2.95e-3

  decode  tile maxima        logits (prefill)   K rows             V rows             ids excused  floors (same order)                 smallest mutant
  g3      5.45e-4 / 9.74e-4  8.25e-4 / 1.70e-3  9.65e-4 / 2.86e-3  1.07e-3 / 2.52e-3  7 / 5120     2.43e-4, 4.25e-4, 7.15e-4, 6.30e-4  194 x (new token dropped)
  g8      4.50e-4 / 1.33e-3  5.23e-4 / 2.33e-3  1.02e-3 / 2.72e-3  1.04e-3 / 2.72e-3  2 / 5120     3.32e-4, 5.83e-4, 6.80e-4, 6.80e-4  172 x (new token dropped)
  g5      4.57e-4 / 1.35e-3  5.82e-4 / 2.57e-3  1.04e-3 / 2.77e-3  1.03e-3 / 2.81e-3  7 / 5120     3.38e-4, 6.43e-4, 6.92e-4, 7.03e-4  162 x (new token dropped)
  g1      4.21e-4 / 1.23e-3  6.45e-4 / 2.21e-3  9.47e-4 / 2.76e-3  8.96e-4 / 2.54e-3  1 / 5120     3.07e-4, 5.52e-4, 6.90e-4, 6.34e-4  144 x (partner dropped)

The packing-invariance comparison (P2's sequences alone vs in the pack, both layers) was bit-exact in
all four configs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import attn_keys_ref as K  # noqa: E402
import decode_edges_ref as R  # noqa: E402
import test_gpu_decode_edges as DE  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from mapsum.engine import Engine  # noqa: E402
from mapsum.weights import load_logical  # noqa: E402

NAMES = sorted(K.CONFIGS)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _engine(name, monkeypatch, env=None, max_batch=8, max_ctx=704, n_pages=0):
    for k in DE.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    e = Engine(K.CONFIGS[name], device=0, max_batch=max_batch, max_ctx=max_ctx, max_prefill_tokens=1024,
               n_pages=n_pages)
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
        n, ref, kinds = len(p), K.probes(name, p), K.row_kinds(len(p))
        for l in range(2):
            d = R.row_rel(hid[l][off:off + n], ref[l])
            worst[l] = max(worst[l], float(d.max()))
            print(f"  {name} {case} sequence {i} ({n} rows) layer {l}: {d.max():.2e} / {bnd[l]:.2e}")
            bad = np.argwhere(d > bnd[l]).ravel()
            if bad.size:
                lines = [f"config {name} case {case} sequence {i} row {r} layer {l}: distance {d[r]:.3e} > bound "
                         f"{bnd[l]:.3e} ({kinds[r]} row)" for r in bad[:12]]
                raise AssertionError(f"{bad.size} rows beyond the bound\n" + "\n".join(lines))
        off += n
    assert off == hid[0].shape[0]


def _report(name, what, worst):
    bnd = K.golden()["configs"][name]["prefill"]["bound"]
    print(f"KEYS {name} {what}: " + " ".join(f"layer{l} {worst[l]:.2e}/{bnd[l]:.2e}" for l in range(2)))


@pytest.mark.parametrize("name", NAMES)
def test_p1_single_sequences(monkeypatch, name):
    """13 prompts, one per call: 1 .. 700 tokens (11 tiles, 6 q-blocks, a ragged last block of 60
    rows, dead waves), planted rows around every multiple of 16."""
    worst = [0.0, 0.0]
    e = _engine(name, monkeypatch)
    try:
        for p in K.prefill_prompts("P1"):
            _check_rows(name, f"P1/{len(p)}", [p], _probe(e, [p]), worst)
    finally:
        e.close()
    _report(name, "P1", worst)


@pytest.mark.parametrize("name", NAMES)
def test_p2_pack_and_packing_invariance(monkeypatch, name):
    """One pack with every qstart unaligned and a heaviest-first order unlike the pack order; then
    every sequence alone: bit for bit the rows it has in the pack, both layers."""
    worst = [0.0, 0.0]
    ps = K.prefill_prompts("P2")
    e = _engine(name, monkeypatch)
    try:
        hid = _probe(e, ps)
        _check_rows(name, "P2", ps, hid, worst)
        off = 0
        for i, p in enumerate(ps):
            alone = _probe(e, [p])
            for l in range(2):
                same = (alone[l].view(np.uint32) == hid[l][off:off + len(p)].view(np.uint32)).all(axis=1)
                assert same.all(), f"config {name} P2 sequence {i} layer {l}: rows {np.argwhere(~same).ravel()[:12]} " \
                                   f"differ between the pack and the sequence alone"
            off += len(p)
    finally:
        e.close()
    _report(name, "P2", worst)


@pytest.mark.parametrize("name", NAMES)
def test_p3_full_batch(monkeypatch, name):
    """Eight sequences at max_batch 8, two of one token and one of two."""
    worst = [0.0, 0.0]
    ps = K.prefill_prompts("P3")
    e = _engine(name, monkeypatch)
    try:
        _check_rows(name, "P3", ps, _probe(e, ps), worst)
    finally:
        e.close()
    _report(name, "P3", worst)


@pytest.mark.parametrize("paged", ["n_pages", "env"])
def test_p2_block_table_pools(monkeypatch, paged):
    """g3's pack through block-table pages (page_of): a pool of exactly the 16 pages the pack needs,
    after a generate of more chunks than the pool holds at once has permuted the free list; and
    MS_KV_PAGED=1 on the default pool."""
    name, worst = "g3", [0.0, 0.0]
    ps = K.prefill_prompts("P2")
    need = sum((len(p) + K.PAGE - 1) // K.PAGE for p in ps)
    assert need == 16
    e = _engine(name, monkeypatch, {} if paged == "n_pages" else {"MS_KV_PAGED": 1}, n_pages=need if paged == "n_pages" else 0)
    try:
        if paged == "n_pages":
            warm = [K.build_prompt(n, 7 * i, 8600 + i, planted=False) for i, n in enumerate((100, 250, 300, 7, 180, 90, 400, 30, 60, 130))]
            res = e.generate(warm, num_predict=4, ignore_eos=True)
            assert all(r.finish == "length" and len(r.ids) == 4 for r in res)
        _check_rows(name, f"P2 {paged}", ps, _probe(e, ps), worst)
    finally:
        e.close()
    _report(name, f"P2 pool {paged}", worst)


@pytest.mark.parametrize("name", NAMES)
def test_decode_forced_partners(monkeypatch, name):
    """Forced runs as tests/test_gpu_decode_edges.py's: prefill logits, per-step tile maxima and
    ids, both slot-major pools against the oracle's cache with the stray-write check."""
    cfg = K.CONFIGS[name]
    gold = K.golden()["configs"][name]["decode"]
    bnd, refs, prompts = gold["bound"], K.decode_reference(name), K.decode_prompts()
    B, V = len(prompts), cfg.vocab
    c = dict(max_batch=B, max_ctx=K.DEC_MAX_CTX)
    worst, excused = dict.fromkeys(R.FAMILIES, 0.0), 0
    assert [r["fed"] for r in refs] == gold["forced"]
    e = _engine(name, monkeypatch, {"MS_ATTN_PPB": K.DEC_PPB}, max_batch=B, max_ctx=K.DEC_MAX_CTX)
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
            DE._check_stray(before, after, lens, new_lens)
            DE._check_content(after, refs, new_lens, bnd, worst)
            before, lens = after, new_lens
        e.collect()
        got = e.take(tags)
        for t, p in zip(tags, prompts):
            assert got[t].finish == "length" and len(got[t].ids) == K.NPRED and got[t].n_prompt == len(p)
    finally:
        e.close()
    print(f"KEYS {name} decode: " + " ".join(f"{f} {worst[f]:.2e}/{bnd[f]:.2e}" for f in R.FAMILIES) +
          f", {excused} of {B * DE.TILES * (K.NPRED - 1)} tile ids excused")
