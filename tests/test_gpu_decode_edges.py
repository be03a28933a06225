"""Decode attention and the KV cache, number by number, at page and split edges (needs a GPU).

Every case of tests/decode_edges_ref.py fills every slot of one TINY engine, the longest sequence
in the last slot, and decodes 10 tokens.  Through hooks the engine already has -- teacher forcing
(one decode step per step()) and ms_debug_read -- each step is compared with the CPU oracle:

  K / V rows   every cached (layer, slot, position, kv head) row of both pools against the oracle's
               cache, relative L2 per row: the prompt rows the (packed) prefill wrote, and each
               decoded token's row, written by the attention prologue or the GEMV RoPE epilogue;
  stray writes both pools are snapshotted before every step(); afterwards the only bytes that may
               differ are the rows of that step's new positions of every slot (slot s = the s-th
               submitted sequence, page p of slot s = pool page s * max_pages + p, asserted on
               each slot's first page before the rest: _check_slots);
  tile maxima  the {max, id} partial of every 16-column tile the greedy lm_head leaves per row
               (the un-scaled lm_head sums), relative L2 over the row's 256 maxima; the tile's id
               must be the oracle's argmax of the tile unless the oracle's top two of that tile
               are closer than bound x the row's largest |maximum|;
  logits       the full fp32 logits of the prefill's first token, and of every step of a sampling
               run (top_k = 1: the draw is the argmax), relative L2 over the row.

The bounds are read from tests/golden/decode_edges_bounds.json: 4 x the distance between the
fp32- and the fp64-accumulating oracle, none of them taken from a GPU; tests/test_decode_edges_ref.py
shows on the CPU that a dropped key, two swapped V rows, a RoPE position off by one, the other kv
head's K/V or an un-permuted K row each sit at >= 2 x these bounds on what the case itself reads
(f reads no pool, g the partials of every third step).  No row of the issue's table is reduced: the
engine accepted every combination.  Case g keeps plain greedy submits and device-chained steps but
reads the partials after each chained run of 3 steps, not only after the last: two swapped V rows
in the one-key sequence move the last step's maxima by 0.97 x the bound only.

Measured on an MI355X: the largest distance over all sequences and steps / the bound, and the tile
ids excused as oracle near-ties.  Every distance is ~1.4 x its floor, a third of its bound.  The
last column is the case's smallest mutant ratio (the CPU test, scored on what the case asserts):
every bound is at most 1/6 of its smallest mutant distance, in f 1/2.5 (a RoPE position off by one,
visible there through the logits alone).

  case, variant               tile maxima        logits (prefill;   K rows             V rows             ids      smallest
                                                 h: every step)                                           excused  mutant
  a  ppb 4                    4.91e-4 / 1.63e-3  8.41e-4 / 2.91e-3  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3  12/13824  7.1 x
  a  ppb 4, ticket            4.91e-4 / 1.63e-3  8.41e-4 / 2.91e-3  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3  12/13824
  a  ppb 9                    4.90e-4 / 1.63e-3  8.41e-4 / 2.91e-3  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3  12/13824
  a  ppb 9, ticket            4.90e-4 / 1.63e-3  8.41e-4 / 2.91e-3  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3  12/13824
  b  v1, ppw 2                5.17e-4 / 1.64e-3  9.93e-4 / 2.92e-3  1.09e-3 / 3.60e-3  1.12e-3 / 3.71e-3   7/13824  6.8 x
  b  v1, ppw 1                5.49e-4 / 1.64e-3  9.93e-4 / 2.92e-3  1.09e-3 / 3.60e-3  1.12e-3 / 3.71e-3   8/13824
  c  GEMV epilogue            4.88e-4 / 1.63e-3  8.41e-4 / 2.91e-3  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3   9/13824  7.1 x
  c  GEMV epilogue, no resid  4.94e-4 / 1.63e-3  8.41e-4 / 2.91e-3  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3  10/13824
  d  v2                       5.13e-4 / 1.57e-3  8.63e-4 / 2.81e-3  1.06e-3 / 3.38e-3  1.09e-3 / 3.37e-3   9/9216  10.3 x
  d  v1                       5.47e-4 / 1.57e-3  8.63e-4 / 2.81e-3  1.06e-3 / 3.38e-3  1.09e-3 / 3.37e-3   8/9216
  e  24 slots                 5.11e-4 / 1.71e-3  8.86e-4 / 2.91e-3  1.09e-3 / 3.66e-3  1.09e-3 / 3.48e-3  33/55296  6.6 x
  f  n_pages 20               5.52e-4 / 1.60e-3  8.56e-4 / 2.84e-3  -                  -                  16/13824  2.5 x
  f  MS_KV_PAGED=1            5.52e-4 / 1.60e-3  8.56e-4 / 2.84e-3  -                  -                  16/13824
  g  chained runs of 3        4.71e-4 / 1.63e-3  -                  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3   3/4608   7.1 x
  h  sampled, top_k 1         -                  8.98e-4 / 2.91e-3  1.10e-3 / 3.43e-3  1.08e-3 / 3.45e-3  -         7.2 x

Recorded floors (fp32 vs fp64 oracle): tile maxima 3.9e-4 - 4.3e-4, logits 7.0e-4 - 7.3e-4, K / V
rows 7.9e-4 - 9.3e-4 over both layers; layer 0's rows alone 1.4e-4 - 2.3e-4 (K) and 1.1e-4 - 2.1e-4
(V): nearly exact, one fp16 flip in a row now and then.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_edges_ref as R  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from mapsum.config import TINY  # noqa: E402
from mapsum.engine import Engine, Sampling  # noqa: E402

V, TILES = TINY.vocab, TINY.vocab // 16
NL, HK, D, PAGE = TINY.n_layers, TINY.n_kv_heads, TINY.head_dim, R.PAGE
KNOBS = ("MS_ATTN_PPB", "MS_ATTN_TICKET", "MS_ATTN_V2", "MS_ATTN_PPW", "MS_ATTN_SLABS", "MS_RESID_FUSED",
         "MS_KV_PAGED", "MS_DECODE_RUN", "MS_GRAPH_STEPS")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _engine(case, monkeypatch, env, n_pages=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    c = R.CASES[case]
    e = Engine(TINY, device=0, max_batch=c["max_batch"], max_ctx=c["max_ctx"], max_prefill_tokens=4096,
               n_pages=c["n_pages"] if n_pages is None else n_pages)
    e.init_synthetic(R.SEED, R.STD, R.JITTER)
    return e


class Pools:
    """Both pools as [layer][slot][page][kv head][64][head_dim] fp16 bit patterns (slot-major pool).
    ``hk``: the engine's kv heads where it is not TINY (tests/test_gpu_attn_keys.py)."""

    def __init__(self, e, c, hk=HK):
        self.B, self.max_pages, self.hk = c["max_batch"], (c["max_ctx"] + PAGE - 1) // PAGE, hk
        shape = (NL, self.B, self.max_pages, hk, PAGE, D)
        nbytes = int(np.prod(shape)) * 2
        self.k = e.debug_read(L.MS_DBG_KPOOL, 0, nbytes).view(np.uint16).reshape(shape)
        self.v = e.debug_read(L.MS_DBG_VPOOL, 0, nbytes).view(np.uint16).reshape(shape)

    def rows(self, which, layer, slot, n):
        """[n][kv head][head_dim] fp32: positions 0..n-1 of one slot."""
        p = getattr(self, which)[layer, slot].view(np.float16)
        return p.transpose(0, 2, 1, 3).reshape(self.max_pages * PAGE, self.hk, D)[:n].astype(np.float32)


def _check_stray(before, after, old_lens, new_lens):
    """Only the rows of positions [old_len, new_len) of each slot may have changed."""
    allowed = np.zeros(before.k.shape[:-1], bool)
    for s, (a, b) in enumerate(zip(old_lens, new_lens)):
        for pos in range(a, b):
            allowed[:, s, pos // PAGE, :, pos % PAGE] = True
    for which in ("k", "v"):
        changed = (getattr(before, which) != getattr(after, which)).any(axis=-1)
        stray = np.argwhere(changed & ~allowed)
        assert stray.size == 0, f"{which} pool: {len(stray)} rows outside the step's new positions changed, " \
                                f"first (layer, slot, page, kv head, offset) = {stray[0].tolist()}"


def _check_slots(pools, refs, lens, bnd):
    """Slot s holds the s-th submitted sequence, its page p at pool page s * max_pages + p: the
    first page of every slot (layer 0, K) must be nearest to its own sequence's first rows among
    all the batch's sequences, and within the bound of them -- before anything else is compared."""
    for s, n in enumerate(lens):
        m = min(n, PAGE)
        got = pools.rows("k", 0, s, m)
        d = [float(R.row_rel(got[:min(m, len(r["k"][0]))], r["k"][0][:m]).max()) for r in refs]
        assert int(np.argmin(d)) == s and d[s] <= bnd["k"], \
            f"slot {s} does not hold the {s}-th submitted sequence: distance of its first page to each " \
            f"sequence's first K rows {[f'{x:.1e}' for x in d]}"


def _check_content(pools, refs, lens, bnd, worst):
    for s, (ref, n) in enumerate(zip(refs, lens)):
        for which in ("k", "v"):
            for l in range(NL):
                d = R.row_rel(pools.rows(which, l, s, n), ref[which][l][:n])
                worst[which] = max(worst[which], float(d.max()))
                bad = np.argwhere(d > bnd[which])
                assert bad.size == 0, f"{which} pool, layer {l}, slot {s} (the {s}-th submitted sequence): " \
                                      f"{len(bad)} rows off the oracle's cache, first (position, kv head) = " \
                                      f"{bad[0].tolist()} at {d[tuple(bad[0])]:.2e} > {bnd[which]:.2e}"


def _partials(e, B):
    p = e.debug_read(L.MS_DBG_DECODE_LOGITS, 0, B * TILES * 8).view(np.float32).reshape(B, TILES, 2)
    ids = np.ascontiguousarray(p[..., 1]).view(np.int32)
    assert np.array_equal(ids // 16, np.broadcast_to(np.arange(TILES), ids.shape)), "not {max, id} per 16-column tile"
    return p[..., 0].copy(), ids


def _check_partials(pmax, pid, refs, j, bnd, worst):
    """Row i of the decode batch is sequence i; j = the decode step.  Returns the tiles excused."""
    excused = 0
    for i, ref in enumerate(refs):
        row = ref["unscaled"][j]
        m = R.tile_max(row)
        d = R.rel(pmax[i], m)
        print(f"  step {j} row {i}: tile maxima {d:.2e}")
        worst["tilemax"] = max(worst["tilemax"], d)
        assert d <= bnd["tilemax"], (j, i, d, bnd["tilemax"])
        tiles = row.reshape(TILES, 16)
        want = tiles.argmax(axis=1) + 16 * np.arange(TILES)
        top2 = np.sort(tiles, axis=1)[:, -2:]
        near = (top2[:, 1] - top2[:, 0]) <= bnd["tilemax"] * np.abs(m).max()
        wrong = pid[i] != want
        assert not (wrong & ~near).any(), (j, i, np.argwhere(wrong & ~near).ravel().tolist())
        excused += int(wrong.sum())
    return excused


def _check_logits(got, refs, j, bnd, worst, what):
    for i, ref in enumerate(refs):
        d = R.rel(got[i], ref["logits"][j])
        print(f"  {what} row {i}: logits {d:.2e}")
        worst["logits"] = max(worst["logits"], d)
        assert d <= bnd["logits"], (what, i, d, bnd["logits"])


def _report(case, env, worst, bnd, excused, tiles):
    print(f"EDGES {case} {env}: " + " ".join(f"{f} {worst[f]:.2e}/{bnd[f]:.2e}" for f in R.FAMILIES if worst[f]) +
          f", {excused} of {tiles} tile ids excused")


def _run_forced(case, monkeypatch, env, pools=True, n_pages=None):
    c, refs, bnd = R.CASES[case], R.reference(case), R.golden()["cases"][case]["bound"]
    prompts, B = R.prompts(case), c["max_batch"]
    worst, excused = dict.fromkeys(R.FAMILIES, 0.0), 0
    e = _engine(case, monkeypatch, env, n_pages)
    try:
        before = Pools(e, c) if pools else None
        tags = [e.submit_forced(p, r["fed"], R.NPRED) for p, r in zip(prompts, refs)]
        lens = [0] * B
        for j in range(1, R.NPRED):  # step() 1 = admission + prefill (token 0) + decode step 1
            pending = e.step()
            assert (pending == 0) == (j == R.NPRED - 1), (j, pending)
            if j == 1:
                first = e.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, B * V * 4).view(np.float32).reshape(B, V)
                _check_logits(first, refs, 0, bnd, worst, "prefill")
            pmax, pid = _partials(e, B)
            excused += _check_partials(pmax, pid, refs, j, bnd, worst)
            new_lens = [len(p) + j for p in prompts]
            if pools:
                after = Pools(e, c)
                if j == 1:
                    _check_slots(after, refs, new_lens, bnd)
                _check_stray(before, after, lens, new_lens)
                _check_content(after, refs, new_lens, bnd, worst)
                before = after
            lens = new_lens
        e.collect()
        got = e.take(tags)
        for t, p in zip(tags, prompts):
            assert got[t].finish == "length" and len(got[t].ids) == R.NPRED and got[t].n_prompt == len(p)
    finally:
        e.close()
    _report(case, env, worst, bnd, excused, B * TILES * (R.NPRED - 1))


@pytest.mark.parametrize("ticket", [0, 1])
@pytest.mark.parametrize("ppb", [None, 9])
def test_a_v2_page_and_split_crossings(monkeypatch, ppb, ticket):
    """v2 (one page per wave): sequences cross a page at 64 and a split at 256 (ppb 4) / 576 (ppb 9)
    keys mid-run, so the block that owns the new token changes; the last slot's grid is rounded
    to 1792 keys, 3 pages past its 25 and past the pool's end, and its run ends at max_ctx."""
    env = {"MS_ATTN_TICKET": ticket}
    if ppb:
        env["MS_ATTN_PPB"] = ppb
    _run_forced("a", monkeypatch, env)


@pytest.mark.parametrize("ppw", [None, 1])
def test_b_v1_split_boundaries(monkeypatch, ppw):
    """v1 (4 waves x ppw pages per block): split boundaries at 512 keys (ppw 2) and 256 (ppw 1);
    every split but the first is empty for the short rows."""
    env = {"MS_ATTN_V2": 0}
    if ppw:
        env["MS_ATTN_PPW"] = ppw
    _run_forced("b", monkeypatch, env)


@pytest.mark.parametrize("resid", [None, 0])
def test_c_kv_from_the_gemv_epilogue(monkeypatch, resid):
    """MS_ATTN_SLABS=0: the new token's K/V are written by the QKV GEMV's RoPE epilogue."""
    env = {"MS_ATTN_SLABS": 0}
    if resid is not None:
        env["MS_RESID_FUSED"] = resid
    _run_forced("c", monkeypatch, env)


@pytest.mark.parametrize("v2", [None, 0])
def test_d_partial_last_page(monkeypatch, v2):
    """max_ctx 1000: the last page holds 40 rows, the last RoPE table row is position 999."""
    _run_forced("d", monkeypatch, {} if v2 is None else {"MS_ATTN_V2": v2})


def test_e_large_regime_one_long_row(monkeypatch):
    """24 slots (the skinny-GEMM regime, v1): 23 rows of 1..139 keys and one that owns 3 of 4 splits."""
    _run_forced("e", monkeypatch, {})


@pytest.mark.parametrize("paged", ["n_pages", "env"])
def test_f_block_table_pool(monkeypatch, paged):
    """A pool of exactly the 20 pages the batch needs, and MS_KV_PAGED=1 on the default pool: page
    ids come from the block table, which no hook reads, so only the logits are checked (and no
    slot mapping: row i of the decode batch is sequence i whatever pages it was given)."""
    if paged == "n_pages":
        _run_forced("f", monkeypatch, {}, pools=False)
    else:
        _run_forced("f", monkeypatch, {"MS_KV_PAGED": 1}, pools=False, n_pages=0)


_OWN = {}


def _own_refs(case, ids):
    """The oracle over each prompt + the engine's own ids (cached by the tokens)."""
    out = []
    for p, t in zip(R.prompts(case), ids):
        key = (tuple(p.tolist()), tuple(t))
        if key not in _OWN:
            _OWN[key] = R.run_sequence(R.oracle(), p, feed=t[:-1])
        out.append(_OWN[key])
    return out


def test_g_chained_greedy_run(monkeypatch):
    """Plain greedy submits at ppb 9, no forcing: every step() is one run of 3 decode steps chained
    on the device in one captured graph (MS_DECODE_RUN = MS_GRAPH_STEPS = 3).  After each run the
    partials of its last step (decode steps 3, 6, 9) and the pools' stray bytes are checked, after
    the last every K/V row, against the oracle run on the engine's own ids."""
    case, env = "g", {"MS_ATTN_PPB": 9, "MS_DECODE_RUN": 3, "MS_GRAPH_STEPS": 3}
    c, bnd = R.CASES[case], R.golden()["cases"][case]["bound"]
    prompts, B = R.prompts(case), c["max_batch"]
    worst = dict.fromkeys(R.FAMILIES, 0.0)
    e = _engine(case, monkeypatch, env)
    try:
        before = Pools(e, c)
        tags = [e.submit(p, R.NPRED, True) for p in prompts]
        partials, lens = {}, [0] * B
        for j in c["steps"]:
            pending = e.step()
            assert (pending == 0) == (j == R.NPRED - 1), (j, pending)
            assert e.stats()["decode_steps"] == j  # the run was 3 steps long
            partials[j] = _partials(e, B)
            after = Pools(e, c)
            new_lens = [len(p) + j for p in prompts]
            _check_stray(before, after, lens, new_lens)
            before, lens = after, new_lens
        assert e.stats()["graphs_built"] >= 1
        e.collect()
        got = e.take(tags)
        ids = [got[t].ids for t in tags]
        assert all(len(t) == R.NPRED for t in ids)
        refs = _own_refs(case, ids)
        _check_slots(before, refs, lens, bnd)
        excused = sum(_check_partials(*partials[j], refs, j, bnd, worst) for j in c["steps"])
        _check_content(before, refs, lens, bnd, worst)
    finally:
        e.close()
    _report(case, env, worst, bnd, excused, B * TILES * len(c["steps"]))


def test_h_sampled_full_logits(monkeypatch):
    """A sampling run with top_k = 1 and no penalty draws the argmax and leaves the full scaled
    fp32 logits of the step behind: every step's rows against the oracle on the engine's ids."""
    case, env = "h", {"MS_DECODE_RUN": 1}
    c, bnd = R.CASES[case], R.golden()["cases"][case]["bound"]
    prompts, B = R.prompts(case), c["max_batch"]
    worst = dict.fromkeys(R.FAMILIES, 0.0)
    samp = Sampling(temperature=1.0, top_k=1, top_p=1.0, min_p=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=3)
    e = _engine(case, monkeypatch, env)
    try:
        before = Pools(e, c)
        tags = [e.submit(p, R.NPRED, True, sampling=samp) for p in prompts]
        logits, lens = [], [0] * B
        for j in range(1, R.NPRED):
            pending = e.step()
            assert (pending == 0) == (j == R.NPRED - 1), (j, pending)
            if j == 1:
                logits.append(e.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, B * V * 4).view(np.float32).reshape(B, V).copy())
            logits.append(e.debug_read(L.MS_DBG_DECODE_LOGITS, 0, B * V * 4).view(np.float32).reshape(B, V).copy())
            after = Pools(e, c)
            new_lens = [len(p) + j for p in prompts]
            _check_stray(before, after, lens, new_lens)
            before, lens = after, new_lens
        e.collect()
        got = e.take(tags)
        ids = [got[t].ids for t in tags]
        for i, t in enumerate(ids):  # the draw is the argmax of the stored row
            assert t == [int(np.argmax(logits[j][i])) for j in range(R.NPRED)], i
        refs = _own_refs(case, ids)
        for j in range(R.NPRED):
            _check_logits(logits[j], refs, j, bnd, worst, f"step {j}")
        _check_slots(before, refs, lens, bnd)
        _check_content(before, refs, lens, bnd, worst)
    finally:
        e.close()
    _report(case, env, worst, bnd, 0, 0)
