"""QK-norm engines (Qwen3): the fused norm + RoPE + K/V scatter kernel and everything above it (needs a GPU).

Op level (ms_op_qk_norm_rope, csrc/k_qknorm.hip): both input forms against the float64 evaluation
of the contract's steps 2-4 (tests/qwen3_ref.py qk_norm_rope_f64), element by element within one
fp16 ulp, V rows bit-exact at the right page and offset, and not one byte of either pool changed
outside the written rows.  Engine level on TINY_QWEN3: ms_forward against OracleQwen3, packed
prefill bitwise equal to each prompt alone, teacher-forced and free-running greedy decode in every
regime (8 slots with decode attention v2 and v1, 20 slots, 32 slots: the skinny-GEMM regime; and
the GEMV's fp16-rows form behind MS_ATTN_SLABS=0) with the cached K / V rows of prompt and decoded
positions inside the CPU-derived bounds of tests/golden/qwen3_bounds.json, batch invariance per
regime, a Q4_K_M-mix engine, and two layers at Qwen3-8B's widths.

Measured on an MI355X (printed by the tests; DESIGN.md §2 carries the figures).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import qwen3_ref as R  # noqa: E402
from decode_edges_ref import rel, row_rel  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from mapsum.config import QWEN3_8B, TINY, TINY_QWEN3  # noqa: E402
from mapsum.engine import Engine, Sampling  # noqa: E402
from mapsum.weights import f32_to_f16_bits, load_logical, load_quantized  # noqa: E402
from oracle.llama_ref import OracleLlama, rope_tables  # noqa: E402
from oracle.synth import make_weights  # noqa: E402

CFG = TINY_QWEN3
HQ, HK, D, PAGE, NL = CFG.n_heads, CFG.n_kv_heads, CFG.head_dim, 64, CFG.n_layers
NH = HQ + 2 * HK
ROW = NH * D
PERM = np.array([16 * (i >> 3) + (i & 7) if i < 64 else 16 * ((i - 64) >> 3) + 8 + ((i - 64) & 7) for i in range(128)])
KNOBS = ("MS_ATTN_PPB", "MS_ATTN_TICKET", "MS_ATTN_V2", "MS_ATTN_PPW", "MS_ATTN_SLABS", "MS_RESID_FUSED",
         "MS_KV_PAGED", "MS_DECODE_RUN", "MS_GRAPH_STEPS", "MS_PERSIST")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ op level
N_SLOTS, MAX_PAGES, POOL_PAGES, N_POS = 4, 3, 16, 192


class OpCase:
    """T tokens at positions 62 .. 62 + T - 1 (T = 130: past one 128-row q-block, over the page
    edges at 64 and 128), spread over block-table rows 2, 0, 3 of a shuffled table."""

    def __init__(self, T, seed):
        rng = np.random.default_rng(seed)
        self.T = T
        self.pos = (62 + np.arange(T)).astype(np.int32)
        self.slot = np.array([2, 0, 3], np.int32)[np.arange(T) % 3]
        self.bt = rng.permutation(POOL_PAGES)[:N_SLOTS * MAX_PAGES].reshape(N_SLOTS, MAX_PAGES).astype(np.int32)
        assert not np.array_equal(self.bt.ravel(), np.arange(N_SLOTS * MAX_PAGES))
        self.qg = (1 + 0.3 * rng.standard_normal(D)).astype(np.float16)
        self.kg = (1 + 0.3 * rng.standard_normal(D)).astype(np.float16)
        self.cos, self.sin = rope_tables(CFG, np.arange(N_POS))
        # the pools' pattern: no two neighbouring rows alike, no NaN patterns needed (compared as bits)
        n = POOL_PAGES * HK * PAGE * D
        self.k0 = ((np.arange(n, dtype=np.int64) * 7919 + 13) % 30011).astype(np.uint16)
        self.v0 = ((np.arange(n, dtype=np.int64) * 104729 + 5) % 30013).astype(np.uint16)

    def rows_from_natural(self, t):
        """[T, NH, D] logical order -> the qkv rows: Q / K heads rope-permuted, V as is."""
        out = t.copy()
        out[:, :HQ + HK, PERM] = t[:, :HQ + HK, :]
        return out.reshape(self.T, ROW)

    def natural_from_rows(self, rows):
        t = rows.reshape(self.T, NH, D).copy()
        t[:, :HQ + HK, :] = t[:, :HQ + HK, :][:, :, PERM]
        return t

    def run(self, lib, qkv16, slabs=None, S=0):
        """-> (qkv rows after, k pool, v pool) as uint16 arrays."""
        qkv = _dev(qkv16.view(np.uint16).astype(np.int16).reshape(self.T, ROW))
        kp, vp = _dev(self.k0.astype(np.int16)), _dev(self.v0.astype(np.int16))
        pos, slot, bt = _dev(self.pos), _dev(self.slot), _dev(self.bt)
        cs, sn = _dev(self.cos), _dev(self.sin)
        qg, kg = _dev(self.qg.view(np.int16)), _dev(self.kg.view(np.int16))
        sl = _dev(slabs) if slabs is not None else None
        rc = lib.ms_op_qk_norm_rope(qkv.data_ptr(), sl.data_ptr() if sl is not None else None, S, self.T, HQ, HK,
                                    pos.data_ptr(), slot.data_ptr(), cs.data_ptr(), sn.data_ptr(), qg.data_ptr(),
                                    kg.data_ptr(), CFG.norm_eps, kp.data_ptr(), vp.data_ptr(), bt.data_ptr(),
                                    MAX_PAGES, _stream())
        assert rc == 0, lib.ms_last_error(None)
        torch.cuda.synchronize()
        u16 = lambda t: t.cpu().numpy().view(np.uint16)  # noqa: E731
        return u16(qkv), u16(kp).reshape(POOL_PAGES, HK, PAGE, D), u16(vp).reshape(POOL_PAGES, HK, PAGE, D)

    def cached(self, pool):
        """[T, HK, D]: the rows of every token's (page, offset)."""
        pages = self.bt[self.slot, self.pos // PAGE]
        return pool[pages, :, self.pos % PAGE, :]

    def check_stray(self, kp, vp):
        written = np.zeros((POOL_PAGES, HK, PAGE), bool)
        written[self.bt[self.slot, self.pos // PAGE], :, self.pos % PAGE] = True
        assert written.sum() == self.T * HK
        for name, pool, init in (("k", kp, self.k0), ("v", vp, self.v0)):
            same = (pool == init.reshape(pool.shape)).all(axis=-1)
            stray = np.argwhere(~same & ~written)
            assert stray.size == 0, f"{name} pool: {len(stray)} rows outside the written ones changed, first " \
                                    f"(page, kv head, offset) = {stray[0].tolist()}"
            assert not same[written].all(), f"{name} pool: nothing was written"

    def ref(self, t):
        """float64 steps 2-4 of Q and K heads over the tokens' positions: ([T, HQ, D], [T, HK, D])."""
        c, s = self.cos[self.pos], self.sin[self.pos]
        tf = t.astype(np.float32)
        return (R.qk_norm_rope_f64(tf[:, :HQ], self.qg.astype(np.float32), c, s, CFG.norm_eps),
                R.qk_norm_rope_f64(tf[:, HQ:HQ + HK], self.kg.astype(np.float32), c, s, CFG.norm_eps))


def _ulps(got_u16, ref64):
    got = np.ascontiguousarray(got_u16).view(np.float16)
    want = ref64.astype(np.float16)
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp


def _check_qk(case, qkv_after, kp, t, what, alt=None):
    """Q rows and cached K rows within one fp16 ulp of the float64 steps 2-4 on the fp16 values t
    [T, NH, D].  alt = (other, amb) from _step1 (slabs form with a row scale): where a head misses,
    its elements whose step-1 rounding an ulp of the fp32 row factor can turn (amb) are tried at
    their other fp16 neighbour too."""
    q64, k64 = case.ref(t)
    got_q, got_k = qkv_after.reshape(case.T, NH, D)[:, :HQ], case.cached(kp)
    dq, dk = _ulps(got_q, q64), _ulps(got_k, k64)
    retried = 0
    if alt is not None:
        other, amb = alt
        for d, got, h0, gain in ((dq, got_q, 0, case.qg), (dk, got_k, HQ, case.kg)):
            for tok, h in np.argwhere(d.max(axis=-1) > 1):
                dims = np.nonzero(amb[tok, h0 + h])[0]
                assert 0 < len(dims) <= 4, (what, int(tok), int(h), dims.tolist())
                c, s = case.cos[case.pos[tok:tok + 1]], case.sin[case.pos[tok:tok + 1]]
                for mask in range(1, 1 << len(dims)):
                    th = t[tok, h0 + h].copy()
                    flip = dims[[i for i in range(len(dims)) if mask >> i & 1]]
                    th[flip] = other[tok, h0 + h][flip]
                    r64 = R.qk_norm_rope_f64(th[None, None].astype(np.float32), gain.astype(np.float32), c, s, CFG.norm_eps)
                    d[tok, h] = np.minimum(d[tok, h].max(), _ulps(got[tok, h][None, None], r64).max())
                retried += 1
    print(f"{what}: Q max {dq.max():.0f} ulp ({(dq > 0).mean():.2%} off by one), cached K max {dk.max():.0f} ulp "
          f"({(dk > 0).mean():.2%}){f', {retried} head(s) at a step-1 rounding boundary' if retried else ''}")
    assert dq.max() <= 1, np.argwhere(dq > 1)[:4].tolist()
    assert dk.max() <= 1, np.argwhere(dk > 1)[:4].tolist()


def _step1(slabs, ssq_h, hidden, eps):
    """Step 1 as the contract states it -- the fp32 fold in slab order, times the fp32 row factor
    16 / sqrt(sum / hidden + eps), rounded to fp16 -- as (t, other, amb) in row layout: where the fp32
    product lies within 8 fp32 ulps of the midpoint between t and its fp16 neighbour `other`, an ulp
    of the factor (the device's reciprocal square root is good to one; its statistics sum has its
    own order) may round the element to `other`: amb marks those elements."""
    acc = slabs[0].copy()
    for q in range(1, len(slabs)):
        acc = (acc + slabs[q]).astype(np.float32)
    ss = ssq_h.sum(axis=0, dtype=np.float32)
    r = (np.float32(16.0) / np.sqrt(ss * np.float32(1.0 / hidden) + np.float32(eps))).astype(np.float32)
    v = (acc * r[:, None]).astype(np.float32)
    t = v.astype(np.float16)
    v64, t64 = v.astype(np.float64), t.astype(np.float64)
    other = np.where(v64 >= t64, np.nextafter(t, np.float16(np.inf)), np.nextafter(t, np.float16(-np.inf))).astype(np.float16)
    mid = (t64 + other.astype(np.float64)) / 2
    return t, other, np.abs(v64 - mid) <= 8 * 2.0 ** -24 * np.abs(v64)


@pytest.mark.parametrize("T", [1, 3, 130])
def test_op_rows_form(lib, T):
    case = OpCase(T, 100 + T)
    rng = np.random.default_rng(T)
    t = (rng.standard_normal((T, NH, D)) * rng.choice([0.25, 1.0, 6.0], size=(T, NH, 1))).astype(np.float16)
    rows = case.rows_from_natural(t)
    after, kp, vp = case.run(lib, rows)
    _check_qk(case, after, kp, t, f"rows form T={T}")
    assert np.array_equal(case.cached(vp), t[:, HQ + HK:].view(np.uint16)), "V rows are not bit-exact copies"
    assert np.array_equal(after.reshape(T, NH, D)[:, HQ:], rows.view(np.uint16).reshape(T, NH, D)[:, HQ:]), \
        "the rows form must leave the K / V part of the qkv rows alone"
    case.check_stray(kp, vp)
    # the fixture's gains must matter: the same rows with the gains in rope-permuted order are far off
    q64, _ = case.ref(t)
    wrong = R.qk_norm_rope_f64(t[:, :HQ].astype(np.float32), case.qg.astype(np.float32)[PERM], case.cos[case.pos],
                               case.sin[case.pos], CFG.norm_eps)
    assert rel(wrong, q64) > 0.1


@pytest.mark.parametrize("S", [1, 4, 6])
def test_op_slabs_form_equals_rows_form_on_exact_folds(lib, S):
    """Integer-valued slabs fold exactly in fp32 and in fp16; a row scale of an exact power of two
    (256 statistics tiles summing to hidden * 4^k, eps 0: rinv = 16 / 2^k) keeps step 1 exact too.
    Both ways the slabs form must leave the bits of the rows form run on the folded rows."""
    T = 5
    case = OpCase(T, 200 + S)
    rng = np.random.default_rng(S)
    slabs = rng.integers(-6, 7, size=(S, T, ROW)).astype(np.float32)
    scrap = np.full((T, ROW), 0x7e00, np.uint16)  # the slabs form reads no qkv row: NaNs there
    for scaled in (False, True):
        fold = slabs.sum(axis=0, dtype=np.float32)
        ssq = None
        if scaled:
            k = np.array([0, 1, 2, 0, 1])[:T]
            ssq = _dev(np.broadcast_to((CFG.hidden * 4.0 ** k / 256).astype(np.float32), (256, T)))
            assert lib.ms_op_set_row_scale(ssq.data_ptr(), 256, CFG.hidden, 0.0) == 0
            fold = fold * (16.0 / 2.0 ** k)[:, None].astype(np.float32)
        try:
            got = case.run(lib, scrap.copy(), slabs, S)
        finally:
            lib.ms_op_set_row_scale(None, 0, 0, 0.0)
        folded = fold.astype(np.float16)
        assert np.array_equal(folded.astype(np.float32), fold)
        want = case.run(lib, folded)
        for name, g, w in zip(("qkv rows", "k pool", "v pool"), got, want):
            assert np.array_equal(g, w), f"S={S} scaled={scaled}: {name} differ from the rows form"
        case.check_stray(got[1], got[2])
        _check_qk(case, got[0], got[1], case.natural_from_rows(folded), f"slabs form S={S} scaled={scaled}")


@pytest.mark.parametrize("S,tiles", [(1, 1), (4, 256), (6, 7)])
def test_op_slabs_form_with_row_scale(lib, S, tiles):
    """Real-valued slabs and statistics: step 1 (the fp32 fold in slab order times the fp32 row
    factor, rounded to fp16) then steps 2-4 against float64, one ulp.  The reference takes step 1 in
    fp32 as the contract states it: evaluated in float64 too, 4 of the 4608 elements of the S = 6
    case round to the other fp16 neighbour (six N(0, 20) partial sums cancel), and a head built on
    another t is up to 2 ulps away -- measured on an MI355X at token 0, head 3, dim 28."""
    T = 3
    case = OpCase(T, 300 + S)
    rng = np.random.default_rng(40 + S)
    slabs = (rng.standard_normal((S, T, ROW)) * 20).astype(np.float32)
    ssq_h = (rng.random((tiles, T)) * 900 * CFG.hidden / tiles + 1).astype(np.float32)
    ssq = _dev(ssq_h)
    assert lib.ms_op_set_row_scale(ssq.data_ptr(), tiles, CFG.hidden, CFG.norm_eps) == 0
    try:
        after, kp, vp = case.run(lib, np.zeros((T, ROW), np.uint16), slabs, S)
    finally:
        lib.ms_op_set_row_scale(None, 0, 0, 0.0)
    t_rows, other_rows, amb_rows = _step1(slabs, ssq_h, CFG.hidden, CFG.norm_eps)
    t = case.natural_from_rows(t_rows)
    _check_qk(case, after, kp, t, f"slabs form S={S}, {tiles} statistics tiles",
              alt=(case.natural_from_rows(other_rows), case.natural_from_rows(amb_rows)))
    dv = _ulps(case.cached(vp), t[:, HQ + HK:].astype(np.float64))
    assert dv.max() <= 1
    # ... and step 1 itself against float64 all the way
    rinv = 16.0 / np.sqrt(ssq_h.astype(np.float64).sum(axis=0) / CFG.hidden + np.float64(np.float32(CFG.norm_eps)))
    fold64 = slabs.astype(np.float64).sum(axis=0) * rinv[:, None]
    # the row keeps the folded K / V the cache rows were made from
    dr = _ulps(after.reshape(T, NH, D)[:, HQ:], fold64.reshape(T, NH, D)[:, HQ:])
    assert dr.max() <= 1
    assert np.array_equal(case.cached(vp), after.reshape(T, NH, D)[:, HQ + HK:])
    case.check_stray(kp, vp)


# ------------------------------------------------------------------ engine level
def _engine(monkeypatch, max_batch, env=None, max_ctx=256, cfg=CFG, weights=None, prefill=1024):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    e = Engine(cfg, device=0, max_batch=max_batch, max_ctx=max_ctx, max_prefill_tokens=prefill)
    load_logical(e, R.tiny_weights() if weights is None else weights)
    return e


@pytest.fixture(scope="module")
def eng():
    mp = pytest.MonkeyPatch()
    e = _engine(mp, 8)
    yield e
    e.close()
    mp.undo()


def _prompt(n, seed):
    return np.random.default_rng(seed).integers(0, 4000, size=n).astype(np.int32)


def test_forward_vs_oracle(eng):
    """Per-layer hidden states and all-position logits within the project's 2e-2 of un-rounded Qwen3
    (OracleQwen3 fp32 mode); the distance to the engine-mode mirror is printed."""
    ids = _prompt(200, 21)
    o32, oe = R.tiny_oracle("fp32"), R.tiny_oracle("engine")
    ref, probes = o32.forward(ids, collect=True, all_logits=True)
    mir, mprobes = oe.forward(ids, collect=True, all_logits=True)
    for l in range(NL):
        h, _ = eng.forward(ids, n_layers=l + 1)
        print(f"layer {l}: hidden vs fp32 oracle {rel(h, probes[l]):.2e}, vs engine-mode mirror {rel(h, mprobes[l]):.2e}")
        assert rel(h, probes[l]) < 2e-2
    _, lg = eng.forward(ids, hidden=False, logits=True)
    print(f"QWEN3 ms_forward logits: vs fp32 oracle {rel(lg, ref):.2e}, vs engine-mode mirror {rel(lg, mir):.2e}")
    assert rel(lg, ref) < 2e-2
    # and the norm is seen: Llama arithmetic on the same weights is nowhere near
    far, _ = OracleLlama(CFG, R.tiny_weights(), mode="fp32").forward(ids, all_logits=True)
    assert rel(lg, far) > 0.5


def test_packed_prefill_is_bitwise_each_prompt_alone(eng):
    a, b = _prompt(70, 31), _prompt(131, 32)
    for nl in range(1, NL + 1):
        both, _ = eng.forward_packed([a, b], n_layers=nl)
        ha, _ = eng.forward_packed([a], n_layers=nl)
        hb, _ = eng.forward_packed([b], n_layers=nl)
        assert np.array_equal(both[:70].view(np.uint32), ha.view(np.uint32)), nl
        assert np.array_equal(both[70:].view(np.uint32), hb.view(np.uint32)), nl
    _, lg = eng.forward_packed([a, b], hidden=False, logits=True)
    _, la = eng.forward_packed([a], hidden=False, logits=True)
    assert np.array_equal(lg[:70].view(np.uint32), la.view(np.uint32))


def _pool_rows(e, which, max_batch, max_ctx, slot, n, hk=HK, nl=NL):
    """[layer][n][kv head][D] fp16 bit patterns: positions 0 .. n-1 of one slot (slot-major pool)."""
    mp = (max_ctx + PAGE - 1) // PAGE
    shape = (nl, max_batch, mp, hk, PAGE, D)
    nbytes = int(np.prod(shape)) * 2
    p = e.debug_read(which, 0, nbytes).view(np.uint16).reshape(shape)[:, slot]
    return p.transpose(0, 1, 3, 2, 4).reshape(nl, mp * PAGE, hk, D)[:, :n]


def _agreement(oracle, prompt, gen):
    """tests/test_gpu_parity.py's rule: (agreeing steps, [(step, gap to the oracle's top, top)])."""
    ids = np.concatenate([np.asarray(prompt, np.int32), np.asarray(gen[:-1], np.int32)])
    lg, _ = oracle.forward(ids, all_logits=True)
    lg = lg[len(prompt) - 1:]
    want = np.argmax(lg, 1)
    srt = np.sort(lg, 1)
    flips = [(i, float(srt[i, -1] - lg[i, gen[i]]), float(srt[i, -1])) for i in range(len(gen)) if want[i] != gen[i]]
    return len(gen) - len(flips), flips, srt[:, -1] - srt[:, -2]


def _check_tokens(oracle, prompts, gens, noise, what):
    agree = total = dec_agree = dec_total = 0
    for p, g in zip(prompts, gens):
        assert len(g) == R.NPRED
        a, flips, gap = _agreement(oracle, p, g)
        for pos, d, top in flips:  # every disagreement an oracle near-tie
            assert d <= 1e-2 * (abs(top) + 1.0), (what, pos, d, top)
        dec = gap > 4.0 * noise
        dec_total += int(dec.sum())
        dec_agree += int(dec.sum()) - sum(1 for pos, _, _ in flips if dec[pos])
        agree += a
        total += len(g)
    print(f"{what}: {agree}/{total} steps agree, decisive {dec_agree}/{dec_total}")
    assert dec_agree == dec_total and dec_total > 0, (dec_agree, dec_total, total)


@pytest.mark.parametrize("slots,env", [(8, {}), (8, {"MS_ATTN_V2": 0}), (20, {}), (32, {}), (8, {"MS_ATTN_SLABS": 0})],
                         ids=["8-v2", "8-v1", "20", "32", "8-gemv-rows"])
def test_decode_vs_oracle(monkeypatch, slots, env):
    """100-token prompts + 32 tokens (the decode crosses the 128-key page edge): teacher-forced and
    free-running greedy against OracleQwen3, then every cached K / V row of prompt and decoded
    positions against the reference's cache, inside the CPU-derived bounds."""
    prompts, bnd, forced = R.decode_prompts(), R.bounds()["bound"], R.bounds()["forced"]
    oracle = R.tiny_oracle()
    e = _engine(monkeypatch, slots, env)
    try:
        _, elg = e.forward(prompts[0], hidden=False, logits=True)
        olg, _ = oracle.forward(prompts[0], all_logits=True)
        noise = float(np.sqrt(np.mean((elg - olg) ** 2)))
        res = e.generate_forced(prompts, forced, R.NPRED)
        # teacher forcing: step j saw prompt + forced[:j]; the oracle over the same ids
        worst = {"k": 0.0, "v": 0.0}
        n = R.N_PROMPT + R.NPRED - 1  # the last chosen token is never fed
        for s, (p, f, r) in enumerate(zip(prompts, forced, res)):
            assert len(r.ids) == R.NPRED and r.finish == "length"
            ids = np.concatenate([p, np.asarray(f, np.int32)])
            cache = oracle.new_cache()
            lg, _ = oracle.forward(ids, cache, all_logits=True)
            lg = lg[len(p) - 1:]
            srt = np.sort(lg, 1)
            dec = (srt[:, -1] - srt[:, -2]) > 4.0 * noise
            got, want = np.asarray(r.ids), np.argmax(lg, 1)
            for j in np.nonzero(got != want)[0]:
                assert not dec[j], (s, j)
                assert srt[j, -1] - lg[j, got[j]] <= 1e-2 * (abs(srt[j, -1]) + 1.0), (s, j)
            assert dec.any()
            for which, dbg in (("k", L.MS_DBG_KPOOL), ("v", L.MS_DBG_VPOOL)):
                rows = _pool_rows(e, dbg, slots, 256, s, n).view(np.float16).astype(np.float32)
                for l in range(NL):
                    d = row_rel(rows[l], cache[which][l][:n])
                    worst[which] = max(worst[which], float(d.max()))
                    bad = np.argwhere(d > bnd[which])
                    assert bad.size == 0, f"{which} pool layer {l} slot {s}: {len(bad)} rows off the oracle's cache, " \
                                          f"first (position, kv head) = {bad[0].tolist()} at {d[tuple(bad[0])]:.2e}"
        print(f"QWEN3 decode {slots} slots {env}: K rows {worst['k']:.2e}/{bnd['k']:.2e}, "
              f"V rows {worst['v']:.2e}/{bnd['v']:.2e}")
        free = e.generate(prompts, num_predict=R.NPRED, ignore_eos=True)
        _check_tokens(oracle, prompts, [r.ids for r in free], noise, f"{slots} slots {env} free-running")
        assert e.stats()["graphs_built"] >= 1  # the decode graph captured the extra launch
    finally:
        e.close()


@pytest.mark.parametrize("slots", [8, 20, 32])
def test_batch_invariance(monkeypatch, slots):
    """Chunk 0's ids and cached K rows are identical alone and in a full batch of the regime."""
    prompts = [_prompt(20 + (37 * i) % 90, 500 + i) for i in range(slots)]
    npred, n0 = 12, len(prompts[0])
    out = []
    for batch in (prompts[:1], prompts):
        e = _engine(monkeypatch, slots)
        try:
            ids = e.generate(batch, num_predict=npred, ignore_eos=True)[0].ids
            out.append((ids, _pool_rows(e, L.MS_DBG_KPOOL, slots, 256, 0, n0 + npred - 1),
                        _pool_rows(e, L.MS_DBG_VPOOL, slots, 256, 0, n0 + npred - 1)))
        finally:
            e.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][1].any()


def _quant_model(seed):
    """TINY_QWEN3 in the Q4_K_M mix: raw blocks per matrix + the oracle's view (f16(dequant))."""
    from oracle import quants as Q
    from oracle.synth import f16_rne
    base = R.tiny_weights()
    H, F, V = CFG.hidden, CFG.ffn, CFG.vocab
    shapes = {"wq": (HQ * D, H), "wk": (HK * D, H), "wv": (HK * D, H), "wo": (H, HQ * D), "w_gate": (F, H),
              "w_up": (F, H), "w_down": (H, F)}
    qw, w = {}, {"final_norm": base["final_norm"], "layers": []}
    for i, name in enumerate(("embed", "lm_head")):
        qt = Q.q4_k_m_type(name, 0, NL)
        blk = Q.random_blocks(qt, V * H // 256, seed=seed + i, scale=R.STD)
        qw[name] = (qt, blk)
        w[name] = f16_rne(Q.dequant(blk, qt)).reshape(V, H)
    for l in range(NL):
        ly = {k: base["layers"][l][k] for k in ("attn_norm", "ffn_norm", "q_norm", "k_norm")}
        for i, (name, (r, c)) in enumerate(shapes.items()):
            qt = Q.q4_k_m_type(name, l, NL)
            blk = Q.random_blocks(qt, r * c // 256, seed=seed * 1000 + l * 10 + i, scale=R.STD)
            qw[(l, name)] = (qt, blk)
            ly[name] = f16_rne(Q.dequant(blk, qt)).reshape(r, c)
        w["layers"].append(ly)
    return qw, w


def test_quantized_engine_greedy_vs_oracle(monkeypatch):
    """A Q4_K_M-mix TINY_QWEN3 engine of 8 slots against the oracle on its exact dequantisation
    (tests/test_gpu_parity.py test_quantized_engine_greedy_vs_oracle's shape)."""
    from oracle import quants as Q
    qw, w = _quant_model(3)
    assert {qt for (qt, _) in qw.values()} == {Q.GGML_TYPE_Q4_K, Q.GGML_TYPE_Q6_K}
    oracle_q = R.OracleQwen3(CFG, w)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    e = Engine(CFG, device=0, max_batch=8, max_ctx=512, max_prefill_tokens=2048)
    try:
        load_quantized(e, qw, w)
        prompts = [_prompt(n, 700 + n) for n in (17, 140, 301, 64)]
        res = e.generate(prompts, num_predict=48, ignore_eos=True)
        agree = total = 0
        for p, r in zip(prompts, res):
            a, flips, _ = _agreement(oracle_q, p, r.ids)
            agree += a
            total += len(r.ids)
            for pos, gap, top in flips:
                assert gap <= 1e-2 * (abs(top) + 1.0), (pos, gap, top)
        assert agree / total >= 0.97, (agree, total)
        _, lg = e.forward(prompts[1], hidden=False, logits=True)
        ref_lg, _ = oracle_q.forward(prompts[1], all_logits=True)
        print(f"QWEN3 Q4_K_M: {agree}/{total} steps agree, prefill logits {rel(lg, ref_lg):.2e}")
        assert rel(lg, ref_lg) < 2e-2
    finally:
        e.close()


# ------------------------------------------------------------------ Qwen3-8B widths
WIDE = QWEN3_8B.with_(name="qwen3-8b-2l", n_layers=2, vocab=4096, bos_id=4000, eos_ids=(4001, 4002))
WSEED, WSTD, WJIT = 77, 0.02, 0.1


@pytest.fixture(scope="module")
def wide_weights():
    w = make_weights(WIDE, WSEED, std=WSTD, jitter=WJIT)  # what ms_init_synthetic generates on the device
    rng = np.random.default_rng(5)
    for ly in w["layers"]:
        ly["q_norm"] = (1 + 0.3 * rng.standard_normal(D)).astype(np.float16).astype(np.float32)
        ly["k_norm"] = (1 + 0.3 * rng.standard_normal(D)).astype(np.float16).astype(np.float32)
    return w


@pytest.mark.timeout(600)
@pytest.mark.parametrize("slots", [8, 128])
def test_full_width_two_layers(monkeypatch, wide_weights, slots):
    """hidden 4096, 32 / 8 heads, ffn 12288 (K = 4096 / 12288 in every decode projection), synthetic
    weights with explicit random gains: a 96-token prompt and 8 decode steps; the logits after the
    prefill and after the last step within 2e-2 of the reference."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MS_DECODE_RUN", "1")
    ids = _prompt(96, 9)
    oracle = R.OracleQwen3(WIDE, wide_weights)
    samp = Sampling(temperature=1.0, top_k=1, top_p=1.0, min_p=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=3)
    e = Engine(WIDE, device=0, max_batch=slots, max_ctx=256, max_prefill_tokens=256)
    try:
        e.init_synthetic(WSEED, WSTD, WJIT)
        for l, ly in enumerate(wide_weights["layers"]):
            e.load_tensor(L.MS_T_Q_NORM, l, f32_to_f16_bits(ly["q_norm"]))
            e.load_tensor(L.MS_T_K_NORM, l, f32_to_f16_bits(ly["k_norm"]))
        # top_k = 1 sampling draws the argmax and leaves the step's full fp32 logits behind
        got = e.generate([ids], num_predict=9, ignore_eos=True, sampling=samp)[0].ids
        assert len(got) == 9
        V = WIDE.vocab
        first = e.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, V * 4).view(np.float32)
        last = e.debug_read(L.MS_DBG_DECODE_LOGITS, 0, V * 4).view(np.float32)
        ref, _ = oracle.forward(np.concatenate([ids, np.asarray(got[:-1], np.int32)]), all_logits=True)
        d0, d8 = rel(first, ref[len(ids) - 1]), rel(last, ref[-1])
        print(f"QWEN3 full width, {slots} slots: logits after prefill {d0:.2e}, after 8 decode steps {d8:.2e}")
        assert d0 < 2e-2 and d8 < 2e-2
        assert got[0] == int(np.argmax(first)) and got[-1] == int(np.argmax(last))
    finally:
        e.close()


# ------------------------------------------------------------------ guards
def test_guards(monkeypatch, lib):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    # the switch is per engine: a Llama engine beside a QK-norm one still is the Llama engine
    seed, std, jit = 1234, 0.05, 0.1
    llama = Engine(TINY, device=0, max_batch=8, max_ctx=256, max_prefill_tokens=512)
    qwen = Engine(CFG, device=0, max_batch=8, max_ctx=256, max_prefill_tokens=512)
    try:
        # after a weight load: MS_EBUSY, on both kinds of engine
        llama.init_synthetic(seed, std, jit)
        assert lib.ms_enable_qk_norm(llama.h) == L.MS_EBUSY
        load_logical(qwen, R.tiny_weights())
        assert lib.ms_enable_qk_norm(qwen.h) == L.MS_EBUSY
        # q_norm on an engine without the switch is refused
        one = f32_to_f16_bits(np.ones(D, np.float32))
        assert lib.ms_load_weight(llama.h, L.MS_T_Q_NORM, 0, one.ctypes.data, D) == L.MS_EINVAL
        # the persistent step never runs on a QK-norm engine
        assert qwen.set_persist(True) is False
        # the gains are the last weight regions, two per layer of head_dim fp16 values
        rq, rl = qwen.weight_regions(), llama.weight_regions()
        assert [b for _, b in rq[-2 * NL:]] == [2 * D] * (2 * NL)
        assert len(rq) == len(rl) + 1 + 2 * NL  # + the untied lm_head
        # one token-level assertion of test_gpu_parity's greedy test on the Llama engine, with a
        # QK-norm engine generating in the same process in between
        p = _prompt(130, 230)
        before = llama.generate([p], num_predict=8, ignore_eos=True)[0].ids
        qwen.generate([p], num_predict=8, ignore_eos=True)
        after = llama.generate([p], num_predict=8, ignore_eos=True)[0].ids
        assert before == after
        oracle = OracleLlama(TINY, make_weights(TINY, seed, std=std, jitter=jit))
        a, flips, _ = _agreement(oracle, p, after)
        for pos, gap, top in flips:
            assert gap <= 1e-2 * (abs(top) + 1.0), (pos, gap, top)
    finally:
        llama.close()
        qwen.close()
    # a fresh engine takes the switch once, and again before anything was loaded
    h = C.c_void_p()
    c = L.MsConfig()
    c.abi_version = L.MS_ABI_VERSION
    c.n_layers, c.hidden, c.n_heads, c.n_kv_heads, c.head_dim, c.ffn, c.vocab = 2, 1024, 8, 2, 128, 2048, 4096
    c.rope_theta, c.norm_eps, c.max_batch, c.max_ctx, c.max_prefill_tokens = 1e6, 1e-6, 2, 128, 128
    assert lib.ms_create(C.byref(c), C.byref(h)) == 0
    try:
        assert lib.ms_enable_qk_norm(h) == 0 and lib.ms_enable_qk_norm(h) == 0
        ids = (C.c_int32 * 4)(1, 2, 3, 4)
        assert lib.ms_submit(h, ids, 4, 2, 0, 1) == 0
        assert lib.ms_enable_qk_norm(h) == L.MS_EBUSY
    finally:
        lib.ms_destroy(h)


# ------------------------------------------------------------------ end to end
def test_ollamallm_qwen3_through_the_store(monkeypatch, tmp_path):
    """A tiny qwen3 GGUF with a toy vocabulary (pre = "qwen2") in an Ollama-style store, through
    OllamaLLM(model="qwen3:tiny"): the batched call equals the sequential calls byte for byte, and
    the prompt the engine receives starts with <|im_start|>user\\n and carries no BOS."""
    import test_gguf_qwen3 as G
    from mapsum import compat, template
    from test_ollama_gguf import CHATML, ollama_store_with
    tok_meta = G.toy_qwen_vocab()
    g = str(tmp_path / "model.gguf")
    G.float_qwen3_gguf(g, R.tiny_weights(), tok_meta[1])
    ollama_store_with(str(tmp_path), "qwen3:tiny", g, G.PARAMS, template=CHATML)
    for k in KNOBS + ("MAPSUM_MODEL_DIR", "MAPSUM_GGUF"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (("OLLAMA_MODELS", str(tmp_path)), ("MAPSUM_MAX_BATCH", "4"), ("MAPSUM_MAX_CTX", "1024"),
                 ("MAPSUM_MAX_PREFILL", "4096")):
        monkeypatch.setenv(k, v)
    compat._BACKENDS.pop("qwen3:tiny", None)
    try:
        llm = compat.OllamaLLM("http://localhost:11434", "qwen3:tiny", max_new_tokens=24, clean="none")
        prompts = [template.map_prompt("mapreduce", c) for c in
                   ("Chương 1. Nội dung chính của văn bản.", "Hà Nội, ngày 15 tháng 8 năm 2024.", "Phần II. Điều 7")]
        one_by_one = [llm._call(p) for p in prompts]
        be = compat.get_backend("qwen3:tiny")
        assert be.engine.cfg.qk_norm and be.template is template.render_chatml
        batched = be.generate(prompts, 24)
        assert [b.encode() for b in batched] == [s.encode() for s in one_by_one]
        ids = be.encode_prompt(prompts[0])
        user = be.tok.encode("user\n", add_bos=False)
        assert ids[0] == G.IM_START and ids[1:1 + len(user)] == user and G.ENDOFTEXT not in ids
        # the engine under the drop-in is the model of the file: the same ids on an engine loaded
        # from the logical weights
        e = _engine(monkeypatch, 4, max_ctx=1024, prefill=4096)
        try:
            want = e.generate([ids], num_predict=24, ignore_eos=True)[0].ids
        finally:
            e.close()
        assert be.engine.generate([ids], num_predict=24, ignore_eos=True)[0].ids == want
    finally:
        b = compat._BACKENDS.pop("qwen3:tiny", None)
        if b is not None:
            b.engine.close()
