"""The q8_0 KV cache on the GPU (DESIGN.md §2 "q8_0 KV cache"; CPU half: tests/test_kv_q8_0_ref.py).

Op level, on given bytes:
  ms_op_kv_store_q8_0     pool bytes EQUAL tests/kv_q8_0_ref.py's packer for T = 1 / 3 / 130 tokens at positions
                          62.., over two page edges and a shuffled table; no other byte changes;
  ms_op_attn_decode_q8_0  against float64 on the same bytes, 2e-3 norm-wise per output row (derived: at most
                          four fp16 roundings of <= 2^-11; the CPU emulation stays under half of it, every mutant
                          -- a decisive key dropped, two V rows swapped, a neighbouring block's scale, the other
                          kv head -- at >= 10 x it): G = 3 and 4, lens 1 / 63 / 64 / 65 / 512 / 513 / 1590 in one
                          batch, ppw 2 and 16, table-backed and slot-major pools.  The GPU maximum is recorded in
                          tests/golden/kv_q8_0_bounds.json.

Engine level (TINY, tests/decode_edges_ref.py's weights), a q8_0-KV engine beside an fp16 one:
  prefill logits and first tokens bit-equal; the q8_0 pool bytes of every prompt position in every layer equal
  the reference quantiser applied to the fp16 engine's pool rows; 32 teacher-forced decode steps on the mirror's
  tokens (OracleLlama with mut["attend"] quantising K and V on decode calls) within 2e-2, every decisive
  position agreeing; stray bytes after each step; a prompt alone; a poisoned embedding row; the switches' rules.

The forced (greedy) decode steps leave {max, id} partials per 16-column tile, not logits rows (the engine's
lm_head writes nothing else there): the forced run's distance is taken over each row's 256 tile maxima, as
tests/test_gpu_decode_edges.py does, and a second, sampling run (top_k = 1: the draw is the argmax) gives the
full fp32 logits of every step against the mirror fed the engine's own ids.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import decode_edges_ref as E  # noqa: E402
import kv_q8_0_ref as R  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from mapsum.config import TINY, TINY_QWEN3  # noqa: E402
from mapsum.engine import Engine, Sampling  # noqa: E402

PAGE, D = R.PAGE, R.D
KNOBS = ("MS_ATTN_PPB", "MS_ATTN_TICKET", "MS_ATTN_V2", "MS_ATTN_PPW", "MS_ATTN_SLABS", "MS_RESID_FUSED",
         "MS_KV_PAGED", "MS_DECODE_RUN", "MS_GRAPH_STEPS", "MS_PERSIST")
BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kv_q8_0_bounds.json")
NORTH_STAR = 2e-2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ op level: the writer
S_SLOTS, S_MAX_PAGES, S_POOL_PAGES, S_HK = 4, 3, 16, 2


@pytest.mark.parametrize("T", [1, 3, 130])
def test_op_kv_store_bytes(lib, T):
    rng = np.random.default_rng(100 + T)
    pos = (62 + np.arange(T)).astype(np.int32)  # T = 130: 62 .. 191, over the page edges at 64 and 128
    slot = np.array([2, 0, 3], np.int32)[np.arange(T) % 3]
    bt = rng.permutation(S_POOL_PAGES)[:S_SLOTS * S_MAX_PAGES].reshape(S_SLOTS, S_MAX_PAGES).astype(np.int32)
    assert not np.array_equal(bt.ravel(), np.arange(S_SLOTS * S_MAX_PAGES))
    amp = 10.0 ** rng.uniform(-5, 3, (T, S_HK, 4)).repeat(32, axis=-1)
    k = (rng.standard_normal((T, S_HK, D)) * amp).astype(np.float16)
    v = (rng.standard_normal((T, S_HK, D)) * amp[::-1]).astype(np.float16)
    k[0, 0, :32] = 0                       # an all-zero block
    v[0, 1, 40] = np.nan                   # a NaN block
    k[T - 1, 1, 64:96] = 0
    k[T - 1, 1, 70] = np.float16(2.0 ** -24)  # the smallest subnormal alone
    v[T - 1, 0, 97] = 65504.0
    v[T // 2, 0, 0:4] = [127.0, 0.5, -0.5, 2.5]  # .5 cases of each sign at d = 1
    fill = ((np.arange(S_POOL_PAGES * S_HK * R.SLAB, dtype=np.int64) * 7919 + 13) % 251).astype(np.uint8)
    want_k = fill.reshape(S_POOL_PAGES, S_HK, R.SLAB).copy()
    want_v = want_k.copy()
    kc, ks = R.quantize_rows(k)
    vc, vs = R.quantize_rows(v)
    for t in range(T):
        page = int(bt[slot[t], pos[t] // PAGE])
        for h in range(S_HK):
            R.pack_rows(want_k, page, h, pos[t] % PAGE, kc[t, h], ks[t, h])
            R.pack_rows(want_v, page, h, pos[t] % PAGE, vc[t, h], vs[t, h])
    kp, vp = _dev(fill), _dev(fill)
    kd, vd, pd, sd, bd = _dev(k.view(np.int16)), _dev(v.view(np.int16)), _dev(pos), _dev(slot), _dev(bt)
    rc = lib.ms_op_kv_store_q8_0(kd.data_ptr(), vd.data_ptr(), T, S_HK, pd.data_ptr(), sd.data_ptr(), kp.data_ptr(),
                                 vp.data_ptr(), bd.data_ptr(), S_MAX_PAGES, _stream())
    assert rc == 0, lib.ms_last_error(None)
    torch.cuda.synchronize()
    for name, got, want in (("k", kp, want_k), ("v", vp, want_v)):
        got = got.cpu().numpy().reshape(want.shape)
        diff = np.argwhere(got != want)
        assert diff.size == 0, f"{name} pool: {len(diff)} bytes differ from the packer, first (page, kv head, byte) = " \
                               f"{diff[0].tolist()}: {int(got[tuple(diff[0])])} != {int(want[tuple(diff[0])])}"
        assert (got != fill.reshape(want.shape)).any()


# ------------------------------------------------------------------ op level: decode attention
_GPU_MAX = {}


@pytest.mark.parametrize("slot_major", [0, 1])
@pytest.mark.parametrize("ppw", [2, 16])
@pytest.mark.parametrize("G", [3, 4])
def test_op_attn_decode_against_float64(lib, G, ppw, slot_major):
    oc = R.op_case(G, 4 * ppw * PAGE)
    case, ref, emul = oc["case"], oc["ref"], oc["emul"]
    B, Hq, HK = len(R.LENS), case.Hq, R.HK
    if slot_major:  # page p of slot s is page s * max_pages + p; the table the launch gets is all page 0:
        table = np.arange(B * R.MAX_PAGES, dtype=np.int32).reshape(B, R.MAX_PAGES)  # a lookup would show
        table_dev = np.zeros_like(table)
    else:
        table = np.random.default_rng(9).permutation(B * R.MAX_PAGES + 5)[:B * R.MAX_PAGES]
        table_dev = table = table.reshape(B, R.MAX_PAGES).astype(np.int32)
    kp, vp = case.pools(table)
    row = (Hq + 2 * HK) * D
    qkv = np.zeros((B, row), np.float16)
    qkv[:, :Hq * D] = case.q.reshape(B, Hq * D)
    qkv[:, Hq * D:] = np.float16(np.nan)  # the K / V parts of the rows are not the kernel's business
    max_len = max(R.LENS)
    ws_bytes = lib.ms_op_attn_decode_q8_0_workspace(B, Hq, max_len, ppw)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    out = torch.full((B, Hq * D), float("nan"), dtype=torch.float16, device="cuda")
    qd, kd, vd, td = _dev(qkv.view(np.int16)), _dev(kp), _dev(vp), _dev(table_dev)
    ld, sd = _dev(np.array(R.LENS, np.int32)), _dev(np.arange(B, dtype=np.int32))
    rc = lib.ms_op_attn_decode_q8_0(qd.data_ptr(), Hq, HK, kd.data_ptr(), vd.data_ptr(), td.data_ptr(), R.MAX_PAGES,
                                    slot_major, ld.data_ptr(), sd.data_ptr(), B, max_len, ppw, ws.data_ptr(),
                                    out.data_ptr(), _stream())
    assert rc == 0, lib.ms_last_error(None)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64).reshape(B, Hq, D)
    worst, worst_emul = 0.0, 0.0
    for i in range(B):
        for h in range(Hq):
            d = R.row_rel(got[i, h], ref[i, h])
            worst, worst_emul = max(worst, d), max(worst_emul, R.row_rel(emul[i, h], ref[i, h]))
            assert d <= R.BAR, f"sequence {i} (len {R.LENS[i]}), q head {h} (decisive key {case.pos[i, h]}): " \
                               f"{d:.2e} > {R.BAR:.0e} from float64 on the same bytes"
    print(f"KVQ8 attn G={G} ppw={ppw} slot_major={slot_major}: GPU worst row {worst:.2e}, emulation "
          f"{worst_emul:.2e}, bar {R.BAR:.0e}")
    _GPU_MAX[f"G{G}_ppw{ppw}_sm{slot_major}"] = worst
    with open(BOUNDS) as f:
        rec = json.load(f)
    assert rec["bar"] == R.BAR and worst_emul <= R.BAR / 2


# ------------------------------------------------------------------ engine level
LENS = (33, 64, 127, 190)
NSTEPS = 33  # the prefill's token + 32 decode steps
MAX_CTX = 256


def _prompts():
    return [np.random.default_rng(9100 + n).integers(0, 4000, size=n).astype(np.int32) for n in LENS]


def _engine(kv, max_batch=4, cfg=TINY):
    """TINY on tests/decode_edges_ref.py's synthetic weights, TINY_QWEN3 on tests/qwen3_ref.py's."""
    e = Engine(cfg, device=0, max_batch=max_batch, max_ctx=MAX_CTX, max_prefill_tokens=1024, kv_cache_type=kv)
    if cfg is TINY:
        e.init_synthetic(E.SEED, E.STD, E.JITTER)
    else:
        import qwen3_ref as Q
        from mapsum.weights import load_logical
        load_logical(e, Q.tiny_weights())
    return e


_MIRROR = {}


def _mirror(feed=None, qwen=False):
    """Per prompt: the mirror's run -- greedy on its own tokens, or fed ``feed`` -- as tokens, scaled logits and
    un-scaled lm_head sums per step.  Llama: OracleLlama with mut["attend"] on the decode calls; the QK-norm
    model: tests/kv_q8_0_ref.py's restatement of OracleQwen3.forward with the same edit."""
    key = (qwen, None if feed is None else tuple(tuple(f) for f in feed))
    if key not in _MIRROR:
        import qwen3_ref as Q
        o, out = (Q.tiny_oracle() if qwen else E.oracle()), []

        def fwd(ids, cache, decode):
            if qwen:
                return R.qwen3_mirror_forward(o, ids, cache, decode)
            return o.forward(ids, cache, mut={"attend": R.mirror_hook} if decode else None)[0]

        for i, p in enumerate(_prompts()):
            cache = o.new_cache()
            lg = fwd(p, cache, False)
            logits, uns, toks = [lg], [E._unscaled(o, lg)], [int(np.argmax(lg))]
            for j in range(1, NSTEPS):
                lg = fwd([toks[j - 1] if feed is None else int(feed[i][j - 1])], cache, True)
                logits.append(lg)
                uns.append(E._unscaled(o, lg))
                toks.append(int(np.argmax(lg)))
            out.append({"tokens": toks, "logits": np.stack(logits), "unscaled": np.stack(uns)})
        _MIRROR[key] = out
    return _MIRROR[key]


def _q8_pools(e, cfg, max_batch):
    """(K, V) pools uint8 [layer][slot][page][kv head][8704] of a slot-major q8_0-KV engine."""
    mp = (MAX_CTX + PAGE - 1) // PAGE
    shape = (cfg.n_layers, max_batch, mp, cfg.n_kv_heads, R.SLAB)
    n = int(np.prod(shape))
    return (e.debug_read(L.MS_DBG_KPOOL, 0, n).reshape(shape), e.debug_read(L.MS_DBG_VPOOL, 0, n).reshape(shape))


def _f16_pools(e, cfg, max_batch):
    mp = (MAX_CTX + PAGE - 1) // PAGE
    shape = (cfg.n_layers, max_batch, mp, cfg.n_kv_heads, PAGE, D)
    n = int(np.prod(shape)) * 2
    return (e.debug_read(L.MS_DBG_KPOOL, 0, n).view(np.uint16).reshape(shape),
            e.debug_read(L.MS_DBG_VPOOL, 0, n).view(np.uint16).reshape(shape))


def _check_quantised(q8, f16, lens, layers, what):
    """The q8_0 pools' rows of positions [0, lens[s]) equal the reference quantiser on the fp16 pools' rows."""
    for name, qp, fp in (("k", q8[0], f16[0]), ("v", q8[1], f16[1])):
        codes, scales = R.unpack_pool(qp)
        for l in layers:
            for s, n in enumerate(lens):
                rows = fp[l, s].transpose(0, 2, 1, 3).reshape(-1, fp.shape[3], D)[:n]  # [n][kv head][128]
                wc, wsc = R.quantize_rows(rows)
                gc = codes[l, s].transpose(0, 2, 1, 3).reshape(-1, fp.shape[3], D)[:n]
                gs = scales[l, s].transpose(0, 2, 1, 3).reshape(-1, fp.shape[3], R.NB)[:n]
                bad = np.argwhere((gc != wc).any(axis=-1) | (gs != wsc).any(axis=-1))
                assert bad.size == 0, f"{what}: {name} pool, layer {l}, slot {s}: {len(bad)} rows are not the " \
                                      f"quantiser's, first (position, kv head) = {bad[0].tolist()}"


def _check_stray(before, after, old_lens, new_lens):
    allowed = np.zeros(before[0].shape, bool)
    for s, (a, b) in enumerate(zip(old_lens, new_lens)):
        for pos in range(a, b):
            pg, off = pos // PAGE, pos % PAGE
            allowed[:, s, pg, :, off * D:(off + 1) * D] = True
            allowed[:, s, pg, :, R.CODE_BYTES + off * 8:R.CODE_BYTES + off * 8 + 8] = True
    for name, x, y in (("k", before[0], after[0]), ("v", before[1], after[1])):
        stray = np.argwhere((x != y) & ~allowed)
        assert stray.size == 0, f"{name} pool: {len(stray)} bytes outside the step's new rows changed, first " \
                                f"(layer, slot, page, kv head, byte) = {stray[0].tolist()}"


def _partials(e, B, cfg=TINY):
    tiles = cfg.vocab // 16
    p = e.debug_read(L.MS_DBG_DECODE_LOGITS, 0, B * tiles * 8).view(np.float32).reshape(B, tiles, 2)
    return p[..., 0].copy()


def _fp16_engine_run(cfg, max_batch, prompts, forced, n=2):
    """The fp16-cache engine on the same weights and prompts: prefill logits, pools after its run, ids."""
    B = len(prompts)
    f = _engine("f16", max_batch, cfg=cfg)
    try:
        tags = [f.submit_forced(p, t, n) for p, t in zip(prompts, forced)]
        f.step()
        first = f.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, B * cfg.vocab * 4).view(np.uint32).reshape(B, -1).copy()
        while f.pending():
            f.step()
        pools = _f16_pools(f, cfg, max_batch)
        f.collect()
        got = f.take(tags)
        return first, pools, [got[t].ids for t in tags]
    finally:
        f.close()


def _forced_run_against_mirror(e, cfg, max_batch, prompts, mir, f_first, f_pools, f_ids, what):
    """32 teacher-forced decode steps of a q8_0-KV engine on the mirror's tokens, every check of the module
    docstring after every step."""
    B = len(prompts)
    forced = [m["tokens"][:-1] for m in mir]
    assert e.set_persist(True) is False
    assert e.lib.ms_enable_kv_q8_0(e.h) == L.MS_EBUSY  # after a weight load
    before = _q8_pools(e, cfg, max_batch)
    assert not before[0].any() and not before[1].any()
    tags = [e.submit_forced(p, t, NSTEPS) for p, t in zip(prompts, forced)]
    pad = [0] * (max_batch - B)
    lens, dist, sq, cnt = [0] * B, 0.0, 0.0, 0
    for j in range(1, NSTEPS):
        pending = e.step()
        assert (pending == 0) == (j == NSTEPS - 1), (j, pending)
        after = _q8_pools(e, cfg, max_batch)
        new_lens = [len(p) + j for p in prompts]
        _check_stray(before, after, lens + pad, new_lens + pad)
        if j == 1:
            first = e.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, B * cfg.vocab * 4).view(np.uint32).reshape(B, -1)
            assert np.array_equal(first, f_first), "prefill logits differ in bits from the fp16-cache engine's"
            _check_quantised(after, f_pools, [len(p) for p in prompts], range(cfg.n_layers), "prompt rows")
        pm = _partials(e, B, cfg)
        for i, m in enumerate(mir):
            want = E.tile_max(m["unscaled"][j])
            d = R.row_rel(pm[i], want)
            dist = max(dist, d)
            assert d <= NORTH_STAR, (j, i, d)
            sq += float(((pm[i] - want) ** 2).sum())
            cnt += want.size
        before, lens = after, new_lens
    e.collect()
    got = e.take(tags)
    ids = [got[t].ids for t in tags]
    assert all(got[t].finish == "length" and len(got[t].ids) == NSTEPS for t in tags)
    assert [i[0] for i in ids] == [i[0] for i in f_ids], "first tokens differ from the fp16-cache engine's"
    # decisive positions: the mirror's top-2 gap (un-scaled lm_head sums, the partials' units) exceeds 4 x the
    # run's measured rms difference; each must agree, and they are >= 80 % of all
    rms = (sq / cnt) ** 0.5
    decisive = agree = 0
    for i, m in enumerate(mir):
        for j in range(1, NSTEPS):
            top2 = np.sort(m["unscaled"][j])[-2:]
            if top2[1] - top2[0] > 4 * rms:
                decisive += 1
                assert ids[i][j] == m["tokens"][j], (i, j, ids[i][j], m["tokens"][j], float(top2[1] - top2[0]), rms)
            agree += ids[i][j] == m["tokens"][j]
    total = B * (NSTEPS - 1)
    print(f"KVQ8 engine {what}: tile maxima within {dist:.2e} of the mirror (north star {NORTH_STAR}), "
          f"rms {rms:.2e}, decisive {decisive}/{total}, agreeing {agree}/{total}")
    assert decisive >= 0.8 * total, (decisive, total)
    return before


@pytest.mark.parametrize("max_batch", [4, 20, 72])
def test_engine_against_fp16_engine_and_mirror(max_batch):
    """4 slots (the small regime), 20 (split GEMV + residual_rmsnorm) and 72 (the skinny-GEMM regime)."""
    prompts, mir = _prompts(), _mirror()
    f_first, f_pools, f_ids = _fp16_engine_run(TINY, max_batch, prompts, [m["tokens"][:-1] for m in mir])
    e = _engine("q8_0", max_batch)
    try:
        _forced_run_against_mirror(e, TINY, max_batch, prompts, mir, f_first, f_pools, f_ids, f"{max_batch} slots")
    finally:
        e.close()


def test_engine_full_logits_and_alone(monkeypatch):
    """A sampling run with top_k = 1 leaves the full scaled logits of every step: within 2e-2 of the mirror fed
    the engine's own ids.  Then the 127-token prompt alone gives the ids it gave in the batch."""
    prompts, B = _prompts(), len(LENS)
    samp = Sampling(temperature=1.0, top_k=1, top_p=1.0, min_p=0.0, repeat_penalty=1.0, repeat_last_n=0, seed=3)
    e = _engine("q8_0")
    monkeypatch.setenv("MS_DECODE_RUN", "1")  # one decode step per step(): every step's logits are read
    e2 = _engine("q8_0")
    monkeypatch.delenv("MS_DECODE_RUN")
    try:
        tags = [e2.submit(p, NSTEPS, True, sampling=samp) for p in prompts]
        logits = []
        for j in range(1, NSTEPS):
            e2.step()
            if j == 1:
                logits.append(e2.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, B * 4096 * 4).view(np.float32).reshape(B, -1).copy())
            logits.append(e2.debug_read(L.MS_DBG_DECODE_LOGITS, 0, B * 4096 * 4).view(np.float32).reshape(B, -1).copy())
        e2.collect()
        got = e2.take(tags)
        ids = [got[t].ids for t in tags]
        mir = _mirror([t[:-1] for t in ids])
        worst = max(R.row_rel(logits[j][i], mir[i]["logits"][j]) for i in range(B) for j in range(NSTEPS))
        print(f"KVQ8 engine full logits: worst row {worst:.2e} from the mirror (north star {NORTH_STAR})")
        assert worst <= NORTH_STAR
        # greedy, chained runs, in the batch and alone (slot 0 instead of slot 2)
        batch = [r.ids for r in e.generate(prompts, num_predict=NSTEPS, ignore_eos=True)]
        alone = e.generate([prompts[2]], num_predict=NSTEPS, ignore_eos=True)[0].ids
        assert alone == batch[2]
    finally:
        e.close()
        e2.close()


def test_engine_sampled_ids_across_slots():
    """One sampled request gives the same ids in slot 0 of an idle engine and in slot 3 of a full one."""
    prompts = _prompts()
    samp = Sampling(temperature=0.8, top_k=40, top_p=0.9, min_p=0.0, repeat_penalty=1.1, repeat_last_n=64, seed=77)
    e = _engine("q8_0")
    try:
        alone = e.generate([prompts[1]], num_predict=16, ignore_eos=True, sampling=samp)[0].ids
        full = e.generate([prompts[0], prompts[2], prompts[3], prompts[1]], num_predict=16, ignore_eos=True,
                          sampling=samp)[3].ids
        assert alone == full and len(alone) == 16
    finally:
        e.close()


def test_engine_poisoned_embedding_row():
    """A NaN embedding row reaches the logits through the quantised cache (scale NaN, codes 0): that chunk
    finishes in error, its neighbour does not."""
    from mapsum.weights import f32_to_f16_bits
    from oracle.synth import make_weights
    emb = make_weights(TINY, E.SEED, std=E.STD, jitter=E.JITTER)["embed"].astype(np.float32).copy()
    emb[1234, :] = np.nan
    e = _engine("q8_0")
    try:
        e.load_tensor(L.MS_T_EMBED, 0, f32_to_f16_bits(emb))
        good = np.random.default_rng(1).integers(0, 1000, size=40).astype(np.int32)
        bad = good.copy()
        bad[17] = 1234
        res = e.generate([good, bad], num_predict=6, ignore_eos=True)
        assert res[0].finish == "length" and len(res[0].ids) == 6
        assert res[1].finish == "error"
    finally:
        e.close()


def test_switch_rules():
    """Either order with ms_enable_qk_norm, before any weight load; idempotent; MS_EBUSY afterwards."""
    for order in ("kv_first", "qk_first"):
        e = Engine(TINY, device=0, max_batch=2, max_ctx=128, max_prefill_tokens=128)
        try:
            calls = [e.lib.ms_enable_kv_q8_0, e.lib.ms_enable_qk_norm]
            for fn in (calls if order == "kv_first" else calls[::-1]):
                assert fn(e.h) == 0
            assert e.lib.ms_enable_kv_q8_0(e.h) == 0
            assert e.set_persist(True) is False
            e.init_synthetic(1, 0.03, 0.1)
            assert e.lib.ms_enable_kv_q8_0(e.h) == L.MS_EBUSY
        finally:
            e.close()
    e = Engine(TINY, device=0, max_batch=2, max_ctx=128, max_prefill_tokens=128)
    try:
        e.init_synthetic(1, 0.03, 0.1)
        assert e.lib.ms_enable_kv_q8_0(e.h) == L.MS_EBUSY
    finally:
        e.close()


def test_qwen3_engine_both_switches(monkeypatch):
    """TINY_QWEN3 with both switches against its mirror at the same bars, beside the same model on an fp16 cache
    (MS_ATTN_SLABS=0 for that one: both then run the rows form of the QK-norm kernel).  Layer 0's rows do not
    depend on attention, so under the same forced tokens every DECODED token's layer-0 row is the quantiser's
    image of the fp16 engine's too, bit for bit."""
    cfg, prompts, mir = TINY_QWEN3, _prompts(), _mirror(qwen=True)
    monkeypatch.setenv("MS_ATTN_SLABS", "0")
    f_first, f_pools, f_ids = _fp16_engine_run(cfg, 4, prompts, [m["tokens"][:-1] for m in mir], n=NSTEPS)
    monkeypatch.delenv("MS_ATTN_SLABS")
    e = _engine("q8_0", cfg=cfg)
    try:
        pools = _forced_run_against_mirror(e, cfg, 4, prompts, mir, f_first, f_pools, f_ids, "qwen3, both switches")
    finally:
        e.close()
    _check_quantised(pools, f_pools, [len(p) + NSTEPS - 1 for p in prompts], [0], "layer 0, prompt and decoded rows")
