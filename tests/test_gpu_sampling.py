"""Sampled decoding on the GPU (needs a GPU): the row sampler through ms_op_sample against the
float64 restatement in tests/sampling_ref.py, and the engine's sampling runs (ms_submit_sampled:
the fp32-store lm_head + the fused sampling tail inside the chained decode graphs).

Bars.  Candidate ids: exactly the reference's, in order (the generator redraws on the CPU any case
whose top-p / min-p boundary margin is under 1e-4, so nothing is skipped).  Candidate
probabilities: 1e-5 absolute (fp32 exp of arguments up to ~30 in magnitude is good to ~2e-6
relative, the sum has <= 256 terms, probabilities are <= 1).  Drawn ids: the reference's whenever
u is at least 1e-5 away from every reference CDF boundary, and at most 1 % of the draws may be
excused by that rule (<= 256 boundaries of width 2e-5: 0.5 % in the worst case)."""
import asyncio
import ctypes as C

import numpy as np
import pytest

import sampling_ref as R
from mapsum import _lib as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

P_TOL = 1e-5
EXCUSE_CAP = 0.01


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _params_dev(psets, dev):
    arr = (L.MsSampling * len(psets))(*[L.MsSampling(p.temperature, p.top_k, p.top_p, p.min_p, p.repeat_penalty,
                                                     p.repeat_last_n, p.seed) for p in psets])
    raw = np.frombuffer(arr, dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(dev)


def op_sample(lib, dev, logits, psets, wins, steps, cands=True):
    """ms_op_sample over host arrays; returns (ids, cand_ids, cand_p, cand_n) as numpy."""
    lg = torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev)
    rows, n = lg.shape
    w = np.zeros((rows, 256), np.int32)
    wl = np.zeros(rows, np.int32)
    for r in range(rows):
        t = np.asarray(wins[r], np.int32)[-256:]
        w[r, :t.size], wl[r] = t, t.size
    wd, wld = torch.from_numpy(w).to(dev), torch.from_numpy(wl).to(dev)
    st = torch.from_numpy(np.asarray(steps, np.int32)).to(dev)
    pd = _params_dev(psets, dev)
    ids = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    ci = torch.full((rows, 256), -7, dtype=torch.int32, device=dev)
    cp = torch.zeros((rows, 256), dtype=torch.float32, device=dev)
    cn = torch.full((rows,), -7, dtype=torch.int32, device=dev)
    L.check(lib.ms_op_sample(lg.data_ptr(), rows, n, n, pd.data_ptr(), wd.data_ptr(), wld.data_ptr(), st.data_ptr(),
                             ids.data_ptr(), ci.data_ptr() if cands else None, cp.data_ptr() if cands else None,
                             cn.data_ptr() if cands else None, _stream()), None, "ms_op_sample")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), ci.cpu().numpy(), cp.cpu().numpy(), cn.cpu().numpy()


def _check_rows(ids, ci, cp, cn, cands, psets, steps):
    excused = 0
    for r, (c, p) in enumerate(zip(cands, psets)):
        k = int(cn[r])
        assert k == c.ids.size, (r, k, c.ids.size)
        assert ci[r, :k].tolist() == c.ids.tolist(), r
        err = float(np.abs(cp[r, :k].astype(np.float64) - c.probs).max())
        print(f"row {r}: {k} candidates, max |p - ref| = {err:.2e}")
        assert err <= P_TOL, (r, err)
        uu = R.u(p.seed, int(steps[r]))
        if R.excused(c, uu) and p.temperature > 0:
            excused += 1
        else:
            assert int(ids[r]) == R.draw(c, uu), r
    return excused


# ------------------------------------------------------------------ op level
@pytest.mark.parametrize("n,rows,quantised", R.OP_SHAPES)
def test_candidates_and_probabilities(lib, dev, n, rows, quantised):
    psets, logits, wins, cands, steps, _ = R.op_case(n, rows, quantised)
    ids, ci, cp, cn = op_sample(lib, dev, logits, psets, wins, steps)
    # (tests/test_sampling_ref.py: no draw of these cases is excused by the reference itself)
    assert _check_rows(ids, ci, cp, cn, cands, psets, steps) == 0
    # the ids do not depend on the candidate outputs being asked for
    ids2, *_ = op_sample(lib, dev, logits, psets, wins, steps, cands=False)
    assert ids2.tolist() == ids.tolist()


@pytest.mark.parametrize("n", [8191, 128256])
def test_rows_full_of_ties(lib, dev, n):
    """Four distinct logit values: a quarter of the row ties at the top, so the candidates are
    decided by the exact select over the whole row and the lowest-id rule among thousands of ties."""
    psets, logits, wins, cands, steps, _ = R.tie_case(n)
    ids, ci, cp, cn = op_sample(lib, dev, logits, psets, wins, steps)
    assert _check_rows(ids, ci, cp, cn, cands, psets, steps) == 0


def test_top_k_above_n(lib, dev):
    n = 200
    psets = [R.Params(1.0, 256, 1.0, 0.0, 1.2, 64, seed=3), R.Params(0.9, 256, 0.9, 0.0, 1.1, 64, seed=4),
             R.Params(1.1, 201, 1.0, 0.01, 1.0, 0, seed=5)]
    logits, wins, cands, _ = R.make_case(12, n, psets, False)
    assert cands[0].ids.size == n
    steps = [0, 1, 2]
    ids, ci, cp, cn = op_sample(lib, dev, logits, psets, wins, steps)
    assert _check_rows(ids, ci, cp, cn, cands, psets, steps) == 0


@pytest.mark.parametrize("pi,quantised", R.DRAW_CASES)
def test_drawn_ids_2048_pairs(lib, dev, pi, quantised):
    base, logits, win, c, seeds, steps, _ = R.draw_case(pi, quantised)
    rows = R.DRAWS
    psets = [R.with_seed(base, int(s)) for s in seeds]
    ids, *_ = op_sample(lib, dev, np.repeat(logits, rows, 0), psets, [win] * rows, steps, cands=False)
    excused = 0
    for r in range(rows):
        uu = R.u(int(seeds[r]), int(steps[r]))
        if R.excused(c, uu):
            excused += 1
        else:
            assert int(ids[r]) == R.draw(c, uu), (r, uu)
    print(f"pset {pi}: {c.ids.size} candidates, {excused} of {rows} draws excused")
    assert excused <= EXCUSE_CAP * rows
    assert len(set(ids.tolist())) > 1 or c.ids.size == 1


def test_non_finite_rows(lib, dev):
    n = 4097
    rng = np.random.default_rng(5)
    lg = (rng.standard_normal((6, n)) * 3).astype(np.float32)
    lg[0, :] = np.nan
    lg[1, :] = -np.inf
    lg[2, 77] = np.inf
    lg[3, ::2] = np.nan          # NaN entries never win
    lg[4, :] = -np.inf
    lg[4, 9] = 1.0               # one finite logit: it wins whatever the draw
    lg[5, 100:] = np.nan
    psets = [R.Params(0.8, 40, 0.9, 0.0, 1.1, 64, seed=r) for r in range(5)] + [R.Params(1.0, 256, 1.0, 0.0, 1.0, 0, seed=9)]
    wins = [rng.integers(0, n, size=64) for _ in range(6)]
    ids, ci, cp, cn = op_sample(lib, dev, lg, psets, wins, [0] * 6)
    assert ids[:3].tolist() == [-1, -1, -1] and cn[:3].tolist() == [0, 0, 0]
    assert ids[3] % 2 == 1 and not np.isnan(lg[3, ids[3]])
    assert all(i % 2 == 1 for i in ci[3, :cn[3]])
    assert ids[4] == 9
    assert cn[5] == 100 and sorted(ci[5, :100].tolist()) == list(range(100))
    for r in (3, 4, 5):
        assert int(ids[r]) == R.sample(lg[r], psets[r], wins[r], 0) or R.excused(
            R.candidates(lg[r], psets[r], wins[r]), R.u(psets[r].seed, 0))
    # greedy rows through the sampler: the same -1 rule
    g = [R.Params(0.0)] * 6
    ids, *_ = op_sample(lib, dev, lg, g, wins, [0] * 6, cands=False)
    assert ids[:3].tolist() == [-1, -1, -1] and ids[4] == 9


@pytest.mark.parametrize("n", [1000, 4097, 128256])
def test_top_k_1_is_argmax(lib, dev, n):
    rng = np.random.default_rng(n)
    rows = 8
    lg = np.round(rng.standard_normal((rows, n)) * 3 * 4).astype(np.float32) / 4  # ties at the top
    psets = [R.Params(0.3 + 0.4 * r, 1, 0.9, 0.0, 1.0, 64, seed=r) for r in range(rows)]
    ids, *_ = op_sample(lib, dev, lg, psets, [[1, 2, 3]] * rows, list(range(rows)), cands=False)
    d = torch.from_numpy(lg).to(dev)
    ref = torch.empty(rows, dtype=torch.int32, device=dev)
    L.check(lib.ms_op_argmax(d.data_ptr(), rows, n, ref.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert ids.tolist() == ref.cpu().tolist() == [int(np.argmax(lg[r])) for r in range(rows)]


def test_op_refuses_bad_shapes(lib, dev):
    z = torch.zeros(4096, dtype=torch.int32, device=dev)
    f = torch.zeros(4096, dtype=torch.float32, device=dev)
    args = (z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())
    assert lib.ms_op_sample(f.data_ptr(), 1, 0, 0, *args, None, None, None, _stream()) == L.MS_EINVAL
    assert lib.ms_op_sample(f.data_ptr(), 1, 131073, 131073, *args, None, None, None, _stream()) == L.MS_EINVAL
    assert lib.ms_op_sample(f.data_ptr(), 1, 100, 99, *args, None, None, None, _stream()) == L.MS_EINVAL
    assert lib.ms_op_sample(f.data_ptr(), 1, 100, 100, *args, z.data_ptr(), None, None, _stream()) == L.MS_EINVAL


# ------------------------------------------------------------------ engine level
from mapsum.config import TINY  # noqa: E402
from mapsum.engine import Engine, Sampling  # noqa: E402

NPRED = 48
WSEED, WSTD, WJIT = 7, 0.05, 0.1


def _prompts(k=8):
    rng = np.random.default_rng(17)
    return [rng.integers(0, 4000, size=int(n)).astype(np.int32) for n in rng.integers(70, 131, size=k)]


PROMPTS = _prompts()
OLL = Sampling.ollama_defaults


@pytest.fixture(scope="module")
def engines(dev):
    """(slots, one step per run) -> engine: 8 slots run the GEMV lm_head, 24 the skinny GEMM."""
    import os
    made = {}
    old = os.environ.get("MS_DECODE_RUN")
    try:
        for slots in (8, 24):
            for run1 in (False, True):
                if run1:
                    os.environ["MS_DECODE_RUN"] = "1"
                else:
                    os.environ.pop("MS_DECODE_RUN", None)
                e = Engine(TINY, device=0, max_batch=slots, max_ctx=256, max_prefill_tokens=2048)
                e.init_synthetic(WSEED, WSTD, WJIT)
                made[slots, run1] = e
    finally:
        if old is None:
            os.environ.pop("MS_DECODE_RUN", None)
        else:
            os.environ["MS_DECODE_RUN"] = old
    yield made
    for e in made.values():
        e.close()


def gen(eng, prompts, sampling):
    res = eng.generate(prompts, NPRED, ignore_eos=True, sampling=sampling)
    assert all(r.finish == "length" and len(r.ids) == NPRED for r in res)
    return [r.ids for r in res]


@pytest.fixture(scope="module")
def greedy_ids(engines):
    return {slots: gen(engines[slots, False], PROMPTS[:3], None) for slots in (8, 24)}


@pytest.mark.parametrize("slots", [8, 24])
def test_temperature_zero_and_null_are_ms_submit(engines, greedy_ids, slots):
    eng = engines[slots, False]
    p32 = C.POINTER(C.c_int32)
    for tag, sp in ((901, None), (902, L.MsSampling(0.0, 0, 0.0, 5.0, 0.0, 999, 1))):  # ignored when greedy
        a = np.ascontiguousarray(PROMPTS[0], np.int32)
        rc = eng.lib.ms_submit_sampled(eng.h, a.ctypes.data_as(p32), a.size, NPRED, L.MS_FLAG_IGNORE_EOS, tag,
                                       C.byref(sp) if sp is not None else None)
        assert rc == L.MS_OK, eng.lib.ms_last_error(eng.h)
        while eng.step():
            pass
        eng.collect()
        assert eng.take([tag])[tag].ids == greedy_ids[slots][0]
    assert gen(eng, PROMPTS[:1], Sampling(temperature=0.0))[0] == greedy_ids[slots][0]


@pytest.mark.parametrize("slots", [8, 24])
def test_seed_determinism(engines, greedy_ids, slots):
    eng = engines[slots, False]
    a = gen(eng, PROMPTS[:1], OLL(seed=5))[0]
    assert gen(eng, PROMPTS[:1], OLL(seed=5))[0] == a
    assert gen(eng, PROMPTS[:1], OLL(seed=6))[0] != a
    assert a != greedy_ids[slots][0]
    assert all(0 <= t < TINY.vocab for t in a)


@pytest.mark.parametrize("slots", [8, 24])
def test_batch_invariance(engines, slots):
    eng = engines[slots, False]
    alone = gen(eng, PROMPTS[:1], OLL(seed=5))[0]
    # among seven others, submitted sixth: another slot, other batch-mates, other seeds
    order = [3, 1, 7, 2, 6, 0, 5, 4]
    samp = [OLL(seed=5) if i == 0 else OLL(seed=100 + i) for i in order]
    out = gen(eng, [PROMPTS[i] for i in order], samp)
    assert out[order.index(0)] == alone


@pytest.mark.parametrize("slots", [8, 24])
def test_run_chunking(engines, slots):
    samp = [OLL(seed=5), Sampling(1.2, 256, 0.95, 0.02, 1.3, 256, seed=8), None]
    chained = gen(engines[slots, False], PROMPTS[:3], samp)
    single = gen(engines[slots, True], PROMPTS[:3], samp)
    assert chained == single


@pytest.mark.parametrize("slots", [8, 24])
def test_greedy_neighbours(engines, greedy_ids, slots):
    """A greedy chunk inside a sampling run takes the argmax of the SCALED stored logits; alone it
    takes the argmax of the unscaled partials.  A positive row scale keeps the order, so only a
    rounding tie of the scaled values could tell them apart."""
    eng = engines[slots, False]
    out = gen(eng, [PROMPTS[3], PROMPTS[0], PROMPTS[4], PROMPTS[1]], [OLL(seed=1), None, OLL(seed=2), None])
    assert out[1] == greedy_ids[slots][0]
    assert out[3] == greedy_ids[slots][1]


def _against_reference(eng):
    """One decode step per ms_step: after each, the stored logits of the step, the known window
    (prompt tail + ids so far), seed and step through the CPU reference give the engine's id.
    Covers the window seeding from the prompt, its advance on the device, the per-row step
    counter and the first-token path.

    The logits are the engine's own, so no case can be redrawn: a draw is excused when u is within
    1e-5 of a reference CDF boundary or when the row's top-p / min-p boundary is within 1e-5 (the
    fp32 cumulative sums and ln(min_p) are good to ~3e-6); both count against the 1 % cap."""
    V = TINY.vocab
    samps = [OLL(seed=5), Sampling(1.2, 256, 0.95, 0.02, 1.3, 256, seed=8),
             Sampling(0.7, 40, 1.0, 0.0, 1.1, 64, seed=9), Sampling(1.0, 100, 0.9, 0.0, 1.5, 8, seed=10),
             OLL(seed=11), OLL(seed=12), Sampling(0.8, 40, 0.9, 0.05, 1.1, 64, seed=13), OLL(seed=(1 << 64) - 1)]
    prompts = PROMPTS[:8]
    tags = [eng.submit(p, NPRED, True, sampling=s) for p, s in zip(prompts, samps)]
    B = len(tags)
    logits = []  # logits[j][i]: the row behind token j of request i
    pending = eng.step()  # admission + prefill (token 0) + one decode step (token 1)
    logits.append(eng.debug_read(L.MS_DBG_PREFILL_LOGITS, 0, B * V * 4).view(np.float32).reshape(B, V).copy())
    while True:
        logits.append(eng.debug_read(L.MS_DBG_DECODE_LOGITS, 0, B * V * 4).view(np.float32).reshape(B, V).copy())
        if not pending:
            break
        pending = eng.step()
    eng.collect()
    got = eng.take(tags)
    assert len(logits) >= NPRED
    excused = total = 0
    for i, (t, s) in enumerate(zip(tags, samps)):
        ids = got[t].ids
        assert len(ids) == NPRED
        p = R.Params(s.temperature, s.top_k, s.top_p, s.min_p, s.repeat_penalty, s.repeat_last_n, s.seed)
        hist = list(prompts[i])
        for j, tok in enumerate(ids):
            c = R.candidates(logits[j][i], p, hist)
            uu = R.u(s.seed, j)
            total += 1
            if R.excused(c, uu) or (c is not None and c.margin < R.U_EXCUSE):
                print(f"request {i} token {j}: excused (boundary margin {c.margin:.2e}, u {uu:.8f})")
                excused += 1
            else:
                assert tok == R.draw(c, uu), (i, j)
            hist.append(tok)
    print(f"{excused} of {total} draws excused")
    assert excused <= EXCUSE_CAP * total


@pytest.mark.parametrize("slots", [8, 24])
def test_engine_against_reference(engines, slots):
    _against_reference(engines[slots, True])


@pytest.mark.parametrize("form", ["fp16-96-gemm-tile", "q4km-8-qgemv", "q4km-72-large"])
def test_engine_against_reference_other_lm_head_forms(dev, monkeypatch, form):
    """The remaining weight forms of a sampling run's lm_head: the 128x128 GEMM tile (>= 96 slots),
    the Q-GEMV on the packed K-quant lm_head, and a K-quant engine in the large regime."""
    monkeypatch.setenv("MS_DECODE_RUN", "1")
    kind, slots, _ = form.split("-", 2)
    with Engine(TINY, device=0, max_batch=int(slots), max_ctx=256, max_prefill_tokens=2048) as eng:
        if kind == "q4km":
            eng.init_synthetic_q(seed=9, scale=0.05, norm_jitter=0.1)
        else:
            eng.init_synthetic(WSEED, WSTD, WJIT)
        _against_reference(eng)


def test_bad_parameters(engines, greedy_ids):
    eng = engines[8, False]
    p32 = C.POINTER(C.c_int32)
    a = np.ascontiguousarray(PROMPTS[0], np.int32)
    ok = dict(temperature=0.8, top_k=40, top_p=0.9, min_p=0.0, repeat_penalty=1.1, repeat_last_n=64, seed=1)
    for field, bad in (("top_k", 0), ("top_k", 257), ("top_p", 0.0), ("repeat_penalty", 0.0), ("repeat_last_n", 257),
                       ("min_p", 1.0), ("top_k", -1)):
        sp = L.MsSampling(**{**ok, field: bad})
        rc = eng.lib.ms_submit_sampled(eng.h, a.ctypes.data_as(p32), a.size, NPRED, 0, 77, C.byref(sp))
        assert rc == L.MS_EINVAL, field
        assert field in eng.lib.ms_last_error(eng.h).decode(), field
        assert eng.pending() == 0
        with pytest.raises(ValueError, match=field):
            Sampling(**{**ok, field: bad}).validate()
    assert gen(eng, PROMPTS[:1], None)[0] == greedy_ids[8][0]


def test_ollamallm_options_end_to_end(dev):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers
    from mapsum import compat, template
    from mapsum.tokenizer import Tokenizer as MT
    tk = Tokenizer(models.BPE())
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    specials = ["<|begin_of_text|>", "<|eot_id|>", "<|start_header_id|>", "<|end_header_id|>"]
    tr = trainers.BpeTrainer(vocab_size=900, special_tokens=specials,
                             initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    tk.train_from_iterator([template.MAP_PROMPT_MAPREDUCE, "Văn bản tiếng Việt về kinh tế và xã hội."] * 4, tr)
    n = tk.get_vocab_size()
    tk.add_tokens([f"<x{i}>" for i in range((-n) % 16 + 16)])
    toy = MT.from_object(tk)
    cfg = TINY.with_(vocab=toy.tk.get_vocab_size(), bos_id=toy.bos_id, eos_ids=(toy.tk.token_to_id("<|eot_id|>"),))
    with Engine(cfg, device=0, max_batch=8, max_ctx=1024, max_prefill_tokens=2048) as eng:
        eng.init_synthetic(11, 0.05, 0.1)
        compat.register_backend("mapsum:tiny-sampled", compat.MapBackend(eng, toy))
        try:
            prompt = template.map_prompt("mapreduce", "Kinh tế Việt Nam tăng trưởng ổn định trong năm qua.")
            greedy = compat.OllamaLLM("u", "mapsum:tiny-sampled", 32, clean="none")
            sampled = compat.OllamaLLM("u", "mapsum:tiny-sampled", 32, clean="none",
                                       options={"temperature": 0.8, "seed": 7})
            a = sampled._call(prompt)
            assert sampled._call(prompt) == a
            assert asyncio.run(sampled.ainvoke(prompt)) == a
            g = greedy._call(prompt)
            assert greedy._call(prompt) == g
            assert a != g
        finally:
            compat._BACKENDS.pop("mapsum:tiny-sampled", None)
