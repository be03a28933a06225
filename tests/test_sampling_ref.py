"""CPU tests of sampled decoding (no GPU): known answers of the float64 restatement in
tests/sampling_ref.py, the counter-based random numbers, the inputs the GPU tests commit to, and
the host plumbing (options parsing, the wire shim's 400s, the journal key, OllamaLLM)."""
import asyncio
import math

import numpy as np
import pytest

import sampling_ref as R
from mapsum import compat
from mapsum.engine import RequestQueue, Result, Sampling
from mapsum.resume import CallJournal, JournaledLLM, call_key
from mapsum.server import OllamaShim


# ------------------------------------------------------------------ known answers
def test_top_k_1_is_the_argmax_with_ties_to_the_lowest_id():
    l = np.array([0.5, 2.0, -1.0, 2.0, 1.5], np.float32)
    for seed in range(8):
        assert R.sample(l, R.Params(0.8, 1, 0.9, 0.0, 1.0, 64, seed), [], seed) == 1
    assert R.sample(l, R.Params(0.0), [3, 3], 0) == 1  # greedy ignores every other field


def test_penalty_divides_positive_multiplies_negative_once_per_id():
    l = np.array([4.0, -2.0, 1.0, 3.0], np.float32)
    p = R.Params(1.0, 4, 1.0, 0.0, 2.0, 64, 0)
    c = R.candidates(l, p, [0, 1, 0, 0, 1])  # duplicates: penalised once
    # 4 -> 2, -2 -> -4, the others untouched: order 3 (3.0), 0 (2.0), 2 (1.0), 1 (-4.0)
    assert c.ids.tolist() == [3, 0, 2, 1]
    e = np.exp(np.array([3.0, 2.0, 1.0, -4.0]) - 3.0)
    assert np.allclose(c.probs, e / e.sum(), rtol=1e-12)
    # the window is the LAST repeat_last_n ids; 0 or rp == 1 turn it off
    assert R.candidates(l, R.Params(1.0, 4, 1.0, 0.0, 2.0, 1, 0), [0, 1]).ids.tolist() == [0, 3, 2, 1]
    assert R.candidates(l, R.Params(1.0, 4, 1.0, 0.0, 2.0, 0, 0), [0, 1]).ids.tolist() == [0, 3, 2, 1]
    assert R.candidates(l, R.Params(1.0, 4, 1.0, 0.0, 1.0, 64, 0), [0, 1]).ids.tolist() == [0, 3, 2, 1]


def test_top_p_min_p_and_temperature():
    l = np.log(np.array([0.5, 0.25, 0.125, 0.125], np.float64)).astype(np.float32)
    assert R.candidates(l, R.Params(1.0, 4, 1e-6, 0.0, 1.0, 0), []).ids.tolist() == [0]  # one candidate
    assert R.candidates(l, R.Params(1.0, 4, 0.7, 0.0, 1.0, 0), []).ids.tolist() == [0, 1]  # 0.5, 0.75 >= 0.7
    assert R.candidates(l, R.Params(1.0, 4, 1.0, 0.3, 1.0, 0), []).ids.tolist() == [0, 1]  # p >= 0.3 * 0.5
    assert R.candidates(l, R.Params(1.0, 3, 1.0, 0.0, 1.0, 0), []).ids.tolist() == [0, 1, 2]  # tie -> lowest id
    c = R.candidates(l, R.Params(0.5, 2, 1.0, 0.0, 1.0, 0), [])
    assert np.allclose(c.probs, [0.8, 0.2])  # (0.5^2, 0.25^2) normalised
    assert R.draw(c, 0.79) == 0 and R.draw(c, 0.81) == 1 and R.draw(c, 1.0) == 1  # none exceeds u: the last


def test_non_finite_rows():
    p = R.Params()
    assert R.sample(np.full(8, np.nan, np.float32), p, [], 0) == -1
    assert R.sample(np.full(8, -np.inf, np.float32), p, [], 0) == -1
    assert R.sample(np.array([0.0, np.inf, 1.0], np.float32), p, [], 0) == -1
    assert R.sample(np.array([np.nan, -1.0, np.nan], np.float32), p, [], 0) == 1  # NaN is never a candidate
    assert R.sample(np.full(8, np.nan, np.float32), R.Params(0.0), [], 0) == -1


# ------------------------------------------------------------------ random numbers
def test_u_known_values_and_asymmetry():
    assert R.mix64(0) == 0 and R.mix64(1) == 0x5692161D100B05E5
    assert R.u(1, 2) != R.u(2, 1)
    assert all(0.0 <= R.u(s, t) < 1.0 for s in (0, 1, (1 << 64) - 1) for t in (0, 1, (1 << 31) - 1))
    assert R.u(3, 4) * 2 ** 24 == int(R.u(3, 4) * 2 ** 24)  # 24 bits


def test_u_is_uniform_chi_square():
    seeds = [0, 1, 2, 3, 1 << 32, (1 << 63) + 5, (1 << 64) - 1, 0xDEADBEEF, 12345678901234567, 42]
    vals = np.array([R.u(s, t) for s in seeds for t in range(10000)])
    assert vals.size == 100000
    obs = np.bincount((vals * 64).astype(int), minlength=64)
    chi2 = float(((obs - vals.size / 64) ** 2 / (vals.size / 64)).sum())
    k, z = 63, 3.7190  # the 99.99 % normal quantile; Wilson-Hilferty
    q = k * (1 - 2 / (9 * k) + z * math.sqrt(2 / (9 * k))) ** 3
    print(f"chi-square {chi2:.1f} (99.99 % quantile {q:.1f})")
    assert 113 < q < 116 and chi2 < q


# ------------------------------------------------------------------ the GPU tests' inputs
def test_committed_cases_need_few_redraws_and_excuse_few_draws():
    redraws = 0
    for n, rows, q in R.OP_SHAPES:
        psets, logits, wins, cands, steps, red = R.op_case(n, rows, q)
        redraws += red
        assert all(c.margin >= R.MARGIN for c in cands)
        assert len({tuple(w[-64:]) for w in wins}) == rows
        for w, l in zip(wins, logits):  # duplicates, and ids on both signs
            assert len(set(w[-16:].tolist())) < 16 and (l[w[-64:]] > 0).any() and (l[w[-64:]] < 0).any()
        # no draw of a candidate-set case is excused by the reference itself
        assert not any(R.excused(c, R.u(p.seed, s)) and p.temperature > 0 for c, p, s in zip(cands, psets, steps))
    for n in (8191, 128256):
        psets, logits, _, cands, steps, red = R.tie_case(n)
        redraws += red
        assert all((l == l.max()).sum() > 1024 for l in logits)  # more ties at the top than fit in LDS
        assert [c.ids.size for c in cands][:1] == [256] and all(c.margin >= R.MARGIN for c in cands)
        assert not any(R.excused(c, R.u(p.seed, s)) for c, p, s in zip(cands, psets, steps))
    assert redraws <= 8, redraws
    for pi, q in R.DRAW_CASES:
        _, _, _, c, seeds, steps, red = R.draw_case(pi, q)
        assert red <= 2
        ex = sum(R.excused(c, R.u(int(a), int(b))) for a, b in zip(seeds, steps))
        assert ex <= 0.01 * R.DRAWS, (pi, q, ex)


# ------------------------------------------------------------------ host plumbing
def test_sampling_options_parsing():
    assert Sampling.from_options(None) is None and Sampling.from_options({"num_predict": 5}) is None
    s = Sampling.from_options({"temperature": 0.5, "num_predict": 9})
    assert s == Sampling(0.5, 40, 0.9, 0.0, 1.1, 64, None)  # Ollama's defaults for the rest, no seed
    assert Sampling.ollama_defaults() == Sampling(0.8, 40, 0.9, 0.0, 1.1, 64, None)
    d = Sampling.from_options({"num_predict": 5}, Sampling.ollama_defaults())
    assert d == Sampling.ollama_defaults()
    assert Sampling.from_options({"seed": 7}).seed == 7 and Sampling.from_options({"seed": -1}).seed == (1 << 64) - 1
    assert Sampling.from_options({"temperature": 0}).greedy
    assert Sampling.from_options({"temperature": 0, "top_k": 0}).greedy  # greedy: the rest is ignored
    for bad, field in (({"top_k": 0}, "top_k"), ({"top_k": 257}, "top_k"), ({"top_p": 0}, "top_p"),
                       ({"repeat_penalty": 0}, "repeat_penalty"), ({"repeat_last_n": 257}, "repeat_last_n"),
                       ({"min_p": 1}, "min_p"), ({"top_k": "x"}, "top_k"), ({"top_k": 1.5}, "top_k")):
        with pytest.raises(ValueError, match=field):
            Sampling.from_options({"temperature": 0.8, **bad})
    a, b = Sampling.ollama_defaults().with_seed(), Sampling.ollama_defaults().with_seed()
    assert a.seed is not None and a.seed != b.seed and Sampling.ollama_defaults(3).with_seed().seed == 3
    c = Sampling(0.8, 40, 0.9, 0.0, 1.1, 64, (1 << 64) - 1).to_c()
    assert (c.top_k, c.repeat_last_n, c.seed) == (40, 64, (1 << 64) - 1) and abs(c.temperature - 0.8) < 1e-7


class FakeEngine(RequestQueue):
    """submit/step/poll double (as tests/test_host.py): a chunk's output is its prompt reversed,
    preceded by its seed when it samples; records what each submit carried."""

    def __init__(self, fail_first=()):
        self.q, self.done, self.seen = {}, [], []
        self._tag, self._mailbox = 1, {}
        self.fail_first = set(fail_first)

    def submit(self, ids, n, ignore_eos=False, tag=None, sampling=None):
        if sampling is not None:
            sampling.validate()
            assert sampling.seed is not None
        if tag is None:
            tag, self._tag = self._tag, self._tag + 1
        self.q[tag] = (list(ids), n, sampling)
        self.seen.append(sampling)
        return tag

    def step(self):
        for tag, (ids, n, s) in self.q.items():
            if tuple(ids) in self.fail_first:
                self.fail_first.discard(tuple(ids))
                self.done.append(Result(tag, [], "error", len(ids)))
            else:
                self.done.append(Result(tag, (([s.seed % 251] if s else []) + ids[::-1])[:n], "length", len(ids)))
        self.q = {}
        return 0

    def poll(self, cap=256):
        out, self.done = self.done[:cap], self.done[cap:]
        return out


def test_generate_takes_one_sampling_or_one_per_prompt_and_requeue_keeps_the_seed():
    eng = FakeEngine(fail_first=[(7,)])
    res = eng.generate([[7], [8], [9]], 4, retries=1, sampling=[Sampling.ollama_defaults(), None, Sampling(0.5, seed=3)])
    assert [r.finish for r in res] == ["length"] * 3
    first, again = eng.seen[0], eng.seen[3]
    assert first.seed is not None and again == first  # the re-queued chunk: same fresh seed
    assert eng.seen[1] is None and eng.seen[2].seed == 3
    eng = FakeEngine()
    eng.generate([[1], [2]], 4, sampling=Sampling.ollama_defaults(5))
    assert [s.seed for s in eng.seen] == [5, 5]
    with pytest.raises(ValueError):
        eng.generate([[1], [2]], 4, sampling=[None])


class ToyTok:
    bos_id = 1

    def encode(self, text, add_bos=True):
        return ([1] if add_bos else []) + [2 + (ord(ch) % 200) for ch in text][:32]

    def decode(self, ids):
        return " ".join(str(i) for i in ids)


@pytest.fixture
def backend():
    eng = FakeEngine()
    compat.register_backend("fake:sampling", compat.MapBackend(eng, ToyTok()))
    yield eng
    compat._BACKENDS.pop("fake:sampling", None)


def test_ollamallm_positional_construction_unchanged_and_options(backend, monkeypatch):
    monkeypatch.delenv("MAPSUM_SAMPLING", raising=False)
    m = compat.OllamaLLM("http://h:1", "fake:sampling", 16)
    assert (m.ollama_url, m.model_name, m.max_new_tokens, m.clean, m.options) == \
        ("http://h:1", "fake:sampling", 16, "pipeline", None)
    assert compat.OllamaLLM("u", "fake:sampling", 16, "none").clean == "none"
    with pytest.raises(TypeError):
        compat.OllamaLLM("u", "fake:sampling", 16, "none", {"temperature": 1})  # options is keyword-only
    g = m._call("xin chào")
    assert m.sampling is None and backend.seen == [None]
    s = compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0.8, "seed": 7})
    assert s.sampling == Sampling(0.8, 40, 0.9, 0.0, 1.1, 64, 7)
    out = s._call("xin chào")
    assert out != g and s._call("xin chào") == out and asyncio.run(s.ainvoke("xin chào")) == out
    assert [x.seed for x in backend.seen[1:]] == [7, 7, 7]
    # no seed: a fresh one per call
    f = compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0.8})
    f._call("a"), f._call("a")
    assert backend.seen[-1].seed != backend.seen[-2].seed
    with pytest.raises(ValueError, match="top_k"):
        compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0.8, "top_k": 0})
    # an unchanged runner samples like Ollama with MAPSUM_SAMPLING=ollama
    monkeypatch.setenv("MAPSUM_SAMPLING", "ollama")
    assert compat.OllamaLLM("u", "fake:sampling", 16).sampling == Sampling.ollama_defaults()
    assert compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0}).sampling is None
    monkeypatch.setenv("MAPSUM_SAMPLING", "nonsense")
    with pytest.raises(ValueError):
        compat.OllamaLLM("u", "fake:sampling", 16)


def test_server_honours_options_and_answers_400(backend):
    be = compat._BACKENDS["fake:sampling"]
    with OllamaShim({"m": be}, port=0) as shim:
        code, g = shim.generate({"model": "m", "prompt": "a", "options": {"num_predict": 8}})
        assert code == 200 and backend.seen[-1] is None
        code, s = shim.generate({"model": "m", "prompt": "a", "options": {"num_predict": 8, "temperature": 0.7,
                                                                         "top_k": 5, "seed": 11}})
        assert code == 200 and backend.seen[-1] == Sampling(0.7, 5, 0.9, 0.0, 1.1, 64, 11)
        assert s["response"] != g["response"]
        for bad, field in (({"top_k": 0}, "top_k"), ({"top_k": 257}, "top_k"), ({"top_p": 0}, "top_p"),
                           ({"repeat_penalty": 0}, "repeat_penalty"), ({"repeat_last_n": 257}, "repeat_last_n")):
            code, r = shim.generate({"model": "m", "prompt": "a", "options": {"temperature": 0.8, **bad}})
            assert code == 400 and field in r["error"], (bad, r)
        assert shim.generate({"model": "m", "prompt": "a", "options": 3})[0] == 400
    with OllamaShim({"m": be}, port=0, ollama_defaults=True) as shim:
        assert shim.generate({"model": "m", "prompt": "a"})[0] == 200
        assert backend.seen[-1].temperature == 0.8 and backend.seen[-1].seed is not None
        assert shim.generate({"model": "m", "prompt": "a", "options": {"temperature": 0}})[0] == 200
        assert backend.seen[-1] is None


def test_server_maps_an_engine_einval_to_400():
    class Refusing(FakeEngine):
        def submit(self, ids, n, ignore_eos=False, tag=None, sampling=None):
            if sampling is not None:
                raise RuntimeError("libmapsum ms_submit_sampled failed (-22): sampling: vocab above 131072")
            return super().submit(ids, n, ignore_eos, tag)
    be = compat.MapBackend(Refusing(), ToyTok())
    with OllamaShim({"m": be}, port=0) as shim:
        code, r = shim.generate({"model": "m", "prompt": "a", "options": {"temperature": 0.8}})
        assert code == 400 and "vocab" in r["error"]
        assert shim.generate({"model": "m", "prompt": "a"})[0] == 200


def test_resume_key_changes_only_for_non_greedy_calls(tmp_path, backend, monkeypatch):
    monkeypatch.delenv("MAPSUM_SAMPLING", raising=False)
    greedy = compat.OllamaLLM("u", "fake:sampling", 16)
    zero = compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0, "seed": 4})
    s7 = compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0.8, "seed": 7})
    s8 = compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0.8, "seed": 8})
    t9 = compat.OllamaLLM("u", "fake:sampling", 16, options={"temperature": 0.9, "seed": 7})
    with CallJournal(str(tmp_path / "j.jsonl")) as j:
        keys = [JournaledLLM(m, j, "doc")._key("p") for m in (greedy, zero, s7, s8, t9)]
        assert keys[0] == keys[1] == call_key("fake:sampling|pipeline", 16, "doc", "p")  # as before
        assert len(set(keys[1:])) == 4
        jl = JournaledLLM(s7, j, "doc")
        a = jl.invoke("p")
        assert jl.invoke("p") == a and (jl.hits, jl.misses) == (1, 1)
        assert JournaledLLM(s8, j, "doc").invoke("p") != a  # another seed: another call
