"""CPU tests: the QK-norm oracle (tests/qwen3_ref.py) pinned against transformers.Qwen3ForCausalLM.

tests/golden/hf_tiny_qwen3.npz holds Qwen3ForCausalLM's outputs at TINY_QWEN3 on the oracle's own
seeded weights (tests/golden/make_qwen3_golden.py).  OracleQwen3 in fp32 mode must reproduce them
to fp32 round-off (test_oracle.py's bar for Llama); the rounded modes stay within test_oracle.py's
bars; and the same weights through OracleLlama -- no Q/K norm -- are far from the fixture, so the
fixture does see the norm.
"""
import os

import numpy as np
import pytest

from mapsum.config import CONFIGS, QWEN3_8B, TINY_QWEN3
from oracle.llama_ref import OracleLlama
from qwen3_ref import OracleQwen3, make_qwen3_weights, qk_norm_rope_f64

GOLD = os.path.join(os.path.dirname(__file__), "golden", "hf_tiny_qwen3.npz")
# Prefill of 40 tokens + 8 single-token steps against one 48-token forward, engine mode, last-token
# logits: the reference's own chunking noise (numpy sums a [1, K] and a [48, K] matmul in different
# orders, and the fp16 rounding points amplify the flips).  Recorded where this file was written.
CHUNK_NOISE = 4.9e-4


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


@pytest.fixture(scope="module")
def weights(gold):
    return make_qwen3_weights(TINY_QWEN3, int(gold["seed"]), std=float(gold["std"]), jitter=float(gold["jitter"]),
                              gain_seed=int(gold["gain_seed"]))


def test_configs():
    assert CONFIGS["qwen3-8b"] is QWEN3_8B and CONFIGS["tiny-qwen3"] is TINY_QWEN3
    c = QWEN3_8B
    assert (c.n_layers, c.hidden, c.n_heads, c.n_kv_heads, c.head_dim, c.ffn, c.vocab) == \
        (36, 4096, 32, 8, 128, 12288, 151936)
    assert c.qk_norm and not c.tie_embeddings and c.rope_factor == 0 and c.rope_theta == 1e6 and c.norm_eps == 1e-6
    # what ms_create checks
    assert c.hidden == c.n_heads * 128 and c.n_heads + c.n_kv_heads <= 64 and c.n_heads // c.n_kv_heads <= 16
    assert c.hidden % 256 == 0 and c.ffn % 256 == 0 and c.vocab % 16 == 0
    t = TINY_QWEN3
    assert (t.n_layers, t.hidden, t.n_heads, t.n_kv_heads, t.ffn, t.vocab) == (2, 1024, 8, 2, 2048, 4096)
    assert t.qk_norm and not t.tie_embeddings and not CONFIGS["tiny"].qk_norm


def test_fp32_matches_transformers(gold, weights):
    o = OracleQwen3(TINY_QWEN3, weights, mode="fp32")
    lg, probes = o.forward(gold["ids"], collect=True, all_logits=True)
    top_idx, top_val = gold["top16_idx"], gold["top16_val"]
    assert np.allclose(np.take_along_axis(lg, top_idx, 1), top_val, rtol=1e-4, atol=1e-4)
    assert np.array_equal(np.argmax(lg, 1), top_idx[:, 0])
    assert np.allclose(lg[-1], gold["last_logits"], rtol=1e-4, atol=1e-4)
    print(f"fp32: last-token logits rel err vs transformers {rel(lg[-1], gold['last_logits']):.2e}")
    assert rel(lg[-1], gold["last_logits"]) < 1e-4
    for l in range(TINY_QWEN3.n_layers):
        assert np.allclose(probes[l][:, :32], gold["hidden_head"][l], rtol=1e-4, atol=1e-4)
        assert np.allclose(np.linalg.norm(probes[l], axis=1), gold["hidden_norm"][l], rtol=1e-5)


def test_fp32_greedy_matches_transformers(gold, weights):
    o = OracleQwen3(TINY_QWEN3, weights, mode="fp32")
    toks, fin = o.generate(gold["ids"], len(gold["greedy"]), ignore_eos=True)
    assert toks == gold["greedy"].tolist() and fin == "length"


@pytest.mark.parametrize("mode,tol", [("engine", 2e-3), ("f16", 2e-3), ("bf16", 2e-2)])
def test_rounded_modes_within_tolerance(gold, weights, mode, tol):
    o = OracleQwen3(TINY_QWEN3, weights, mode=mode)
    lg, _ = o.forward(gold["ids"])
    err = rel(lg, gold["last_logits"])
    print(f"{mode}: last-token logits rel err vs transformers fp32 {err:.2e}")
    assert err < tol


def test_f64_accumulation_runs(gold, weights):
    """acc=np.float64 (the bounds' reference) is the same model to summation-order noise."""
    a, _ = OracleQwen3(TINY_QWEN3, weights, mode="engine").forward(gold["ids"])
    b, _ = OracleQwen3(TINY_QWEN3, weights, mode="engine", acc=np.float64).forward(gold["ids"])
    assert rel(a, b) < 2e-3


def test_without_the_norm_is_far(gold, weights):
    """The Llama oracle on the same weights (q_norm / k_norm ignored) is nowhere near the fixture."""
    lg, _ = OracleLlama(TINY_QWEN3, weights, mode="fp32").forward(gold["ids"])
    err = rel(lg, gold["last_logits"])
    print(f"no Q/K norm: last-token logits rel err vs transformers {err:.2f}")
    assert err > 0.5


def test_permuted_or_swapped_gain_is_far(gold, weights):
    """The fixture also sees WHICH gain meets which dimension: the gains in the engine's
    rope-permuted row order, or Q's gain on K, are errors of the order of the norm itself."""
    perm = np.array([16 * (i >> 3) + (i & 7) if i < 64 else 16 * ((i - 64) >> 3) + 8 + ((i - 64) & 7)
                     for i in range(128)])
    for kind in ("permuted", "swapped"):
        w = dict(weights)
        w["layers"] = [dict(L) for L in weights["layers"]]
        for L in w["layers"]:
            if kind == "permuted":
                L["q_norm"], L["k_norm"] = L["q_norm"][perm], L["k_norm"][perm]
            else:
                L["q_norm"], L["k_norm"] = L["k_norm"], L["q_norm"]
        lg, _ = OracleQwen3(TINY_QWEN3, w, mode="fp32").forward(gold["ids"])
        err = rel(lg, gold["last_logits"])
        print(f"{kind} gains: {err:.2f}")
        assert err > 0.1, kind


def test_chunked_equals_one_pass(gold, weights):
    o = OracleQwen3(TINY_QWEN3, weights, mode="engine")
    ids = gold["ids"]
    one, _ = o.forward(ids)
    cache = o.new_cache()
    lg, _ = o.forward(ids[:40], cache)
    for t in ids[40:]:
        lg, _ = o.forward([int(t)], cache)
    err = rel(lg, one)
    print(f"40 + 8 x 1 vs 48 at once, engine mode: {err:.2e} (recorded {CHUNK_NOISE:.1e})")
    assert err <= 4 * CHUNK_NOISE
    full = o.new_cache()
    o.forward(ids, full)
    for l in range(TINY_QWEN3.n_layers):  # and the cache holds the same rotated keys
        assert rel(cache["k"][l], full["k"][l]) <= 4 * CHUNK_NOISE


def test_f64_head_function_matches_the_oracle_step():
    """qk_norm_rope_f64 (the GPU op tests' reference) is the oracle's steps 2-4."""
    from oracle.llama_ref import _f16, apply_rope, rms_rinv, rope_tables
    rng = np.random.default_rng(5)
    t = _f16(rng.standard_normal((7, 3, 128)).astype(np.float32))
    g = _f16(1 + 0.3 * rng.standard_normal(128).astype(np.float32))
    cos, sin = rope_tables(TINY_QWEN3, np.arange(60, 67))
    want = apply_rope(((t * rms_rinv(t, 1e-6)) * g).astype(np.float32), cos, sin, _f16)
    got = qk_norm_rope_f64(t, g, cos, sin, 1e-6)
    ulp = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64)
    assert np.all(np.abs(got - want) <= ulp)
