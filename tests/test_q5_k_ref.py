"""Q5_K on the CPU: the numpy reference itself (tests/q5_k_ref.py) against the project's Q4_K
restatement and hand-built blocks, its quantiser, the GGUF loader's Q5_K route (mapsum/gguf.py)
through a recording engine for the Q5_K_M and a Q4_K_S-style mix, and the exports.  Also the model
of the GPU engine tests (tests/test_gpu_q5_k.py) and the count of its oracle's near-ties."""
import os

import numpy as np
import pytest

import q5_k_ref as R
from mapsum import _lib as L
from mapsum import gguf, ollama_store
from mapsum.config import TINY
from oracle import quantize as QZ
from oracle import quants as Q
from oracle.synth import f16_rne, make_weights
from test_gguf import META, _NAMES, _T, Recorder, rope_freqs, write_gguf

SHAPES = {"wq": (TINY.n_heads * 128, TINY.hidden), "wk": (TINY.n_kv_heads * 128, TINY.hidden),
          "wv": (TINY.n_kv_heads * 128, TINY.hidden), "wo": (TINY.hidden, TINY.n_heads * 128),
          "w_gate": (TINY.ffn, TINY.hidden), "w_up": (TINY.ffn, TINY.hidden), "w_down": (TINY.hidden, TINY.ffn)}
MIXES = {"q5_k_m": R.q5_k_m_type, "q4_k_s": R.q4_k_s_type}
BYTES = {12: 144, 13: 176, 14: 210}


def dequant_any(blocks, qt):
    return R.dequant_q5_k(blocks) if qt == R.GGML_TYPE_Q5_K else Q.dequant(blocks, qt)


def quantize_any(x, qt):
    return R.quantize_q5_k(x) if qt == R.GGML_TYPE_Q5_K else QZ.quantize(x, qt)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ the reference
def test_qh_zero_is_the_q4_k_block():
    """A Q5_K block with qh = 0 dequantises bit for bit to the Q4_K block of the same header and qs."""
    b5 = R.random_blocks_q5_k(512, seed=1, scale=0.3)
    b5[:, 16:48] = 0
    b4 = np.concatenate([b5[:, :16], b5[:, 48:]], axis=1)
    assert b4.shape[1] == Q.Q4_K_BYTES
    assert np.array_equal(_bits(R.dequant_q5_k(b5)), _bits(Q.dequant_q4_K(b4)))


def test_qh_all_ones_adds_16_to_every_code():
    b5 = R.random_blocks_q5_k(256, seed=2, scale=0.3)
    b5[:, 16:48] = 0xFF
    y = R.dequant_q5_k(b5).reshape(-1, 8, 32).astype(np.float64)
    d = b5[:, 0:2].copy().view(np.float16).astype(np.float32)[:, 0]
    dmin = b5[:, 2:4].copy().view(np.float16).astype(np.float32)[:, 0]
    qs = b5[:, 48:].astype(np.int32)
    for s in range(8):
        sc, m = R.scale_min_k4(b5[:, 4:16], s)
        d1 = (d * sc.astype(np.float32)).astype(np.float32)
        m1 = (dmin * m.astype(np.float32)).astype(np.float32)
        byte = qs[:, 32 * (s >> 1):32 * (s >> 1) + 32]
        nib = (byte >> 4) if s & 1 else (byte & 0xF)
        want = ((d1[:, None] * (nib + 16).astype(np.float32)).astype(np.float32) - m1[:, None]).astype(np.float32)
        assert np.array_equal(y[:, s], want.astype(np.float64)), s
    assert R.codes(b5).min() == 16 and R.codes(b5).max() == 31


def test_kat_blocks():
    b = R.kat_blocks()
    assert b.shape == (6, 176)
    y = R.dequant_q5_k(b).reshape(6, 8, 32).astype(np.float64)
    s8, l = np.arange(8)[:, None], np.arange(32)[None, :]
    # 0: q = t & 31 crosses 16 inside every sub-block, so both qh values occur under every scale
    assert np.array_equal(R.codes(b)[0].reshape(8, 32), np.broadcast_to(l, (8, 32)))
    assert np.array_equal(y[0], 0.5 * (s8 + 1) * l - 0.25 * (2 * s8 + 1))
    # 1: 6-bit scale / min 63 in sub-blocks 4-7 (two high bits from bytes 0-7, low four from 8-11)
    for s in range(8):
        sc, m = R.scale_min_k4(b[1:2, 4:16], s)
        assert (int(sc[0]), int(m[0])) == ((63, 63) if s >= 4 else (1, 2)), s
    sc1, m1 = np.where(s8 >= 4, 63, 1), np.where(s8 >= 4, 63, 2)
    assert np.array_equal(y[1], 0.5 * sc1 * (31 - l) - 0.25 * m1)
    # 2: d = 0 leaves -m1; 3: negative d; 4: the smallest subnormal d and dmin
    assert np.array_equal(y[2], np.broadcast_to(-0.25 * (2 * s8 + 1), (8, 32)))
    assert np.array_equal(y[3], -0.5 * (s8 + 1) * l - 0.25 * (2 * s8 + 1))
    assert np.array_equal(y[4], 2.0 ** -24 * ((s8 + 1) * l - (2 * s8 + 1)))
    # 5: the largest code, scale and min: 63 * 31 - 63
    assert np.all(y[5] == 63.0 * 31.0 - 63.0) and np.all(b[5, 16:] == 0xFF)
    assert np.all(np.isfinite(y))


def test_product_is_exact_and_blocks_are_centred():
    """d1 * q is exact in fp32 (11 + 6 + 5 bits), so the two-rounding form equals fp64's one-rounding
    d1 * q - m1; the random blocks cover every code and have std ~ scale."""
    b = R.random_blocks_q5_k(2048, seed=3, scale=0.7)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)[:, 0]
    dmin = b[:, 2:4].copy().view(np.float16).astype(np.float32)[:, 0]
    q = R.codes(b).reshape(-1, 8, 32)
    want = np.empty(q.shape, np.float32)
    for s in range(8):
        sc, m = R.scale_min_k4(b[:, 4:16], s)
        d1 = (d * sc.astype(np.float32)).astype(np.float64)
        m1 = (dmin * m.astype(np.float32)).astype(np.float64)
        want[:, s] = (d1[:, None] * q[:, s] - m1[:, None]).astype(np.float32)
    y = R.dequant_q5_k(b)
    assert np.array_equal(_bits(y), _bits(want.reshape(-1)))
    assert set(np.unique(q)) == set(range(32))
    assert abs(float(y.mean())) < 0.02 * 0.7 and 0.5 * 0.7 <= float(y.std()) <= 2 * 0.7


def test_round_trip_beats_q4_k():
    """quantize -> dequant on Gaussian rows: relative Frobenius error below Q4_K's (oracle.quantize)
    on the same rows.  Measured: Q5_K 3.82e-2, Q4_K 7.85e-2."""
    x = (np.random.default_rng(0).standard_normal((256, 768)) * 0.05).astype(np.float32)
    b5 = R.quantize_q5_k(x)
    assert b5.shape == (256 * 3, 176)
    e5 = np.linalg.norm(R.dequant_q5_k(b5).reshape(x.shape) - x.astype(np.float64)) / np.linalg.norm(x)
    b4 = QZ.quantize(x, Q.GGML_TYPE_Q4_K)
    e4 = np.linalg.norm(Q.dequant_q4_K(b4).reshape(x.shape) - x.astype(np.float64)) / np.linalg.norm(x)
    print(f"relative Frobenius error: Q5_K {e5:.3e}, Q4_K {e4:.3e}")
    assert e5 < e4
    assert R.codes(b5).max() == 31 and R.codes(b5).min() == 0
    z = R.quantize_q5_k(np.zeros(256, np.float32))
    assert np.all(z == 0) and np.all(R.dequant_q5_k(z) == 0)


def test_type_mixes():
    n = 28  # llama3.2:3b
    m5 = [R.q5_k_m_type("wv", l, n) for l in range(n)]
    assert m5 == [13 if t == 12 else t for t in (Q.q4_k_m_type("wv", l, n) for l in range(n))]
    assert R.q5_k_m_type("wq", 5, n) == 13 and R.q5_k_m_type("embed", 0, n) == 14
    s4 = [R.q4_k_s_type("w_down", l, n) for l in range(n)]
    assert s4 == [13] * 3 + [12] * 25 and R.q4_k_s_type("wv", 0, 2) == 13 and R.q4_k_s_type("wv", 1, 2) == 12
    assert R.q4_k_s_type("w_gate", 0, n) == 12 and R.q4_k_s_type("lm_head", 0, n) == 14


# ------------------------------------------------------------------ the model of the engine tests
def quant_model(mix: str):
    """make_weights(TINY, 1234, 0.05, 0.1) quantised per matrix by the mix's type: -> (qw for
    load_quantized, the oracle's weights f16_rne(dequant), {name: type})."""
    base = make_weights(TINY, 1234, std=0.05, jitter=0.1)
    ty = MIXES[mix]
    qw, w, types = {}, {"final_norm": base["final_norm"], "layers": []}, {}
    qt = ty("embed", 0, TINY.n_layers)
    eb = quantize_any(base["embed"], qt)
    qw["embed"], types["embed"] = (qt, eb.reshape(-1)), qt
    w["embed"] = f16_rne(dequant_any(eb, qt)).reshape(base["embed"].shape)
    w["lm_head"] = w["embed"]
    for l, ly in enumerate(base["layers"]):
        o = {"attn_norm": ly["attn_norm"], "ffn_norm": ly["ffn_norm"]}
        for n in SHAPES:
            qt = ty(n, l, TINY.n_layers)
            blk = quantize_any(ly[n], qt)
            qw[(l, n)], types[(l, n)] = (qt, blk.reshape(-1)), qt
            o[n] = f16_rne(dequant_any(blk, qt)).reshape(ly[n].shape)
        w["layers"].append(o)
    return qw, w, types


# (length, seed) of the engine tests' prompts.  test_gpu_parity's lengths; the seeds are, per length,
# the one of 110 scanned (2000 .. 2109) whose oracle continuations have the fewest near-ties over
# both models -- test_gpu_parity's own seeds (700 + n) give 28 of 192 on the Q5_K_M model
PROMPTS = [(17, 2081), (140, 2034), (301, 2019), (64, 2048)]


def prompts():
    return [np.random.default_rng(seed).integers(0, 4000, size=n).astype(np.int32) for n, seed in PROMPTS]


def test_mixes_put_q5_k_beside_both_neighbours():
    """TINY's two layers: the Q5_K_M QKV is Q5_K, Q5_K, Q5_K in layer 0 and Q5_K, Q5_K, Q6_K in layer
    1; the Q4_K_S-style QKV is Q4_K, Q4_K, Q5_K in layer 0 and all Q4_K in layer 1."""
    t5 = [[R.q5_k_m_type(n, l, 2) for n in ("wq", "wk", "wv")] for l in range(2)]
    t4 = [[R.q4_k_s_type(n, l, 2) for n in ("wq", "wk", "wv")] for l in range(2)]
    assert t5 == [[13, 13, 13], [13, 13, 14]] and t4 == [[12, 12, 13], [12, 12, 12]]
    assert [R.q5_k_m_type("w_down", l, 2) for l in range(2)] == [13, 14]


NEAR_TIES = {"q5_k_m": 9, "q4_k_s": 11}  # counted below, of 4 x 48 positions


@pytest.mark.parametrize("mix", list(MIXES))
def test_oracle_near_ties_are_counted(mix):
    """The GPU engine tests excuse a token that differs from the oracle's only at a near-tie of the
    oracle's logits (gap <= 1e-2 (|top| + 1)) and cap the differing positions at 3 % (5 of 192).
    How many positions of the oracle's own greedy runs are such near-ties: 9 (Q5_K_M) and 11
    (Q4_K_S-style) of 192 with the scanned seeds -- 4.7 % and 5.7 %, not under 3 %: the random tiny
    model's logits are flat (no seed of the scan gave fewer than 1 per prompt and model on
    average), so the cap is the binding half of the bar, tighter than the near-tie excuse.  This
    test pins the count, so a change of the model or the prompts shows up here first."""
    from oracle.llama_ref import OracleLlama
    _, w, _ = quant_model(mix)
    oracle = OracleLlama(TINY, w)
    ties = total = 0
    for p in prompts():
        gen, _ = oracle.generate(p, 48, ignore_eos=True)
        lg, _ = oracle.forward(np.concatenate([p, np.asarray(gen[:-1], np.int32)]), all_logits=True)
        srt = np.sort(lg[len(p) - 1:], 1)
        ties += int(np.sum(srt[:, -1] - srt[:, -2] <= 1e-2 * (np.abs(srt[:, -1]) + 1.0)))
        total += len(gen)
    print(f"{mix}: {ties} near-ties in {total} oracle positions")
    assert total == 192 and ties <= NEAR_TIES[mix]


# ------------------------------------------------------------------ GGUF
def write_kq_gguf(path, qw, norms, bad=None):
    """TINY as a K-quant GGUF from load_quantized-style qw (un-permuted blocks): Q/K rows permuted as
    llama.cpp's converter does, tied token_embd, F32 norms, rope_freqs.  bad: ("q8", layer, name)
    swaps in a Q8_0 matrix, ("k288", layer, name) a Q5_K one of row length 288."""
    H, V = TINY.hidden, TINY.vocab
    f32 = lambda a: np.asarray(a, np.float32).tobytes()  # noqa: E731
    et, eb = qw["embed"]
    ts = [("token_embd.weight", et, [H, V], np.asarray(eb).tobytes()),
          ("output_norm.weight", gguf.GGML_F32, [H], f32(norms["final_norm"])), rope_freqs()]
    heads = {"wq": TINY.n_heads, "wk": TINY.n_kv_heads}
    for i in range(TINY.n_layers):
        for n in ("attn_norm", "ffn_norm"):
            ts.append((f"blk.{i}.{n}.weight", gguf.GGML_F32, [H], f32(norms["layers"][i][n])))
        for n, g in _NAMES.items():
            r, k = SHAPES[n]
            t, blk = qw[(i, n)]
            b = np.asarray(blk).reshape(r, -1)
            a = gguf.permute_rows(b, heads[n]) if n in heads else b
            dims, raw = [k, r], a.tobytes()
            if bad == ("q8", i, n):
                t, raw = gguf.GGML_Q8_0, np.zeros(r * k // 32 * 34, np.uint8).tobytes()
            if bad == ("k288", i, n):
                t, dims, raw = gguf.GGML_Q5_K, [288, r], np.zeros(r * 288 // 256 * 176, np.uint8).tobytes()
            ts.append((f"blk.{i}.{g}.weight", t, dims, raw))
    write_gguf(path, META, ts)


def random_kq(mix, seed=0):
    """Random blocks per matrix in the mix's types -> (qw, norms)."""
    rng = np.random.default_rng(seed)
    H, V = TINY.hidden, TINY.vocab
    ty = MIXES[mix]

    def blocks(qt, n, s):
        return (R.random_blocks_q5_k(n, s, 0.05) if qt == 13 else Q.random_blocks(qt, n, s, 0.05)).reshape(-1)

    jit = lambda: (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)  # noqa: E731
    norms = {"final_norm": jit(), "layers": [{"attn_norm": jit(), "ffn_norm": jit()} for _ in range(TINY.n_layers)]}
    qt = ty("embed", 0, TINY.n_layers)
    qw = {"embed": (qt, blocks(qt, V * H // 256, seed + 1))}
    for i in range(TINY.n_layers):
        for j, (n, (r, k)) in enumerate(SHAPES.items()):
            qt = ty(n, i, TINY.n_layers)
            qw[(i, n)] = (qt, blocks(qt, r * k // 256, seed + 100 * i + 10 + j))
    return qw, norms


def _check_recorded(eng, qw):
    assert eng.q[(L.MS_T_EMBED, 0)][0] == 14  # the tied Q6_K token_embd, loaded once
    assert np.array_equal(eng.q[(L.MS_T_EMBED, 0)][1], qw["embed"][1])
    n = 0
    for key, (qt, b) in qw.items():
        if key == "embed":
            continue
        i, name = key
        got_t, got = eng.q[(_T[name], i)]
        assert got_t == qt and got.size == b.size and np.array_equal(got, b), key
        n += 1
    assert n == 7 * TINY.n_layers and len(eng.q) == n + 1 and len(eng.f16) == 1 + 2 * TINY.n_layers
    for key, bits in eng.f16.items():  # the F32 norms, uploaded as fp16
        assert np.asarray(bits).size == TINY.hidden, key


@pytest.mark.parametrize("mix", list(MIXES))
def test_gguf_loads_unpermuted_blocks(tmp_path, mix):
    qw, norms = random_kq(mix)
    kinds = {t for t, _ in qw.values()}
    assert kinds == ({13, 14} if mix == "q5_k_m" else {12, 13, 14})
    path = str(tmp_path / f"tiny-{mix}.gguf")
    write_kq_gguf(path, qw, norms)
    eng = Recorder()
    gguf.load_gguf(eng, path)
    _check_recorded(eng, qw)
    _, ts = gguf.read_gguf(path)  # the Q/K rows really were permuted in the file
    assert not np.array_equal(np.asarray(ts["blk.0.attn_q.weight"][2]), qw[(0, "wq")][1])
    assert ts["blk.0.attn_q.weight"][0] == (13 if mix == "q5_k_m" else 12)
    assert gguf.QBLOCK[gguf.GGML_Q5_K] == (256, 176) and gguf.GGML_Q5_K == 13


def test_gguf_refuses_q5_k_among_q8_0(tmp_path):
    """One Q5_K matrix in an otherwise Q8_0 file (and the reverse) is refused: K-quants and Q8_0 do
    not share an engine."""
    from test_q8_0_ref import q8_gguf
    path = str(tmp_path / "q8.gguf")
    q8_gguf(path)
    _, ts = gguf.read_gguf(path)
    r, k = SHAPES["wo"]
    keep = [(n, t, d, bytes(raw)) for n, (t, d, raw) in ts.items() if n != "blk.1.attn_output.weight"]
    keep.append(("blk.1.attn_output.weight", gguf.GGML_Q5_K, [k, r], R.random_blocks_q5_k(r * k // 256, 2).tobytes()))
    bad = str(tmp_path / "q5-in-q8.gguf")
    write_gguf(bad, META, keep)
    with pytest.raises(gguf.GGUFError, match="Q8_0"):
        gguf.load_gguf(Recorder(), bad)
    qw, norms = random_kq("q5_k_m")
    bad2 = str(tmp_path / "q8-in-q5.gguf")
    write_kq_gguf(bad2, qw, norms, bad=("q8", 0, "w_up"))
    with pytest.raises(gguf.GGUFError, match="Q8_0"):
        gguf.load_gguf(Recorder(), bad2)


def test_gguf_refuses_row_length_288(tmp_path):
    qw, norms = random_kq("q5_k_m")
    path = str(tmp_path / "k288.gguf")
    write_kq_gguf(path, qw, norms, bad=("k288", 0, "wv"))
    with pytest.raises(gguf.GGUFError, match="multiple of 256"):
        gguf.read_gguf(path)


def test_q5_k_m_tag_resolves_through_an_ollama_store(tmp_path):
    from test_ollama_gguf import PARAMS, ollama_store_with
    root, g = str(tmp_path / "models"), str(tmp_path / "model.gguf")
    qw, norms = random_kq("q5_k_m", seed=5)
    write_kq_gguf(g, qw, norms)
    ollama_store_with(root, "llama3.2:3b-instruct-q5_K_M", g, PARAMS)
    os.remove(g)
    m = ollama_store.resolve("llama3.2:3b-instruct-q5_K_M", root)
    assert os.path.basename(m.gguf).startswith("sha256-")
    eng = Recorder()
    gguf.load_gguf(eng, m.gguf)
    _check_recorded(eng, qw)


def test_exports_and_constants():
    assert "ms_init_synthetic_q5_k_m" in L.EXPORTED and "ms_op_qgemv_resid" in L.EXPORTED
    assert L.MS_GGML_Q5_K == 13 == R.GGML_TYPE_Q5_K == gguf.GGML_Q5_K
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mapsum.h")).read()
    assert "#define MS_GGML_Q5_K 13" in hdr and "ms_init_synthetic_q5_k_m(" in hdr
