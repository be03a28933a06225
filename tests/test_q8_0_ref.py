"""Q8_0 on the CPU: the numpy reference itself (tests/q8_0_ref.py), the GGUF loader's Q8_0
route (mapsum/gguf.py) through a recording engine and an Ollama-layout store, and the export."""
import os

import numpy as np
import pytest

import q8_0_ref as R
from mapsum import _lib as L
from mapsum import gguf, ollama_store
from mapsum.config import TINY
from test_gguf import META, _NAMES, _T, Recorder, rope_freqs, write_gguf

SHAPES = {"wq": (TINY.n_heads * 128, TINY.hidden), "wk": (TINY.n_kv_heads * 128, TINY.hidden),
          "wv": (TINY.n_kv_heads * 128, TINY.hidden), "wo": (TINY.hidden, TINY.n_heads * 128),
          "w_gate": (TINY.ffn, TINY.hidden), "w_up": (TINY.ffn, TINY.hidden), "w_down": (TINY.hidden, TINY.ffn)}


def test_kat_blocks():
    b = R.kat_blocks()
    y = R.dequant_q8_0(b).reshape(-1, 32)
    q = b[:, 2:].view(np.int8).astype(np.float64)
    assert list(q[0, :3]) == [-128.0, 127.0, 0.0]
    d = np.array([1.0, 0.0, 2.0 ** -24, 65504.0, -0.5, -65504.0])
    assert np.array_equal(y[0, :3], np.float32([-128.0, 127.0, 0.0]))
    assert np.all(y[1] == 0.0)                                          # d = 0
    assert y[2, 0] == np.float32(-128 * 2.0 ** -24) and y[2, 1] == np.float32(127 * 2.0 ** -24)
    assert y[3, 0] == np.float32(-128 * 65504.0) and y[3, 1] == np.float32(127 * 65504.0)
    assert y[4, 0] == np.float32(64.0) and y[4, 1] == np.float32(-63.5)  # negative d
    # the fp32 product is the fp64 product: 11 x 8 significant bits fit in 24
    assert np.array_equal(y.astype(np.float64), d[:, None] * q)
    assert np.all(np.isfinite(y))


def test_fp32_product_is_exact_on_random_blocks():
    b = R.random_blocks_q8_0(4096, seed=3, scale=0.7)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float64)
    q = b[:, 2:].view(np.int8).astype(np.float64)
    assert np.array_equal(R.dequant_q8_0(b).astype(np.float64).reshape(-1, 32), d * q)
    assert (b[:, 2:].view(np.int8) == -128).any() and (d < 0).any()
    std = float(R.dequant_q8_0(b).std())
    assert 0.5 * 0.7 <= std <= 2 * 0.7


@pytest.mark.parametrize("sigma", [1.0, 0.02])
def test_round_trip(sigma):
    """|x - y| <= d/2 (rounding of q) + 127 d 2^-11 (d's fp16 rounding) = amax (1/254 + 2^-11) =
    4.43e-3 amax; the bound 4.5e-3 leaves the fp32 slack.  Measured on these inputs: relative
    Frobenius error 5.36e-3, worst block 4.37e-3 amax."""
    x = (np.random.default_rng(0).standard_normal((768, 768)) * sigma).astype(np.float32)
    b = R.quantize_q8_0(x)
    assert b.shape == (768 * 768 // 32, 34)
    y = R.dequant_q8_0(b).reshape(x.shape)
    fro = float(np.linalg.norm(x.astype(np.float64) - y) / np.linalg.norm(x.astype(np.float64)))
    xb, yb = x.reshape(-1, 32).astype(np.float64), y.reshape(-1, 32).astype(np.float64)
    worst = float(np.max(np.max(np.abs(xb - yb), 1) / np.max(np.abs(xb), 1)))
    print(f"sigma {sigma}: relative Frobenius error {fro:.3e}, worst block {worst:.3e} amax")
    assert fro <= 1e-2
    assert np.all(np.max(np.abs(xb - yb), 1) <= 4.5e-3 * np.max(np.abs(xb), 1))


def test_quantizer_edge_cases():
    x = np.zeros(64, np.float32)
    x[32:] = np.linspace(-1, 1, 32)
    b = R.quantize_q8_0(x)
    assert np.all(b[0] == 0)                      # amax = 0: d = 0, id = 0, q = 0
    q = b[1, 2:].view(np.int8)
    assert q[0] == -127 and q[-1] == 127          # the reference quantiser never emits -128
    h = R.quantize_q8_0(np.float32([0.5, 127.0, -0.5, 1.5] + [0.0] * 28))[0, 2:].view(np.int8)
    assert list(h[:4]) == [1, 127, -1, 2]         # d = 1: halves round away from zero (roundf)


def write_q8_gguf(path, emb, mats, norms, bad=None, meta=None):
    """TINY as an all-Q8_0 GGUF: emb [vocab][bytes] and mats[(layer, name)] [rows][bytes] raw blocks
    in the engine's row order (Q/K rows are permuted here, as llama.cpp's converter does), F32
    norms, rope_freqs.  bad: ("q4k" | "k288", layer, name) swaps in a faulty tensor."""
    H, V = TINY.hidden, TINY.vocab
    f32 = lambda a: np.asarray(a, np.float32).tobytes()  # noqa: E731
    ts = [("token_embd.weight", gguf.GGML_Q8_0, [H, V], emb.tobytes()),
          ("output_norm.weight", gguf.GGML_F32, [H], f32(norms["final_norm"])), rope_freqs()]
    heads = {"wq": TINY.n_heads, "wk": TINY.n_kv_heads}
    for i in range(TINY.n_layers):
        for n in ("attn_norm", "ffn_norm"):
            ts.append((f"blk.{i}.{n}.weight", gguf.GGML_F32, [H], f32(norms["layers"][i][n])))
        for n, g in _NAMES.items():
            r, k = SHAPES[n]
            b = mats[(i, n)].reshape(r, -1)
            a = gguf.permute_rows(b, heads[n]) if n in heads else b
            t, dims, raw = gguf.GGML_Q8_0, [k, r], a.tobytes()
            if bad == ("q4k", i, n):
                from oracle import quants as Q
                t, raw = gguf.GGML_Q4_K, Q.random_blocks(Q.GGML_TYPE_Q4_K, r * k // 256, seed=2).tobytes()
            if bad == ("k288", i, n):
                dims, raw = [288, r], R.random_blocks_q8_0(r * 9, seed=2).tobytes()
            ts.append((f"blk.{i}.{g}.weight", t, dims, raw))
    write_gguf(path, dict(META, **(meta or {})), ts)


def q8_gguf(path, seed=0, bad=None, meta=None):
    """A random TINY Q8_0 GGUF.  -> the un-permuted blocks per matrix."""
    rng = np.random.default_rng(seed)
    H, V = TINY.hidden, TINY.vocab
    jit = lambda: (1 + 0.1 * rng.standard_normal(H)).astype(np.float32)  # noqa: E731
    norms = {"final_norm": jit(), "layers": [{"attn_norm": jit(), "ffn_norm": jit()} for _ in range(TINY.n_layers)]}
    want = {"embed": R.random_blocks_q8_0(V * H // 32, seed=seed + 1, scale=0.05).reshape(V, -1)}
    for i in range(TINY.n_layers):
        for j, (n, (r, k)) in enumerate(SHAPES.items()):
            want[(i, n)] = R.random_blocks_q8_0(r * k // 32, seed=seed + 100 * i + 10 + j, scale=0.05).reshape(r, -1)
    write_q8_gguf(path, want["embed"], want, norms, bad=bad, meta=meta)
    return want, norms


def _check_recorded(eng, want):
    assert eng.q[(L.MS_T_EMBED, 0)][0] == 8
    assert np.array_equal(eng.q[(L.MS_T_EMBED, 0)][1], want["embed"].reshape(-1))
    n = 0
    for key, b in want.items():
        if key == "embed":
            continue
        i, name = key
        got_t, got = eng.q[(_T[name], i)]
        assert got_t == gguf.GGML_Q8_0 == 8 and np.array_equal(got, b.reshape(-1)), key
        n += 1
    assert n == 7 * TINY.n_layers and len(eng.q) == n + 1 and len(eng.f16) == 1 + 2 * TINY.n_layers


def test_q8_0_gguf_loads_unpermuted_blocks(tmp_path):
    path = str(tmp_path / "tiny-q8_0.gguf")
    want, _ = q8_gguf(path)
    eng = Recorder()
    gguf.load_gguf(eng, path)
    _check_recorded(eng, want)
    # the Q/K rows really were permuted in the file
    _, ts = gguf.read_gguf(path)
    assert not np.array_equal(np.asarray(ts["blk.0.attn_q.weight"][2]), want[(0, "wq")].reshape(-1))
    assert gguf.QBLOCK[gguf.GGML_Q8_0] == (32, 34)


def test_q8_0_gguf_refuses_a_k_quant_among_q8_0(tmp_path):
    path = str(tmp_path / "mixed.gguf")
    q8_gguf(path, bad=("q4k", 1, "wo"))
    with pytest.raises(gguf.GGUFError, match="Q8_0"):
        gguf.load_gguf(Recorder(), path)


def test_q8_0_gguf_refuses_a_float_matrix_among_q8_0(tmp_path):
    path = str(tmp_path / "ok.gguf")
    q8_gguf(path)
    _, ts = gguf.read_gguf(path)
    r, k = SHAPES["wv"]
    keep = [(n, t, d, bytes(raw)) for n, (t, d, raw) in ts.items() if n != "blk.0.attn_v.weight"]
    keep.append(("blk.0.attn_v.weight", gguf.GGML_F32, [k, r], np.zeros((r, k), np.float32).tobytes()))
    bad = str(tmp_path / "float-mixed.gguf")
    write_gguf(bad, META, keep)
    with pytest.raises(gguf.GGUFError, match="mixed"):
        gguf.load_gguf(Recorder(), bad)


def test_q8_0_gguf_refuses_row_length_288(tmp_path):
    path = str(tmp_path / "k288.gguf")
    q8_gguf(path, bad=("k288", 0, "wv"))
    gguf.read_gguf(path)  # a valid Q8_0 tensor (288 = 9 blocks) ...
    with pytest.raises(gguf.GGUFError, match="multiple of 256"):
        gguf.load_gguf(Recorder(), path)  # ... that the engine's 256-weight units cannot hold


def test_q8_0_tag_resolves_through_an_ollama_store(tmp_path):
    from test_ollama_gguf import PARAMS, ollama_store_with
    root = str(tmp_path / "models")
    g = str(tmp_path / "model.gguf")
    want, _ = q8_gguf(g, seed=5)
    ollama_store_with(root, "llama3.2:3b-instruct-q8_0", g, PARAMS)
    os.remove(g)
    m = ollama_store.resolve("llama3.2:3b-instruct-q8_0", root)
    assert os.path.basename(m.gguf).startswith("sha256-")
    eng = Recorder()
    gguf.load_gguf(eng, m.gguf)
    _check_recorded(eng, want)


def test_exports_and_constants():
    assert "ms_init_synthetic_q8_0" in L.EXPORTED
    assert L.MS_GGML_Q8_0 == 8 == R.GGML_TYPE_Q8_0
