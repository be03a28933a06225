"""A qwen3-architecture GGUF through the loader, the config, the tokenizer, the template check and
the drop-in (mapsum/gguf.py, ollama_store.py, tokenizer.py, template.py, compat.py).

No Qwen3 GGUF, vocabulary or Ollama template exists offline, so the files are written here with
tests/test_gguf.py's writer the way llama.cpp's converter writes a qwen3 model: metadata under
``qwen3.*``, HF's row order for attn_q / attn_k (the converter permutes them for the llama
architecture only), ``blk.N.attn_q_norm.weight`` / ``attn_k_norm.weight``, an ``output.weight``, no
``rope_freqs``; the vocabulary is a byte-level BPE trained on the reference's Vietnamese map prompt
with the published "qwen2" pre-tokenizer pattern, ChatML specials, and no BOS.  Parity against a
real Qwen3 blob, its vocabulary and Ollama's qwen3 template is unpinned.
"""
import json

import numpy as np
import pytest

import qwen3_ref as R
from mapsum import _lib as L
from mapsum import compat, gguf, ollama_store, template
from mapsum.config import TINY_QWEN3 as CFG
from mapsum.tokenizer import PRE_TOKENIZERS, gguf_stop_ids, tokenizer_from_gguf
from mapsum.weights import f32_to_f16_bits
from oracle import quants as Q
from test_gguf import _NAMES, _T, Recorder, write_gguf
from test_ollama_gguf import CHATML, CORPUS, LLAMA3_LIKE, SAMPLES, RecordingEngine, ollama_store_with

ENDOFTEXT, IM_START, IM_END = 4000, 4001, 4002
SPECIALS = {ENDOFTEXT: "<|endoftext|>", IM_START: "<|im_start|>", IM_END: "<|im_end|>"}
META = {"general.architecture": "qwen3", "general.name": "tiny-qwen3-test", "qwen3.block_count": CFG.n_layers,
        "qwen3.embedding_length": CFG.hidden, "qwen3.attention.head_count": CFG.n_heads,
        "qwen3.attention.head_count_kv": CFG.n_kv_heads, "qwen3.attention.key_length": CFG.head_dim,
        "qwen3.attention.value_length": CFG.head_dim, "qwen3.feed_forward_length": CFG.ffn,
        "qwen3.rope.freq_base": CFG.rope_theta, "qwen3.attention.layer_norm_rms_epsilon": CFG.norm_eps}
SHAPES = {"wq": (CFG.n_heads * 128, CFG.hidden), "wk": (CFG.n_kv_heads * 128, CFG.hidden),
          "wv": (CFG.n_kv_heads * 128, CFG.hidden), "wo": (CFG.hidden, CFG.n_heads * 128),
          "w_gate": (CFG.ffn, CFG.hidden), "w_up": (CFG.ffn, CFG.hidden), "w_down": (CFG.hidden, CFG.ffn)}
PARAMS = {"stop": ["<|im_start|>", "<|im_end|>"]}


_VOCAB = []


@pytest.fixture(scope="module")
def tok_meta():
    return toy_qwen_vocab()


def toy_qwen_vocab():
    """(reference tokenizer object, GGUF tokenizer metadata) of a 4096-entry toy Qwen vocabulary
    (pre = "qwen2", ChatML specials, no BOS)."""
    if not _VOCAB:
        _VOCAB.append(_train_vocab())
    return _VOCAB[0]


def _train_vocab():
    from tokenizers import Regex, decoders, models, pre_tokenizers, trainers
    from tokenizers import Tokenizer as T
    pat, ignore_merges = PRE_TOKENIZERS["qwen2"]
    assert not ignore_merges and r"|\p{N}|" in pat  # digits one at a time
    tk = T(models.BPE())
    tk.pre_tokenizer = pre_tokenizers.Sequence([
        pre_tokenizers.Split(Regex(pat), behavior="isolated", invert=False),
        pre_tokenizers.ByteLevel(add_prefix_space=False, trim_offsets=False, use_regex=False)])
    tk.decoder = decoders.ByteLevel()
    tk.train_from_iterator(CORPUS, trainers.BpeTrainer(vocab_size=700, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                                        show_progress=False))
    model = json.loads(tk.to_str())["model"]
    merges = [m if isinstance(m, str) else " ".join(m) for m in model["merges"]]
    tokens, types = [None] * CFG.vocab, [1] * CFG.vocab
    for t, i in model["vocab"].items():
        tokens[i] = t
    for i in range(CFG.vocab):
        if tokens[i] is None:
            tokens[i], types[i] = SPECIALS.get(i, f"<|reserved_{i}|>"), 3
    meta = {"tokenizer.ggml.model": "gpt2", "tokenizer.ggml.pre": "qwen2", "tokenizer.ggml.tokens": tokens,
            "tokenizer.ggml.token_type": types, "tokenizer.ggml.merges": merges,
            "tokenizer.ggml.bos_token_id": ENDOFTEXT, "tokenizer.ggml.eos_token_id": IM_END,
            "tokenizer.ggml.padding_token_id": ENDOFTEXT, "tokenizer.ggml.add_bos_token": False}
    return tk, meta


def _norm_tensors(w):
    f = lambda a: np.asarray(a, np.float32).tobytes()  # noqa: E731
    ts = [("output_norm.weight", gguf.GGML_F32, [CFG.hidden], f(w["final_norm"]))]
    for i, ly in enumerate(w["layers"]):
        for n in ("attn_norm", "ffn_norm"):
            ts.append((f"blk.{i}.{n}.weight", gguf.GGML_F32, [CFG.hidden], f(ly[n])))
        ts.append((f"blk.{i}.attn_q_norm.weight", gguf.GGML_F32, [CFG.head_dim], f(ly["q_norm"])))
        ts.append((f"blk.{i}.attn_k_norm.weight", gguf.GGML_F32, [CFG.head_dim], f(ly["k_norm"])))
    return ts


def float_qwen3_gguf(path, w, extra_meta=None):
    """F32 matrices in HF's row order (no Q/K permutation), the gains, an untied output.weight."""
    f = lambda a: np.asarray(a, np.float32).tobytes()  # noqa: E731
    ts = [("token_embd.weight", gguf.GGML_F32, [CFG.hidden, CFG.vocab], f(w["embed"])),
          ("output.weight", gguf.GGML_F32, [CFG.hidden, CFG.vocab], f(w["lm_head"]))] + _norm_tensors(w)
    for i, ly in enumerate(w["layers"]):
        for n, g in _NAMES.items():
            ts.append((f"blk.{i}.{g}.weight", gguf.GGML_F32, [ly[n].shape[1], ly[n].shape[0]], f(ly[n])))
    write_gguf(path, dict(META, **(extra_meta or {})), ts)


def quant_qwen3_gguf(path, w):
    """The Q4_K_M mix: Q6_K embedding / lm_head / V, Q4_K elsewhere; -> {key: (type, blocks [rows][bytes])}."""
    want, ts = {}, _norm_tensors(w)
    for name, gname in (("embed", "token_embd"), ("lm_head", "output")):
        b = Q.random_blocks(Q.GGML_TYPE_Q6_K, CFG.vocab * CFG.hidden // 256, seed=len(name)).reshape(CFG.vocab, -1)
        want[name] = (Q.GGML_TYPE_Q6_K, b)
        ts.append((f"{gname}.weight", gguf.GGML_Q6_K, [CFG.hidden, CFG.vocab], b.tobytes()))
    for i in range(CFG.n_layers):
        for n, g in _NAMES.items():
            qt = Q.GGML_TYPE_Q6_K if n == "wv" else Q.GGML_TYPE_Q4_K
            r, k = SHAPES[n]
            b = Q.random_blocks(qt, r * k // 256, seed=10 * i + len(n)).reshape(r, -1)
            want[(i, n)] = (qt, b)
            ts.append((f"blk.{i}.{g}.weight", qt, [k, r], b.tobytes()))
    write_gguf(path, META, ts)
    return want


class QwenRecorder(Recorder):
    cfg = CFG


def _check_norms(eng, w):
    assert np.array_equal(eng.f16[(L.MS_T_FINAL_NORM, 0)], f32_to_f16_bits(w["final_norm"]))
    for i, ly in enumerate(w["layers"]):
        for key, t in (("attn_norm", L.MS_T_ATTN_NORM), ("ffn_norm", L.MS_T_FFN_NORM), ("q_norm", L.MS_T_Q_NORM),
                       ("k_norm", L.MS_T_K_NORM)):
            assert np.array_equal(eng.f16[(t, i)], f32_to_f16_bits(ly[key])), (i, key)
        assert not np.array_equal(eng.f16[(L.MS_T_Q_NORM, i)], eng.f16[(L.MS_T_K_NORM, i)])


def test_float_qwen3_gguf_loads_hf_row_order(tmp_path):
    w = R.tiny_weights()
    path = str(tmp_path / "tiny-qwen3-f32.gguf")
    float_qwen3_gguf(path, w)
    eng = QwenRecorder()
    gguf.load_gguf(eng, path)
    assert np.array_equal(eng.f16[(L.MS_T_EMBED, 0)], f32_to_f16_bits(w["embed"]))
    assert np.array_equal(eng.f16[(L.MS_T_LM_HEAD, 0)], f32_to_f16_bits(w["lm_head"]))  # output.weight
    assert not np.array_equal(w["embed"], w["lm_head"])
    for i, ly in enumerate(w["layers"]):
        for n, t in _T.items():  # Q / K rows exactly as written: no un-permutation for qwen3
            assert np.array_equal(eng.f16[(t, i)], f32_to_f16_bits(ly[n])), (i, n)
        assert not np.array_equal(gguf.unpermute_rows(ly["wq"], CFG.n_heads), ly["wq"])
    _check_norms(eng, w)


def test_quant_qwen3_gguf_loads_blocks_as_written(tmp_path):
    w = R.tiny_weights()
    path = str(tmp_path / "tiny-qwen3-q4km.gguf")
    want = quant_qwen3_gguf(path, w)
    eng = QwenRecorder()
    gguf.load_gguf(eng, path)
    assert {qt for qt, _ in want.values()} == {Q.GGML_TYPE_Q4_K, Q.GGML_TYPE_Q6_K}
    for key, (qt, b) in want.items():
        tensor, layer = ((L.MS_T_EMBED if key == "embed" else L.MS_T_LM_HEAD), 0) if isinstance(key, str) \
            else (_T[key[1]], key[0])
        got_t, got = eng.q[(tensor, layer)]
        assert got_t == qt and np.array_equal(got, b.reshape(-1)), key
    _check_norms(eng, w)


def test_architecture_and_config_must_agree(tmp_path):
    w = R.tiny_weights()
    path = str(tmp_path / "q.gguf")
    float_qwen3_gguf(path, w)

    class LlamaCfg(Recorder):
        cfg = CFG.with_(qk_norm=False)
    with pytest.raises(gguf.GGUFError, match="Q/K norm"):
        gguf.load_gguf(LlamaCfg(), path)
    meta, ts = gguf.read_gguf(path)
    keep = [(n, t, d, bytes(raw)) for n, (t, d, raw) in ts.items() if n != "blk.1.attn_k_norm.weight"]
    write_gguf(path, META, keep)
    with pytest.raises(gguf.GGUFError, match="blk.1.attn_k_norm.weight"):
        gguf.load_gguf(QwenRecorder(), path)
    write_gguf(path, dict(META, **{"general.architecture": "gemma3"}), [])
    with pytest.raises(gguf.GGUFError, match="gemma3"):
        gguf.load_gguf(QwenRecorder(), path)
    write_gguf(path, dict(META, **{"qwen3.block_count": 3}), [])
    with pytest.raises(gguf.GGUFError, match="qwen3.block_count"):
        gguf.load_gguf(QwenRecorder(), path)


def test_config_tokenizer_and_stop_ids_from_qwen3_metadata(tmp_path, tok_meta):
    tk, tm = tok_meta
    path = str(tmp_path / "q.gguf")
    float_qwen3_gguf(path, R.tiny_weights(), tm)
    meta, ts = gguf.read_gguf(path)
    cfg = ollama_store.config_from_gguf(meta)
    assert (cfg.n_layers, cfg.hidden, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.ffn, cfg.vocab) == \
        (CFG.n_layers, CFG.hidden, CFG.n_heads, CFG.n_kv_heads, 128, CFG.ffn, CFG.vocab)
    assert cfg.qk_norm and cfg.rope_factor == 0 and cfg.rope_theta == CFG.rope_theta
    assert abs(cfg.norm_eps - CFG.norm_eps) < 1e-12
    assert IM_END in cfg.eos_ids and ENDOFTEXT in cfg.eos_ids and gguf_stop_ids(meta)[0] == IM_END
    g = tokenizer_from_gguf(meta)
    assert g.bos_id is None
    for s in CORPUS + SAMPLES:
        assert g.encode(s) == tk.encode(s).ids, s[:40]  # no BOS in front
        assert g.decode(g.encode(s)) == s
    assert len(g.encode("12345", add_bos=False)) == 5  # single digits, never merged across
    ids = g.encode(template.render_chatml("Xin chào"))
    assert ids[0] == IM_START and ids.count(IM_START) == 2 and ids.count(IM_END) == 1 and ENDOFTEXT not in ids
    assert template.render_chatml("P") == "<|im_start|>user\nP<|im_end|>\n<|im_start|>assistant\n"
    # a llama file's metadata still gives a llama config
    assert not ollama_store.config_from_gguf({"general.architecture": "llama"}).qk_norm


@pytest.mark.parametrize("name,hidden,heads,kv,ffn", [("qwen3-4b", 2560, 32, 8, 9728), ("qwen3-0.6b", 1024, 16, 8, 3072),
                                                      ("qwen3-32b", 5120, 64, 8, 25600)])
def test_unsupported_qwen3_sizes_are_refused_with_the_named_check(name, hidden, heads, kv, ffn):
    meta = dict(META, **{"general.name": name, "qwen3.embedding_length": hidden, "qwen3.attention.head_count": heads,
                         "qwen3.attention.head_count_kv": kv, "qwen3.feed_forward_length": ffn,
                         "qwen3.vocab_size": 151936})
    with pytest.raises(gguf.GGUFError) as ei:
        ollama_store.config_from_gguf(meta)
    msg = str(ei.value)
    assert name in msg and ("hidden must equal n_heads*head_dim" in msg or "at most 64 query+key heads" in msg)
    if name != "qwen3-32b":
        assert "hidden must equal n_heads*head_dim" in msg
    # Qwen3-8B's header passes
    ok = dict(META, **{"qwen3.embedding_length": 4096, "qwen3.attention.head_count": 32, "qwen3.block_count": 36,
                       "qwen3.feed_forward_length": 12288, "qwen3.vocab_size": 151936})
    cfg = ollama_store.config_from_gguf(ok)
    assert (cfg.hidden, cfg.ffn, cfg.vocab, cfg.n_layers) == (4096, 12288, 151936, 36)


@pytest.fixture(scope="module")
def qstore(tok_meta, tmp_path_factory):
    root = tmp_path_factory.mktemp("ollama_models_qwen3")
    g = str(root / "model.gguf")
    float_qwen3_gguf(g, R.tiny_weights(), tok_meta[1])
    ollama_store_with(str(root), "qwen3:tiny", g, PARAMS, template=CHATML)
    ollama_store_with(str(root), "qwen3:llama-template", g, PARAMS, template=LLAMA3_LIKE)
    return str(root)


def test_template_family_follows_the_architecture(qstore, tmp_path):
    assert ollama_store.template_problems(CHATML, "qwen3") == []
    assert ollama_store.template_problems(CHATML) != [] and ollama_store.template_problems(LLAMA3_LIKE, "qwen3") != []
    assert ollama_store.resolve("qwen3:tiny", qstore).template == CHATML
    with pytest.raises(ollama_store.OllamaStoreError, match="template is not ChatML"):
        ollama_store.resolve("qwen3:llama-template", qstore)
    # a llama model with a ChatML template is still refused
    from test_gguf import META as LLAMA_META
    lg = str(tmp_path / "llama.gguf")
    write_gguf(lg, LLAMA_META, [])
    ollama_store_with(qstore, "llama3.2:chatml", lg, {}, template=CHATML)
    with pytest.raises(ollama_store.OllamaStoreError, match="template is not Llama-3"):
        ollama_store.resolve("llama3.2:chatml", qstore)


def test_ollamallm_qwen3_tag_renders_chatml_without_bos(qstore, tok_meta, monkeypatch):
    monkeypatch.setenv("OLLAMA_MODELS", qstore)
    monkeypatch.delenv("MAPSUM_MODEL_DIR", raising=False)
    monkeypatch.delenv("MAPSUM_GGUF", raising=False)
    import mapsum.engine
    monkeypatch.setattr(mapsum.engine, "Engine", RecordingEngine)
    compat._BACKENDS.pop("qwen3:tiny", None)
    RecordingEngine.made.clear()
    try:
        llm = compat.OllamaLLM("http://localhost:11434", "qwen3:tiny", max_new_tokens=4096)
        prompt = template.map_prompt("mapreduce", "Chương 1. Nội dung chính.")
        out = llm._call(prompt)
        eng = RecordingEngine.made[0]
        assert eng.cfg.qk_norm and not eng.cfg.tie_embeddings and eng.cfg.vocab == CFG.vocab
        assert IM_END in eng.eos_ids and IM_START in eng.eos_ids  # GGUF eos + the params layer's stops
        assert (L.MS_T_Q_NORM, 1) in eng.f16 and (L.MS_T_LM_HEAD, 0) in eng.f16
        tok = tokenizer_from_gguf(tok_meta[1])
        ids = tok.encode(template.render_chatml(prompt))
        user = tok.encode("user\n", add_bos=False)
        assert ids[0] == IM_START and ids[1:1 + len(user)] == user and ENDOFTEXT not in ids
        assert out == compat.CLEANERS["pipeline"](tok.decode(ids[::-1]))  # the double's 'summary': the ids reversed
    finally:
        compat._BACKENDS.pop("qwen3:tiny", None)
