"""CPU half of the q8_0 KV cache tests: the numpy contract (tests/kv_q8_0_ref.py) on known answers, the
host interface (kv_cache_type, the environment spellings, the new exports), the model mirror, and what the
GPU op test's 2e-3 bar can tell apart: the float32 emulation of the engine's arithmetic stays under half of
it, every mutant moves the float64 reference by at least ten times it."""
import inspect
import math

import numpy as np
import pytest

import kv_q8_0_ref as R


def _row(**at):
    t = np.zeros(128, np.float16)
    for i, v in at.items():
        t[int(i[1:])] = v
    return t


def _f16bits(x):
    return int(np.float16(x).view(np.uint16))


def test_known_answer_rows():
    c, s = R.quantize_rows(_row())
    assert not c.any() and not s.any()  # all zero: id = 0, codes 0, scale +0
    assert not R.dequantize(c, s).any()

    c, s = R.quantize_rows(_row(i5=1.0))  # one value: 127 at it, d = 1/127
    assert c[5] == 127 and c.sum() == 127
    assert s.tolist() == [_f16bits(np.float32(1.0) / np.float32(127.0)), 0, 0, 0]

    c, s = R.quantize_rows(_row(i0=2.0, i1=-2.0, i40=-3.0, i41=3.0))  # +-amax ties
    assert c[:2].tolist() == [127, -127] and c[40:42].tolist() == [-127, 127]

    # amax = 127 -> d = 1, id = 1: x.5 rounds away from zero, in both signs (RNE would give 0, 2, -2)
    c, s = R.quantize_rows(_row(i64=127.0, i65=0.5, i66=-0.5, i67=2.5, i68=-2.5, i69=1.5))
    assert c[64:70].tolist() == [127, 1, -1, 3, -3, 2] and s[2] == _f16bits(1.0)

    tiny = np.float16(2.0 ** -24)  # the smallest fp16 subnormal: the code survives, the fp16 scale underflows to 0
    c, s = R.quantize_rows(_row(i96=tiny))
    assert c[96] == 127 and s[3] == 0 and R.dequantize(c, s)[96] == 0.0

    c, s = R.quantize_rows(_row(i3=65504.0))  # d = 515.78 -> f16 516: dequantises to 127 * 516
    assert c[3] == 127 and s[0] == _f16bits(516.0) and R.dequantize(c, s)[3] == 127 * 516.0

    t = _row(i1=1.0, i33=np.nan, i70=np.inf, i100=-4.0, i101=1.0)  # non-finite blocks: scale NaN, codes 0
    c, s = R.quantize_rows(t)
    assert s[1] == R.NAN_SCALE and s[2] == R.NAN_SCALE and not c[32:96].any()
    assert c[1] == 127 and c[100] == -127 and c[101] == 32  # 1 * (127 / 4) = 31.75
    dq = R.dequantize(c, s)
    assert np.isnan(dq[32:96]).all() and np.isfinite(dq[:32]).all() and np.isfinite(dq[96:]).all()


def test_quantiser_matches_a_scalar_restatement():
    """The vectorised quantiser against the textbook loop, on rows with block amplitudes from 1e-6 to 1e4."""
    rng = np.random.default_rng(5)
    t = (rng.standard_normal((64, 128)) * 10.0 ** rng.uniform(-6, 4, (64, 4)).repeat(32, axis=1)).astype(np.float16)
    c, s = R.quantize_rows(t)
    for r in range(0, 64, 7):
        for b in range(4):
            blk = t[r, 32 * b:32 * b + 32].astype(np.float32)
            d = np.float32(np.abs(blk).max()) / np.float32(127.0)
            inv = np.float32(1.0) / d if d != 0 else np.float32(0.0)
            want = [int(math.copysign(math.floor(abs(float(np.float32(x * inv))) + 0.5), float(x))) for x in blk]
            assert c[r, 32 * b:32 * b + 32].tolist() == want
            assert s[r, b] == _f16bits(d)
    err = np.abs(R.dequantize(c, s) - t.astype(np.float32)).reshape(64, 4, 32).max(axis=-1)
    amax = np.abs(t.astype(np.float32)).reshape(64, 4, 32).max(axis=-1)
    # half a code step + the scale's fp16 rounding (2^-11 relative, 2^-25 absolute where it is subnormal) x 127
    assert (err <= amax * (0.5 / 127 + 2.0 ** -11) + 127 * 2.0 ** -25).all()


def test_pool_packer_layout():
    assert (R.CODE_BYTES, R.SCALE_BYTES, R.SLAB) == (8192, 512, 8704)
    # Llama-3.2-3B (28 layers, 8 kv heads): K and V bytes per token
    assert 28 * 8 * 2 * R.SLAB // 64 == 60928 and 28 * 8 * 2 * 128 * 2 == 114688
    rng = np.random.default_rng(2)
    pool = np.full((3, 2, R.SLAB), 0xA5, np.uint8)
    t = rng.standard_normal((5, 128)).astype(np.float16)
    c, s = R.quantize_rows(t)
    where = [(0, 0, 0), (0, 0, 63), (2, 1, 17), (1, 0, 1), (2, 0, 62)]
    for (page, kvh, off), cr, sr in zip(where, c, s):
        R.pack_rows(pool, page, kvh, off, cr, sr)
    codes, scales = R.unpack_pool(pool)
    touched = np.zeros(pool.shape, bool)
    for (page, kvh, off), cr, sr in zip(where, c, s):
        assert np.array_equal(codes[page, kvh, off], cr) and np.array_equal(scales[page, kvh, off], sr)
        assert pool[page, kvh, off * 128 + 5] == cr.view(np.uint8)[5]
        assert pool[page, kvh, 8192 + off * 8 + 2] == sr.view(np.uint8)[2]  # scales [token][block], little endian
        touched[page, kvh, off * 128:(off + 1) * 128] = True
        touched[page, kvh, 8192 + off * 8:8192 + off * 8 + 8] = True
    assert (pool[~touched] == 0xA5).all()


def test_host_interface(monkeypatch):
    """Engine(kv_cache_type=...), the environment spellings of the default factory, the refusals, the exports."""
    from mapsum import _lib, compat
    from mapsum.engine import Engine, check_kv_cache_type

    for name in ("ms_enable_kv_q8_0", "ms_op_kv_store_q8_0", "ms_op_attn_decode_q8_0",
                 "ms_op_attn_decode_q8_0_workspace"):
        assert name in _lib.EXPORTED
    assert inspect.signature(Engine.__init__).parameters["kv_cache_type"].default == "f16"
    assert check_kv_cache_type("f16") == "f16" and check_kv_cache_type(" Q8_0 ") == "q8_0"
    for bad in ("q4_0", "q8", "", "fp16", None):
        with pytest.raises(ValueError, match="'f16', 'q8_0'"):
            check_kv_cache_type(bad)
    from mapsum.config import TINY
    with pytest.raises(ValueError, match="q4_0"):  # refused before any library or device is touched
        Engine(TINY, kv_cache_type="q4_0")

    monkeypatch.delenv("MAPSUM_KV_CACHE_TYPE", raising=False)
    monkeypatch.delenv("OLLAMA_KV_CACHE_TYPE", raising=False)
    assert compat.kv_cache_type_from_env() == "f16" and compat._engine_kwargs()["kv_cache_type"] == "f16"
    monkeypatch.setenv("OLLAMA_KV_CACHE_TYPE", "q8_0")
    assert compat._engine_kwargs()["kv_cache_type"] == "q8_0"
    monkeypatch.setenv("MAPSUM_KV_CACHE_TYPE", "f16")  # the project's own spelling wins
    assert compat.kv_cache_type_from_env() == "f16"
    monkeypatch.setenv("MAPSUM_KV_CACHE_TYPE", "q4_0")
    with pytest.raises(ValueError, match="MAPSUM_KV_CACHE_TYPE.*'f16', 'q8_0'"):
        compat.kv_cache_type_from_env()
    monkeypatch.delenv("MAPSUM_KV_CACHE_TYPE")
    monkeypatch.setenv("OLLAMA_KV_CACHE_TYPE", "q4_0")
    with pytest.raises(ValueError, match="OLLAMA_KV_CACHE_TYPE"):
        compat.kv_cache_type_from_env()


def test_mirror_quantises_decode_calls_only():
    """The mirror is OracleLlama with mut["attend"] on the decode calls: the prefill call is the fp16-cache
    model's, the cache itself stays fp16 (the hook edits what a call attends to), and the decode logits move
    by the quantisation -- inside the 2e-2 north star, but not by nothing."""
    import decode_edges_ref as E

    o = E.oracle()
    prompt = np.random.default_rng(41).integers(0, 4000, size=70).astype(np.int32)
    plain, mirror = o.new_cache(), o.new_cache()
    a, _ = o.forward(prompt, plain)
    b, _ = o.forward(prompt, mirror)
    assert np.array_equal(a, b)
    tok = int(np.argmax(a))
    for _ in range(3):
        a, _ = o.forward([tok], plain)
        b, _ = o.forward([tok], mirror, mut={"attend": R.mirror_hook})
        # layer 0's rows do not depend on attention: the hook left the cache fp16 (later layers see moved inputs)
        assert np.array_equal(plain["k"][0], mirror["k"][0]) and np.array_equal(plain["v"][0], mirror["v"][0])
        d = R.row_rel(b, a)
        assert 1e-4 < d < 2e-2, d
        tok = int(np.argmax(a))


@pytest.mark.parametrize("G,split_keys", [(3, 512), (4, 512), (3, 4096), (4, 4096)])
def test_emulation_and_mutants(G, split_keys):
    """On the GPU op test's inputs: the emulation (float32, the contract's fp16 roundings) within half the
    bar of float64 on the same bytes; every mutant at >= 10 x the bar wherever it can occur."""
    oc = R.op_case(G, split_keys)
    case, ref, emul = oc["case"], oc["ref"], oc["emul"]
    assert np.isfinite(ref).all()
    worst = max(R.row_rel(emul[i, h], ref[i, h]) for i in range(len(R.LENS)) for h in range(case.Hq))
    print(f"KVQ8 emulation G={G} split={split_keys}: worst row {worst:.2e} (bar {R.BAR:.0e})")
    assert worst <= R.BAR / 2
    # every placement kind occurs, and the decisive key carries real weight without being alone
    kinds = {R.KINDS[(h % G + i) % len(R.KINDS)] for i in range(len(R.LENS)) for h in range(case.Hq)}
    assert kinds == set(R.KINDS)
    ratios = R.mutant_ratios(case, ref)
    print("KVQ8 mutant ratios (x bar): " + ", ".join(f"{k} {v:.0f}" for k, v in ratios.items()))
    for kind, ratio in ratios.items():
        assert ratio >= R.MUTANT_FACTOR, (kind, ratio)


def test_qwen3_mirror_restates_the_oracle():
    """Without the quantising edit the QK-norm mirror is OracleQwen3.forward bit for bit (prefill and decode);
    with it a decode call moves, inside the north star."""
    import qwen3_ref as Q

    o = Q.tiny_oracle()
    prompt = np.random.default_rng(43).integers(0, 4000, size=40).astype(np.int32)
    a, b, c = o.new_cache(), o.new_cache(), o.new_cache()
    la, _ = o.forward(prompt, a)
    assert np.array_equal(la, R.qwen3_mirror_forward(o, prompt, b, False))
    R.qwen3_mirror_forward(o, prompt, c, False)
    tok = int(np.argmax(la))
    la, _ = o.forward([tok], a)
    assert np.array_equal(la, R.qwen3_mirror_forward(o, [tok], b, False))
    d = R.row_rel(R.qwen3_mirror_forward(o, [tok], c, True), la)
    assert 1e-4 < d < 2e-2, d
