"""Q8_0 weights on the GPU (needs one): the dequantiser, the fp16 copy, the dequant-fused GEMV
with every op-level epilogue, the grid-stride lm_head, split-K, and a Q8_0 engine end to end in
each decode regime -- against tests/q8_0_ref.py and the CPU oracle.

The GEMV reference is fp64 of X . dequant(W)^T on the exact weights d * q: the kernel multiplies
q as exact fp16 integers and applies d in fp32, so only the summation order and the matrix
core's internal rounding differ (the project's 1e-5 bar for its exact-weight MFMA form)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import q8_0_ref as R  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from mapsum import gguf  # noqa: E402
from mapsum.config import TINY  # noqa: E402
from mapsum.engine import Engine  # noqa: E402
from mapsum.weights import load_quantized  # noqa: E402
from oracle import quants as Q  # noqa: E402
from oracle.llama_ref import OracleLlama  # noqa: E402
from oracle.synth import f16_rne, make_weights  # noqa: E402
from test_gpu_parity import _prompt, _stream, _teacher_forced_agreement, rel  # noqa: E402
from test_q8_0_ref import SHAPES, write_q8_gguf  # noqa: E402

Q8 = L.MS_GGML_Q8_0
UNIT = 272  # packed (and raw) bytes per 256 weights


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _last_error(lib, handle=None):
    msg = lib.ms_last_error(handle)
    return msg.decode() if msg else ""


# ------------------------------------------------------------------ op level
def test_dequant_bit_exact(lib, dev):
    """777 units (6216 blocks), the hand-built blocks first: q = -128 / 127 / 0 under d = 1, 0,
    the smallest subnormal, 65504 and negative d."""
    b = R.random_blocks_q8_0(777 * 8, seed=5)
    kat = R.kat_blocks()
    b[:kat.shape[0]] = kat
    want = R.dequant_q8_0(b)
    bd = torch.from_numpy(b.reshape(-1)).to(dev)
    out = torch.empty(want.size, dtype=torch.float32, device=dev)
    L.check(lib.ms_op_dequant(Q8, bd.data_ptr(), 777, out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "dequant must be bit-exact"


def _packed(lib, dev, rows, K, seed, scale=1.0):
    b = R.random_blocks_q8_0(rows * K // 32, seed=seed, scale=scale)
    bd = torch.from_numpy(b.reshape(-1)).to(dev)
    wbf = torch.empty(rows, K, dtype=torch.float16, device=dev)
    pk = torch.empty(rows * (K // 256) * UNIT, dtype=torch.uint8, device=dev)
    L.check(lib.ms_op_quant_rows(Q8, bd.data_ptr(), rows, K, wbf.data_ptr(), pk.data_ptr(), _stream()))
    torch.cuda.synchronize()
    W = torch.from_numpy(R.dequant_q8_0(b).reshape(rows, K)).double()
    return b, wbf, pk, W


def test_quant_rows_f16_copy_is_rounded_dequant(lib, dev):
    b, wbf, pk, W = _packed(lib, dev, 48, 768, 6)
    assert np.array_equal(wbf.float().cpu().numpy(), f16_rne(W.float().numpy()))
    # the packed unit: the 8 scales, then byte 16 + 64 (s >> 1) + 16 g + 8 (s & 1) + i = q[32 s + 8 g + i]
    raw = b.reshape(48, 3, 8, 34)
    want = np.empty((48, 3, UNIT), np.uint8)
    want[:, :, :16] = raw[:, :, :, :2].reshape(48, 3, 16)
    q = raw[:, :, :, 2:].reshape(48, 3, 4, 2, 4, 8)        # [s >> 1][s & 1][g][i]
    want[:, :, 16:] = q.transpose(0, 1, 2, 4, 3, 5).reshape(48, 3, 256)  # [s >> 1][g][s & 1][i]
    assert np.array_equal(pk.cpu().numpy().reshape(48, 3, UNIT), want)


_MAXERR = {}


_GEMV_SHAPES = [(256, 768, L.MS_EPI_STORE_F16), (512, 2048, L.MS_EPI_ADD_F32), (1024, 768, L.MS_EPI_SWIGLU),
                (128, 8192, L.MS_EPI_STORE_F32), (16, 256, L.MS_EPI_STORE_F32)]


@pytest.mark.parametrize("M", [1, 8, 16, 33, 64])
@pytest.mark.parametrize("N,K,epi,rs", [c + (False,) for c in _GEMV_SHAPES] +
                         [c + (True,) for c in _GEMV_SHAPES if c[2] != L.MS_EPI_ADD_F32])
def test_qgemv_vs_fp64(lib, dev, M, N, K, epi, rs):
    """out = sum_b d_b (sum_k x_k q_k) against fp64 of X . dequant(W)^T: one tile and one unit
    (16 x 256), 3 units, 8 units on 8 waves, the 2-units-per-wave form (K = 8192), ragged MT (33),
    with and without the rows' deferred-norm scale where the epilogue takes one (ADD_F32 takes
    none).  Measured maxima on the MI355X: fp32 outputs 1.27e-7 (bar 1e-5), fp16 outputs 2.72e-4
    (bar 4e-3)."""
    b, wbf, pk, W = _packed(lib, dev, N, K, 7 + M)
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    # sums of squares of rows of rms 16 .. 32 (the engine's xb is pre-scaled by 2^-4): factors
    # 0.5 .. 1, so the fp16 outputs stay in range
    ssq = ((torch.rand(M, generator=g) * 3.0 + 1.0) * K * 256.0).to(dev)
    ref = X.double().cpu() @ W.T
    if rs:  # rows scaled by 16 / sqrt(ssq / K + eps) (kernels.h RowScale)
        ref = ref * (16.0 / torch.sqrt(ssq.double().cpu() / K + 1e-5))[:, None]
    f32 = epi in (L.MS_EPI_STORE_F32, L.MS_EPI_ADD_F32)
    tol = 1e-5 if f32 else 4e-3
    if epi == L.MS_EPI_SWIGLU:
        out = torch.zeros(M, N // 2, dtype=torch.float16, device=dev)
        r = ref.view(M, N // 32, 2, 16)
        exp = (torch.nn.functional.silu(r[:, :, 0, :]) * r[:, :, 1, :]).reshape(M, N // 2)
        ldo = N // 2
    elif epi == L.MS_EPI_STORE_F16:
        out = torch.zeros(M, N, dtype=torch.float16, device=dev)
        exp, ldo = ref, N
    elif epi == L.MS_EPI_ADD_F32:
        out = torch.randn(M, N, generator=g).to(dev)
        exp, ldo = out.double().cpu() + ref, N
    else:
        out = torch.full((M, N), float("nan"), dtype=torch.float32, device=dev)
        exp, ldo = ref, N
    if rs:
        L.check(lib.ms_op_set_row_scale(ssq.data_ptr(), 1, K, 1e-5))
    try:
        L.check(lib.ms_op_qgemv(X.data_ptr(), Q8, pk.data_ptr(), out.data_ptr(), M, N, K, ldo, epi, _stream()))
    finally:
        if rs:
            L.check(lib.ms_op_set_row_scale(None, 0, 0, 0.0))
    torch.cuda.synchronize()
    err = rel(out.double().cpu(), exp)
    key = "fp32" if f32 else "fp16"
    _MAXERR[key] = max(_MAXERR.get(key, 0.0), err)
    print(f"M {M} N {N} K {K} epi {epi} rs {rs}: rel err {err:.3e} (max so far: {_MAXERR})")
    assert err < tol


@pytest.mark.parametrize("M", [1, 8, 33])
@pytest.mark.parametrize("N,K", [(4096, 768), (1040, 3072)])
def test_qgemv_argmax_vs_fp64(lib, dev, M, N, K):
    """{max, id} partials per 16-column tile merge to the fp64 argmax of the dequantised product,
    unless the top two are within fp32 noise (the K-quant test's cases and decisiveness rule)."""
    b, wbf, pk, W = _packed(lib, dev, N, K, 5 + M)
    g = torch.Generator(device="cpu").manual_seed(3 * M + N + K)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    ref = X.double().cpu() @ W.T
    part = torch.full((M, N // 16, 2), float("nan"), device=dev)
    ids = torch.empty(M, dtype=torch.int32, device=dev)
    L.check(lib.ms_op_qgemv(X.data_ptr(), Q8, pk.data_ptr(), part.data_ptr(), M, N, K, N // 16,
                            L.MS_EPI_ARGMAX, _stream()))
    L.check(lib.ms_op_argmax_partials(part.data_ptr(), M, N // 16, ids.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(part).any(), "every 16-column tile writes its partial"
    srt = torch.sort(ref, 1).values
    got = ids.cpu().long()
    for r in range(M):
        if srt[r, -1] - srt[r, -2] > 1e-4 * (abs(float(srt[r, -1])) + 1.0):
            assert int(got[r]) == int(torch.argmax(ref[r])), r


@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("M,N", [(8, 16400), (1, 1040), (16, 8192), (5, 1040)])
def test_q8_lm_head_grid_stride_bit_exact(lib, dev, M, N, rs):
    """The grid-stride two-stage Q8_0 lm_head writes the same {max, id} partials, bit for bit, as
    the one-tile blocks: 1025 tiles over 512 blocks (unequal walks), 512 tiles (one each), 65 tiles
    (fewer than blocks), with and without a row scale."""
    K = 3072
    b, wbf, pk, W = _packed(lib, dev, N, K, 11 + M)
    g = torch.Generator(device="cpu").manual_seed(N + M)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    ssq = (torch.rand(M, generator=g) * K + 1.0).to(dev)
    outs = []
    try:
        for gs in (1, 0):
            L.check(lib.ms_set_qgemv_gs(gs))
            part = torch.full((M, N // 16, 2), float("nan"), device=dev)
            if rs:
                L.check(lib.ms_op_set_row_scale(ssq.data_ptr(), 1, K, 1e-5))
            try:
                L.check(lib.ms_op_qgemv(X.data_ptr(), Q8, pk.data_ptr(), part.data_ptr(), M, N, K, N // 16,
                                        L.MS_EPI_ARGMAX, _stream()))
            finally:
                if rs:
                    L.check(lib.ms_op_set_row_scale(None, 0, 0, 0.0))
            torch.cuda.synchronize()
            outs.append(part.cpu())
    finally:
        L.check(lib.ms_set_qgemv_gs(1))
    assert not torch.isnan(outs[0]).any() and not torch.isnan(outs[1]).any()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    # and they are the product's maxima: tile 0 of row 0 against fp64
    ref = (X[0].double().cpu() @ W[:16].T)
    assert abs(float(outs[0][0, 0, 0]) - float(ref.max())) <= 1e-4 * (abs(float(ref.max())) + 1.0)


@pytest.mark.parametrize("M", [1, 8, 16, 33, 40, 64])
@pytest.mark.parametrize("N,K,S", [(256, 3072, 6), (512, 3072, 4), (128, 8192, 4), (256, 8192, 2),
                                   (64, 768, 3)])
def test_qgemv_split_slabs_vs_fp64(lib, dev, M, N, K, S):
    """Split-K: slab s is the dequantised partial product over its K range; the slabs add up to
    the full product; S = 5 is refused (the K-quant test's shapes, M = 40 at K / S = 2048
    included)."""
    b, wbf, pk, Wd = _packed(lib, dev, N, K, 11 + M + S)
    g = torch.Generator(device="cpu").manual_seed(M + N + K + S)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    slabs = torch.full((S, M, N), float("nan"), device=dev)
    L.check(lib.ms_op_qgemv_split(X.data_ptr(), Q8, pk.data_ptr(), slabs.data_ptr(), M, N, K, S, _stream()))
    torch.cuda.synchronize()
    Xd, ks = X.double().cpu(), K // S
    for s_ in range(S):
        exp = Xd[:, s_ * ks:(s_ + 1) * ks] @ Wd[:, s_ * ks:(s_ + 1) * ks].T
        assert rel(slabs[s_].double().cpu(), exp) < 1e-5, s_
    assert rel(slabs.double().sum(0).cpu(), Xd @ Wd.T) < 1e-5
    assert lib.ms_op_qgemv_split(X.data_ptr(), Q8, pk.data_ptr(), slabs.data_ptr(), M, N, K, 5, _stream()) != 0


def test_qdgemm_refuses_q8_0(lib, dev):
    """The large-batch skinny GEMM has no packed Q8_0 form: MS_EINVAL with a message."""
    b, wbf, pk, W = _packed(lib, dev, 64, 768, 3)
    X = torch.zeros(128, 768, dtype=torch.float16, device=dev)
    out = torch.zeros(128, 64, dtype=torch.float32, device=dev)
    rc = lib.ms_op_qdgemm(X.data_ptr(), Q8, pk.data_ptr(), out.data_ptr(), 128, 64, 768, 1, 64, L.MS_EPI_STORE_F32,
                          _stream())
    assert rc == L.MS_EINVAL
    assert "Q8_0" in _last_error(lib)


# ------------------------------------------------------------------ engine
NAMES = ("wq", "wk", "wv", "wo", "w_gate", "w_up", "w_down")


@pytest.fixture(scope="module")
def model():
    """make_weights(TINY, 1234, 0.05, 0.1) quantised by the reference quantiser; the oracle runs
    on f16_rne(dequant), the engine's prefill weights."""
    base = make_weights(TINY, 1234, std=0.05, jitter=0.1)
    qw, w = {}, {"final_norm": base["final_norm"], "layers": []}
    eb = R.quantize_q8_0(base["embed"])
    qw["embed"] = (Q8, eb.reshape(-1))
    w["embed"] = f16_rne(R.dequant_q8_0(eb)).reshape(base["embed"].shape)
    w["lm_head"] = w["embed"]
    for l, ly in enumerate(base["layers"]):
        o = {"attn_norm": ly["attn_norm"], "ffn_norm": ly["ffn_norm"]}
        for n in NAMES:
            blk = R.quantize_q8_0(ly[n])
            qw[(l, n)] = (Q8, blk.reshape(-1))
            o[n] = f16_rne(R.dequant_q8_0(blk)).reshape(ly[n].shape)
        w["layers"].append(o)
    prompts = [_prompt(n, 700 + n) for n in (17, 140, 301, 64)]
    return qw, w, OracleLlama(TINY, w), prompts


def _check_vs_oracle(oracle, prompts, res):
    agree = total = 0
    for p, r in zip(prompts, res):
        assert len(r.ids) == 48
        a, flips = _teacher_forced_agreement(oracle, p, r.ids)
        agree += a
        total += len(r.ids)
        for pos, gap, top in flips:  # only at a near-tie of the oracle's own logits
            assert gap <= 1e-2 * (abs(top) + 1.0), (pos, gap, top)
    print(f"teacher-forced agreement {agree}/{total}")
    assert agree / total >= 0.97, (agree, total)


@pytest.fixture(scope="module")
def run4(dev, model):
    """The 4-slot engine (residual-fused Q-GEMV regime): ids in the batch, one prompt alone, the
    prefill logits of one prompt."""
    qw, w, oracle, prompts = model
    with Engine(TINY, device=0, max_batch=4, max_ctx=512, max_prefill_tokens=2048) as e:
        load_quantized(e, qw, w)
        res = e.generate(prompts, num_predict=48, ignore_eos=True)
        alone = e.generate(prompts[2:3], num_predict=48, ignore_eos=True)[0]
        _, lg = e.forward(prompts[1], hidden=False, logits=True)
        manifest = e.quant_manifest()
    return res, alone, lg, manifest


def test_engine_4_slots_vs_oracle(model, run4):
    qw, w, oracle, prompts = model
    res, alone, lg, manifest = run4
    ref_lg, _ = oracle.forward(prompts[1], all_logits=True)
    err = rel(lg, ref_lg)
    print(f"prefill logits rel err {err:.3e}")
    assert err < 2e-2
    _check_vs_oracle(oracle, prompts, res)
    assert alone.ids == res[2].ids, "a prompt alone yields the ids it yields in the batch"
    assert len(manifest) == 7 * TINY.n_layers + 1 and all(ty == Q8 for _, _, ty in manifest)


@pytest.mark.parametrize("nb", [20, 72])
def test_engine_other_regimes_vs_oracle(dev, model, nb):
    """20 slots: split Q-GEMV + residual_rmsnorm (MT = 2 tiles); 72 slots: the fp16 copies on the
    large-regime kernels (qd() stays false for Q8_0)."""
    qw, w, oracle, prompts = model
    with Engine(TINY, device=0, max_batch=nb, max_ctx=512, max_prefill_tokens=2048) as e:
        load_quantized(e, qw, w)
        res = e.generate(prompts, num_predict=48, ignore_eos=True)
        _, lg = e.forward(prompts[1], hidden=False, logits=True)
    ref_lg, _ = oracle.forward(prompts[1], all_logits=True)
    assert rel(lg, ref_lg) < 2e-2
    _check_vs_oracle(oracle, prompts, res)


def test_engine_from_q8_0_gguf(dev, model, run4, tmp_path):
    """A Q8_0 GGUF (permuted Q/K rows) loads through mapsum.gguf and reproduces the ids of the
    engine loaded from the blocks directly."""
    qw, w, oracle, prompts = model
    mats = {k: v[1].reshape(SHAPES[k[1]][0], -1) for k, v in qw.items() if k != "embed"}
    path = str(tmp_path / "tiny-q8_0.gguf")
    write_q8_gguf(path, qw["embed"][1].reshape(TINY.vocab, -1), mats, w)
    with Engine(TINY, device=0, max_batch=4, max_ctx=512, max_prefill_tokens=2048) as e:
        gguf.load_gguf(e, path)
        res = e.generate(prompts, num_predict=48, ignore_eos=True)
    assert [r.ids for r in res] == [r.ids for r in run4[0]]


def test_weight_regions_broadcast(dev, model, run4):
    """An engine that only declared the Q8_0 layout and received every weight region by device copy
    generates the same ids (what the RCCL weight broadcast moves)."""
    from mapsum.dist import region_views
    qw, w, oracle, prompts = model
    a = Engine(TINY, device=0, max_batch=4, max_ctx=512, max_prefill_tokens=2048)
    b = Engine(TINY, device=0, max_batch=4, max_ctx=512, max_prefill_tokens=2048)
    try:
        load_quantized(a, qw, w)
        man = a.quant_manifest()
        assert len(man) == 7 * TINY.n_layers + 1 and all(ty == Q8 for _, _, ty in man)
        for t, l, ty in man:
            b.declare_weight_q(t, l, ty)
        va, vb = region_views(a), region_views(b)
        assert [v.numel() for v in va] == [v.numel() for v in vb]
        for x, y in zip(va, vb):
            y.copy_(x)
        torch.cuda.synchronize()
        rb = b.generate(prompts, num_predict=48, ignore_eos=True)
        assert [r.ids for r in rb] == [r.ids for r in run4[0]]
    finally:
        a.close()
        b.close()


def test_quant_families_do_not_mix(lib, dev):
    H = TINY.hidden
    q8 = R.random_blocks_q8_0(H * H // 32, seed=1, scale=0.05).reshape(-1)
    q4 = Q.random_blocks(Q.GGML_TYPE_Q4_K, H * H // 256, seed=1).reshape(-1)
    for first, second in (((Q8, q8), (Q.GGML_TYPE_Q4_K, q4)), ((Q.GGML_TYPE_Q4_K, q4), (Q8, q8))):
        with Engine(TINY, device=0, max_batch=2, max_ctx=256, max_prefill_tokens=256) as e:
            e.load_tensor_q(L.MS_T_WO, 0, first[0], first[1])
            rc = lib.ms_load_weight_q(e.h, L.MS_T_WO, 1, second[0], second[1].ctypes.data, second[1].size)
            assert rc == L.MS_EINVAL
            msg = _last_error(lib, e.h)
            assert "Q8_0" in msg and "Q4_K" in msg, msg
            assert lib.ms_declare_weight_q(e.h, L.MS_T_WO, 1, second[0]) == L.MS_EINVAL
            e.load_tensor_q(L.MS_T_WO, 1, first[0], first[1])  # the engine's own family still loads


def test_synthetic_q8_0(dev):
    """init_synthetic_q8_0 then generate: length finishes only; through the fp16 copies (the
    rounded dequantised weights) every weight is finite with std within [0.5, 2] x scale."""
    from mapsum.dist import region_views
    scale = 0.05
    with Engine(TINY, device=0, max_batch=4, max_ctx=256, max_prefill_tokens=1024) as e:
        e.init_synthetic_q8_0(seed=9, scale=scale, norm_jitter=0.1)
        res = e.generate([_prompt(n, 60 + n) for n in (5, 77, 130)], num_predict=12, ignore_eos=True)
        assert all(r.finish == "length" and len(r.ids) == 12 for r in res)
        man = e.quant_manifest()
        assert len(man) == 7 * TINY.n_layers + 1 and all(ty == Q8 for _, _, ty in man)
        views = region_views(e)
        # ms_weight_regions' order (tied embedding): embed, final_norm, then per layer attn_norm,
        # ffn_norm, wqkv, wo, wgu, wdown -- the fp16 copies of the matrices
        idx = [0] + [2 + 6 * l + j for l in range(TINY.n_layers) for j in (2, 3, 4, 5)]
        for i in idx:
            wts = views[i].view(torch.float16).float()
            assert torch.isfinite(wts).all(), i
            std = float(wts.std())
            assert 0.5 * scale <= std <= 2 * scale, (i, std)
