"""Q5_K weights on the GPU (needs one): the dequantiser, the fp16 copy and the packed layout, the
dequant-fused GEMV with every op-level epilogue, split-K, the residual epilogue, the packed-row
skinny GEMM, and Q5_K_M / Q4_K_S-style engines end to end in each decode regime -- against
tests/q5_k_ref.py and the CPU oracle.

The GEMV reference is fp64 of X . dequant(W)^T on the exact fp32 weights d1 * q - m1: the kernel
feeds the 5-bit codes to the fp16 MFMA as the subnormals q * 2^-24 and applies d1 and m1 in fp32
(Q4_K's form), so the bars are Q4_K's (test_gpu_parity._qtol: 1e-5 on fp32 outputs, 4e-3 on fp16
ones)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import q5_k_ref as R  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from mapsum import gguf  # noqa: E402
from mapsum.config import TINY  # noqa: E402
from mapsum.engine import Engine  # noqa: E402
from mapsum.weights import load_quantized  # noqa: E402
from oracle import quants as Q  # noqa: E402
from oracle.llama_ref import OracleLlama  # noqa: E402
from oracle.synth import f16_rne  # noqa: E402
from test_gpu_parity import XG_SCALE, _qtol, _stream, rel  # noqa: E402
from test_gpu_q8_0 import _check_vs_oracle  # noqa: E402
from test_q5_k_ref import MIXES, prompts, quant_model, write_kq_gguf  # noqa: E402

Q5 = L.MS_GGML_Q5_K
BLK = 176  # raw and packed bytes per 256 weights
TOL32 = _qtol(Q.GGML_TYPE_Q4_K)  # 1e-5: the subnormal-code MFMA form's bar


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
    """777 blocks, the hand-built ones first (q = t & 31 under rising scales, sc = m = 63 in
    sub-blocks 4-7, d = 0, negative d, the smallest subnormal d, every field at its maximum)."""
    b = R.random_blocks_q5_k(777, seed=5)
    kat = R.kat_blocks()
    b[:kat.shape[0]] = kat
    want = R.dequant_q5_k(b)
    bd = torch.from_numpy(b.reshape(-1)).to(dev)
    out = torch.empty(want.size, dtype=torch.float32, device=dev)
    L.check(lib.ms_op_dequant(Q5, bd.data_ptr(), 777, out.data_ptr(), _stream()))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "dequant must be bit-exact"


_PK = {}


def _packed(lib, dev, rows, K, seed, scale=1.0):
    """(raw blocks, fp16 copy, packed rows, fp64 exact weights) of seeded random blocks."""
    key = (rows, K, seed, scale)
    if key not in _PK:
        _PK.clear()
        b = R.random_blocks_q5_k(rows * K // 256, seed=seed, scale=scale)
        bd = torch.from_numpy(b.reshape(-1)).to(dev)
        wbf = torch.empty(rows, K, dtype=torch.float16, device=dev)
        pk = torch.empty(rows * (K // 256) * BLK, dtype=torch.uint8, device=dev)
        L.check(lib.ms_op_quant_rows(Q5, bd.data_ptr(), rows, K, wbf.data_ptr(), pk.data_ptr(), _stream()))
        torch.cuda.synchronize()
        W = torch.from_numpy(R.dequant_q5_k(b).reshape(rows, K)).double()
        _PK[key] = (b, wbf, pk, W)
    return _PK[key]


def test_quant_rows_f16_copy_and_packed_layout(lib, dev):
    b, wbf, pk, W = _packed(lib, dev, 48, 768, 6)
    assert np.array_equal(wbf.float().cpu().numpy(), f16_rne(W.float().numpy()))
    # the packed block: the header, byte 16 + 64 (s >> 2) + 16 g + 4 (s & 3) + i = nib(k) | nib(k + 4)
    # << 4 for k = 32 s + 8 g + i (Q4_K's packed order), then qh in its raw order at 144
    raw = b.reshape(48 * 3, BLK)
    nib = R.codes(raw) & 0xF                                   # [n][256] in weight order
    nb = nib.reshape(-1, 2, 4, 4, 2, 4)                        # [s >> 2][s & 3][g][half][i]
    byte = (nb[:, :, :, :, 0, :] | (nb[:, :, :, :, 1, :] << 4)).astype(np.uint8)  # [s >> 2][s & 3][g][i]
    want = np.empty((48 * 3, BLK), np.uint8)
    want[:, :16] = raw[:, :16]
    want[:, 16:144] = byte.transpose(0, 1, 3, 2, 4).reshape(-1, 128)             # [s >> 2][g][s & 3][i]
    want[:, 144:] = raw[:, 16:48]
    assert np.array_equal(pk.cpu().numpy().reshape(-1, BLK), want)


_MAXERR = {}

_GEMV_SHAPES = [(16, 256, L.MS_EPI_STORE_F32), (256, 768, L.MS_EPI_STORE_F16), (512, 2048, L.MS_EPI_ADD_F32),
                (1024, 768, L.MS_EPI_SWIGLU), (128, 8192, L.MS_EPI_STORE_F32)]


@pytest.mark.parametrize("M", [1, 8, 16, 33, 64])
@pytest.mark.parametrize("N,K,epi,rs", [c + (False,) for c in _GEMV_SHAPES] +
                         [c + (True,) for c in _GEMV_SHAPES if c[2] != L.MS_EPI_ADD_F32])
def test_qgemv_vs_fp64(lib, dev, M, N, K, epi, rs):
    """sum_s (2^24 d1_s) A_s - m1_s X_s against fp64 of X . dequant(W)^T: one tile and one block
    (16 x 256, X in registers), 3 blocks, 8 blocks on 8 waves, the two-blocks-per-wave form
    (K = 8192), MT 1-4 with a ragged last tile (33), with and without the rows' deferred-norm scale
    where the epilogue takes one (ADD_F32 takes none).  Measured maxima on the MI355X
    (profiles/q5_k/test_gpu_q5_k.log): fp32 outputs 2.22e-6 (bar 1e-5), fp16 outputs 2.21e-4 (bar
    4e-3)."""
    b, wbf, pk, W = _packed(lib, dev, N, K, 7 + N % 5)
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    # sums of squares of rows of rms 16 .. 32 (the engine's xb is pre-scaled by 2^-4): factors
    # 0.5 .. 1, so the fp16 outputs stay in range
    ssq = ((torch.rand(M, generator=g) * 3.0 + 1.0) * K * 256.0).to(dev)
    ref = X.double().cpu() @ W.T
    if rs:  # rows scaled by 16 / sqrt(ssq / K + eps) (kernels.h RowScale)
        ref = ref * (16.0 / torch.sqrt(ssq.double().cpu() / K + 1e-5))[:, None]
    f32 = epi in (L.MS_EPI_STORE_F32, L.MS_EPI_ADD_F32)
    tol = TOL32 if f32 else 4e-3
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
        L.check(lib.ms_op_qgemv(X.data_ptr(), Q5, pk.data_ptr(), out.data_ptr(), M, N, K, ldo, epi, _stream()))
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
    b, wbf, pk, W = _packed(lib, dev, N, K, 5)
    g = torch.Generator(device="cpu").manual_seed(3 * M + N + K)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    ref = X.double().cpu() @ W.T
    part = torch.full((M, N // 16, 2), float("nan"), device=dev)
    ids = torch.empty(M, dtype=torch.int32, device=dev)
    L.check(lib.ms_op_qgemv(X.data_ptr(), Q5, pk.data_ptr(), part.data_ptr(), M, N, K, N // 16,
                            L.MS_EPI_ARGMAX, _stream()))
    L.check(lib.ms_op_argmax_partials(part.data_ptr(), M, N // 16, ids.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert not torch.isnan(part).any(), "every 16-column tile writes its partial"
    srt = torch.sort(ref, 1).values
    got = ids.cpu().long()
    for r in range(M):
        if srt[r, -1] - srt[r, -2] > 1e-4 * (abs(float(srt[r, -1])) + 1.0):
            assert int(got[r]) == int(torch.argmax(ref[r])), r


@pytest.mark.parametrize("M", [8, 40])
@pytest.mark.parametrize("N,K,S", [(256, 3072, 6), (512, 3072, 4), (128, 8192, 4)])
def test_qgemv_split_slabs_vs_fp64(lib, dev, M, N, K, S):
    """Split-K: slab s is the dequantised partial product over its K range; the slabs add up to the
    full product; S = 5 is refused.  M = 40 at K / S = 2048 takes the global-X path."""
    b, wbf, pk, Wd = _packed(lib, dev, N, K, 11 + S)
    g = torch.Generator(device="cpu").manual_seed(M + N + K + S)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    slabs = torch.full((S, M, N), float("nan"), device=dev)
    L.check(lib.ms_op_qgemv_split(X.data_ptr(), Q5, pk.data_ptr(), slabs.data_ptr(), M, N, K, S, _stream()))
    torch.cuda.synchronize()
    Xd, ks = X.double().cpu(), K // S
    for s_ in range(S):
        exp = Xd[:, s_ * ks:(s_ + 1) * ks] @ Wd[:, s_ * ks:(s_ + 1) * ks].T
        assert rel(slabs[s_].double().cpu(), exp) < TOL32, s_
    assert rel(slabs.double().sum(0).cpu(), Xd @ Wd.T) < TOL32
    assert lib.ms_op_qgemv_split(X.data_ptr(), Q5, pk.data_ptr(), slabs.data_ptr(), M, N, K, 5, _stream()) != 0


@pytest.mark.parametrize("M,rt", [(1, 12), (8, 12), (13, 16)])
def test_qgemv_resid_epilogue(lib, dev, M, rt):
    """Decode O / down of a <= 16-slot engine with the residual update fused (ms_op_qgemv_resid,
    test_gpu_parity.test_gemv_resid_epilogue's checks on Q5_K rows): x += X . W^T on rt-row tiles
    (12-row tiles: lanes 12-15 load the tile's last row again, never stored), xg = f16(x * gamma *
    2^-4) from the stored x exactly, per-tile sums of the new x^2.  Measured: x within 1.2e-6 of
    fp64 (bar 1e-5)."""
    g = torch.Generator(device="cpu").manual_seed(M * 100 + rt)
    N, K = 3072, 3072
    b, wbf, pk, W = _packed(lib, dev, N, K, 21, scale=0.03)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    x = (torch.randn(M, N, generator=g) * 2).to(dev)
    gamma = (1 + 0.1 * torch.randn(N, generator=g)).to(torch.float16).to(dev)
    x_ref = x.double().cpu() + X.double().cpu() @ W.T
    xg = torch.empty(M, N, dtype=torch.float16, device=dev)
    tiles = N // rt
    ssq = torch.full((tiles, M), float("nan"), device=dev)
    L.check(lib.ms_op_qgemv_resid(X.data_ptr(), Q5, pk.data_ptr(), x.data_ptr(), xg.data_ptr(), gamma.data_ptr(),
                                  ssq.data_ptr(), M, N, K, rt, _stream()))
    torch.cuda.synchronize()
    err = rel(x.double().cpu(), x_ref)
    print(f"M {M} rt {rt}: residual rel err {err:.3e}")
    assert err < TOL32
    want = (x * gamma.float() * XG_SCALE).to(torch.float16)  # from the stored x exactly
    assert torch.equal(xg, want)
    assert not torch.isnan(ssq).any()
    for t in (0, tiles // 2, tiles - 1):
        exp = (x[:, t * rt:(t + 1) * rt].double() ** 2).sum(-1).cpu()
        assert rel(ssq[t].double().cpu(), exp) < 1e-6, t


@pytest.mark.parametrize("N,K,epi", [(256, 768, L.MS_EPI_STORE_F32), (128, 8192, L.MS_EPI_STORE_F32),
                                     (1024, 768, L.MS_EPI_SWIGLU)])
def test_qgemv_rows_independent_of_batch(lib, dev, N, K, epi):
    """Row r of an M = 64 launch equals the same row launched alone, bitwise (rows 0, 17, 63: one
    per m-tile position that matters -- first, inside, last)."""
    b, wbf, pk, W = _packed(lib, dev, N, K, 7 + N % 5)
    g = torch.Generator(device="cpu").manual_seed(N + K)
    X = torch.randn(64, K, generator=g).to(torch.float16).to(dev)
    ncol, dt = (N // 2, torch.float16) if epi == L.MS_EPI_SWIGLU else (N, torch.float32)
    full = torch.zeros(64, ncol, dtype=dt, device=dev)
    L.check(lib.ms_op_qgemv(X.data_ptr(), Q5, pk.data_ptr(), full.data_ptr(), 64, N, K, ncol, epi, _stream()))
    for r in (0, 17, 63):
        one = torch.zeros(1, ncol, dtype=dt, device=dev)
        xr = X[r:r + 1].contiguous()
        L.check(lib.ms_op_qgemv(xr.data_ptr(), Q5, pk.data_ptr(), one.data_ptr(), 1, N, K, ncol, epi, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(one[0].cpu(), full[r].cpu()), r


# ------------------------------------------------------------------ the packed-row skinny GEMM
QD_SHAPES = [(1024, 768, 1, L.MS_EPI_STORE_F32), (5120, 3072, 6, L.MS_EPI_STORE_F32),
             (3072, 8192, 8, L.MS_EPI_STORE_F32), (4096, 3072, 1, L.MS_EPI_ARGMAX), (2048, 768, 1, L.MS_EPI_SWIGLU)]


@pytest.mark.parametrize("M", [1, 17, 128, 256])
@pytest.mark.parametrize("N,K,S,epi", QD_SHAPES)
def test_qdgemm_bit_identical_to_fp16_rows(lib, dev, M, N, K, S, epi):
    """ms_op_qdgemm on packed Q5_K rows dequantises each weight to the fp16 copy's value
    (fma(d1, q, -m1) rounded to fp16) and its MFMA order depends only on (K, S): the result is
    bit-identical to the same call on the fp16 copy (type 1).  W fetch rings of 4, 3 and 2
    super-blocks (K / S / 256 = 12 and 4, 3, 2)."""
    b, wbf, pk, W = _packed(lib, dev, N, K, 31, scale=0.02)
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N + K + S + epi)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    ncol = N // 2 if epi == L.MS_EPI_SWIGLU else (N // 16 if epi == L.MS_EPI_ARGMAX else N)
    dt = torch.float16 if epi == L.MS_EPI_SWIGLU else torch.float32
    width = ncol * (2 if epi == L.MS_EPI_ARGMAX else 1)
    outs = []
    for ty, rows in ((Q5, pk), (1, wbf)):
        o = torch.full((S, M, width), float("nan"), dtype=dt, device=dev)
        L.check(lib.ms_op_qdgemm(X.data_ptr(), ty, rows.data_ptr(), o.data_ptr(), M, N, K, S, ncol, epi, _stream()))
        torch.cuda.synchronize()
        outs.append(o.cpu())
    assert not torch.isnan(outs[0].float()).any()
    it = torch.int16 if dt == torch.float16 else torch.int32
    assert torch.equal(outs[0].view(it), outs[1].view(it))
    if epi == L.MS_EPI_STORE_F32:  # and it is the product: slab 0 against fp64 of the fp16 copy
        ks = K // S
        exp = X.double().cpu()[:, :ks] @ wbf.double().cpu()[:, :ks].T
        assert rel(outs[0][0].double(), exp) < 2e-6


def test_qdgemm_refuses_bad_shapes(lib, dev):
    b, wbf, pk, W = _packed(lib, dev, 1024, 768, 31, scale=0.02)
    X = torch.zeros(8, 768, dtype=torch.float16, device=dev)
    out = torch.zeros(4, 8, 1024, device=dev)
    for M, N, K, S, epi in ((257, 1024, 768, 1, L.MS_EPI_STORE_F32), (8, 1000, 768, 1, L.MS_EPI_STORE_F32),
                            (8, 1024, 768, 2, L.MS_EPI_STORE_F32), (8, 1024, 768, 3, L.MS_EPI_SWIGLU),
                            (8, 1024, 768, 3, L.MS_EPI_STORE_F32), (8, 1024, 768, 1, L.MS_EPI_STORE_F16)):
        assert lib.ms_op_qdgemm(X.data_ptr(), Q5, pk.data_ptr(), out.data_ptr(), M, N, K, S, N, epi,
                                _stream()) == L.MS_EINVAL


# ------------------------------------------------------------------ engines
@pytest.fixture(scope="module", params=list(MIXES))
def model(request):
    """make_weights(TINY, 1234, 0.05, 0.1) quantised by the reference quantisers in the Q5_K_M mix
    (QKV: Q5_K x 3 in layer 0, Q5_K, Q5_K, Q6_K in layer 1) or the Q4_K_S-style one (QKV of layer 0:
    Q4_K, Q4_K, Q5_K); the oracle runs on f16_rne(dequant), the engine's prefill weights.

    The oracle's own greedy runs over these prompts have near-ties (top-2 gap <= 1e-2 (|top| + 1))
    at 9 (Q5_K_M) and 11 (Q4_K_S) of the 4 x 48 positions (test_q5_k_ref.py counts them) -- the random tiny model's logits are
    flat, and no prompt seed of 110 scanned per length came near 3 %.  The 0.97 bar therefore is not
    slack the near-tie excuse can fill: of the 9 to 11 excusable positions at most 5 may differ."""
    qw, w, types = quant_model(request.param)
    return request.param, qw, w, types, OracleLlama(TINY, w), prompts()


def _engine(nb):
    return Engine(TINY, device=0, max_batch=nb, max_ctx=512, max_prefill_tokens=2048)


@pytest.fixture(scope="module")
def run4(dev, model):
    """The 4-slot engine (residual-fused Q-GEMV regime): ids in the batch, one prompt alone, the
    prefill logits of one prompt, the manifest."""
    mix, qw, w, types, oracle, ps = model
    with _engine(4) as e:
        load_quantized(e, qw, w)
        res = e.generate(ps, num_predict=48, ignore_eos=True)
        alone = e.generate(ps[2:3], num_predict=48, ignore_eos=True)[0]
        _, lg = e.forward(ps[1], hidden=False, logits=True)
        manifest = e.quant_manifest()
    return res, alone, lg, manifest


_TENSOR = {"wq": L.MS_T_WQ, "wk": L.MS_T_WK, "wv": L.MS_T_WV, "wo": L.MS_T_WO, "w_gate": L.MS_T_WGATE,
           "w_up": L.MS_T_WUP, "w_down": L.MS_T_WDOWN}


def test_engine_4_slots_vs_oracle(model, run4):
    mix, qw, w, types, oracle, ps = model
    res, alone, lg, manifest = run4
    ref_lg, _ = oracle.forward(ps[1], all_logits=True)
    err = rel(lg, ref_lg)
    print(f"{mix}: prefill logits rel err {err:.3e}")
    assert err < 2e-2
    _check_vs_oracle(oracle, ps, res)
    assert alone.ids == res[2].ids, "a prompt alone yields the ids it yields in the batch"
    got = {(t, l): ty for t, l, ty in manifest}
    want = {(_TENSOR[k[1]], k[0]): ty for k, ty in types.items() if k != "embed"}
    want[(L.MS_T_EMBED, 0)] = types["embed"]
    assert got == want
    assert sum(ty == Q5 for ty in got.values()) == (12 if mix == "q5_k_m" else 2)


@pytest.mark.parametrize("nb", [20, 72])
def test_engine_other_regimes_vs_oracle(dev, model, nb):
    """20 slots: split Q-GEMV + residual_rmsnorm (MT = 2 tiles); 72 slots: the large regime (all-Q4_K
    and all-Q5_K matrices on the packed-row skinny GEMM, Q6_K and mixed ones on their fp16
    copies)."""
    mix, qw, w, types, oracle, ps = model
    with _engine(nb) as e:
        load_quantized(e, qw, w)
        res = e.generate(ps, num_predict=48, ignore_eos=True)
        _, lg = e.forward(ps[1], hidden=False, logits=True)
    ref_lg, _ = oracle.forward(ps[1], all_logits=True)
    assert rel(lg, ref_lg) < 2e-2
    _check_vs_oracle(oracle, ps, res)


def test_engine_72_slots_on_fp16_copies(dev, model, monkeypatch):
    """MS_QDGEMM=3 takes the all-Q5_K matrices of a >= 65-slot engine off the packed-row skinny GEMM
    (their fp16 copies through the fp16 kernels, the A/B's other side): the same bars."""
    mix, qw, w, types, oracle, ps = model
    monkeypatch.setenv("MS_QDGEMM", "3")
    with _engine(72) as e:
        load_quantized(e, qw, w)
        res = e.generate(ps, num_predict=48, ignore_eos=True)
    _check_vs_oracle(oracle, ps, res)


def test_engine_from_gguf(dev, model, run4, tmp_path):
    """The mix as a GGUF (permuted Q/K rows, tied Q6_K token_embd) loads through mapsum.gguf and
    reproduces the ids of the engine loaded from the blocks directly."""
    mix, qw, w, types, oracle, ps = model
    path = str(tmp_path / f"tiny-{mix}.gguf")
    write_kq_gguf(path, qw, w)
    with _engine(4) as e:
        gguf.load_gguf(e, path)
        res = e.generate(ps, num_predict=48, ignore_eos=True)
    assert [r.ids for r in res] == [r.ids for r in run4[0]]


def test_weight_regions_broadcast(dev, model, run4):
    """An engine that only declared the layout and received every weight region by device copy
    generates the same ids (what the RCCL weight broadcast moves)."""
    from mapsum.dist import region_views
    mix, qw, w, types, oracle, ps = model
    a, b = _engine(4), _engine(4)
    try:
        load_quantized(a, qw, w)
        man = a.quant_manifest()
        assert any(ty == Q5 for _, _, ty in man)
        for t, l, ty in man:
            b.declare_weight_q(t, l, ty)
        va, vb = region_views(a), region_views(b)
        assert [v.numel() for v in va] == [v.numel() for v in vb]
        for x, y in zip(va, vb):
            y.copy_(x)
        torch.cuda.synchronize()
        rb = b.generate(ps, num_predict=48, ignore_eos=True)
        assert [r.ids for r in rb] == [r.ids for r in run4[0]]
    finally:
        a.close()
        b.close()


def test_q8_0_after_q5_k_is_refused(lib, dev):
    import q8_0_ref
    H = TINY.hidden
    q5 = R.random_blocks_q5_k(H * H // 256, seed=1, scale=0.05).reshape(-1)
    q8 = q8_0_ref.random_blocks_q8_0(H * H // 32, seed=1, scale=0.05).reshape(-1)
    q4 = Q.random_blocks(Q.GGML_TYPE_Q4_K, H * H // 256, seed=1).reshape(-1)
    with Engine(TINY, device=0, max_batch=2, max_ctx=256, max_prefill_tokens=256) as e:
        e.load_tensor_q(L.MS_T_WO, 0, Q5, q5)
        rc = lib.ms_load_weight_q(e.h, L.MS_T_WO, 1, L.MS_GGML_Q8_0, q8.ctypes.data, q8.size)
        assert rc == L.MS_EINVAL
        msg = _last_error(lib, e.h)
        assert "Q8_0" in msg and "Q5_K" in msg, msg
        assert lib.ms_declare_weight_q(e.h, L.MS_T_WO, 1, L.MS_GGML_Q8_0) == L.MS_EINVAL
        e.load_tensor_q(L.MS_T_WO, 1, Q.GGML_TYPE_Q4_K, q4)  # the K-quant family still loads


def test_synthetic_q5_k_m(dev):
    """init_synthetic_q5_k_m then generate: length finishes only; the manifest is the Q5_K_M mix;
    through the fp16 copies (the rounded dequantised weights) every weight of a Q5_K matrix is
    finite with std within [0.5, 2] x scale."""
    from mapsum.dist import region_views
    scale = 0.05
    with Engine(TINY, device=0, max_batch=4, max_ctx=256, max_prefill_tokens=1024) as e:
        e.init_synthetic_q5_k_m(seed=9, scale=scale, norm_jitter=0.1)
        res = e.generate([np.random.default_rng(60 + n).integers(0, 4000, size=n).astype(np.int32) for n in (5, 77, 130)],
                         num_predict=12, ignore_eos=True)
        assert all(r.finish == "length" and len(r.ids) == 12 for r in res)
        man = {(t, l): ty for t, l, ty in e.quant_manifest()}
        assert len(man) == 7 * TINY.n_layers + 1
        for (name, t) in _TENSOR.items():
            for l in range(TINY.n_layers):
                assert man[(t, l)] == R.q5_k_m_type(name, l, TINY.n_layers), (name, l)
        assert man[(L.MS_T_EMBED, 0)] == 14
        views = region_views(e)
        # ms_weight_regions' order (tied embedding): embed, final_norm, then per layer attn_norm,
        # ffn_norm, wqkv, wo, wgu, wdown -- the fp16 copies; layer 0's four are all Q5_K, layer 1's
        # wo and wgu are
        for i in [2 + 6 * 0 + j for j in (2, 3, 4, 5)] + [2 + 6 * 1 + j for j in (3, 4)]:
            wts = views[i].view(torch.float16).float()
            assert torch.isfinite(wts).all(), i
            std = float(wts.std())
            print(f"region {i}: std {std:.4f}")
            assert 0.5 * scale <= std <= 2 * scale, (i, std)
