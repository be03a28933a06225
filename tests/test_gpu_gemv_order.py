"""Issue orders of the fp16 decode GEMVs (k_gemv.hip, ms_set_gemv_order) give the same bits (needs a GPU).

Order 0 queues the statistics DMA, the residual prefetch and the X DMA ahead of the weight
stream; order 1 sends each wave's first weight step ahead of them; order 2 adds per-wave X
slices (each wave copies only its own k-slice into its own LDS region and passes no X barrier).
None of them touches the summation order -- per wave MFMAs in step order, then the waves in wave
order -- so the bar is BIT IDENTITY with order 0 on the same inputs, not a tolerance.

Shapes are the smallest that reach every code path: K = 192 / 512 / 576 (3 / 8 / 9 waves of one
step), 1280 (10 waves of two steps), 3072 and 8192 (16 waves of 3 and 8 steps); M = 1, 5, 8, 16 (row
clamps, a partly filled 8-row DMA piece, the full MFMA tile; at K = 8192 and M = 16 the image no
longer fits in LDS and X comes from global memory in every order).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mapsum import _lib as L  # noqa: E402
from mapsum.config import TINY  # noqa: E402
from mapsum.engine import Engine  # noqa: E402

KS = (192, 512, 576, 1280, 3072, 8192)
MS = (1, 5, 8, 16)
ORDERS = (0, 1, 2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    lib = L.load()
    yield lib
    lib.ms_set_gemv_order(L.GEMV_ORDER_DEFAULT)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _operands(dev, M, N, K, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn(M, K, generator=g).to(torch.float16).to(dev)
    W = (torch.randn(N, K, generator=g) * 0.05).to(torch.float16).to(dev)
    return g, X, W


def _under_orders(lib, run):
    """run() -> tuple of output tensors, under every order; all must equal order 0's bits."""
    ref = None
    for o in ORDERS:
        L.check(lib.ms_set_gemv_order(o))
        try:
            outs = run()
            torch.cuda.synchronize()
        finally:
            L.check(lib.ms_set_gemv_order(L.GEMV_ORDER_DEFAULT))
        if ref is None:
            ref = outs
            continue
        for i, (a, b) in enumerate(zip(ref, outs)):
            assert torch.equal(_bits(a), _bits(b)), f"order {o}: output {i} differs from order 0"


@pytest.mark.parametrize("N", [36, 40])
def test_resid_ssq_orders_bit_identical(lib, dev, N):
    """RESID_SSQ on 12-row tiles (O / down): x, xg and the statistics.  N = 40 leaves a ragged
    last tile.  (The residual epilogue needs >= 4 waves, so K starts at 512.)"""
    rt, tiles = 12, (N + 11) // 12
    for K in KS[1:]:
        for M in MS:
            g, X, W = _operands(dev, M, N, K, 7 * K + M)
            x0 = (torch.randn(M, N, generator=g) * 2).to(dev)
            gamma = (1 + 0.1 * torch.randn(N, generator=g)).to(torch.float16).to(dev)

            def run():
                x = x0.clone()
                xg = torch.zeros(M, N, dtype=torch.float16, device=dev)
                ssq = torch.zeros(tiles, M, device=dev)
                L.check(lib.ms_op_gemv_resid(X.data_ptr(), W.data_ptr(), x.data_ptr(), xg.data_ptr(),
                                             gamma.data_ptr(), ssq.data_ptr(), M, N, K, rt, _stream()))
                return x, xg, ssq

            _under_orders(lib, run)


@pytest.mark.parametrize("case,N,epi,rs_tiles", [
    ("swiglu", 64, L.MS_EPI_SWIGLU, 0),
    ("swiglu_rs4", 64, L.MS_EPI_SWIGLU, 4),
    ("argmax", 48, L.MS_EPI_ARGMAX, 0),
    ("f16_rs1", 32, L.MS_EPI_STORE_F16, 1),
    ("f16_rs4", 32, L.MS_EPI_STORE_F16, 4),
])
def test_epilogue_orders_bit_identical(lib, dev, case, N, epi, rs_tiles):
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    for K in KS:
        for M in MS:
            g, X, W = _operands(dev, M, N, K, 11 * K + M + N)
            ssq = (torch.rand(max(rs_tiles, 1), M, generator=g) * K / max(rs_tiles, 1) + 1.0).to(dev)
            if epi == L.MS_EPI_SWIGLU:
                shape, dt, ldo = (M, N // 2), torch.float16, N // 2
            elif epi == L.MS_EPI_ARGMAX:
                shape, dt, ldo = (M, N // 16, 2), torch.float32, N // 16
            else:
                shape, dt, ldo = (M, N), torch.float16, N

            def run():
                out = torch.zeros(shape, dtype=dt, device=dev)
                if rs_tiles:
                    L.check(lib.ms_op_set_row_scale(ssq.data_ptr(), rs_tiles, K, 1e-5))
                try:
                    L.check(lib.ms_op_gemv(X.data_ptr(), W.data_ptr(), out.data_ptr(), M, N, K, ldo, epi,
                                           ws.data_ptr(), _stream()))
                finally:
                    L.check(lib.ms_op_set_row_scale(None, 0, 0, 0.0))
                return (out,)

            _under_orders(lib, run)


@pytest.mark.parametrize("rs_tiles", [0, 4])
def test_split_k_orders_bit_identical(lib, dev, rs_tiles):
    """Split-K STORE_F32 slabs (the QKV projection's form), S = 2: each half of 2 K runs one of the
    K paths above."""
    S, N = 2, 32
    for K in KS:
        for M in MS:
            g, X, W = _operands(dev, M, N, S * K, 13 * K + M)
            ssq = (torch.rand(max(rs_tiles, 1), M, generator=g) * K + 1.0).to(dev)

            def run():
                slabs = torch.zeros(S, M, N, device=dev)
                if rs_tiles:
                    L.check(lib.ms_op_set_row_scale(ssq.data_ptr(), rs_tiles, S * K, 1e-5))
                try:
                    L.check(lib.ms_op_gemv_split(X.data_ptr(), W.data_ptr(), slabs.data_ptr(), M, N, S * K, S, 0,
                                                 _stream()))
                finally:
                    L.check(lib.ms_op_set_row_scale(None, 0, 0, 0.0))
                return (slabs,)

            _under_orders(lib, run)


def _engine_run(lib, order, slots):
    rng = np.random.default_rng(100 + slots)
    prompts = [rng.integers(0, 4000, size=int(n)).astype(np.int32) for n in rng.integers(20, 90, size=slots)]
    L.check(lib.ms_set_gemv_order(order))  # read when the engine captures its decode graphs
    try:
        e = Engine(TINY, device=0, max_batch=slots, max_ctx=256, max_prefill_tokens=1024)
        try:
            e.init_synthetic(1234, 0.05, 0.1)
            res = e.generate(prompts, num_predict=24, ignore_eos=True)
            x = e.debug_read(L.MS_DBG_DECODE_X, 0, slots * TINY.hidden * 4)
        finally:
            e.close()
    finally:
        L.check(lib.ms_set_gemv_order(L.GEMV_ORDER_DEFAULT))
    return [r.ids for r in res], x


@pytest.mark.parametrize("slots", [3, 8])
def test_engine_orders_same_ids_and_residual(lib, dev, slots):
    """The 2-layer toy engine, 24 greedy tokens: ids and the final residual under every order."""
    ids0, x0 = _engine_run(lib, 0, slots)
    assert all(len(i) == 24 for i in ids0)
    for o in ORDERS[1:]:
        ids, x = _engine_run(lib, o, slots)
        assert ids == ids0, f"order {o}: greedy ids differ"
        assert np.array_equal(x, x0), f"order {o}: final residual differs"
