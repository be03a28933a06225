"""Line-exact weight loads of the fp16 decode GEMVs (k_gemv.hip, orders 3..8) give order 0's bits (needs a GPU).

Orders 0..2 load a weight step with an instruction pair in which lane (fr, fg) reads bytes
[32 fg, 32 fg + 16) and [32 fg + 16, 32 fg + 32) of row fr: both instructions touch all sixteen
128-byte lines of the tile.  The line-exact forms give instruction A the whole lines of rows 0-7
and instruction B those of rows 8-15 (lane (fr, fg) reads row fr & 7 [+ 8], 16-byte chunk
2 fg + (fr >> 3)) and swap one value per dword between lanes fr and fr ^ 8, after which every lane
holds the registers it held before.  Order = issue order (0 X first, 1 first weight step first,
2 per-wave X slices) + 3 x load form (0 pair, 1 line-exact, 2 line-exact non-temporal).  The MFMA
order and the epilogues are shared, so the bar is BIT IDENTITY with order 0, not a tolerance.

The shapes are the smallest that reach each edge of the mapping: M = 1, 8, 16; K = 512 (8 waves of
one step) and 3072 (16 waves of three steps); 12-row residual tiles (rows 8-11 live, 12-15 clamped:
all in instruction B), N = 36 and the ragged N = 40; N = 40 with the plain stores (the row clamp falls
inside rows 8-15 of the last tile) and N = 24 (instruction B of the last tile is clamped whole);
the two-tile SwiGLU block; split-K slabs; argmax partials.  A chunk routed to the wrong lane or
row changes the result: every (row, 16-byte chunk) of the weights is distinct, and one case uses
small integers, where the sums are exact in fp32 and the expected output comes from numpy alone.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from mapsum import _lib as L  # noqa: E402

KS = (512, 3072)
MS = (1, 8, 16)
NEW_ORDERS = (3, 4, 5, 6, 7, 8)


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
    X = torch.randn(M, K, generator=g).to(torch.float16)
    W = (torch.randn(N, K, generator=g) * 0.05).to(torch.float16)
    chunks = W.numpy().view(np.uint8).reshape(N * K // 8, 16)
    assert len(np.unique(chunks, axis=0)) == len(chunks), "every (row, 16-byte chunk) must be distinct"
    return g, X.to(dev), W.to(dev)


def _under_orders(lib, run):
    """run() -> tuple of output tensors under order 0 and every line-exact order; returns order 0's."""
    ref = None
    for o in (0,) + NEW_ORDERS:
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
    return ref


def _gemv(lib, dev, X, W, M, N, K, epi, rs=None):
    """One ms_op_gemv launch into a fresh output; rs = (ssq tensor, tiles) for the deferred norm."""
    if epi == L.MS_EPI_SWIGLU:
        shape, dt, ldo = (M, N // 2), torch.float16, N // 2
    elif epi == L.MS_EPI_ARGMAX:
        shape, dt, ldo = (M, N // 16, 2), torch.float32, N // 16
    elif epi == L.MS_EPI_STORE_F32:
        shape, dt, ldo = (M, N), torch.float32, N
    else:
        shape, dt, ldo = (M, N), torch.float16, N
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)
    out = torch.zeros(shape, dtype=dt, device=dev)
    if rs:
        L.check(lib.ms_op_set_row_scale(rs[0].data_ptr(), rs[1], K, 1e-5))
    try:
        L.check(lib.ms_op_gemv(X.data_ptr(), W.data_ptr(), out.data_ptr(), M, N, K, ldo, epi, ws.data_ptr(),
                               _stream()))
    finally:
        L.check(lib.ms_op_set_row_scale(None, 0, 0, 0.0))
    return out


@pytest.mark.parametrize("N", [36, 40])
def test_resid_12_row_tiles(lib, dev, N):
    """RESID_SSQ on 12-row tiles: x, xg and the statistics.  Rows 8-11 and the clamped lanes 12-15
    all come from instruction B; at N = 40 the last tile has 4 live rows and B is clamped whole."""
    rt, tiles = 12, (N + 11) // 12
    for K in KS:
        for M in MS:
            g, X, W = _operands(dev, M, N, K, 17 * K + M + N)
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
    ("f16_n40", 40, L.MS_EPI_STORE_F16, 0),      # the N clamp inside rows 8-15 of the last tile
    ("f16_n24", 24, L.MS_EPI_STORE_F16, 0),      # instruction B of the last tile clamped whole
    ("f16_n40_rs4", 40, L.MS_EPI_STORE_F16, 4),  # ... with the deferred norm folded under the stream
    ("swiglu", 64, L.MS_EPI_SWIGLU, 0),          # two-tile blocks (NT = 2), two of them
    ("swiglu_rs4", 64, L.MS_EPI_SWIGLU, 4),
    ("argmax", 48, L.MS_EPI_ARGMAX, 0),
])
def test_epilogues(lib, dev, case, N, epi, rs_tiles):
    for K in KS:
        for M in MS:
            g, X, W = _operands(dev, M, N, K, 19 * K + M + N)
            ssq = (torch.rand(max(rs_tiles, 1), M, generator=g) * K / max(rs_tiles, 1) + 1.0).to(dev)
            _under_orders(lib, lambda: (_gemv(lib, dev, X, W, M, N, K, epi, (ssq, rs_tiles) if rs_tiles else None),))


@pytest.mark.parametrize("rs_tiles", [0, 4])
def test_split_k_slabs(lib, dev, rs_tiles):
    """Split-K STORE_F32 slabs (the QKV projection's form), S = 2."""
    S, N = 2, 32
    for K in KS:
        for M in MS:
            g, X, W = _operands(dev, M, N, S * K, 23 * K + M)
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


@pytest.mark.parametrize("M", MS)
def test_integer_pattern_against_numpy(lib, dev, M):
    """N = 40, K = 512, fp32 store.  W[n][8 c .. 8 c + 7] = the integer 64 n + c - 1280 (distinct per
    (row, chunk), |w| <= 1280), X small integers in [-3, 3] that differ from chunk to chunk: every
    product and every partial sum is an integer below 2^21, exact in fp32 in any order, so the output
    must equal numpy's integer result, and a chunk taken from another row or column changes it."""
    N, K = 40, 512
    n, c = np.meshgrid(np.arange(N), np.arange(K // 8), indexing="ij")
    Wi = np.repeat(64 * n + c - 1280, 8, axis=1).astype(np.int64)
    Xi = np.random.default_rng(31 + M).integers(-3, 4, size=(M, K)).astype(np.int64)
    assert np.abs(Wi).max() <= 2048 and len(np.unique(Wi[:, ::8])) == N * K // 8
    expect = (Xi @ Wi.T).astype(np.float32)
    assert np.abs(Xi @ Wi.T).max() < 2 ** 24
    X = torch.from_numpy(Xi.astype(np.float16)).to(dev)
    W = torch.from_numpy(Wi.astype(np.float16)).to(dev)
    ref = _under_orders(lib, lambda: (_gemv(lib, dev, X, W, M, N, K, L.MS_EPI_STORE_F32),))
    assert np.array_equal(ref[0].cpu().numpy(), expect)
