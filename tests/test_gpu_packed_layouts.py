"""The packed decode layouts of Q4_K, Q6_K and Q8_0 rows (csrc/qblock.h), byte for byte (needs a GPU):
ms_op_quant_rows on 48 rows x K = 768 of seeded CPU-generated raw blocks against a numpy restatement
of each layout.  (Q5_K's: test_gpu_q5_k.py::test_quant_rows_f16_copy_and_packed_layout.)  The
expectation is exact -- the kernel only moves bytes -- so there is no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import q8_0_ref as R8  # noqa: E402
from mapsum import _lib as L  # noqa: E402
from oracle import quants as Q  # noqa: E402
from test_gpu_parity import _stream  # noqa: E402

ROWS, K = 48, 768
NB = ROWS * K // 256


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _pack(dev, qtype, raw, packed_bytes):
    lib = L.load()
    bd = torch.from_numpy(raw.reshape(-1)).to(dev)
    wbf = torch.empty(ROWS, K, dtype=torch.float16, device=dev)
    pk = torch.full((NB * packed_bytes,), 0xA5, dtype=torch.uint8, device=dev)  # every byte must be written
    L.check(lib.ms_op_quant_rows(qtype, bd.data_ptr(), ROWS, K, wbf.data_ptr(), pk.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return pk.cpu().numpy().reshape(NB, packed_bytes)


def test_q4_k_packed_layout(dev):
    raw = Q.random_blocks(Q.GGML_TYPE_Q4_K, NB, seed=6)
    qs = raw[:, 16:144].reshape(NB, 4, 32)                    # weight 64 c + l: low nibble, + 32: high
    nib = np.stack([qs & 0xF, qs >> 4], axis=2).reshape(NB, 256)
    # byte 16 + 64 (s >> 2) + 16 g + 4 (s & 3) + i = nib(k) | nib(k + 4) << 4, k = 32 s + 8 g + i, i < 4
    nb = nib.reshape(NB, 2, 4, 4, 2, 4)                       # [s >> 2][s & 3][g][half][i]
    byte = (nb[:, :, :, :, 0, :] | (nb[:, :, :, :, 1, :] << 4)).astype(np.uint8)
    want = np.empty((NB, 144), np.uint8)
    want[:, :16] = raw[:, :16]                                # the ggml header as is
    want[:, 16:] = byte.transpose(0, 1, 3, 2, 4).reshape(NB, 128)  # [s >> 2][g][s & 3][i]
    assert np.array_equal(_pack(dev, Q.GGML_TYPE_Q4_K, raw, 144), want)


def test_q6_k_packed_layout(dev):
    raw = Q.random_blocks(Q.GGML_TYPE_Q6_K, NB, seed=7)
    # raw ql[64 hh + 32 half + 16 p + i] -> packed 64 half + 16 (2 hh + p) + i; qh, scales, d unmoved
    ql = raw[:, :128].reshape(NB, 2, 2, 2, 16)                # [hh][half][p][i]
    want = np.empty((NB, 224), np.uint8)
    want[:, :128] = ql.transpose(0, 2, 1, 3, 4).reshape(NB, 128)  # [half][hh][p][i]
    want[:, 128:210] = raw[:, 128:210]
    want[:, 210:] = 0                                         # the zeroed tail
    got = _pack(dev, Q.GGML_TYPE_Q6_K, raw, 224)
    assert np.array_equal(got[:, 210:], np.zeros((NB, 14), np.uint8))
    assert np.array_equal(got, want)


def test_q8_0_packed_layout(dev):
    raw = R8.random_blocks_q8_0(NB * 8, seed=8).reshape(NB, 8, 34)
    # the 8 scales, then byte 16 + 64 (s >> 1) + 16 g + 8 (s & 1) + i = q[32 s + 8 g + i], i < 8
    want = np.empty((NB, 272), np.uint8)
    want[:, :16] = raw[:, :, :2].reshape(NB, 16)
    q = raw[:, :, 2:].reshape(NB, 4, 2, 4, 8)                 # [s >> 1][s & 1][g][i]
    want[:, 16:] = q.transpose(0, 1, 3, 2, 4).reshape(NB, 256)    # [s >> 1][g][s & 1][i]
    assert np.array_equal(_pack(dev, L.MS_GGML_Q8_0, raw, 272), want)
