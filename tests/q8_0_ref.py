"""numpy reference for ggml's Q8_0 (type 8): a block is {fp16 d; int8 qs[32]}, 34 bytes, and
y = d * q.  Restates ggml's published quantize_row_q8_0_ref / dequantize_row_q8_0; the engine
counts 256-weight units of 8 such blocks (272 bytes), which changes nothing in the raw bytes."""
import numpy as np

QK, BLOCK_BYTES, GGML_TYPE_Q8_0 = 32, 34, 8


def quantize_q8_0(x: np.ndarray) -> np.ndarray:
    """float32 values (size % 32 == 0) -> uint8 [n_blocks][34].  Per block: d = amax / 127 in
    fp32, id = d ? 1 / d : 0, q = roundf(x * id) (half away from zero), d stored as fp16."""
    v = np.ascontiguousarray(x, dtype=np.float32).reshape(-1, QK)
    amax = np.max(np.abs(v), axis=1)
    d = (amax / np.float32(127.0)).astype(np.float32)
    inv = np.zeros_like(d)
    np.divide(np.float32(1.0), d, out=inv, where=d != 0)
    y = (v * inv[:, None]).astype(np.float32)
    q = (np.sign(y) * np.floor(np.abs(y) + np.float32(0.5))).astype(np.int32)  # roundf
    assert q.min() >= -128 and q.max() <= 127
    out = np.empty((v.shape[0], BLOCK_BYTES), np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    out[:, 2:] = q.astype(np.int8).view(np.uint8)
    return out


def dequant_q8_0(blocks: np.ndarray) -> np.ndarray:
    """uint8 [n_blocks][34] (any shape of that size) -> float32 [n_blocks * 32]: float(d) * float(q),
    one fp32 multiply (exact: 11 x 8 significant bits)."""
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BLOCK_BYTES)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)  # [n][1]
    q = b[:, 2:].view(np.int8).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (d * q).astype(np.float32).reshape(-1)


def random_blocks_q8_0(n: int, seed: int, scale: float = 1.0) -> np.ndarray:
    """n random blocks: every int8 code occurs (-128 included), scales positive and negative,
    spread over [0.5, 1.5) * scale / 74 (uniform int8 has std 73.9: weights of std ~ scale)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, BLOCK_BYTES), np.uint8)
    out[:, 2:] = rng.integers(0, 256, size=(n, QK), dtype=np.uint8)
    d = (0.5 + rng.random(n)) * (scale / 74.0) * rng.choice([-1.0, 1.0], size=n)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(-1, 2)
    return out


def kat_blocks() -> np.ndarray:
    """Hand-built blocks: q = -128 / 127 / 0 in every one, under d = 1, 0, the smallest fp16
    subnormal, 65504, -0.5 and -65504."""
    ds = np.array([1.0, 0.0, 2.0 ** -24, 65504.0, -0.5, -65504.0], np.float16)
    out = np.zeros((ds.size, BLOCK_BYTES), np.uint8)
    out[:, 0:2] = ds.view(np.uint8).reshape(-1, 2)
    q = np.arange(QK, dtype=np.int32) * 8 - 124  # -124 .. 124
    q[0], q[1], q[2] = -128, 127, 0
    out[:, 2:] = q.astype(np.int8).view(np.uint8)
    return out
