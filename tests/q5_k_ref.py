"""numpy reference for ggml's Q5_K (type 13): a 176-byte block of 256 weights
{fp16 d; fp16 dmin; scales[12]; qh[32]; qs[128]} -- Q4_K with a fifth bit per weight.  For weight
t: s = t >> 5 (sub-block), l = t & 31, c = t >> 6,
    nib = qs[32c + l] >> 4 if t & 32 else qs[32c + l] & 0xF,   q = nib + 16 ((qh[l] >> s) & 1),
    (sc, m) = get_scale_min_k4(s),   y = (d * sc) * q - dmin * m
in fp32, one rounding per operation (ggml's published dequantize_row_q5_K; d1 * q has at most
11 + 6 + 5 significant bits, so that product is exact).  Also a plain min/max quantiser (the engine
only consumes blocks), seeded random blocks, hand-built blocks and the per-tensor type mixes."""
import numpy as np

QK_K, BLOCK_BYTES, GGML_TYPE_Q5_K = 256, 176, 13
GGML_TYPE_Q4_K, GGML_TYPE_Q6_K = 12, 14


def scale_min_k4(sc: np.ndarray, j: int):
    """get_scale_min_k4 over a batch: sc [n][12] uint8 -> (scale, min) int32 [n]."""
    sc = sc.astype(np.int32)
    if j < 4:
        return sc[:, j] & 63, sc[:, j + 4] & 63
    return (sc[:, j + 4] & 0xF) | ((sc[:, j - 4] >> 6) << 4), (sc[:, j + 4] >> 4) | ((sc[:, j] >> 6) << 4)


def pack_scales(s: np.ndarray, m: np.ndarray) -> np.ndarray:
    """6-bit scales / mins int [n][8] -> the 12 scale bytes get_scale_min_k4 reads."""
    s, m = s.astype(np.int32), m.astype(np.int32)
    sc = np.zeros((s.shape[0], 12), np.int32)
    for j in range(4):
        sc[:, j] = s[:, j] | ((s[:, j + 4] >> 4) << 6)
        sc[:, j + 4] = m[:, j] | ((m[:, j + 4] >> 4) << 6)
        sc[:, j + 8] = (s[:, j + 4] & 0xF) | ((m[:, j + 4] & 0xF) << 4)
    return sc.astype(np.uint8)


def codes(blocks: np.ndarray) -> np.ndarray:
    """The 5-bit codes q, int32 [n][256], in weight order."""
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BLOCK_BYTES)
    qh, qs = b[:, 16:48].astype(np.int32), b[:, 48:176].astype(np.int32)
    q = np.empty((b.shape[0], QK_K), np.int32)
    for s in range(8):
        c = s >> 1
        byte = qs[:, 32 * c:32 * c + 32]
        nib = (byte >> 4) if (s & 1) else (byte & 0xF)
        q[:, 32 * s:32 * s + 32] = nib + 16 * ((qh >> s) & 1)
    return q


def dequant_q5_k(blocks: np.ndarray) -> np.ndarray:
    """uint8 [n][176] (any shape of that size) -> float32 [n * 256]."""
    b = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, BLOCK_BYTES)
    d = b[:, 0:2].copy().view(np.float16).astype(np.float32)[:, 0]
    dmin = b[:, 2:4].copy().view(np.float16).astype(np.float32)[:, 0]
    q = codes(b).astype(np.float32)
    y = np.empty((b.shape[0], QK_K), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(8):
            sc, m = scale_min_k4(b[:, 4:16], s)
            d1 = (d * sc.astype(np.float32)).astype(np.float32)
            m1 = (dmin * m.astype(np.float32)).astype(np.float32)
            prod = (d1[:, None] * q[:, 32 * s:32 * s + 32]).astype(np.float32)
            y[:, 32 * s:32 * s + 32] = (prod - m1[:, None]).astype(np.float32)
    return y.reshape(-1)


def assemble(d, dmin, s, m, q) -> np.ndarray:
    """fp16-able d, dmin [n]; scales, mins int [n][8]; codes int [n][256] -> uint8 [n][176]."""
    q = np.asarray(q, np.int32).reshape(-1, 8, 32)
    n = q.shape[0]
    b = np.zeros((n, BLOCK_BYTES), np.uint8)
    b[:, 0:2] = np.asarray(d, np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    b[:, 2:4] = np.asarray(dmin, np.float16).reshape(n).view(np.uint8).reshape(n, 2)
    b[:, 4:16] = pack_scales(np.asarray(s).reshape(n, 8), np.asarray(m).reshape(n, 8))
    qh = np.zeros((n, 32), np.int32)
    for j in range(8):
        qh |= (q[:, j] >> 4) << j
    b[:, 16:48] = qh.astype(np.uint8)
    for c in range(4):
        b[:, 48 + 32 * c:80 + 32 * c] = ((q[:, 2 * c] & 0xF) | ((q[:, 2 * c + 1] & 0xF) << 4)).astype(np.uint8)
    return b


def quantize_q5_k(x: np.ndarray) -> np.ndarray:
    """float32 values (size % 256 == 0) -> uint8 [n][176].  Per 32-weight sub-block the minimum
    (if negative) becomes dmin * m and the span / 31 becomes d * sc; d and dmin put the largest of
    the 8 at 63.  A min/max quantiser, not ggml's error-minimising search."""
    x = np.asarray(x, np.float32).reshape(-1, 8, 32)
    mn = np.maximum(-x.min(axis=2), 0.0)
    step = (x.max(axis=2) + mn) / 31.0
    d = (step.max(axis=1) / 63.0).astype(np.float16)
    dmin = (mn.max(axis=1) / 63.0).astype(np.float16)
    d32, dm32 = d.astype(np.float32), dmin.astype(np.float32)
    s = np.where(d32[:, None] > 0, np.rint(step / np.where(d32 > 0, d32, 1)[:, None]), 0).clip(0, 63).astype(np.int32)
    m = np.where(dm32[:, None] > 0, np.rint(mn / np.where(dm32 > 0, dm32, 1)[:, None]), 0).clip(0, 63).astype(np.int32)
    ds = d32[:, None] * s
    q = np.where(ds[:, :, None] > 0, np.rint((x + (dm32[:, None] * m)[:, :, None]) / np.where(ds > 0, ds, 1)[:, :, None]), 0)
    return assemble(d, dmin, s, m, q.clip(0, 31).astype(np.int32))


def random_blocks_q5_k(n: int, seed: int, scale: float = 1.0) -> np.ndarray:
    """n random blocks: every byte uniform (so sc, m cover 0..63 and q 0..31), d = u scale / 548 with
    u on [0.5, 1.5) and dmin = 15.5 d, which centres sc q - 15.5 m (std 527; weights of std ~ scale)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, size=(n, BLOCK_BYTES), dtype=np.uint8)
    d = ((0.5 + rng.random(n)) * (scale / 548.0)).astype(np.float16)
    b[:, 0:2] = d.view(np.uint8).reshape(-1, 2)
    b[:, 2:4] = (d.astype(np.float32) * np.float32(15.5)).astype(np.float16).view(np.uint8).reshape(-1, 2)
    return b


def kat_blocks() -> np.ndarray:
    """Hand-built blocks.  0: q(t) = t & 31, sc_s = s + 1, m_s = 2s + 1, d = 0.5, dmin = 0.25.
    1: sc = m = 63 in sub-blocks 4-7 (the high-2-bit packing), 1 and 2 in 0-3, q = 31 - (t & 31).
    2-4: block 0's codes and scales under d = 0, d = -0.5, d = the smallest fp16 subnormal.
    5: every code 31 (qh = 0xFF, qs = 0xFF) with sc = m = 63, d = dmin = 1."""
    t = np.arange(256)
    s8 = np.arange(8)
    q0, sc0, m0 = t & 31, s8 + 1, 2 * s8 + 1
    sc1, m1 = np.where(s8 >= 4, 63, 1), np.where(s8 >= 4, 63, 2)
    rows = [(0.5, 0.25, sc0, m0, q0), (0.5, 0.25, sc1, m1, 31 - (t & 31)), (0.0, 0.25, sc0, m0, q0),
            (-0.5, 0.25, sc0, m0, q0), (2.0 ** -24, 2.0 ** -24, sc0, m0, q0),
            (1.0, 1.0, np.full(8, 63), np.full(8, 63), np.full(256, 31))]
    return np.concatenate([assemble(np.float16([d]), np.float16([dm]), s[None], m[None], q[None])
                           for d, dm, s, m, q in rows])


def _more_bits(layer: int, n_layers: int) -> bool:
    return layer < n_layers // 8 or layer >= 7 * n_layers // 8 or (layer - n_layers // 8) % 3 == 2


def q5_k_m_type(name: str, layer: int, n_layers: int) -> int:
    """Q5_K_M per-tensor type: Q4_K_M's mix (oracle.quants.q4_k_m_type) with Q5_K in place of Q4_K."""
    if name in ("embed", "lm_head"):
        return GGML_TYPE_Q6_K
    if name in ("wv", "w_down") and _more_bits(layer, n_layers):
        return GGML_TYPE_Q6_K
    return GGML_TYPE_Q5_K


def q4_k_s_type(name: str, layer: int, n_layers: int) -> int:
    """Q4_K_S-style mix: Q4_K everywhere, Q5_K for wv / w_down in the first max(1, n_layers / 8)
    layers, a Q6_K embedding."""
    if name in ("embed", "lm_head"):
        return GGML_TYPE_Q6_K
    if name in ("wv", "w_down") and layer < max(1, n_layers // 8):
        return GGML_TYPE_Q5_K
    return GGML_TYPE_Q4_K
