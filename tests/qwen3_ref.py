"""TEST INFRASTRUCTURE ONLY -- the numpy oracle of a QK-norm model (Qwen3).

``OracleQwen3`` is ``oracle.llama_ref.OracleLlama`` with one more piece of arithmetic: each Q head
and each K head is RMS-normalised over its ``head_dim`` values and multiplied by the layer's gain
(``q_norm`` / ``k_norm`` [head_dim], shared by the heads) between the QKV projection and RoPE --
the public Qwen3 architecture, pinned against ``transformers.Qwen3ForCausalLM`` by
``tests/golden/make_qwen3_golden.py``.  Its ``forward`` restates the oracle's forward with the
engine's QK-norm contract inserted:

  1. Q, K, V = f16(r * acc), the projection's rounding point, as ever;
  2. per Q / K head t (its 128 fp16 values): rho = 1 / sqrt(mean(t^2) + eps) in fp32;
  3. n = (t * rho) * w in fp32, w the fp16 gain indexed by the logical head dimension;
  4. RoPE (rotate-half) in fp32 on n, then ONE rounding to fp16 (Llama: round, rotate, round).

Modes as OracleLlama's: "engine" / "bf16" round at 1 and 4; "f16" (ggml) keeps Q / K fp32 from
the projection through the norm and RoPE and rounds once at the end; "fp32" rounds nowhere.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

from oracle.llama_ref import OracleLlama, _f16, _f32, apply_rope, norm_input, rms_rinv, rms_rinv_f64, rope_tables, silu
from oracle.synth import bf16_rne, make_weights

GAIN_SEED, GAIN_SPREAD = 97, 0.3


def make_qwen3_weights(cfg, seed: int, std: float = 0.02, jitter: float = 0.0, gain_seed: int = GAIN_SEED,
                       spread: float = GAIN_SPREAD) -> dict:
    """``oracle.synth.make_weights`` plus per-layer ``q_norm`` / ``k_norm`` = 1 + spread * N(0, 1)
    from a fixed numpy seed, held like every other weight as float32 arrays of bf16 values (which
    fp16 holds exactly).  The wide spread makes a gain indexed in the rope-permuted order, or a
    Q gain used for K, an error of order one."""
    w = make_weights(cfg, seed, std=std, jitter=jitter)
    rng = np.random.default_rng(gain_seed)
    for L in w["layers"]:
        L["q_norm"] = bf16_rne((1.0 + spread * rng.standard_normal(cfg.head_dim)).astype(np.float32))
        L["k_norm"] = bf16_rne((1.0 + spread * rng.standard_normal(cfg.head_dim)).astype(np.float32))
    return w


def qk_norm_rope_f64(t, gain, cos, sin, eps: float) -> np.ndarray:
    """Steps 2-4 evaluated in float64, unrounded: t [T, heads, D] (fp16 values, logical dim order),
    gain [D], cos / sin [T, D/2] -> [T, heads, D] float64."""
    t = np.asarray(t, np.float64)
    rho = 1.0 / np.sqrt(np.mean(t * t, axis=-1, keepdims=True) + np.float64(np.float32(eps)))
    n = (t * rho) * np.asarray(gain, np.float64)
    h = t.shape[-1] // 2
    a, b = n[..., :h], n[..., h:]
    c, s = np.asarray(cos, np.float64)[:, None, :], np.asarray(sin, np.float64)[:, None, :]
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


class OracleQwen3(OracleLlama):
    """Greedy Qwen3 (QK-norm) over ``make_qwen3_weights``' layout."""

    def forward(self, ids, cache=None, collect: bool = False, all_logits: bool = False, mut=None):
        """OracleLlama.forward with the per-head Q / K RMSNorm in front of RoPE (``mut`` is not
        supported here)."""
        assert not mut, "OracleQwen3 takes no mutations"
        cfg, w = self.cfg, self.w
        ids = np.asarray(ids, dtype=np.int64)
        T = ids.shape[0]
        cache = cache if cache is not None else self.new_cache()
        p0 = cache["len"]
        pos = np.arange(p0, p0 + T)
        cos, sin = rope_tables(cfg, pos)
        D, Hq, Hk = cfg.head_dim, cfg.n_heads, cfg.n_kv_heads
        G = Hq // Hk
        scale = np.float32(1.0 / math.sqrt(D))
        rnd = self.rnd
        f16 = self.mode == "f16"
        eps = cfg.norm_eps
        wide = self.acc == np.float64
        self.last_rinv = None

        def mm(a, b):
            if wide:
                return np.matmul(a.astype(np.float64), b.astype(np.float64)).astype(np.float32)
            return np.matmul(a, b)

        def rinv(x):
            return rms_rinv_f64(x, eps) if wide else rms_rinv(x, eps)

        def normed(x, g):
            if f16:
                return _f16((x * rms_rinv_f64(x, eps)) * g), np.float32(1.0)
            if self.mode == "engine":
                return rnd((x * g).astype(np.float32) * np.float32(0.0625)), rinv(x) * np.float32(16.0)
            return norm_input(x, g, rnd), rinv(x)

        def head_norm(t, g):
            """[T, heads, D] -> (t * rho) * g in fp32, unrounded (ggml: the sum of squares in double);
            the gain as the engine holds it, fp16, in the modes that hold fp16 weights."""
            rho = rms_rinv_f64(t, eps) if (f16 or wide) else rms_rinv(t, eps)
            g = _f16(g) if self.mode in ("engine", "f16") else _f32(g)
            return ((t * rho).astype(np.float32) * g).astype(np.float32)

        pre = _f32 if f16 else rnd
        x = w["embed"][ids].astype(np.float32)
        probes = []
        for l, L in enumerate(w["layers"]):
            xg, r = normed(x, L["attn_norm"])
            q = pre(r * mm(xg, L["wq"].T)).reshape(T, Hq, D)
            k = pre(r * mm(xg, L["wk"].T)).reshape(T, Hk, D)
            v = rnd(r * mm(xg, L["wv"].T)).reshape(T, Hk, D)
            q = apply_rope(head_norm(q, L["q_norm"]), cos, sin, rnd)  # rotated in fp32, rounded once
            k = apply_rope(head_norm(k, L["k_norm"]), cos, sin, rnd)
            if cache["k"][l] is not None:
                k = np.concatenate([cache["k"][l], k], axis=0)
                v = np.concatenate([cache["v"][l], v], axis=0)
            cache["k"][l], cache["v"][l] = k, v
            S = k.shape[0]
            kq = np.repeat(k, G, axis=1)
            vq = np.repeat(v, G, axis=1)
            s = mm(q.transpose(1, 0, 2), kq.transpose(1, 2, 0)) * scale
            mask = (np.arange(S)[None, :] > (p0 + np.arange(T))[:, None])
            s = np.where(mask[None], np.float32(-np.inf), s)
            s = s - s.max(axis=-1, keepdims=True)
            p = np.exp(s)
            den = p.sum(axis=-1, keepdims=True, dtype=self.acc).astype(np.float32)
            if self.mode == "engine":
                pv = mm(_f16(p), vq.transpose(1, 0, 2)) / den
            else:
                p = p / den
                if f16:
                    p = _f16(p)
                pv = mm(p.astype(np.float32), vq.transpose(1, 0, 2))
            o = rnd(pv.transpose(1, 0, 2))
            x = x + mm(o.reshape(T, Hq * D), L["wo"].T)
            xg, r = normed(x, L["ffn_norm"])
            g = r * mm(xg, L["w_gate"].T)
            u = r * mm(xg, L["w_up"].T)
            h = rnd(silu(g) * u)
            x = x + mm(h, L["w_down"].T)
            if collect:
                probes.append(x.copy())
        cache["len"] = p0 + T
        xs = x if all_logits else x[-1:]
        xg, r = normed(xs, w["final_norm"])
        logits = r * mm(xg, w["lm_head"].T)
        self.last_rinv = r
        return (logits if all_logits else logits[0]), probes


# ------------------------------------------------------------------ decode reference + bounds
# tests/test_gpu_qwen3.py's decode runs: two 100-token prompts, 32 tokens each (the decode crosses
# the 128-key page edge), teacher-forced with the ids recorded in tests/golden/qwen3_bounds.json.
# The K / V row and logits bounds there are 4 x the distance between the fp32- and the
# fp64-accumulating oracle (tests/decode_edges_ref.py's derivation): none comes from a GPU.
# Written by `python tests/golden/make_qwen3_bounds.py` (CPU).
SEED, STD, JITTER = 1234, 0.05, 0.1
N_PROMPT, NPRED, MARGIN = 100, 32, 4.0
BOUNDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen3_bounds.json")
_ORACLES, _BOUNDS = {}, {}


def tiny_weights():
    from mapsum.config import TINY_QWEN3
    if "w" not in _ORACLES:
        _ORACLES["w"] = make_qwen3_weights(TINY_QWEN3, SEED, std=STD, jitter=JITTER)
    return _ORACLES["w"]


def tiny_oracle(mode="engine", acc=np.float32) -> OracleQwen3:
    from mapsum.config import TINY_QWEN3
    key = (mode, np.dtype(acc).name)
    if key not in _ORACLES:
        _ORACLES[key] = OracleQwen3(TINY_QWEN3, tiny_weights(), mode=mode, acc=acc)
    return _ORACLES[key]


def decode_prompts() -> list:
    return [np.random.default_rng(8100 + 17 * i).integers(0, 4000, size=N_PROMPT).astype(np.int32) for i in range(2)]


def bounds() -> dict:
    if not _BOUNDS:
        with open(BOUNDS) as f:
            _BOUNDS.update(json.load(f))
    return _BOUNDS


def write_bounds() -> None:
    from decode_edges_ref import distances, run_sequence
    ps = decode_prompts()
    r32 = [run_sequence(tiny_oracle(), p, steps=NPRED) for p in ps]
    r64 = [run_sequence(tiny_oracle(acc=np.float64), p, feed=r["fed"], steps=NPRED) for p, r in zip(ps, r32)]
    floor = {}
    for a, b in zip(r32, r64):
        for f, d in distances(a, b).items():
            floor[f] = max(floor.get(f, 0.0), d)
    out = {"forced": [r["fed"] for r in r32], "floor": floor, "bound": {f: MARGIN * d for f, d in floor.items()}}
    with open(BOUNDS, "w") as f:
        json.dump(out, f, indent=1)
    print("floors", floor)

