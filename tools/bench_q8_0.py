"""Decode cost of the weight forms on one GPU: fp16, Q4_K_M and Q8_0 (and, with --dtypes, the
Q5_K_M mix q5_k_m) at the full Llama-3.2-3B shape with synthetic weights, 2048-token prompts, engines of 8 and 64 slots,
ignore_eos.

Per slot count the three engines live side by side, every slot filled first; then runs of 64
chained decode steps, timed by the engine's own events (ms_stats.decode_ms / decode_steps), are
taken in turn -- fp16, Q4_K_M, Q8_0, fp16, ... -- so drift of the box hits all three alike.  The
first run of each engine (graph capture) is dropped, --reps (>= 3) are kept.  A last pass with
the class timers on gives the GEMV (K_GEMV: the layers' projections) and lm_head (K_LMHEAD)
kernel times per step; for the quantised engines it is taken twice, with every grid-stride form
off and on (ms_set_qgemv_gs 0 / 1: profiled steps launch kernel by kernel, so the setting
applies at once).  The timed runs before them use the library's start-up setting (MS_QGEMV_GS,
default 3: the K-quant forms on, the Q8_0 lm_head's off); ms_set_qgemv_gs cannot restore it,
so every slot count runs in a child process of its own.  Prints one JSON line per (dtype,
slots) with the weight bytes a step streams, computed from the shapes, and the classes' bytes
per second as a fraction of 8 TB/s (quantised engines: of the setting named in "frac_setting").

usage: python tools/bench_q8_0.py [--slots 8,64] [--prompt-len 2048] [--reps 3]
                                  [--dtypes fp16,q4_k_m,q8_0 | fp16,q4_k_m,q5_k_m | ...]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd")]

RUN = 64  # chained decode steps per timed run (the engine's kMaxRun)
HBM = 8.0e12
BITS = {"f16": 16.0, 8: 8.5, 12: 4.5, 13: 5.5, 14: 6.5625}  # per weight: 34 B / 32, 144, 176, 210 B / 256


def q4_k_m_type(name, layer, n_layers):  # engine.cpp q4_k_m_type
    if name in ("embed", "lm_head"):
        return 14
    if name in ("wv", "w_down"):
        more = layer < n_layers // 8 or layer >= 7 * n_layers // 8 or (layer - n_layers // 8) % 3 == 2
        return 14 if more else 12
    return 12


def step_bytes(cfg, dtype):
    """(layer matrices, lm_head) bytes one decode step streams in its small-batch form."""
    qd, kd = cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim
    mats = {"wq": qd * cfg.hidden, "wk": kd * cfg.hidden, "wv": kd * cfg.hidden, "wo": cfg.hidden * qd,
            "w_gate": cfg.ffn * cfg.hidden, "w_up": cfg.ffn * cfg.hidden, "w_down": cfg.hidden * cfg.ffn}
    def kind(n, l):
        if dtype in ("fp16", "q8_0"):
            return "f16" if dtype == "fp16" else 8
        t = q4_k_m_type(n, l, cfg.n_layers)
        return 13 if dtype == "q5_k_m" and t == 12 else t  # Q5_K_M: Q5_K in place of Q4_K

    layers = sum(w * BITS[kind(n, l)] / 8 for l in range(cfg.n_layers) for n, w in mats.items())
    return int(layers), int(cfg.vocab * cfg.hidden * BITS[kind("lm_head", 0)] / 8)


def fill(eng, prompts, num_predict):
    total = sum(len(p) for p in prompts)
    for p in prompts:
        eng.submit(p, num_predict, True)
    while eng.stats()["prefill_tokens"] < total:
        eng.step()


def timed_run(eng):
    eng.reset_stats()
    eng.step()
    st = eng.stats()
    return st["decode_ms"] / max(st["decode_steps"], 1), st["decode_steps"]


def profiled_run(eng, L):
    eng.set_profiling((1 << L.K_GEMV) | (1 << L.K_LMHEAD))
    eng.reset_stats()
    eng.step()
    st = eng.stats()
    eng.set_profiling(0)
    n = max(st["decode_steps"], 1)
    return st["kernel_ms"][L.K_GEMV] / n, st["kernel_ms"][L.K_LMHEAD] / n, st["decode_steps"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,64")
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtypes", default="fp16,q4_k_m,q8_0")
    args = ap.parse_args()
    reps = max(args.reps, 3)
    if "," in args.slots:  # one fresh process per slot count (see the module docstring)
        for s in args.slots.split(","):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--slots", s, "--prompt-len",
                            str(args.prompt_len), "--reps", str(reps), "--dtypes", args.dtypes], check=True)
        return

    from mapsum import _lib as L
    from mapsum.config import LLAMA32_3B as cfg
    from mapsum.engine import Engine

    lib = L.load()
    init = {"fp16": lambda e: e.init_synthetic(seed=0, std=0.02, norm_jitter=0.0),
            "q4_k_m": lambda e: e.init_synthetic_q(seed=0, scale=0.02, norm_jitter=0.0),
            "q8_0": lambda e: e.init_synthetic_q8_0(seed=0, scale=0.02, norm_jitter=0.0),
            "q5_k_m": lambda e: e.init_synthetic_q5_k_m(seed=0, scale=0.02, norm_jitter=0.0)}
    dtypes = args.dtypes.split(",")
    for slots in [int(s) for s in args.slots.split(",")]:
        rng = np.random.default_rng(slots)
        prompts = [np.concatenate([[cfg.bos_id], rng.integers(0, 128000, size=args.prompt_len - 1)]).astype(np.int32)
                   for _ in range(slots)]
        ramp = (slots + 7) // 8 + 1
        num_predict = ramp + RUN * (reps + 4) + 8
        engines = {}
        try:
            for d in dtypes:
                e = Engine(cfg, device=0, max_batch=slots, max_ctx=args.prompt_len + num_predict + 16,
                           max_prefill_tokens=min(slots, 8) * args.prompt_len)
                engines[d] = e
                init[d](e)
                fill(e, prompts, num_predict)
            runs = {d: [] for d in dtypes}
            for _ in range(reps + 1):  # the first run of each engine captures its graphs: dropped
                for d in dtypes:
                    runs[d].append(timed_run(engines[d]))
            for d in dtypes:
                e = engines[d]
                gs = {}
                if d == "fp16":
                    gemv_ms, lm_ms, psteps = profiled_run(e, L)
                else:  # one-tile blocks everywhere, then every grid-stride form
                    for name, on in (("off", 0), ("on", 1)):
                        L.check(lib.ms_set_qgemv_gs(on))
                        gs[name] = profiled_run(e, L)
                    # the fractions below: the faster lm_head setting of this dtype
                    best = min(gs, key=lambda k: gs[k][1])
                    gemv_ms, lm_ms, psteps = gs[best]
                kept = [r[0] for r in runs[d][1:]]
                lay_b, lm_b = step_bytes(cfg, d)
                out = {"dtype": d, "slots": slots, "prompt_len": args.prompt_len,
                       "decode_ms_per_step": round(float(np.median(kept)), 4),
                       "runs_ms_per_step": [round(x, 4) for x in kept],
                       "spread_ms": round(max(kept) - min(kept), 4),
                       "first_run_ms_per_step": round(runs[d][0][0], 4),
                       "steps_per_run": [r[1] for r in runs[d][1:]],
                       "layer_weight_bytes_per_step": lay_b, "lm_head_weight_bytes_per_step": lm_b,
                       "weight_bytes_per_step": lay_b + lm_b,
                       "gemv_class_ms_per_step": round(gemv_ms, 4), "lm_head_class_ms_per_step": round(lm_ms, 4),
                       "gemv_class_frac_of_8TBs": round(lay_b / (gemv_ms * 1e-3) / HBM, 3) if gemv_ms > 0 else None,
                       "lm_head_frac_of_8TBs": round(lm_b / (lm_ms * 1e-3) / HBM, 3) if lm_ms > 0 else None,
                       "profiled_steps": psteps}
                if gs:
                    out["frac_setting"] = "gs_" + best
                    out["timed_runs_qgemv_gs_mask"] = int(os.environ.get("MS_QGEMV_GS", "3"))
                    for name, (g_ms, l_ms, _) in gs.items():
                        out["gemv_class_ms_per_step_gs_" + name] = round(g_ms, 4)
                        out["lm_head_class_ms_per_step_gs_" + name] = round(l_ms, 4)
                print(json.dumps(out), flush=True)
        finally:
            for e in engines.values():
                e.close()


if __name__ == "__main__":
    main()
