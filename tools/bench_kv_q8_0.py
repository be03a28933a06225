"""fp16 KV cache against the q8_0 KV cache (Engine(kv_cache_type="q8_0")), paired, at the Llama-3.2-3B shape.

Per slot count (default 8, 128, 256) two engines on the same synthetic fp16 weights -- one per cache type --
are created once, each given `slots` prompts of --prompt-len tokens and --num-predict greedy tokens
(ignore_eos); after one warm-up run each (code objects, graph capture) they are measured in turn, fp16 then
q8_0, over --rounds paired rounds, and once more with the class timers on.  Recorded per slot count and
cache type: decode ms per step of every round (the engine's own device events around each decode run), the
decode-attention class in us per layer and step, the norm / rope / misc class per step (it holds the q8_0
engine's writer launch: one per layer that the fp16 engine folds into attention's prologue, the QKV GEMV's
epilogue or the persistent step), and the K/V bytes per token.  At 8 slots the fp16 engine runs the v2
attention and the slab prologue; the q8_0 engine runs neither.

No hardware counters are collected: the traffic figures are the pools' byte counts, not measurements.

Writes one JSON line per measurement to stdout and to --out (default profiles/kv_q8_0/bench_kv_q8_0.jsonl).

usage: python tools/bench_kv_q8_0.py [--slots 8,128,256] [--prompt-len 2048] [--num-predict 64] [--rounds 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd")]

KINDS = ("f16", "q8_0")


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def kv_bytes_per_token(cfg, kind):
    per_head = 2 * cfg.head_dim * 2 if kind == "f16" else 2 * 8704 // 64  # K and V
    return cfg.n_layers * cfg.n_kv_heads * per_head


def bench(out, slots, prompt_len, num_predict, rounds, layers):
    from mapsum.config import LLAMA32_3B
    from mapsum.engine import Engine
    cfg = LLAMA32_3B if not layers else LLAMA32_3B.with_(n_layers=layers, name=f"llama3.2-3b-{layers}-layers")
    rng = np.random.default_rng(slots)
    prompts = [rng.integers(0, 128000, size=prompt_len).astype(np.int32) for _ in range(slots)]
    engines = {}
    try:
        for kind in KINDS:
            e = Engine(cfg, device=0, max_batch=slots, max_ctx=prompt_len + num_predict + 16,
                       max_prefill_tokens=min(slots * prompt_len, 65536), kv_cache_type=kind)
            e.init_synthetic(seed=0, std=0.02, norm_jitter=0.0)
            engines[kind] = e
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)  # warm-up of this shape
        ms = {k: [] for k in KINDS}
        for _ in range(rounds):
            for kind in KINDS:  # the same order in every round
                e = engines[kind]
                e.reset_stats()
                e.generate(prompts, num_predict=num_predict, ignore_eos=True)
                s = e.stats()
                ms[kind].append(round(s["decode_ms"] / max(s["decode_steps"], 1), 4))
        for kind in KINDS:
            e = engines[kind]
            e.set_profiling(0xFF)
            e.reset_stats()
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)
            s = e.stats()
            steps = max(s["decode_steps"], 1)
            emit(out, {"model": cfg.name + " (synthetic fp16 weights)", "kv_cache_type": kind, "slots": slots,
                       "prompt_len": prompt_len, "num_predict": num_predict,
                       "decode_ms_per_step_rounds": ms[kind],
                       "decode_ms_per_step_median": sorted(ms[kind])[len(ms[kind]) // 2],
                       "attn_decode_us_per_layer_step": round(1e3 * s["kernel_ms"][3] / steps / cfg.n_layers, 2),
                       "attn_decode_launches_per_step": s["kernel_launches"][3] / steps,
                       "misc_us_per_step": round(1e3 * s["kernel_ms"][5] / steps, 2),
                       "misc_launches_per_step": round(s["kernel_launches"][5] / steps, 2),
                       "gemv_us_per_step": round(1e3 * s["kernel_ms"][2] / steps, 2),
                       "persist_steps": s["persist_steps"],
                       "kv_bytes_per_token": kv_bytes_per_token(cfg, kind),
                       "note": "class timers (eager launches, no graphs) include the prefill pass's launches of class 5; "
                               "decode_ms_per_step is from the graph runs; no hardware counters collected"})
    finally:
        for e in engines.values():
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,128,256")
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--num-predict", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers than the model's 28 (a quick look; 0 = all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_q8_0", "bench_kv_q8_0.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_kv_q8_0: no GPU (there is no CPU fallback: a CPU time says nothing about the engine)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        for n in [int(x) for x in args.slots.split(",") if x]:
            bench(out, n, args.prompt_len, args.num_predict, max(args.rounds, 1), args.layers)


if __name__ == "__main__":
    main()
