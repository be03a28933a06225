"""Decode cost of sampled decoding against greedy on one GPU: the full Llama-3.2-3B shape with
synthetic weights, 2048-token prompts, engines of 8 and 128 slots, ignore_eos.

Per engine and mode (greedy; Ollama's default sampling: temperature 0.8, top_k 40, top_p 0.9,
repeat_penalty 1.1 over 64 tokens) every slot is filled first, then one decode run of 64 chained
steps is timed by the engine's own events (ms_stats.decode_ms / decode_steps), repeated --reps
times; a last run with the class timers on gives the lm_head (K_LMHEAD) and misc (K_MISC: the
greedy tail or the fused sampling tail, one launch per step, plus the run's first embedding
gather and, in engines of >= 24 slots, the layers' residual_rmsnorm launches) kernel times per
step -- the tail's own cost is the difference of the two modes' misc times.  Prints one JSON
line per (slots, mode).

A build without the sampling entry points (MAPSUM_LIB=<the parent commit's library>) measures
greedy only: the A/B for "the greedy path launches what it launched before".

usage: python tools/bench_sampling.py [--slots 8,128] [--prompt-len 2048] [--reps 2]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd")]

RUN = 64  # chained decode steps per timed run (the engine's kMaxRun)


def fill(eng, prompts, num_predict, sampling):
    """Submit every prompt and step until all are prefilled (admission ramps 8 prompts a step)."""
    total = sum(len(p) for p in prompts)
    for i, p in enumerate(prompts):
        kw = {} if sampling is None else {"sampling": sampling(i)}
        eng.submit(p, num_predict, True, **kw)
    steps = 0
    while eng.stats()["prefill_tokens"] < total:
        eng.step()
        steps += 1
    return steps


def drain(eng):
    while eng.step():
        pass
    eng.collect()
    eng._mailbox.clear()


def measure(eng, prompts, sampling, reps, L):
    ramp = (len(prompts) + 7) // 8 + 1
    num_predict = ramp + RUN * (reps + 3) + 8
    eng.reset_stats()
    fill(eng, prompts, num_predict, sampling)
    runs = []
    for _ in range(reps + 1):  # the first timed run also captures its graphs: dropped
        eng.reset_stats()
        eng.step()
        st = eng.stats()
        runs.append((st["decode_ms"] / max(st["decode_steps"], 1), st["decode_steps"]))
    eng.set_profiling((1 << L.K_LMHEAD) | (1 << L.K_MISC))
    eng.reset_stats()
    eng.step()
    st = eng.stats()
    eng.set_profiling(0)
    drain(eng)
    n = max(st["decode_steps"], 1)
    return {"decode_ms_per_step": [round(r[0], 4) for r in runs[1:]], "steps_per_run": [r[1] for r in runs[1:]],
            "first_run_ms_per_step": round(runs[0][0], 4),
            "lm_head_ms_per_step": round(st["kernel_ms"][L.K_LMHEAD] / n, 4),
            "lm_head_launches_per_step": st["kernel_launches"][L.K_LMHEAD] / n,
            "misc_ms_per_step": round(st["kernel_ms"][L.K_MISC] / n, 4),
            "misc_launches_per_step": st["kernel_launches"][L.K_MISC] / n,
            "profiled_steps": st["decode_steps"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,128")
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()

    from mapsum import _lib as L
    from mapsum.config import LLAMA32_3B as cfg
    from mapsum.engine import Engine, Sampling

    have_sampling = hasattr(L.load(), "ms_submit_sampled")
    for slots in [int(s) for s in args.slots.split(",")]:
        rng = np.random.default_rng(slots)
        prompts = [np.concatenate([[cfg.bos_id], rng.integers(0, 128000, size=args.prompt_len - 1)]).astype(np.int32)
                   for _ in range(slots)]
        max_ctx = args.prompt_len + (slots + 7) // 8 + RUN * (args.reps + 3) + 16
        with Engine(cfg, device=0, max_batch=slots, max_ctx=max_ctx,
                    max_prefill_tokens=min(slots, 8) * args.prompt_len) as eng:
            eng.init_synthetic(seed=0, std=0.02, norm_jitter=0.0)
            modes = [("greedy", None)]
            if have_sampling:
                modes.append(("ollama_defaults", lambda i: Sampling.ollama_defaults(seed=1000 + i)))
            for name, sampling in modes:
                r = measure(eng, prompts, sampling, args.reps, L)
                print(json.dumps({"slots": slots, "mode": name, "prompt_len": args.prompt_len,
                                  "lib": os.environ.get("MAPSUM_LIB", "in-tree"), **r}), flush=True)


if __name__ == "__main__":
    main()
