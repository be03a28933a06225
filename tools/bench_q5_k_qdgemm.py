"""Large-regime A/B of the all-Q5_K matrices of a Q5_K_M engine: their packed rows through
k_qdgemm.hip (MS_QDGEMM=1, the default) against their fp16 copies through k_dgemm.hip (MS_QDGEMM=3:
the all-Q4_K matrices only, of which a Q5_K_M engine has none).

Two synthetic Q5_K_M engines of --slots slots at the full Llama-3.2-3B shape live side by side,
one per mode (the mode is read when an engine is created), every slot filled; then runs of 64
chained decode steps, timed by the engine's own events, are taken in turn -- copies, packed, copies,
... -- so drift of the box hits both alike.  The first run of each engine (graph capture) is
dropped.  A last pass with the class timers on gives the GEMV class (the layers' projections) per
step.  Prints one JSON line per round and a summary line; "packed_faster_in_every_round" is the
condition DESIGN.md section 5 sets for keeping the form on by default.

usage: python tools/bench_q5_k_qdgemm.py [--slots 128] [--prompt-len 512] [--rounds 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd"),
                os.path.join(ROOT, "tools")]

from bench_q8_0 import RUN, fill, profiled_run, timed_run  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=128)
    ap.add_argument("--prompt-len", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    rounds = max(args.rounds, 3)

    from mapsum import _lib as L
    from mapsum.config import LLAMA32_3B as cfg
    from mapsum.engine import Engine

    rng = np.random.default_rng(args.slots)
    prompts = [np.concatenate([[cfg.bos_id], rng.integers(0, 128000, size=args.prompt_len - 1)]).astype(np.int32)
               for _ in range(args.slots)]
    num_predict = (args.slots + 7) // 8 + 1 + RUN * (rounds + 3) + 8
    modes = {"fp16_copies": "3", "packed_q5_k": "1"}
    engines = {}
    try:
        for name, mode in modes.items():
            os.environ["MS_QDGEMM"] = mode
            e = Engine(cfg, device=0, max_batch=args.slots, max_ctx=args.prompt_len + num_predict + 16,
                       max_prefill_tokens=8 * args.prompt_len)
            engines[name] = e
            e.init_synthetic_q5_k_m(seed=0, scale=0.02, norm_jitter=0.0)
            fill(e, prompts, num_predict)
        os.environ.pop("MS_QDGEMM", None)
        for e in engines.values():  # graph capture: dropped
            timed_run(e)
        wins = 0
        for r in range(rounds):
            ms = {name: timed_run(e)[0] for name, e in engines.items()}
            wins += ms["packed_q5_k"] < ms["fp16_copies"]
            print(json.dumps({"round": r, "slots": args.slots, "prompt_len": args.prompt_len,
                              "decode_ms_per_step": {k: round(v, 4) for k, v in ms.items()}}), flush=True)
        gemv = {name: round(profiled_run(e, L)[0], 4) for name, e in engines.items()}
        print(json.dumps({"summary": True, "slots": args.slots, "rounds": rounds, "packed_faster_rounds": int(wins),
                          "packed_faster_in_every_round": bool(wins == rounds),
                          "gemv_class_ms_per_step": gemv}), flush=True)
    finally:
        for e in engines.values():
            e.close()


if __name__ == "__main__":
    main()
