"""Qwen3-8B on the engine: prefill ms per pass and decode ms per step, synthetic weights.

Two engines in turn at the full Qwen3-8B shape (36 layers, hidden 4096, 32 / 8 heads, ffn 12288,
vocab 151936) -- fp16 weights, then the Q4_K_M mix -- each given --chunks prompts of --prompt-len
tokens and --num-predict greedy tokens (ignore_eos), the reference's map call shape
(8 x 2048 -> 256).  Times are the engine's own device events (ms_stats prefill_ms / decode_ms); a
second pass with the class timers on gives the per-class kernel time, where class 5 (norm / rope /
misc) holds the QK-norm kernel.  --kernel times the kernel alone through ms_op_qk_norm_rope with
device events: the rows form at T = 16384 on the Llama-3.2-3B head counts (24 / 8, beside
rope_kv_kernel's figures in DESIGN.md §5) and on Qwen3-8B's (32 / 8), and both forms at B = 8.
There is no parent figure for Qwen3: the numbers are stated, not compared.

Writes one JSON line per measurement to stdout and to --out (default profiles/qwen3/bench_qwen3.jsonl).

usage: python tools/bench_qwen3.py [--chunks 8] [--prompt-len 2048] [--num-predict 256] [--weights fp16,q4_k_m] [--kernel]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd")]


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def bench_engine(out, weights, chunks, prompt_len, num_predict):
    from mapsum.config import QWEN3_8B as cfg
    from mapsum.engine import Engine
    rng = np.random.default_rng(chunks)
    prompts = [rng.integers(0, 150000, size=prompt_len).astype(np.int32) for _ in range(chunks)]
    e = Engine(cfg, device=0, max_batch=chunks, max_ctx=prompt_len + num_predict + 16,
               max_prefill_tokens=chunks * prompt_len)
    try:
        if weights == "fp16":
            e.init_synthetic(seed=0, std=0.02, norm_jitter=0.0)
        else:
            e.init_synthetic_q(seed=0, scale=0.02, norm_jitter=0.0)
        e.generate(prompts[:1], num_predict=20, ignore_eos=True)  # code objects, graph capture at B = 1
        for prof in (False, True):
            e.set_profiling(0xFF if prof else 0)
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)  # warm-up of this shape (graphs at B)
            e.reset_stats()
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)
            s = e.stats()
            rec = {"model": "qwen3-8b (synthetic)", "weights": weights, "chunks": chunks, "prompt_len": prompt_len,
                   "num_predict": num_predict, "class_timers": prof,
                   "prefill_ms_per_pass": round(s["prefill_ms"] / max(s["prefill_passes"], 1), 3),
                   "prefill_passes": s["prefill_passes"],
                   "decode_ms_per_step": round(s["decode_ms"] / max(s["decode_steps"], 1), 4),
                   "decode_steps": s["decode_steps"]}
            if prof:
                rec["kernel_ms"] = [round(x, 3) for x in s["kernel_ms"][:7]]
                rec["kernel_launches"] = s["kernel_launches"][:7]
            emit(out, rec)
    finally:
        e.close()


def bench_kernel(out):
    import torch
    from mapsum import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda:0")

    def run(form, T, hq, hk, S=0, iters=50):
        nh = hq + 2 * hk
        max_pages = 1
        qkv = torch.randn(T, nh * 128, device=dev).to(torch.float16)
        slabs = torch.randn(max(S, 1), T, nh * 128, device=dev) if S else None
        pos = torch.arange(T, dtype=torch.int32, device=dev) % 64
        slot = (torch.arange(T, dtype=torch.int32, device=dev) // 64).contiguous()
        n_slots = (T + 63) // 64
        bt = torch.arange(n_slots * max_pages, dtype=torch.int32, device=dev)
        kp = torch.zeros(n_slots * max_pages * hk * 64 * 128, dtype=torch.float16, device=dev)
        vp = torch.zeros_like(kp)
        cs, sn = torch.rand(64, 64, device=dev), torch.rand(64, 64, device=dev)
        qg, kg = torch.ones(128, dtype=torch.float16, device=dev), torch.ones(128, dtype=torch.float16, device=dev)

        def go():
            rc = lib.ms_op_qk_norm_rope(qkv.data_ptr(), slabs.data_ptr() if S else None, S, T, hq, hk, pos.data_ptr(),
                                        slot.data_ptr(), cs.data_ptr(), sn.data_ptr(), qg.data_ptr(), kg.data_ptr(),
                                        1e-6, kp.data_ptr(), vp.data_ptr(), bt.data_ptr(), max_pages, st)
            assert rc == 0, lib.ms_last_error(None)
        for _ in range(5):
            go()
        ts = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            go()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        ts.sort()
        emit(out, {"kernel": "qk_norm_rope", "form": form, "T": T, "n_heads": hq, "n_kv_heads": hk, "slabs": S,
                   "us_per_launch_median": round(ts[len(ts) // 2], 2), "us_min": round(ts[0], 2),
                   "us_p90": round(ts[int(0.9 * len(ts))], 2), "timing": "device events around one launch"})

    run("rows", 16384, 24, 8)
    run("rows", 16384, 32, 8)
    run("rows", 8, 32, 8)
    run("slabs", 8, 32, 8, S=4)
    run("rows", 8, 24, 8)
    run("slabs", 8, 24, 8, S=6)


def bench_extra_launch(out, layers=4, prompt_len=2048, num_predict=64):
    """What the QK-norm decode layer's extra launch costs at the LLAMA-3.2-3B shape, 8 slots: a
    Llama engine (decode attention folds the QKV slabs, rotates and scatters in its prologue --
    exactly the parent commit's launches) beside the same shape with ms_enable_qk_norm (gains 1.0:
    the norm kernel folds, normalises, rotates and scatters, attention reads rows).  Class timers:
    3 = decode attention, 5 = norm / rope / misc; per launch and per decode step."""
    from mapsum.config import LLAMA32_3B
    from mapsum.engine import Engine
    rng = np.random.default_rng(1)
    prompts = [rng.integers(0, 128000, size=prompt_len).astype(np.int32) for _ in range(8)]
    for qk in (False, True, False, True):
        cfg = LLAMA32_3B.with_(n_layers=layers, qk_norm=qk, name=f"llama-shape-{'qknorm' if qk else 'plain'}")
        e = Engine(cfg, device=0, max_batch=8, max_ctx=prompt_len + num_predict + 16, max_prefill_tokens=8 * prompt_len)
        try:
            e.init_synthetic(seed=0, std=0.02, norm_jitter=0.0)
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)
            e.reset_stats()
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)
            plain = e.stats()
            e.set_profiling(0xFF)
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)
            e.reset_stats()
            e.generate(prompts, num_predict=num_predict, ignore_eos=True)
            s = e.stats()
            steps = max(s["decode_steps"], 1)
            emit(out, {"extra_launch": True, "shape": "llama3.2-3b widths", "layers": layers, "slots": 8, "qk_norm": qk,
                       "decode_ms_per_step_graphs": round(plain["decode_ms"] / max(plain["decode_steps"], 1), 4),
                       "attn_decode_us_per_layer_step": round(1e3 * s["kernel_ms"][3] / steps / layers, 2),
                       "attn_decode_launches_per_step": s["kernel_launches"][3] / steps,
                       "misc_us_per_step": round(1e3 * s["kernel_ms"][5] / steps, 2),
                       "misc_launches_per_step": s["kernel_launches"][5] / steps,
                       "gemv_us_per_step": round(1e3 * s["kernel_ms"][2] / steps, 2),
                       "note": "class timers include the prefill pass's launches of classes 0, 1 and 5"})
        finally:
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--prompt-len", type=int, default=2048)
    ap.add_argument("--num-predict", type=int, default=256)
    ap.add_argument("--weights", default="fp16,q4_k_m")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--extra-launch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen3", "bench_qwen3.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_qwen3: no GPU (there is no CPU fallback: a CPU time says nothing about the engine)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        if args.kernel:
            bench_kernel(out)
        if args.extra_launch:
            bench_extra_launch(out)
        for w in [x for x in args.weights.split(",") if x]:
            if w not in ("fp16", "q4_k_m"):
                sys.exit(f"bench_qwen3: unknown weights {w!r}")
            bench_engine(out, w, args.chunks, args.prompt_len, args.num_predict)


if __name__ == "__main__":
    main()
