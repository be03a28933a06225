"""Timeline of the fp16 decode GEMV (k_gemv.hip gemv_body) from its in-kernel stamps, per issue order.

Launches the bench's decode projections at M = 8 through the op-level entry points -- QKV
(split-K 6 slabs, 256 statistics tiles), O and down (residual epilogue on 12-row tiles), gate/up
(SwiGLU, 256 statistics tiles) -- under every issue order (ms_set_gemv_order), with
MS_GEMV_STAMPS=1 selecting the stamped twins of the kernels.  Weights rotate over copies and a
1 GiB sweep runs before every launch, so each launch streams from HBM as a decode step does.
Reads the latest launch's s_memrealtime stamps (100 MHz) of wave 0 and of the last wave of every
block (ms_debug_gemv_stamps; the first 1024 blocks) and prints, per phase, the median over blocks and
launches and the slowest block's value, in us since that block's own entry.
Diagnostic only: the stamped kernels wait for the first and the last weight step on their own.

  usage: python3 tools/gemv_stamps.py [--orders 0,1,2] [--reps 5]
         python3 tools/gemv_stamps.py --time     (no stamps: us per launch of every shape and order)
         python3 tools/gemv_stamps.py --time --orders 0,1,2,3,4,5,6,7,8
           (orders 3..8 = the issue orders on the line-exact weight loads, default policy and
            non-temporal; timing only: the stamped twins exist for the pair form)
"""
import argparse
import ctypes as C
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--orders", default="0,1,2")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--m", type=int, default=8)
ap.add_argument("--time", action="store_true", help="time the plain kernels instead (HIP events, rotating weights)")
args = ap.parse_args()
if not args.time:
    os.environ["MS_GEMV_STAMPS"] = "1"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mapsum import _lib as L  # noqa: E402

NB, NS = 1024, 32
PHASES = [(2, "first weight pair issued"), (3, "X and statistics issued"), (4, "all weight loads issued"),
          (5, "own wait for X passed"), (6, "X barrier passed"), (7, "first weight step landed"),
          (8, "last weight step landed"), (9, "MFMAs issued"), (10, "partials written"),
          (11, "epilogue stores issued")]
H, F, QKVN, V = 3072, 8192, 5120, 128256


def main():
    lib = L.load()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    M = args.m
    g = torch.Generator(device="cpu").manual_seed(5)
    flush = torch.empty(256 * 1024 * 1024, dtype=torch.float32, device=dev)
    ws = torch.zeros(256, dtype=torch.uint8, device=dev)

    def weights(N, K):
        # enough copies that the rotation streams > 600 MB: the 256 MB MALL never holds the next matrix
        w = (torch.randn(N, K, device=dev, dtype=torch.float16) * 0.02)
        return [w] + [w.clone() for _ in range(max(2, -(-600 * 2**20 // (N * K * 2))) - 1)]

    def xin(K):
        return torch.randn(M, K, generator=g).to(torch.float16).to(dev)

    ssq256 = (torch.rand(256, M, generator=g) * 12 + 1).to(dev)
    gamma = torch.ones(H, dtype=torch.float16, device=dev)
    shapes = []

    def qkv():
        Ws, X, slabs = weights(QKVN, H), xin(H), torch.zeros(6, M, QKVN, device=dev)

        def go(i):
            L.check(lib.ms_op_set_row_scale(ssq256.data_ptr(), 256, H, 1e-5))
            try:
                L.check(lib.ms_op_gemv_split(X.data_ptr(), Ws[i % len(Ws)].data_ptr(), slabs.data_ptr(), M, QKVN, H, 6, 0, st))
            finally:
                L.check(lib.ms_op_set_row_scale(None, 0, 0, 0.0))
        return go

    def resid(K):
        Ws, X = weights(H, K), xin(K)
        x, xg, ssq = torch.zeros(M, H, device=dev), torch.zeros(M, H, dtype=torch.float16, device=dev), \
            torch.zeros(256, M, device=dev)

        def go(i):
            L.check(lib.ms_op_gemv_resid(X.data_ptr(), Ws[i % len(Ws)].data_ptr(), x.data_ptr(), xg.data_ptr(),
                                         gamma.data_ptr(), ssq.data_ptr(), M, H, K, 12, st))
        return go

    def gate_up():
        Ws, X, out = weights(2 * F, H), xin(H), torch.zeros(M, F, dtype=torch.float16, device=dev)

        def go(i):
            L.check(lib.ms_op_set_row_scale(ssq256.data_ptr(), 256, H, 1e-5))
            try:
                L.check(lib.ms_op_gemv(X.data_ptr(), Ws[i % len(Ws)].data_ptr(), out.data_ptr(), M, 2 * F, H, F,
                                       L.MS_EPI_SWIGLU, ws.data_ptr(), st))
            finally:
                L.check(lib.ms_op_set_row_scale(None, 0, 0, 0.0))
        return go

    def lm_head():
        Ws, X, out = weights(V, H), xin(H), torch.zeros(M, V // 16, 2, device=dev)

        def go(i):
            L.check(lib.ms_op_gemv(X.data_ptr(), Ws[i % len(Ws)].data_ptr(), out.data_ptr(), M, V, H, V // 16,
                                   L.MS_EPI_ARGMAX, ws.data_ptr(), st))
        return go

    shapes = [("qkv split-6", qkv), ("o", lambda: resid(H)), ("gate/up", gate_up), ("down", lambda: resid(F))]
    if args.time:
        shapes.append(("lm_head", lm_head))
    orders = [int(o) for o in args.orders.split(",")]
    for name, make in shapes:
        go = make()
        if args.time:
            time_orders(lib, name, go, orders, flush)
        else:
            for o in orders:
                stamp_order(lib, name, go, o, flush)
        del go
        torch.cuda.empty_cache()
    lib.ms_set_gemv_order(L.GEMV_ORDER_DEFAULT)


def time_orders(lib, name, go, orders, flush, rounds=7, reps=24):
    """Interleaved rounds; a round times `reps` launches over rotating weight copies."""
    res = {o: [] for o in orders}
    s = torch.cuda.current_stream()
    k = 0
    for _ in range(rounds):
        for o in orders:
            L.check(lib.ms_set_gemv_order(o))
            flush.zero_()
            go(k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(reps):
                k += 1
                go(k)
            e1.record(s)
            torch.cuda.synchronize()
            res[o].append(e0.elapsed_time(e1) * 1e3 / reps)
    line = f"{name:12s}"
    for o in orders:
        v = np.array(res[o])
        line += f" | order {o}: median {np.median(v):6.2f} min {v.min():6.2f} max {v.max():6.2f} us"
    print(line, flush=True)


def stamp_order(lib, name, go, order, flush):
    L.check(lib.ms_set_gemv_order(order))
    runs = []
    for i in range(args.reps + 1):
        flush.zero_()
        go(i)
        torch.cuda.synchronize()
        buf = (C.c_uint64 * (NB * NS))()
        L.check(lib.ms_debug_gemv_stamps(C.cast(buf, C.c_void_p), NB * NS))
        st = np.frombuffer(buf, dtype=np.uint64).reshape(NB, NS).astype(np.int64)
        if i:  # the first launch loads the code object
            runs.append(st[st[:, 0] > 0])
    nblk = len(runs[0])
    print(f"\n{name}, order {order}: {nblk} stamped blocks x {len(runs)} launches; us since the block's entry "
          f"(wave 0 | last wave): median, and the slowest block of the last launch")
    if nblk == 0:
        print("  no stamps: this shape has no stamped kernel")
        return
    t0 = [r[:, 0].min() for r in runs]
    span = [(r[:, [11, 27]].max() - t) / 100.0 for r, t in zip(runs, t0)]
    entry = np.concatenate([(r[:, 0] - t) / 100.0 for r, t in zip(runs, t0)])
    print(f"  launch span (first entry -> last epilogue store): median {np.median(span):.2f} us; "
          f"block entry after the first: median {np.median(entry):.2f}, max {entry.max():.2f} us")
    last = runs[-1]
    slow = int(np.argmax(last[:, [11, 27]].max(axis=1)))
    for k, label in PHASES:
        a = np.concatenate([(r[:, k] - r[:, 0])[r[:, k] > 0] for r in runs]) / 100.0
        b = np.concatenate([(r[:, 16 + k] - r[:, 16])[r[:, 16 + k] > 0] for r in runs]) / 100.0
        if len(a) == 0:
            continue
        sa = (last[slow, k] - last[slow, 0]) / 100.0
        sb = (last[slow, 16 + k] - last[slow, 16]) / 100.0
        print(f"  {label:28s} {np.median(a):6.2f} | {np.median(b):6.2f}    slowest block: {sa:6.2f} | {sb:6.2f}")


if __name__ == "__main__":
    main()
