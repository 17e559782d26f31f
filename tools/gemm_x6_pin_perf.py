"""csrc/gemm_x6.hip: the loop whose order is left to the scheduler (tiles 2 / 3, the production form) against a step's MFMAs fenced
ahead of its closing wait and barrier (developer tiles 42 / 43), plain epilogue, on the main loops of the two fused production GEMMs:
4644 x 512 -> 3072 ([w1; w3]) and 3822 x (5 x 512) -> 1024 (the WaveNet taps as one K = 2560 GEMM).  The forms alternate, ROUNDS times and in
changing order, so that a drift of the clocks shows as a spread within a column and favours neither.  us per call (CUDA events).  Usage: python tools/gemm_x6_pin_perf.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice_tts_amd import gemm as G  # noqa: E402

dev = torch.device("cuda:0")
ROUNDS = 6


def bench(fn, n=40):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


for name, M, K, N in [("w1|w3", 4644, 512, 3072), ("wavenet taps", 3822, 2560, 1024)]:
    x = torch.randn(M, K, device=dev)
    pl = G.PackedLinear(torch.randn(N, K, device=dev) / K ** 0.5)
    planes, out = G.split(x), torch.empty(M, N, device=dev)
    for free, fenced in ((2, 42), (3, 43)):
        t = {fenced: [], free: []}
        bench(lambda: G.linear(planes, pl, out=out, bias=False, tile=free), n=200)  # (clocks settled before the first column)
        for r in range(ROUNDS):
            for tile in ((free, fenced) if r % 2 == 0 else (fenced, free)):  # neither form always runs second
                t[tile].append(bench(lambda: G.linear(planes, pl, out=out, bias=False, tile=tile)))
        fmt = lambda v: " ".join(f"{u:6.1f}" for u in v)  # noqa: E731
        print(f"{name:12s} M={M} K={K} N={N}: tile {free} unfenced [{fmt(t[free])}] us | tile {fenced} fenced [{fmt(t[fenced])}] us | "
              f"min {min(t[free]):6.1f} vs {min(t[fenced]):6.1f}", flush=True)
