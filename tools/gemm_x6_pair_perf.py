"""The fused-epilogue split-product GEMMs of the s2mel glue (csrc/gemm_x6.hip `ixtts_gemm_x6_pair_f32`) against the library forms they
replace, at the bench's segment (T = 2322 DiT rows per batch entry, Th = 1909 WaveNet frames), TunableOp file on as the glue runs it:
  [w1; w3] + SwiGLU:       F.linear + swiglu_kernel                    vs  split + one GEMM with the SwiGLU epilogue
  WaveNet in_layer + gate: 5 tap addmm_ + wn_gate_rows                 vs  split + one K = 5 x 512 GEMM with the gate epilogue
us per call (CUDA events), fp32-equivalent TFLOP/s.  Usage: python tools/gemm_x6_pair_perf.py [--pmc]  (--pmc: only the fused GEMMs,
a few calls each, for a `rocprofv3 --pmc` run)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice_tts_amd import gemm as G  # noqa: E402
from voice_tts_amd import s2mel as S2  # noqa: E402

dev = torch.device("cuda:0")
S2.use_tuned_gemms()


def bench(fn, n=30):
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


pmc = "--pmc" in sys.argv
H, Fd, B, T, Th, k = 512, 1536, 2, 2322, 1909, 5
g = torch.Generator(device=dev).manual_seed(0)

# DiT feed-forward: x [2T, H] -> silu(x w1^T) * (x w3^T) [2T, Fd]
x = torch.randn(B * T, H, device=dev, generator=g)
w13 = torch.randn(2 * Fd, H, device=dev, generator=g) / H ** 0.5
pl13 = G.PackedLinear(G.interleave_halves(w13[:Fd], w13[Fd:]))
u = torch.empty(B * T, Fd, device=dev)
fl = 2.0 * B * T * 2 * Fd * H
if pmc:
    for _ in range(5):
        G.pair_linear(x, pl13, G.SWIGLU, out=u)
else:
    t_lib = bench(lambda: S2.swiglu(torch.nn.functional.linear(x, w13)))
    t_gemm = bench(lambda: torch.nn.functional.linear(x, w13))
    xp = G.split(x)
    line = f"w1|w3+swiglu M={B * T} K={H} N={2 * Fd}: library {t_lib:6.1f} us (GEMM {t_gemm:6.1f}, {fl / t_gemm / 1e6:5.1f} TF)"
    line += f" | fused with split {bench(lambda: G.pair_linear(x, pl13, G.SWIGLU, out=u)):6.1f}"
    for tile in (2, 3):
        t = bench(lambda: G.pair_linear(xp, pl13, G.SWIGLU, out=u, tile=tile))
        line += f" | tile{tile} {t:6.1f} us ({fl / t / 1e6:5.1f} TF)"
    print(line, flush=True)

# WaveNet in_layer: padded rows [B (Th + 4), H] -> gate(sum_j rows[j:] W_j^T + b, g) [B (Th + 4) - 4, H]
Tp = Th + k - 1
P = torch.randn(B * Tp, H, device=dev, generator=g)
M = B * Tp - (k - 1)
taps = [torch.randn(2 * H, H, device=dev, generator=g) / (H * k) ** 0.5 for _ in range(k)]
bias = torch.randn(2 * H, device=dev, generator=g) * 0.1
gate = torch.randn(B, 2 * H * 8, device=dev, generator=g)
wcat = torch.cat(taps, 1)
plwn = G.PackedLinear(G.interleave_halves(wcat[:H], wcat[H:]), G.interleave_halves(bias[:H], bias[H:]))
acts = torch.empty(M, H, device=dev)
fl = 2.0 * M * 2 * H * H * k


def lib_wn():
    acc = torch.addmm(bias, P[:M], taps[0].t())
    for j in range(1, k):
        acc.addmm_(P[j:j + M], taps[j].t())
    return S2.wn_gate_rows(acc, gate, 0, H, Tp)


if pmc:
    for _ in range(5):
        G.pair_linear(G.split(P), plwn, G.GATE, taps=k, out=acts, gate=gate, rows_per_batch=Tp)
else:
    t_lib = bench(lib_wn)
    Pp = G.split(P)
    line = f"wavenet taps+gate M={M} K={k}x{H} N={2 * H}: library {t_lib:6.1f} us ({fl / t_lib / 1e6:5.1f} TF incl. gate)"
    line += f" | fused with split {bench(lambda: G.pair_linear(G.split(P), plwn, G.GATE, taps=k, out=acts, gate=gate, rows_per_batch=Tp)):6.1f}"
    for tile in (2, 3):
        t = bench(lambda: G.pair_linear(Pp, plwn, G.GATE, taps=k, out=acts, gate=gate, rows_per_batch=Tp, tile=tile))
        line += f" | tile{tile} {t:6.1f} us ({fl / t / 1e6:5.1f} TF)"
    print(line, flush=True)
    # tile 3 (two workgroups per CU by design, one in fact at 240 tiles) against tile 6 (the pipelined loop), alternating
    for rnd in range(4):
        t3, t6 = (bench(lambda: G.pair_linear(Pp, plwn, G.GATE, taps=k, out=acts, gate=gate, rows_per_batch=Tp, tile=tile), n=100) for tile in (3, 6))
        print(f"  round {rnd}: tile3 {t3:6.1f} us | tile6 {t6:6.1f} us ({fl / t6 / 1e6:5.1f} TF) | tile6 / tile3 {t6 / t3:.3f}", flush=True)
