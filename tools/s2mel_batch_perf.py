"""Per-segment against packed s2mel solves (`S2Mel.__call__` n times vs ONE `S2Mel.solve_many`) at production width: S2MEL_CFG,
synthetic weights, 430-frame prompts, 25 Euler steps, on three shapes:
  (a) the headline's 2 x 1100 codes;  (b) 4 x 150 codes;  (c) 16 segments of mixed64's length distribution, 4 distinct prompts.
Also: HIP launches per Euler step (both forms), the packed result against the per-segment one, and the varlen attention against
the per-segment attention (with its key-range split) on the same rows.

    python tools/s2mel_batch_perf.py [--reps 2] [--steps 25]
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voice_tts_amd.s2mel as S2  # noqa: E402
from voice_tts_amd import gemm as G  # noqa: E402
from voice_tts_amd import sharding  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=25)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(16)
    cfg = S2.S2MEL_CFG
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=1234), cfg, device=dev)
    g = torch.Generator().manual_seed(5)
    Tp = 430
    prompts = [(torch.randn(1, Tp, 512, generator=g).to(dev), (torch.randn(1, 80, Tp, generator=g) * 2 - 5).to(dev),
                torch.randn(1, 192, generator=g).to(dev)) for _ in range(4)]

    def item(n, p):
        return (torch.randn(1, n, 1280, generator=g).to(dev) * 0.3, torch.randint(0, 8192, (1, n), generator=g).to(dev)) + prompts[p]

    mixed = [11 * t for r in sharding.mixed_requests() for t in r][:16]
    shapes = {"a: 2 x 1100": [item(1100, 0), item(1100, 0)], "b: 4 x 150": [item(150, 0) for _ in range(4)],
              f"c: 16 mixed64 ({min(mixed)}-{max(mixed)} codes)": [item(n, i % 4) for i, n in enumerate(mixed)]}

    def frames(it):
        return Tp + int(it[1].shape[1] * 1.72)

    def per_segment(items, noises):
        return [m(it[0], it[1], torch.tensor([it[1].shape[1]], device=dev), *it[2:], n_timesteps=args.steps, noise=z) for it, z in zip(items, noises)]

    def packed(items, noises):
        return m.solve_many(items, n_timesteps=args.steps, noises=noises)

    def timed(fn, *a):
        fn(*a)  # warm: allocations, library kernel choice per shape
        torch.cuda.synchronize()
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = fn(*a)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        return best, out

    print(f"budget IXTTS_S2MEL_BATCH_FRAMES = {os.environ.get('IXTTS_S2MEL_BATCH_FRAMES', S2.S2MEL_BATCH_FRAMES)}; {args.steps} steps; best of {args.reps}")
    for name, items in shapes.items():
        noises = [torch.randn(1, 80, frames(it), generator=g).to(dev) for it in items]
        F_ = sum(frames(it) for it in items)
        t_seg, ref = timed(per_segment, items, noises)
        t_pk, out = timed(packed, items, noises)
        err = max(float((o - r).abs().max()) / max(1.0, float(r.abs().max())) for o, r in zip(out, ref))
        print(f"({name}) {len(items)} segments, {F_} frames: per-segment {t_seg * 1e3:8.1f} ms ({t_seg * 1e6 / F_:6.1f} us/frame), "
              f"packed {t_pk * 1e3:8.1f} ms ({t_pk * 1e6 / F_:6.1f} us/frame), x{t_seg / t_pk:.2f}; max rel diff {err:.1e}", flush=True)

    # HIP launches per Euler step: torch's library GEMMs / element kernels excluded, the HIP entries of this package counted
    log = []
    real_call, real_attn, real_attn1, real_pair, real_split, real_lin = S2._hip_call, S2.attn_full_packed, S2.attn_full, G.pair_linear, G.split, G.linear
    S2._hip_call = lambda *a: (log.append(a[0]), real_call(*a))[1]
    S2.attn_full_packed = lambda *a, **k: (log.append("attn"), real_attn(*a, **k))[1]
    S2.attn_full = lambda *a, **k: (log.append("attn"), real_attn1(*a, **k))[1]
    G.pair_linear = lambda *a, **k: (log.append("pair"), real_pair(*a, **k))[1]
    G.split = lambda *a, **k: (log.append("split"), real_split(*a, **k))[1]
    items = shapes["b: 4 x 150"]
    noises = [torch.randn(1, 80, frames(it), generator=g).to(dev) for it in items]
    counts = {}
    for steps in (1, 2):
        log.clear()
        m(items[0][0], items[0][1], torch.tensor([150], device=dev), *items[0][2:], n_timesteps=steps, noise=noises[0])
        counts[("one segment", steps)] = len(log)
        for n in (1, 4):
            log.clear()
            m.solve_many(items[:n], n_timesteps=steps, noises=noises[:n])
            counts[(f"packed x{n}", steps)] = len(log)
    S2._hip_call, S2.attn_full_packed, S2.attn_full, G.pair_linear, G.split = real_call, real_attn, real_attn1, real_pair, real_split
    for k in ("one segment", "packed x1", "packed x4"):
        print(f"HIP entry calls per Euler step, {k}: {counts[(k, 2)] - counts[(k, 1)]}")

    # the attention alone: varlen (no key-range split) against the per-segment entry (which splits the key range when its grid is small)
    H = cfg["num_heads"]
    for lens in ([2322, 2322], [2322] * 4, [688] * 8, [688] * 2):
        pk = S2.RowPack(lens, dev)
        qkv = torch.randn(pk.rows, 3, H, 64, device=dev)
        q, k, v = qkv[:, 0], qkv[:, 1], qkv[:, 2]

        def one():
            for s in range(0, pk.n, 2):  # what a per-segment step runs: the CFG pair of one segment as B = 2
                a, b = pk.off[s], pk.off[s + 2]
                T = lens[s]
                S2.attn_full(q[a:b].view(2, T, H, 64), k[a:b].view(2, T, H, 64), v[a:b].view(2, T, H, 64))

        def var():
            S2.attn_full_packed(q, k, v, pk)

        res = {}
        for nm, fn in (("per-segment (split)", one), ("varlen", var)):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            res[nm] = (time.perf_counter() - t0) / 20 * 1e6
        print(f"attention {len(lens)} x {lens[0]} rows x {H} heads: " + ", ".join(f"{k} {v:7.1f} us" for k, v in res.items()))


if __name__ == "__main__":
    main()
