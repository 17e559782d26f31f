"""Decode step time per batch, greedy, context ~300-700: us/step.

    python tools/step_perf.py [--dtype {bf16,f16,f32}]... [--repeat N] [B ...]

B = 1..4 run on the register GEMVs, 5..16 (5..32 for bf16 / f16) on the wide (matrix-core) engine.  With no argument: bf16, B = 2 and 3, one line
per B.  `--dtype` may be given several times: the engines of one B are then timed ALTERNATELY, `--repeat N` rounds of 800
steps each, every round printed (an A/B in one process, same clocks, same neighbours)."""
import argparse, sys, time, torch
sys.path.insert(0, ".")
import voice_tts_amd.weights as WR
from voice_tts_amd.gpt_engine import GptEngine
ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=["bf16", "f16", "f32"], action="append")
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("batches", nargs="*", type=int, default=[2, 3])
args = ap.parse_args()
dtypes = args.dtype or ["bf16"]
plain = dtypes == ["bf16"] and args.repeat == 1  # today's output, unchanged
dev = torch.device("cuda:0")
W = WR.make_gpt_weights(WR.GPT_CFG, seed=1234)
emb = torch.randn(136, 1280, generator=torch.Generator().manual_seed(1)) * 0.5
for B in args.batches:
    engines = {dt: GptEngine(WR.GPT_CFG, dtype=dt, max_seq=2048, max_batch=B, device=dev).load_state_dict(W) for dt in dtypes}
    for r in range(args.repeat):
        for dt, eng in engines.items():
            for b in range(B):
                eng.prefill(b, emb, 0)
            eng.decode(B, 64, suppress_stop=True)
            torch.cuda.synchronize(); t0 = time.time()
            eng.decode(B, 800, suppress_stop=True)
            torch.cuda.synchronize()
            print(f"{'' if plain else dt + ' '}B={B}{'' if plain else f' round {r}'}: {(time.time()-t0)/800*1e6:.1f} us/step", flush=True)
    del engines
