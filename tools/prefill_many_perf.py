"""A refill of N decode slots two ways on one engine, at production width (model_dim 1280, 24 layers, synthetic weights):
N x `prefill` (one sequence per pass over the weights) against one `prefill_many` (one packed pass, cut by max_seq rows).

    python tools/prefill_many_perf.py [--dtypes bf16,f16,f32] [--out profiles/prefill_many.json] [--tag run1]

Two row mixes: every prompt of 137 rows (bench.py's prompt), and the prompt lengths of the first N segments of the `mixed64`
list (sharding.mixed_requests: 34 conditioning rows + tokens + 2).  The two ways alternate in one process, every shape is warmed
up first, a window is REPS refills between two device events (tens of milliseconds at the least), and each figure is the median
of WINDOWS windows with their min and max beside it.  Run the same command twice (--tag) for the run-to-run spread; a second
run appends to the same file.  The first-step logits of both ways are compared bit for bit on the way."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import voice_tts_amd.weights as WR
from voice_tts_amd import sharding
from voice_tts_amd.gpt_engine import GptEngine

ap = argparse.ArgumentParser()
ap.add_argument("--dtypes", default="bf16,f16,f32")
ap.add_argument("--max-seq", type=int, default=2048)  # infer_v2's default: what cuts a production refill into passes
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--out", default=None)
ap.add_argument("--tag", default="run")
args = ap.parse_args()
dev = torch.device("cuda:0")
W = WR.make_gpt_weights(WR.GPT_CFG, seed=1234)
g = torch.Generator().manual_seed(5)
mixed_rows = [34 + n + 2 for toks in sharding.mixed_requests() for n in toks]
res = dict(tag=args.tag, max_seq=args.max_seq, windows=args.windows, reps=args.reps, rows=[])


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


for dt in args.dtypes.split(","):
    slots = 16 if dt == "f32" else 32
    eng = GptEngine(WR.GPT_CFG, dtype=dt, max_seq=args.max_seq, max_batch=slots, device=dev).load_state_dict(W)
    for mix in ("all137", "mixed64"):
        for N in (2, 4, 8, 16, 32):
            if N > slots:
                continue
            rows = [136] * N if mix == "all137" else mixed_rows[:N]
            entries = [(b, (torch.randn(r, 1280, generator=g) * 0.5).to(dev), 0) for b, r in enumerate(rows)]
            serial = lambda: [eng.prefill(b, e, p) for b, e, p in entries]
            batch = lambda: eng.prefill_many(entries)
            serial()
            want = [eng.read_logits(b).copy() for b in range(N)]
            batch()
            same = all(np.array_equal(eng.read_logits(b), want[b]) for b in range(N))
            t = dict(serial=[], batch=[])
            for _ in range(args.windows):  # alternating
                t["serial"].append(window(serial))
                t["batch"].append(window(batch))
            row = dict(dtype=dt, mix=mix, slots=N, packed_rows=sum(r + 1 for r in rows),
                       passes=GptEngine.prefill_plan(rows, [0] * N, args.max_seq)[1], bit_equal=bool(same))
            for k, v in t.items():
                row[f"{k}_ms"] = round(statistics.median(v), 3)
                row[f"{k}_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
            row["batch_over_serial"] = round(row["batch_ms"] / row["serial_ms"], 4)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    del eng
    torch.cuda.empty_cache()
if args.out:
    runs = json.load(open(args.out)) if os.path.exists(args.out) else []
    json.dump(runs + [res], open(args.out, "w"), indent=1)
