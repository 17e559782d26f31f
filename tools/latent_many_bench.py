"""The latent forward of N segments two ways on one engine, at production width (model_dim 1280, 24 layers, synthetic weights):
the loop of `latent` calls (one pass over the weights per segment) against one `latent_many` (packed passes, cut by max_seq cache
positions).

    python tools/latent_many_bench.py [--dtypes bf16,f32] [--out profiles/latent_many.json] [--tag run1] [--serial-only] [--mixed64]

Shapes: 8 x (80 prefix + 150 codes), 32 x the same, the first 16 segments of the `mixed64` list (sharding.mixed_requests: 34
conditioning rows + n tokens + 2, then 11 n codes), and 2 x (137 + 1100), which cannot pack at max_seq 2048 and must not get slower.
The two ways alternate in one process, every shape is warmed up first, a window is REPS rounds between two device events, and each
figure is the median of WINDOWS windows with their min and max beside it.  Run the same command twice (--tag) for the run-to-run
spread; a second run appends to the same file.  The latents of both ways are compared bit for bit on the way.

--serial-only times the loop alone and needs nothing this file's commit added: it runs on the parent commit, whose figures are the
baseline of the record.  --mixed64 runs the latent stage of the WHOLE mixed64 list (143 segments, what `infer_many` hands to the
latent pass after decode) both ways, each way first once: the wall time the IXTTS_LATENT_BATCH switch moves."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import voice_tts_amd.weights as WR
from voice_tts_amd import sharding
from voice_tts_amd.gpt_engine import GptEngine

ap = argparse.ArgumentParser()
ap.add_argument("--dtypes", default="bf16,f32")
ap.add_argument("--max-seq", type=int, default=2048)  # infer_v2's default: what cuts a call into passes
ap.add_argument("--windows", type=int, default=5)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--out", default=None)
ap.add_argument("--tag", default="run")
ap.add_argument("--serial-only", action="store_true")
ap.add_argument("--mixed64", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
W = WR.make_gpt_weights(WR.GPT_CFG, seed=1234)
g = torch.Generator().manual_seed(5)
mixed = [(34 + n + 2, 11 * n) for toks in sharding.mixed_requests() for n in toks]
SHAPES = [("8x(80+150)", [(80, 150)] * 8), ("32x(80+150)", [(80, 150)] * 32), ("mixed16", mixed[:16]), ("2x(137+1100)", [(137, 1100)] * 2)]
res = dict(tag=args.tag, max_seq=args.max_seq, windows=args.windows, reps=args.reps, serial_only=args.serial_only, rows=[])


def entries_of(shape):
    return [((torch.randn(P, 1280, generator=g) * 0.5).to(dev), torch.randint(0, 8192, (n,), generator=g, dtype=torch.int32).to(dev)) for P, n in shape]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def plan_of(shape):
    return GptEngine.latent_plan([P for P, _ in shape], [n for _, n in shape], args.max_seq)[1]


for dt in args.dtypes.split(","):
    eng = GptEngine(WR.GPT_CFG, dtype=dt, max_seq=args.max_seq, max_batch=3, device=dev).load_state_dict(W)  # IndexTTS2.gpt's shape
    if args.mixed64:
        entries = entries_of(mixed)
        serial = lambda: [eng.latent(p, c) for p, c in entries]
        batch = lambda: eng.latent_many(entries)
        serial(), batch()  # warm-up
        torch.cuda.synchronize()
        for first in ("serial", "batch"):
            walls = {}
            for way in ([first] + [w for w in ("serial", "batch") if w != first]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                (serial if way == "serial" else batch)()
                torch.cuda.synchronize()
                walls[way] = round(time.perf_counter() - t0, 4)
            row = dict(dtype=dt, shape="mixed64 latent stage", segments=len(mixed), rows=sum(P + n for P, n in mixed), passes=plan_of(mixed), first=first,
                       serial_wall_s=walls["serial"], batch_wall_s=walls["batch"], batch_over_serial=round(walls["batch"] / walls["serial"], 4))
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    else:
        for name, shape in SHAPES:
            entries = entries_of(shape)
            serial = lambda: [eng.latent(p, c) for p, c in entries]
            want = [t.clone() for t in serial()]
            row = dict(dtype=dt, shape=name, segments=len(shape), rows=sum(P + n for P, n in shape))
            t = dict(serial=[])
            if not args.serial_only:
                batch = lambda: eng.latent_many(entries)
                row["passes"] = plan_of(shape)
                row["bit_equal"] = all(torch.equal(a, b) for a, b in zip(batch(), want))
                t["batch"] = []
            for _ in range(args.windows):  # alternating
                t["serial"].append(window(serial, args.reps))
                if not args.serial_only:
                    t["batch"].append(window(batch, args.reps))
            for k, v in t.items():
                row[f"{k}_ms"] = round(statistics.median(v), 3)
                row[f"{k}_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
            if not args.serial_only:
                row["batch_over_serial"] = round(row["batch_ms"] / row["serial_ms"], 4)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    del eng
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    runs = json.load(open(args.out)) if os.path.exists(args.out) else []
    json.dump(runs + [res], open(args.out, "w"), indent=1)
