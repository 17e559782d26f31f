"""One batched vocoder pass (`BigVGAN.forward_many`) against the loop of `forward` calls on the same rows (what `infer_many` ran
before), at production width (BIGVGAN_CFG, synthetic weights), on three shapes:
  (a) 16 x 258 frames (150-code segments);  (b) 8 rows of mixed length, 86 .. 1892 frames;  (c) the headline's 2 x 1892 frames.
The two forms alternate inside one process, every window repeats its form until it is `--window` seconds long, and a shape is
reported as the median of `--rounds` windows with their min .. max (the run-to-run spread a difference has to exceed).  The batch
runs under each `--caps` value of IXTTS_BV_BATCH_FRAMES; every result is compared bit for bit with the loop's.

    python tools/bv_batch_perf.py [--rounds 5] [--window 0.4] [--caps 2048,4096,8192] [--out profiles/bv_batch_perf.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import voice_tts_amd.weights as WR  # noqa: E402
from voice_tts_amd.bigvgan import BigVGAN, plan_vocoder_batches  # noqa: E402

SHAPES = {
    "a: 16 x 258": [258] * 16,
    "b: 8 mixed 86-1892": [86, 129, 258, 344, 516, 860, 1204, 1892],
    "c: 2 x 1892": [1892, 1892],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--caps", default="2048,4096,8192")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bv_batch_perf.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bv_batch_perf needs a GPU"
    dev = torch.device("cuda:0")
    caps = [int(c) for c in args.caps.split(",")]
    cfg = dict(WR.BIGVGAN_CFG)
    m = BigVGAN(cfg, max_frames=2048, device=dev).load_state_dict(WR.make_bigvgan_weights(cfg, seed=8))
    g = torch.Generator().manual_seed(5)

    def loop(mels):
        return [m(x) for x in mels]

    def window(fn, mels):
        """calls per window fixed by a first timed call; -> seconds per call of `fn` over a window of about args.window seconds"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(mels)
        torch.cuda.synchronize()
        n = max(2, int(args.window / max(time.perf_counter() - t0, 1e-6)))
        t0 = time.perf_counter()
        for _ in range(n):
            fn(mels)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    results = []
    for name, frames in SHAPES.items():
        mels = [(torch.randn(1, 80, f, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev) for f in frames]
        forms = {"loop": loop}
        for cap in caps:
            def many(x, cap=cap):
                os.environ["IXTTS_BV_BATCH_FRAMES"] = str(cap)
                return m.forward_many(x)
            forms[f"batch cap {cap}"] = many
        ref = loop(mels)
        identical = {}
        for k, fn in forms.items():  # warm every form (workspace growth, code objects) and check its result
            out = fn(mels)
            identical[k] = all(torch.equal(a, b) for a, b in zip(out, ref))
            fn(mels)
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(args.rounds):  # alternate the forms: a drift of the machine lands on all of them
            for k, fn in forms.items():
                times[k].append(window(fn, mels) * 1e3)
        total = sum(frames)
        row = dict(shape=name, frames=frames, total_frames=total, rounds=args.rounds, window_s=args.window, forms={})
        for k, ts in times.items():
            cap = int(k.split()[-1]) if k != "loop" else None
            row["forms"][k] = dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3),
                                   ms_per_1000_frames=round(statistics.median(ts) * 1000 / total, 3), bit_identical_to_loop=identical[k],
                                   groups=[len(gr) for gr in plan_vocoder_batches(frames, cap)] if cap else None)
            print(f"({name}) {k:16s}: median {statistics.median(ts):8.2f} ms  [{min(ts):8.2f} .. {max(ts):8.2f}]  "
                  f"{statistics.median(ts) * 1000 / total:6.2f} ms / 1000 frames  x{statistics.median(times['loop']) / statistics.median(ts):.2f} vs loop  "
                  f"bit-identical {identical[k]}" + (f"  groups {row['forms'][k]['groups']}" if cap else ""), flush=True)
        results.append(row)
    os.environ.pop("IXTTS_BV_BATCH_FRAMES", None)
    doc = dict(tool="tools/bv_batch_perf.py", device=torch.cuda.get_device_name(0), config="BIGVGAN_CFG, synthetic weights, x3 convs",
               method="forms alternate in one process; a window repeats one form for about window_s seconds and ends in a device "
                      "synchronise; median / min / max over the rounds",
               shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
