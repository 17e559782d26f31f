"""The output stage (`output.finish_pcm`: resample, convert, lay out, ONE copy to the host) against the vocoder pass that feeds it, at
production width (BIGVGAN_CFG, synthetic weights), on two shapes:
  (a) the headline request's 2 x 1892 frames;  (b) one 150-code segment, 258 frames
and two formats: 48 000 Hz pcm_s16le and 8 000 Hz mu-law, each without and with a loudness target (`loudness=-23.0`: the measurement
and gating launches of DESIGN.md 4.3c before the conversion).  The forms alternate inside one process, every window repeats its form
until it is `--window` seconds long and ends in a device synchronise (the output stage ends in its copy to the host, which waits),
and a form is reported as the median of `--rounds` windows with their min .. max.  The vocoder is `pipeline.vocode_many` on the
same mels, which this stage leaves as it was.

    python tools/output_stage_perf.py [--rounds 5] [--window 0.4] [--out profiles/output_stage.json]
    python tools/output_stage_perf.py --stage-only 20      # 20 calls per format and shape, nothing else: the run to put under a kernel trace
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
from voice_tts_amd import output as O  # noqa: E402
from voice_tts_amd.bigvgan import BigVGAN  # noqa: E402
from voice_tts_amd.pipeline import vocode_many  # noqa: E402

SHAPES = {"a: 2 x 1892 frames": [1892, 1892], "b: 1 x 258 frames": [258]}
FORMATS = {"48000 pcm_s16le": (48000, "pcm_s16le"), "8000 mulaw": (8000, "mulaw")}
TARGET = -23.0  # LUFS, the loudness column
LEVELLED = ", %g LUFS" % TARGET


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--stage-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "output_stage.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "output_stage_perf needs a GPU"
    dev = torch.device("cuda:0")
    cfg = dict(WR.BIGVGAN_CFG)
    m = BigVGAN(cfg, max_frames=2048, device=dev).load_state_dict(WR.make_bigvgan_weights(cfg, seed=8))
    g = torch.Generator().manual_seed(5)

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        n = max(2, int(args.window / max(time.perf_counter() - t0, 1e-6)))
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    results = []
    for name, frames in SHAPES.items():
        mels = [(torch.randn(1, 80, f, generator=g) * 2 - 4).clamp(-11.5, 2).to(dev) for f in frames]
        wavs = vocode_many(m, mels)
        assert all(isinstance(w, torch.Tensor) for w in wavs)
        forms = {"vocoder": lambda: vocode_many(m, mels)}
        for k, (sr, enc) in FORMATS.items():
            forms["output stage " + k] = lambda sr=sr, enc=enc: O.finish_pcm(wavs, sr, enc, 200)
        for k, (sr, enc) in FORMATS.items():
            forms["output stage " + k + LEVELLED] = lambda sr=sr, enc=enc: O.finish_pcm(wavs, sr, enc, 200, loudness=TARGET)
        if args.stage_only:
            for k, fn in forms.items():
                if k != "vocoder":
                    for _ in range(args.stage_only):
                        fn()
            torch.cuda.synchronize()
            continue
        for fn in forms.values():  # warm every form: code objects, tap tables, pinned and device allocations
            fn()
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in forms}
        for _ in range(args.rounds):  # alternate the forms: a drift of the machine lands on all of them
            for k, fn in forms.items():
                times[k].append(window(fn) * 1e3)
        samples = sum(w.shape[1] for w in wavs)
        row = dict(shape=name, frames=frames, samples_in=samples, rounds=args.rounds, window_s=args.window, forms={})
        voc = statistics.median(times["vocoder"])
        for k, ts in times.items():
            med = statistics.median(ts)
            row["forms"][k] = dict(median_ms=round(med, 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))
            if k != "vocoder":
                sr, enc = FORMATS[k[len("output stage "):].replace(LEVELLED, "")]
                out_samples = sum(O.resampled_len(w.shape[1], 22050, sr) for w in wavs) + O.gap_len(sr) * (len(wavs) - 1)
                row["forms"][k].update(samples_out=out_samples, share_of_vocoder=round(med / voc, 4))
                if k.endswith(LEVELLED):
                    row["forms"][k].update(over_plain_ms=round(med - statistics.median(times[k[:-len(LEVELLED)]]), 4))
            print(f"({name}) {k:41s}: median {med:8.3f} ms  [{min(ts):8.3f} .. {max(ts):8.3f}]"
                  + (f"  {100 * med / voc:5.2f} % of the vocoder pass" if k != "vocoder" else ""), flush=True)
        results.append(row)
    if args.stage_only:
        return
    doc = dict(tool="tools/output_stage_perf.py", device=torch.cuda.get_device_name(0), config="BIGVGAN_CFG, synthetic weights",
               method="forms alternate in one process; a window repeats one form for about window_s seconds and ends in a device "
                      "synchronise (the output stage: in its copy to the host); median / min / max over the rounds; the vocoder is "
                      "pipeline.vocode_many on the same mels",
               shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
