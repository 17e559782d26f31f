"""The true peak and the limiter of the output stage against the call they extend -- `output.finish_pcm(...,
loudness=-23.0)`, the levelled path of 4.3c -- and against the vocoder pass that feeds the stage, at production width (BIGVGAN_CFG,
synthetic weights), on the two shapes and the two formats of tools/output_stage_perf.py:
  (a) the headline request's 2 x 1892 frames;  (b) one 150-code segment, 258 frames;  48 000 Hz pcm_s16le and 8 000 Hz mu-law.
Forms per format: loudness alone; + true mode; + limiter; + limiter and true mode (the full chain: true peaks, limiter, second
measurement); and the full chain at a target of -5 LUFS, louder than the synthetic vocoder's output, where the limiter has work to
do in most tiles (at -23 LUFS a tile without a sample over the ceiling copies its samples).  Every form reports the share of
samples the limiter reduced.  The forms
alternate inside one process, every window repeats its form until it is `--window` seconds long and ends in a device synchronise
(the stage ends in its copy to the host, which waits), and a form is reported as the median of `--rounds` windows with min .. max.

    python tools/limiter_perf.py [--rounds 5] [--window 0.4] [--out profiles/limiter.json]
    python tools/limiter_perf.py --stage-only 20      # 20 calls per form and shape, nothing else: the run to put under a kernel trace
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
TARGET, HOT = -23.0, -5.0  # LUFS
CONTROLS = {
    "loudness alone": dict(loudness=TARGET),
    "+ true mode": dict(loudness=TARGET, peak_mode="true"),
    "+ limiter": dict(loudness=TARGET, limiter=True),
    "+ limiter, true mode": dict(loudness=TARGET, limiter=True, peak_mode="true"),
    "+ limiter, true mode, %g LUFS" % HOT: dict(loudness=HOT, limiter=True, peak_mode="true"),
}
BASE = "loudness alone"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--stage-only", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "limiter.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "limiter_perf needs a GPU"
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
        forms, reports = {"vocoder": lambda: vocode_many(m, mels)}, {}
        for k, (sr, enc) in FORMATS.items():
            for c, kw in CONTROLS.items():
                forms[k + ", " + c] = lambda sr=sr, enc=enc, kw=kw: O.finish_pcm(wavs, sr, enc, 200, **kw)
                rep = []
                O.finish_pcm(wavs, sr, enc, 200, reports=rep, **kw)
                reports[k + ", " + c] = rep[0]
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
        row = dict(shape=name, frames=frames, samples_in=sum(w.shape[1] for w in wavs), rounds=args.rounds, window_s=args.window, forms={})
        voc = statistics.median(times["vocoder"])
        for k, ts in times.items():
            med = statistics.median(ts)
            row["forms"][k] = dict(median_ms=round(med, 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))
            note = ""
            if k != "vocoder":
                fmt = k.split(", ")[0]
                sr = FORMATS[fmt][0]
                rep = reports[k]
                row["forms"][k].update(samples_out=sum(O.resampled_len(w.shape[1], 22050, sr) for w in wavs) + O.gap_len(sr) * (len(wavs) - 1),
                                       share_of_vocoder=round(med / voc, 4), over_loudness_alone_ms=round(med - statistics.median(times[fmt + ", " + BASE]), 4),
                                       limited_fraction=rep.get("limited_fraction"), gain_db=round(rep["gain_db"], 3), target_met=rep["target_met"])
                note = f"  {100 * med / voc:5.2f} % of the vocoder pass, limited {rep.get('limited_fraction')}"
            print(f"({name}) {k:52s}: median {med:8.3f} ms  [{min(ts):8.3f} .. {max(ts):8.3f}]" + note, flush=True)
        results.append(row)
    if args.stage_only:
        return
    doc = dict(tool="tools/limiter_perf.py", device=torch.cuda.get_device_name(0), config="BIGVGAN_CFG, synthetic weights",
               method="forms alternate in one process; a window repeats one form for about window_s seconds and ends in a device "
                      "synchronise (the output stage: in its copy to the host); median / min / max over the rounds; the vocoder is "
                      "pipeline.vocode_many on the same mels; 'loudness alone' is the call of DESIGN 4.3c, which this work leaves as it was",
               shapes=results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
