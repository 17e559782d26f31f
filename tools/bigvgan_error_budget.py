#!/usr/bin/env python
"""Error budget of the HIP BigVGAN: every case of tests/bigvgan_budget.py, in both conv arithmetic modes (default split-product bf16,
IXTTS_BV_CONV=f32), with the launcher's own tile choice and with every scored tile forced (IXTTS_BV_TILE), against the fp64 twin
(`oracle.vocoder.bigvgan_forward(..., dtype=torch.float64)`), with the fp32 CPU oracle's error on the same inputs beside it.  Errors are
(max |d| / max |twin|, rms(d) / rms(twin)); `launches` are the conv launches of the run by tile shape (`BigVGAN.tile_launches()`).
(An output element is one lane's accumulator over the same sequence of products in whatever tile it falls, so the forced runs of a case
show the same numbers as its first run: `bit_identical_to_by_score`.)

    python tools/bigvgan_error_budget.py [--out profiles/bigvgan_error_budget.json] [--device cuda:0]

tests/test_gpu_bigvgan_fp64.py asserts the relation these numbers show (device <= 3 x CPU leg on max, 2 x on rms)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch

    import bigvgan_budget as BB

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigvgan_error_budget.json"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = torch.device(a.device)
    legs = BB.Legs()
    doc = {"what": "BigVGAN (1-stage production-width handles): error against the fp64 twin, relative to the twin's max and rms; [max, rms]",
           "device": torch.cuda.get_device_name(dev), "torch": torch.__version__, "cases": BB.CASES,
           "margins": {"max": BB.MAX_FACTOR, "rms": BB.RMS_FACTOR, "rms_floor": BB.RMS_FLOOR}, "modes": {}}
    for mode in BB.MODES:
        cases, worst = {}, [0.0, 0.0]
        for c in BB.CASES:
            row = {"fp32_cpu_leg": list(legs.base[c]), "twin_peak": legs.ref[c].abs().max().item(), "runs": {}}
            for tile in (None,) + (BB.TILES[mode] if c in BB.FORCED[mode] else ()):
                err, launches, wav = legs.device(c, mode, tile, dev)
                first = wav if tile is None else first
                ratio = [err[i] / legs.base[c][i] for i in range(2)]
                row["runs"][tile or "by score"] = {"device": list(err), "ratio_to_cpu_leg": ratio, "launches": launches,
                                                   "bit_identical_to_by_score": bool(torch.equal(wav, first))}
                worst = [max(worst[i], ratio[i]) for i in range(2)]
            cases[c] = row
            print(mode, c, json.dumps(row), flush=True)
        doc["modes"][mode] = {"worst_ratio_to_cpu_leg": worst, "cases": cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
