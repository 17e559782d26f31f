#!/usr/bin/env python
"""Error budget of the s2mel DiT's device paths: every case of tests/s2mel_budget.py, in every arithmetic mode (default,
IXTTS_S2MEL_GEMM=library, IXTTS_ATTN_FULL=f32), against the fp64 twin (`S2Mel(..., dtype=torch.float64)`), with the fp32 CPU leg's
error on the same inputs beside it.  Errors are (max |d| / max |twin|, rms(d) / rms(twin)).

    python tools/s2mel_error_budget.py [--out profiles/s2mel_error_budget.json] [--device cuda:0]

tests/test_gpu_s2mel_fp64.py asserts the relation these numbers show (device <= 3 x CPU leg on max, 2 x on rms)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch

    import s2mel_budget as SB

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2mel_error_budget.json"))
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    doc = {"what": "s2mel DiT: error against the fp64 twin, relative to the twin's max and rms; [max, rms]",
           "device": torch.cuda.get_device_name(torch.device(a.device)), "torch": torch.__version__,
           "shapes": {"T": SB.T, "Tp": SB.TP, "pack": SB.PACK, "t": SB.T_EVAL, "steps": SB.STEPS, "cfg_rate": SB.CFG_RATE},
           "margins": {"max": 3.0, "rms": 2.0, "rms_floor": 2e-7}, "configs": {}}
    for name in SB.CONFIGS:
        legs = SB.Legs(name, torch.device(a.device))
        cases = {}
        for c in SB.CASES:
            row = {"fp32_cpu_leg": list(legs.base[c])}
            for m in SB.MODES:
                row[m] = list(legs.device(c, m))
            row["worst_ratio_to_cpu_leg"] = [max(row[m][i] / row["fp32_cpu_leg"][i] for m in SB.MODES) for i in range(2)]
            cases[c] = row
            print(name, c, json.dumps(row), flush=True)
        doc["configs"][name] = cases
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
