#!/usr/bin/env python
"""Error budget of the HIP GPT (rows path and register decode path, tiny model): every case of tests/gpt_budget.py in f32, bf16 and f16 on
both weight sets, against the fp64 twin that rounds where the 16-bit kernels round, with the yardstick legs measured on the CPU beside
each device error, the limits derived from them, and the movement of every mutant of tests/test_gpt_twin.py relative to those limits.
Errors are [max |d| / max |twin|, rms(d) / rms(twin)].

    python tools/gpt_error_budget.py [--out profiles/gpt_error_budget.json] [--device cuda:0] [--cpu-only]

tests/test_gpu_gpt_fp64.py asserts the relation these numbers show (device <= 3 x yardstick on max, 2 x on rms); --cpu-only records the
yardsticks and the mutants without a device."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import torch

    import gpt_budget as GB

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gpt_error_budget.json"))
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--cpu-only", action="store_true")
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    dev = None if a.cpu_only else torch.device(a.device)
    doc = {"what": "GPT tiny model (D 128, 2 layers, 2 heads): error against the fp64 twin with the engine type's rounding sites, relative to the "
                   "twin's max and rms; [max, rms].  yardstick = the larger of fp32_cpu_leg and flip_leg; limit = 3 x max, 2 x rms (rms floor: "
                   "2 x the family's largest yardstick rms)",
           "device": torch.cuda.get_device_name(dev) if dev is not None else None, "torch": torch.__version__,
           "margins": {"max": GB.MAX_FACTOR, "rms": GB.RMS_FACTOR, "kappa": GB.KAPPA},
           "rounding_sites": {"rows": {k: sorted(v) for k, v in GB.ROWS_SITES.items()}, "register_decode": {k: sorted(v) for k, v in GB.REG_SITES.items()}},
           "types": {}}
    legacy = {}
    if dev is not None:  # IXTTS_ROWS_ATTN is read once per process: the legacy row attention runs in a child, as in the test
        import test_gpu_gpt_fp64 as T

        r = subprocess.run([sys.executable, "-c", T._LEGACY_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))],
                           env=dict(os.environ, IXTTS_ROWS_ATTN="legacy"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        for line in r.stdout.splitlines():
            if line.startswith("LEGACY "):
                run = json.loads(line[len("LEGACY "):])
                legacy[run["kind"], tuple(run["key"])] = run["got"]
    for kind in GB.KINDS:
        doc["types"][kind] = {}
        for wset in GB.WSETS:
            L = GB.legs(kind, wset)
            for fam in GB.FAMILIES:
                L.need(fam)
            device = {}
            if dev is not None:
                e1, e3, e4 = (GB.engine(kind, wset, b, dev) for b in (1, 3, 4))
                for n in GB.latent_counts(kind):
                    device["latent", n] = {"flash": GB.device_latent(e1, n)}
                for c in GB.PREFILL_CASES:
                    device["prefill", c] = {"flash": GB.device_prefill(e1, c)}
                for i, g in enumerate(GB.device_packed_latent(e4)):
                    device["packed_latent", i] = {"flash": g}
                for i, g in enumerate(GB.device_packed_prefill(e4)):
                    device["packed_prefill", i] = {"flash": g}
                for slots, eng in ((1, e1), (3, e3)):
                    for (b, step), g in GB.device_decode(eng, slots).items():
                        device.setdefault(("decode", b, step), {})[f"{slots} slot engine"] = g
                if wset == "sharp":
                    for (k, key), got in legacy.items():
                        if k == kind:
                            device[key]["legacy rows attention"] = torch.tensor(got, dtype=torch.float64).view(L.ref[key].shape)
            cases, worst = {}, [0.0, 0.0]
            for key in L.ref:
                if key[0] == "mutants":
                    continue
                row = {"fp32_cpu_leg": list(L.leg32[key]), "flip_leg": list(L.flip[key]) if key in L.flip else None, "yardstick": list(L.base[key]),
                       "limit": list(L.limits(key)), "twin_peak": L.ref[key].abs().max().item(), "device": {}}
                for path, got in device.get(key, {}).items():
                    err = GB.rel_err(got, L.ref[key])
                    ratio = [err[i] / row["limit"][i] for i in range(2)]
                    row["device"][path] = {"error": list(err), "ratio_to_limit": ratio}
                    worst = [max(worst[i], ratio[i]) for i in range(2)]
                cases[" ".join(str(k) for k in key)] = row
            mutants = {}
            for m in GB.MUTANTS:
                if m == "no_rescale" and wset != "sharp":
                    continue
                for key, got in L.mutant(m).items():
                    if m == "pad_visible" and key[1] == "latent":
                        continue
                    moved = GB.rel_err(got, L.ref[key])
                    mutants.setdefault(m, {})[key[1]] = {"moved": list(moved), "ratio_to_max_limit": moved[0] / L.limits(key)[0]}
            doc["types"][kind][wset] = {"worst_device_ratio_to_limit": worst, "roundings_flipped_in_flip_leg": L.n_flipped, "cases": cases,
                                        "mutants": mutants}
            print(kind, wset, "worst device / limit", worst, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
