"""The HIP GPT -- rows path (gpt_rows.hip: prefill, latent pass, their packed forms, flash and legacy row attention) and register decode
path (1..4 slots) -- against the fp64 twin of tests/gpt_budget.py, as an error budget, in f32, bf16 and f16 on two weight sets.

The twin rounds where the 16-bit kernels round (the site tables of gpt_budget.py), so what is left between a device result and the twin
is the arithmetic's noise: the fp32 summation order and the 16-bit roundings that fall the other way.  The yardstick is that noise
measured on the CPU (the fp32 leg and, in the 16-bit types, the flip leg); the criterion is the one of test_gpu_s2mel_fp64.py and
test_gpu_bigvgan_fp64.py: a device path may sit at most 3 x (max) and 2 x (rms) above the yardstick.  Every run prints its error beside
its yardstick.  tests/test_gpt_twin.py shows on the CPU which structural errors these limits catch; tools/gpt_error_budget.py records
the numbers in profiles/gpt_error_budget.json.

The wide engines (5..32 slots) and the beam kernels are not covered: their rounding sites need a table of their own."""
import json
import os
import subprocess
import sys

import pytest
import torch

import gpt_budget as GB

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(k, w) for k in GB.KINDS for w in GB.WSETS]
IDS = [f"{k}-{w}" for k, w in COMBOS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------- 3a. latent pass, all rows
LATENT_RUNS = [(k, w, n) for k, w in COMBOS for n in GB.latent_counts(k)]


@pytest.mark.parametrize("kind,wset,n", LATENT_RUNS, ids=[f"{k}-{w}-T{GB.LATENT_PREFIX + n}" for k, w, n in LATENT_RUNS])
def test_latent_pass_within_the_budget(dev, kind, wset, n):
    """`GptEngine.latent` of n codes behind a 7-row prefix: the device's T = 7 + n rows (and the reference's 7 + n + 2) on every tile edge."""
    got = GB.device_latent(GB.engine(kind, wset, 1, dev), n)
    GB.within(f"latent T {GB.LATENT_PREFIX + n}", GB.legs(kind, wset), ("latent", n), got)


# ------------------------------------------------------------------------------------------------------- 3b. prefill, then head
PREFILL_RUNS = [(k, w, c) for k, w in COMBOS for c in GB.PREFILL_CASES]


@pytest.mark.parametrize("kind,wset,case", PREFILL_RUNS, ids=[f"{k}-{w}-{c}" for k, w, c in PREFILL_RUNS])
def test_prefill_logits_within_the_budget(dev, kind, wset, case):
    got = GB.device_prefill(GB.engine(kind, wset, 1, dev), case)
    GB.within(f"prefill {case}", GB.legs(kind, wset), ("prefill", case), got)


# ------------------------------------------------------------------------------------------------------- 3c. packed passes
@pytest.mark.parametrize("kind,wset", COMBOS, ids=IDS)
def test_latent_many_each_sequence_within_the_budget(dev, kind, wset):
    from voice_tts_amd.gpt_engine import GptEngine

    rows = [p + n for p, n in GB.PACKED_LATENT]
    assert GptEngine.latent_plan([p for p, _ in GB.PACKED_LATENT], [n for _, n in GB.PACKED_LATENT], GB.MAX_SEQ)[1] == 1  # one packed pass
    assert any(sum(rows[:i]) % 128 for i in range(1, len(rows))) and max(rows) > 128
    got = GB.device_packed_latent(GB.engine(kind, wset, 4, dev))
    for i, g in enumerate(got):
        GB.within(f"latent_many seq {i} ({rows[i]} rows)", GB.legs(kind, wset), ("packed_latent", i), g)


@pytest.mark.parametrize("kind,wset", COMBOS, ids=IDS)
def test_prefill_many_each_sequence_within_the_budget(dev, kind, wset):
    from voice_tts_amd.gpt_engine import GptEngine

    assert GptEngine.prefill_plan([p + v for p, v in GB.PACKED_PREFILL], [p for p, _ in GB.PACKED_PREFILL], GB.MAX_SEQ)[1] == 1
    got = GB.device_packed_prefill(GB.engine(kind, wset, 4, dev))
    for i, g in enumerate(got):
        GB.within(f"prefill_many seq {i} (pad {GB.PACKED_PREFILL[i][0]}, {GB.PACKED_PREFILL[i][1] + 1} rows)", GB.legs(kind, wset), ("packed_prefill", i), g)


# ------------------------------------------------------------------------------------------------------- 3d. legacy row attention
_LEGACY_CHILD = r"""
import json, sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import gpt_budget as GB
dev = torch.device("cuda:0")
for kind in GB.KINDS:
    eng = GB.engine(kind, "sharp", 1, dev)
    for n in GB.LEGACY_LATENT:
        print("LEGACY " + json.dumps(dict(kind=kind, key=["latent", n], got=GB.device_latent(eng, n).double().flatten().tolist())), flush=True)
    got = GB.device_prefill(eng, GB.LEGACY_PREFILL)
    print("LEGACY " + json.dumps(dict(kind=kind, key=["prefill", GB.LEGACY_PREFILL], got=got.double().flatten().tolist())), flush=True)
"""


def test_legacy_row_attention_within_the_budget_in_a_child_process():
    """IXTTS_ROWS_ATTN is read once per process: a fresh child, the variable in ITS environment, runs the T = 129 latent cases and the
    65-row-pad prefill in the three types on the sharp set (attn_rows_kernel through attn_sweep / attn_merge); the parent holds what the
    child printed to the twin."""
    env = dict(os.environ, IXTTS_ROWS_ATTN="legacy")
    r = subprocess.run([sys.executable, "-c", _LEGACY_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    runs = [json.loads(line[len("LEGACY "):]) for line in r.stdout.splitlines() if line.startswith("LEGACY ")]
    assert len(runs) == len(GB.KINDS) * (len(GB.LEGACY_LATENT) + 1), r.stdout[-2000:] + r.stderr[-2000:]
    for run in runs:
        L, key = GB.legs(run["kind"], "sharp"), tuple(run["key"])
        L.need(key[0])
        got = torch.tensor(run["got"], dtype=torch.float64).view(L.ref[key].shape)
        GB.within(f"legacy rows attention {key[0]} {key[1]}", L, key, got)


# ------------------------------------------------------------------------------------------------------- 3e. register decode
@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("kind,wset", COMBOS, ids=IDS)
def test_teacher_forced_decode_within_the_budget(dev, kind, wset, slots):
    """Prompts of 200 (150, 9) rows, then 60 forced tokens through the register GEMVs and the split-S attention; with the 200-row prompt
    the context crosses the 256-key bucket at step 55.  The logits before the steps 0, 1, 54, 55, 56 and 59 against the twin's
    `decode_step` over the cache the twin's prefill left (rows-path sites for the prompt, register-path sites for the steps)."""
    got = GB.device_decode(GB.engine(kind, wset, slots, dev), slots)
    assert sorted(got) == [(b, s) for b in range(slots) for s in GB.DECODE_CHECK]
    for (b, step), logits in sorted(got.items()):
        GB.within(f"decode {slots} slot(s), slot {b} step {step}", GB.legs(kind, wset), ("decode", b, step), logits)
