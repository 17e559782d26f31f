"""Token agreement with the fp32 oracle at the benchmarked shape, per GPT weight type, side by side from one run.

    python tools/token_agreement.py [--dtype bf16 --dtype f16 ...] [--steps 1100] [--out FILE.json]

What tests/test_gpu_fullsize.py::test_bench_shape_bf16_1100_steps_vs_oracle computes, for every requested type: 24 x 1280, the
two benchmark prompts (137 rows; 117 rows with 3 left-padding rows) decoded together, free-running greedy for `steps` steps,
then ONE teacher-forced causal pass of the fp32 CPU oracle over the device's own ids per slot.  Reported per slot: the share of
steps at which the device token is the oracle's greedy choice, the largest logit error / logit scale over the read points, and
the number of disagreements that sit outside oracle near-ties (top-2 margin >= 1e-3 of the scale)."""
import argparse, json, sys, time
import numpy as np
import torch
sys.path.insert(0, ".")
import voice_tts_amd.weights as WR
from oracle import gpt as OG
from voice_tts_amd.gpt_engine import GptEngine

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=["bf16", "f16", "f32"], action="append")
ap.add_argument("--steps", type=int, default=1100)
ap.add_argument("--out", default=None)
args = ap.parse_args()
dtypes = args.dtype or ["bf16", "f16"]
N = args.steps
dev = torch.device("cuda:0")
W = WR.make_gpt_weights(WR.GPT_CFG, seed=1234)
orc = OG.GptOracle(W, WR.GPT_CFG["layers"], WR.GPT_CFG["heads"])
g = torch.Generator().manual_seed(100)
prompts = []
for text in (torch.randint(2, 12000, (100,), generator=g), torch.cat((torch.tensor([0, 1, 0]), torch.randint(2, 12000, (77,), generator=g)))):
    conds = torch.randn(34, 1280, generator=g) * 0.5
    fake, embeds, mask = orc.prepare_gpt_inputs(conds, text)
    prompts.append((embeds, mask, int((mask == 0).sum())))
stops = {1, 2, 64, N}
for _, mask, _ in prompts:
    for m in range(1, 6):
        for d in (-2, -1, 0, 1):
            k = 256 * m - len(mask) + d
            if 1 <= k <= N:
                stops.add(k)
result = {"steps": N, "prompt_rows": [len(m) for _, m, _ in prompts], "read_points": len(stops) + 1, "dtypes": {}}
for dt in dtypes:
    eng = GptEngine(WR.GPT_CFG, dtype=dt, max_seq=137 + N + 64, max_batch=2, device=dev).load_state_dict(W)
    for b, (emb, mask, pad) in enumerate(prompts):
        eng.prefill(b, emb, pad)
    got = {0: [eng.read_logits(b).copy() for b in range(2)]}
    done = 0
    for k in sorted(stops):
        eng.decode(2, k - done, repetition_penalty=10.0, suppress_stop=True)
        done = k
        got[k] = [eng.read_logits(b).copy() for b in range(2)]
    ids = [eng.read(b)[0][:N] for b in range(2)]
    del eng
    rows_out = []
    for b, (emb, mask, pad) in enumerate(prompts):
        t0 = time.time()
        rows = OG.teacher_forced_logits(orc, emb, mask, ids[b].tolist())
        picks, margins = OG.greedy_choices(rows, len(mask), ids[b].tolist(), theta=10.0, suppress_stop=True)
        scale = float(rows.abs().max())
        err = max(float(np.abs(got[k][b] - rows[k].numpy()).max()) for k in got) / scale
        differ = [k for k in range(N) if picks[k] != int(ids[b][k])]
        outside = [k for k in differ if margins[k] >= 1e-3 * scale]
        r = {"slot": b, "agreement": 1.0 - len(differ) / N, "differing": len(differ), "differing_outside_near_ties": len(outside),
             "logit_err_over_scale": err, "first_differing_step": differ[0] if differ else None}
        rows_out.append(r)
        print(f"{dt} slot {b}: greedy agreement {r['agreement']:.4f} ({len(differ)} of {N} differ, {len(outside)} outside near-ties), "
              f"logits rel err {err:.2e}  [oracle pass {time.time() - t0:.0f} s]", flush=True)
    result["dtypes"][dt] = rows_out
if args.out:
    json.dump(result, open(args.out, "w"), indent=1)
print(json.dumps(result))
