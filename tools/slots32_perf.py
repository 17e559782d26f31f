"""The `mixed64` segment list (bench.py's: sharding.mixed_requests -- 64 requests of 50..400 characters, seed 5, 11 codes per
token) through the two schedulers at 16 and at 32 decode slots: wall time and the share of busy slot-steps.

    python tools/slots32_perf.py [--dtype {bf16,f16}] [--prefill {batch,serial,both}] [--first {serial,batch}] [--out profiles/slots32_sched.json]

DecodeScheduler: greedy, fixed length, one slot per segment (16 | 32 slots).  BeamGroupScheduler: the served 3-beam beam-sample,
fixed length (5 groups on 15 slots | 10 groups on 30).  The engines share one set of device weights; the 16-slot engine runs the
kernels it always ran, so it is the yardstick of the same build.  Prefills are inside the wall time (they are: a slot is
refilled while the others wait).  --prefill: the refill rounds as one `prefill_many` (batch) or one `prefill` per slot (serial);
`both` runs every shape both ways, one after the other in this process, `--first` way first (profiles/prefill_many_sched.json:
one run with each order, so that what the order does to the second of a pair shows beside the difference; a second run
appends); without it, the schedulers' default."""
import argparse, json, os, sys, time, torch
sys.path.insert(0, ".")
import voice_tts_amd.weights as WR
from voice_tts_amd import sharding
from voice_tts_amd.gpt_engine import GptEngine
from voice_tts_amd.scheduler import BeamGroupScheduler, DecodeScheduler, Segment

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=["bf16", "f16"], default="bf16")
ap.add_argument("--prefill", choices=["batch", "serial", "both"], default=None)
ap.add_argument("--first", choices=["serial", "batch"], default="serial")
ap.add_argument("--out", default=None)
args = ap.parse_args()
dev = torch.device("cuda:0")
reqs = sharding.mixed_requests()
g = torch.Generator().manual_seed(5)
segs = [Segment(i, s, (torch.randn(34 + n + 2, 1280, generator=g) * 0.5).to(dev), 0, 11 * n) for i, toks in enumerate(reqs) for s, n in enumerate(toks)]
max_seq = max(int(s.embeds.shape[0]) + 1 + s.max_new for s in segs) + 64
cfg = dict(WR.GPT_CFG, max_mel_tokens=max(WR.GPT_CFG["max_mel_tokens"], max(s.max_new for s in segs) + 8))
W = WR.make_gpt_weights(cfg, seed=1234)
owner = GptEngine(cfg, dtype=args.dtype, max_seq=max_seq, max_batch=16, device=dev).load_state_dict(W)
del W


def engine(slots):
    return owner if slots == 16 else GptEngine(cfg, dtype=args.dtype, max_seq=max_seq, max_batch=slots, device=dev).share_arena(owner)


def timed(run):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    st = run()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, st


res = dict(dtype=args.dtype, first=args.first, requests=len(reqs), segments=len(segs), codes=sum(s.max_new for s in segs), runs=[])
stop = cfg["stop_mel_token"]
ways = {None: [None], "batch": [True], "serial": [False], "both": [False, True] if args.first == "serial" else [True, False]}[args.prefill]
for kind, shapes in (("slots", (16, 32)), ("beam3", (15, 30))):
    for slots in shapes:
        eng = engine(slots)
        for way in ways:
            if kind == "slots":
                sch = DecodeScheduler(eng, slots, stop, batch_prefill=way)
                run = lambda: sch.run(segs, lambda seg, ids: None, fixed_length=True, repetition_penalty=10.0)
                busy = lambda st: st["busy_slot_steps"] / st["slot_steps"]
            else:
                sch = BeamGroupScheduler(eng, 3, batch_prefill=way)
                run = lambda: sch.run(segs, lambda seg, ids, sc: None, fixed_length=True, repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, seed=7)
                busy = lambda st: st["busy_group_steps"] / st["group_steps"]
            # a short run first: graphs captured, code objects paged in
            sch.run([Segment(s.request, s.index, s.embeds, 0, 24) for s in segs[:slots]], lambda *a: None, fixed_length=True, repetition_penalty=10.0)
            sch.stats = {k: 0 for k in sch.stats}
            wall, st = timed(run)
            row = dict(scheduler=kind, engine_slots=slots, prefill="batch" if sch.batch_prefill else "serial", wall_s=round(wall, 3), busy_share=round(busy(st), 4), **{k: int(v) for k, v in st.items()})
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
        if eng is not owner:
            del eng, sch
            torch.cuda.empty_cache()
if args.prefill == "both":
    for r in res["runs"]:
        if r["prefill"] == "batch":
            ser = [q for q in res["runs"] if (q["scheduler"], q["engine_slots"], q["prefill"]) == (r["scheduler"], r["engine_slots"], "serial")][0]
            r["wall_batch_over_serial"] = round(r["wall_s"] / ser["wall_s"], 4)
            print(json.dumps(dict(scheduler=r["scheduler"], engine_slots=r["engine_slots"], wall_batch_over_serial=r["wall_batch_over_serial"])), flush=True)
    if args.out:
        runs = json.load(open(args.out)) if os.path.exists(args.out) else []
        json.dump(runs + [res], open(args.out, "w"), indent=1)
    sys.exit(0)
by = {(r["scheduler"], r["engine_slots"]): r["wall_s"] for r in res["runs"]}
res["wall_ratio_slots_32_over_16"] = round(by[("slots", 32)] / by[("slots", 16)], 4)
res["wall_ratio_beam3_30_over_15"] = round(by[("beam3", 30)] / by[("beam3", 15)], 4)
print(json.dumps({k: res[k] for k in ("wall_ratio_slots_32_over_16", "wall_ratio_beam3_30_over_15")}), flush=True)
if args.out:
    json.dump(res, open(args.out, "w"), indent=1)
