"""Emotion-model decode at the Qwen3-0.6B shape with seeded random f16 weights (csrc/qwen_engine.hip).

    python tools/prof_qwen.py [--out profiles/qwen_emo.json]
    python tools/prof_qwen.py --slots 4 [--out profiles/qwen_emo_slots.json]

Prints the decode-step time at contexts 128 / 512 / 1024, the `QwenEmotion.inference()` wall time for a 128-token prompt
plus 64 new tokens (tokenization and parsing included; greedy, and sampled as the production generation config does), the
prefill time of that prompt, and the step's HBM bytes over its time as a fraction of 8 TB/s.

`--slots N` times the batch path instead: N different 128-token prompts plus 64 new tokens through `inference_many` (greedy
and sampled) against the same N through N `inference()` calls, the rows prefill of the N prompts alone against N chunk
prefills, and the decode step at context 512 with 1 / 2 / N active slots.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from voice_tts_amd.qwen_emotion import QwenEmotion, QwenEngine  # noqa: E402

PEAK = 8e12
CFG = dict(hidden_size=1024, layers=28, heads=16, kv_heads=8, head_dim=128, intermediate_size=3072, vocab_size=151936, rms_norm_eps=1e-6,
           rope_theta=1e6, tie_word_embeddings=True)


def random_state_dict(seed=0, std=0.02):
    g = torch.Generator().manual_seed(seed)
    D, I, V, qd, kvd = 1024, 3072, 151936, 16 * 128, 8 * 128
    r = lambda *s: torch.randn(*s, generator=g) * std
    one = lambda n: 1.0 + 0.1 * torch.randn(n, generator=g)
    sd = {"model.embed_tokens.weight": r(V, D), "model.norm.weight": one(D)}
    for l in range(28):
        p = f"model.layers.{l}."
        sd.update({p + "self_attn.q_proj.weight": r(qd, D), p + "self_attn.k_proj.weight": r(kvd, D), p + "self_attn.v_proj.weight": r(kvd, D),
                   p + "self_attn.o_proj.weight": r(D, qd), p + "self_attn.q_norm.weight": one(128), p + "self_attn.k_norm.weight": one(128),
                   p + "mlp.gate_proj.weight": r(I, D), p + "mlp.up_proj.weight": r(I, D), p + "mlp.down_proj.weight": r(D, I),
                   p + "input_layernorm.weight": one(D), p + "post_attention_layernorm.weight": one(D)})
    return sd


def step_time(e, ctx, steps=64, reps=3):
    ids = torch.randint(0, 151000, (ctx,), generator=torch.Generator().manual_seed(ctx)).tolist()
    best = None
    for _ in range(reps):
        e.prefill(ids)
        e.step(8)  # graphs built, caches warm
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.step(steps)
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) / steps * 1e3
        best = t if best is None else min(best, t)
    return best


def median_ms(fn, reps=6):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times[1:])), 2)


def slots_step_time(e, n, ctx, steps=64, reps=3):
    prompts = [torch.randint(0, 151000, (ctx,), generator=torch.Generator().manual_seed(ctx + s)).tolist() for s in range(n)]
    best = None
    for _ in range(reps):
        e.prefill_many(prompts)
        e.step_many(8)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.step_many(steps)
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) / steps * 1e3
        best = t if best is None else min(best, t)
    return best


def slots_leg(n, out):
    import qwen_twin as T
    from transformers import AutoTokenizer

    e = QwenEngine(CFG, dtype="f16", max_seq=2048, device="cuda:0", eos_token_id=[151935], slots=n).load_state_dict(random_state_dict())
    res = dict(shape=f"Qwen3-0.6B (28 x 1024, 16/8 heads x 128, ffn 3072, vocab 151936, tied), f16 weights, {n} slots")
    d = tempfile.mkdtemp()
    T.write_tokenizer(d)
    q = QwenEmotion(None, tokenizer=AutoTokenizer.from_pretrained(d, local_files_only=True), engine=e)
    texts = []
    for ch in "wxyzuv"[:n]:
        text = ch * 200
        while len(q.prompt_ids(text)) > 128:
            text = text[:-1]
        assert len(q.prompt_ids(text)) == 128
        texts.append(text)
    for tag, gen in (("", dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0)),
                     ("_sampled", dict(do_sample=True, temperature=0.6, top_k=20, top_p=0.95))):
        q.generation = dict(gen, eos_token_id=[151935])
        many = [None]
        res[f"inference_many_ms_{n}x128_plus_64{tag}"] = median_ms(lambda: many.__setitem__(0, q.inference_many(texts, max_new_tokens=64)))
        res[f"new_tokens{tag}"] = [len(e.read_slot(s)[0]) for s in range(n)]
        serial = [None]
        res[f"serial_inference_ms_{n}x128_plus_64{tag}"] = median_ms(lambda: serial.__setitem__(0, [q.inference(t, max_new_tokens=64) for t in texts]))
        res[f"same_answers{tag}"] = many[0] == serial[0]
    prompts = [q.prompt_ids(t) for t in texts]
    res[f"rows_prefill_ms_{n}x127"] = median_ms(lambda: e.prefill_many(prompts))
    res[f"chunk_prefill_ms_{n}x127_serial"] = median_ms(lambda: [e.prefill(p) for p in prompts])
    res["step_us_ctx512_one_sequence"] = round(step_time(e, 512), 1)
    for k in sorted({1, 2, n}):
        res[f"step_us_ctx512_{k}_slots"] = round(slots_step_time(e, k, 512), 1)
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--slots", type=int, default=0, help="time the batch path with this many slots (2..4) instead")
    args = ap.parse_args()
    torch.cuda.init()
    if args.slots:
        return slots_leg(args.slots, args.out)
    e = QwenEngine(CFG, dtype="f16", max_seq=2048, device="cuda:0", eos_token_id=[151935]).load_state_dict(random_state_dict())
    res = dict(shape="Qwen3-0.6B (28 x 1024, 16/8 heads x 128, ffn 3072, vocab 151936, tied), f16 weights, B=1")
    res["step_bytes_ctx512"] = e.step_bytes(512)
    for ctx in (128, 512, 1024):
        us = step_time(e, ctx)
        res[f"step_us_ctx{ctx}"] = round(us, 1)
        res[f"hbm_fraction_ctx{ctx}"] = round(e.step_bytes(ctx) / (us * 1e-6) / PEAK, 3)
    # detect(): 128 prompt ids (chat template included) + 64 new tokens, through the byte-level tokenizer of the test twin
    import qwen_twin as T
    from transformers import AutoTokenizer

    d = tempfile.mkdtemp()
    T.write_tokenizer(d)
    tok = AutoTokenizer.from_pretrained(d, local_files_only=True)
    q = QwenEmotion(None, tokenizer=tok, engine=e)
    text = "x" * 200
    while len(q.prompt_ids(text)) > 128:
        text = text[:-1]
    assert len(q.prompt_ids(text)) == 128
    times = []
    for _ in range(6):
        t0 = time.perf_counter()
        q.inference(text, max_new_tokens=64)
        times.append((time.perf_counter() - t0) * 1e3)
    n_new = len(e.read()[0])
    res["detect_ms_128_plus_64"] = round(float(np.median(times[1:])), 2)
    res["detect_new_tokens"] = n_new
    # the same with the production generation config, which samples (temperature 0.6, top-k 20, top-p 0.95)
    q.generation = dict(do_sample=True, temperature=0.6, top_k=20, top_p=0.95, eos_token_id=[151935])
    times = []
    for _ in range(6):
        t0 = time.perf_counter()
        q.inference(text, max_new_tokens=64)
        times.append((time.perf_counter() - t0) * 1e3)
    res["detect_ms_128_plus_64_sampled"] = round(float(np.median(times[1:])), 2)
    res["detect_new_tokens_sampled"] = len(e.read()[0])
    # the prompt alone: 127 positions through the layers (31 chunks of 4 + 3 single positions)
    ids = q.prompt_ids(text)
    times = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.prefill(ids)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    res["prefill_ms_128"] = round(float(np.median(times[1:])), 2)
    res["bars"] = dict(step_ms_ctx512=0.65, detect_ms=130.0)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
