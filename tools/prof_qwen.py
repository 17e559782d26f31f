"""Emotion-model decode at the Qwen3-0.6B shape with seeded random f16 weights (csrc/qwen_engine.hip).

    python tools/prof_qwen.py [--out profiles/qwen_emo.json]

Prints the decode-step time at contexts 128 / 512 / 1024, the `QwenEmotion.inference()` wall time for a 128-token prompt
plus 64 new tokens (tokenization and parsing included; greedy, and sampled as the production generation config does), the
prefill time of that prompt, and the step's HBM bytes over its time as a fraction of 8 TB/s.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.init()
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
