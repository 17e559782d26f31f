"""GPU: the Qwen3 decode engine (csrc/qwen_engine.hip) against transformers' Qwen3ForCausalLM in fp32 on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qwen_twin as T  # noqa: E402

torch.set_grad_enabled(False)


def engine_cfg(m):
    c = m.config
    return dict(hidden_size=c.hidden_size, layers=c.num_hidden_layers, heads=c.num_attention_heads, kv_heads=c.num_key_value_heads,
                head_dim=c.head_dim, intermediate_size=c.intermediate_size, vocab_size=c.vocab_size, rms_norm_eps=c.rms_norm_eps,
                rope_theta=float(c.rope_parameters["rope_theta"]) if getattr(c, "rope_parameters", None) else float(c.rope_theta),
                tie_word_embeddings=bool(c.tie_word_embeddings))


def make_engine(m, dtype, eos, max_seq=512):
    from voice_tts_amd.qwen_emotion import QwenEngine

    cfg = engine_cfg(m)
    sd = {k: v for k, v in m.state_dict().items() if k != "lm_head.weight" or not cfg["tie_word_embeddings"]}
    return QwenEngine(cfg, dtype=dtype, max_seq=max_seq, device="cuda:0", eos_token_id=eos).load_state_dict(sd)


def rounded_f16(m):
    """The same model with every weight rounded to fp16 (kept fp32): what an f16 engine computes with."""
    import copy

    r = copy.deepcopy(m)
    for p in r.parameters():
        p.copy_(p.half().float())
    return r


def hf_greedy(m, prompt, n, eos=None):
    ids = torch.tensor([prompt])
    out = m.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=n, do_sample=False, eos_token_id=eos, pad_token_id=0,
                     num_beams=1, top_k=None, top_p=None, temperature=None)
    return out[0, len(prompt):].tolist()


def engine_logits_per_step(e, prompt, n):
    """Greedy steps one at a time, the fp32 logits after each."""
    e.prefill(prompt)
    rows = []
    for _ in range(n):
        e.step(1)
        rows.append(e.read_logits())
    return np.stack(rows), e.read()[0]


@pytest.fixture(scope="module")
def twin():
    m = T.make_model(T.twin_config(layers=3), seed=3, std=0.25)
    g = torch.Generator().manual_seed(4)
    prompt = torch.randint(0, 500, (37,), generator=g).tolist()
    free = hf_greedy(m, prompt, 48)
    # EOS = a token the free run first draws at step >= 30: the greedy run then stops there (an EOS stop inside 48 tokens)
    k = next(i for i in range(30, 48) if free[i] not in free[:i])
    return m, prompt, free[k], k


def test_twin_f32_logits_and_greedy_ids(twin):
    m, prompt, eos, k = twin
    ref = hf_greedy(m, prompt, 48, eos=[eos])
    assert ref[-1] == eos and len(ref) == k + 1
    e = make_engine(m, "f32", [eos])
    assert e.generate(prompt, 48) == ref
    logits, ids = engine_logits_per_step(e, prompt, len(ref))
    assert ids == ref
    full = m(torch.tensor([prompt + ref])).logits[0, len(prompt) - 1: len(prompt) - 1 + len(ref)].numpy()
    scale = np.abs(full).max()
    err = np.abs(logits - full).max(axis=1)
    assert err.max() < 1e-4 * scale, (err.max(), scale)
    # finished: more steps change nothing
    e.step(3)
    assert e.read() == (ref, 1)


def test_twin_f16_against_rounded_weights(twin):
    m, prompt, eos, k = twin
    r = rounded_f16(m)
    ref = hf_greedy(r, prompt, 48, eos=[eos])
    e = make_engine(m, "f16", [eos])
    assert e.generate(prompt, 48) == ref
    logits, ids = engine_logits_per_step(e, prompt, len(ref))
    full = r(torch.tensor([prompt + ref])).logits[0, len(prompt) - 1: len(prompt) - 1 + len(ref)].numpy()
    assert np.abs(logits - full).max() < 2e-3 * np.abs(full).max()


@pytest.fixture(scope="module")
def prod():
    cfg = T.twin_config(layers=T.PROD["num_hidden_layers"], vocab_size=T.PROD["vocab_size"], hidden_size=T.PROD["hidden_size"],
                        intermediate_size=T.PROD["intermediate_size"], heads=T.PROD["num_attention_heads"], kv_heads=T.PROD["num_key_value_heads"])
    m = T.make_model(cfg, seed=11, std=0.02)
    prompt = torch.randint(0, cfg.vocab_size, (128,), generator=torch.Generator().manual_seed(12)).tolist()
    return m, prompt


def test_production_width_f32_ids(prod):
    m, prompt = prod
    ref = hf_greedy(m, prompt, 32, eos=None)
    e = make_engine(m, "f32", [0], max_seq=256)
    got = e.generate(prompt, 32)
    assert got == ref[: len(got)] and (len(got) == 32 or got[-1] == 0)


def test_production_width_f16_logits(prod):
    m, prompt = prod
    r = rounded_f16(m)
    ref = hf_greedy(r, prompt, 32, eos=None)
    full = r(torch.tensor([prompt + ref])).logits[0].numpy()
    e = make_engine(m, "f16", [0], max_seq=256)
    # read points: contexts on both sides of the attention split boundaries (ceil(n / 8) keys per split changes at n = 8j + 1)
    reads = [128, 129, 136, 137, 144, 145, 152, 153, 159, 160]
    seq = prompt + ref
    for n in reads:
        e.prefill(seq[: n])
        e.step(1)
        lg = e.read_logits()
        want = full[n - 1]
        err = np.abs(lg - want).max()
        assert err < 2e-3 * np.abs(want).max(), (n, err)
        top2 = np.sort(want)[-2:]
        if int(lg.argmax()) != int(want.argmax()):
            print(f"context {n}: f16 argmax flipped on a near tie, margin {top2[1] - top2[0]:.3g}")
            assert top2[1] - top2[0] < 2 * err
    got = e.generate(prompt, 32)
    first = next((i for i, (a, b) in enumerate(zip(got, ref)) if a != b), None)
    if first is not None:
        w = full[len(prompt) - 1 + first]
        top2 = np.sort(w)[-2:]
        print(f"f16 ids agree for {first} steps; step {first} margin {top2[1] - top2[0]:.3g}")
        assert top2[1] - top2[0] < 1e-2 * np.abs(w).max()
    else:
        assert got == ref


def test_sampling_matches_hf_warpers_and_draws(twin):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    m, prompt, eos, k = twin
    e = make_engine(m, "f32", [eos])
    kw = dict(do_sample=True, temperature=0.6, top_k=20, top_p=0.95, seed=123)
    e.prefill(prompt)
    e.step(1, **kw)
    lg = torch.from_numpy(e.read_logits()).reshape(1, -1)
    ids, pr = e.read_kept()
    s = lg.clone()
    for w in (TemperatureLogitsWarper(0.6), TopKLogitsWarper(20), TopPLogitsWarper(0.95)):
        s = w(torch.tensor([prompt]), s)
    p = torch.softmax(s, dim=-1)[0]
    keep = torch.nonzero(p > 0).flatten().tolist()
    assert sorted(ids.tolist()) == sorted(keep) and 1 <= len(keep) <= 20
    assert np.abs(pr - p[ids].numpy()).max() < 1e-6
    # 20 000 draws at this position: frequencies within 4 sigma of the probabilities
    n = 20000
    d = e.draw(7, n)
    assert set(d.tolist()) <= set(keep)
    for i, q in zip(ids.tolist(), pr.tolist()):
        c = int((d == i).sum())
        assert abs(c - n * q) <= 4 * np.sqrt(n * q * (1 - q)) + 1, (i, c, n * q)
    # the same seed draws the same ids, another seed other ones
    a = e.generate(prompt, 24, **kw)
    b = e.generate(prompt, 24, **kw)
    c = e.generate(prompt, 24, **dict(kw, seed=124))
    assert a == b and a != c


def test_limits_are_refused(twin):
    m, prompt, eos, k = twin
    e = make_engine(m, "f32", [eos], max_seq=64)
    with pytest.raises(NotImplementedError, match="64"):
        e.generate(prompt, 4, do_sample=True, top_k=0)
    with pytest.warns(UserWarning, match="capped"):
        out = e.generate(prompt, 32768)
    assert len(out) <= 64 - len(prompt)


def test_untied_lm_head_and_a_prompt_off_the_prefill_chunk():
    """A separate lm_head matrix; 42 prompt ids = 10 prefill chunks of 4 positions + 1 single position; eos given as an int."""
    m = T.make_model(T.twin_config(layers=2, tie=False), seed=8, std=0.25)
    assert not torch.equal(m.lm_head.weight, m.model.embed_tokens.weight)
    prompt = torch.randint(0, 500, (42,), generator=torch.Generator().manual_seed(9)).tolist()
    ref = hf_greedy(m, prompt, 24, eos=None)
    e = make_engine(m, "f32", 511)
    assert e.eos == [511]
    logits, ids = engine_logits_per_step(e, prompt, 24)
    full = m(torch.tensor([prompt + ref])).logits[0, len(prompt) - 1: len(prompt) - 1 + 24].numpy()
    assert ids[: len(ref)] == ref[: len(ids)]
    assert np.abs(logits[: len(ids)] - full[: len(ids)]).max() < 1e-4 * np.abs(full).max()


def test_non_finite_logits_stop_with_an_error(twin):
    from voice_tts_amd import _lib

    m, prompt, eos, k = twin
    import copy

    bad = copy.deepcopy(m)
    bad.model.norm.weight[3] = float("nan")
    e = make_engine(bad, "f32", [eos])
    with pytest.raises(_lib.IxttsError, match="not finite"):
        e.generate(prompt, 8)


def test_production_width_sampled_step_matches_hf_warpers(prod):
    """The production generation config samples (temperature 0.6, top-k 20, top-p 0.95) over the 151 936-id vocabulary."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    m, prompt = prod
    e = make_engine(m, "f16", [0], max_seq=256)
    # sharpen the logits so that top-p trims the top-k set: the same sampled step at temperature 0.05 and 0.6
    for temp in (0.6, 0.05):
        e.prefill(prompt)
        e.step(1, do_sample=True, temperature=temp, top_k=20, top_p=0.95, seed=5)
        lg = torch.from_numpy(e.read_logits()).reshape(1, -1)
        ids, pr = e.read_kept()
        s = lg.clone()
        for w in (TemperatureLogitsWarper(temp), TopKLogitsWarper(20), TopPLogitsWarper(0.95)):
            s = w(torch.tensor([prompt]), s)
        p = torch.softmax(s, dim=-1)[0]
        keep = torch.nonzero(p > 0).flatten().tolist()
        assert sorted(ids.tolist()) == sorted(keep), (temp, len(ids), len(keep))
        assert np.abs(pr - p[ids].numpy()).max() < 1e-6
        assert e.read()[0][0] in keep
