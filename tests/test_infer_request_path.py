"""CPU: the helpers `IndexTTS2.infer` and `infer_many` share for a request -- generation arguments, emotion resolution, the prompt
caches, the conditioning, code trimming and the segment builder -- on a bare `IndexTTS2` with CPU tables and a counting fake glue."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from voice_tts_amd import pipeline as PL
from voice_tts_amd.infer_v2 import IndexTTS2
from voice_tts_amd.weights import tiny_gpt_cfg

D = 16
CFG = tiny_gpt_cfg(model_dim=D, layers=1, heads=2)


class CountingGlue:
    def __init__(self):
        self.calls = dict(speaker=0, emotion=0, merge_emovec=0, get_conditioning=0, emo_vector_mix=0)

    def speaker(self, prompt):
        self.calls["speaker"] += 1
        if prompt == "bad.wav":
            raise ValueError("not audio")
        return dict(spk_cond_emb=torch.full((1, 3, 4), float(len(prompt))), style=torch.ones(1, 192), prompt_condition=None, ref_mel=None)

    def emotion(self, prompt):
        self.calls["emotion"] += 1
        if prompt == "bad-emo.wav":
            raise ValueError("not audio")
        return torch.full((1, 3, 4), 10.0 + len(prompt))

    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha):
        self.calls["merge_emovec"] += 1
        base, emo = spk_cond_emb.mean().expand(1, D), emo_cond_emb.mean().expand(1, D)
        return base + alpha * (emo - base)

    def get_conditioning(self, spk_cond_emb):
        self.calls["get_conditioning"] += 1
        return torch.arange(32 * D, dtype=torch.float32).reshape(32, D)

    def emo_vector_mix(self, emo_vector, style, use_random):
        self.calls["emo_vector_mix"] += 1
        return torch.full((1, D), 0.5), float(sum(emo_vector))


@pytest.fixture
def tts():
    m = IndexTTS2.__new__(IndexTTS2)
    g = torch.Generator().manual_seed(3)
    m.device, m.glue, m.prompt, m.cond, m.tokenizer, m.s2mel = torch.device("cpu"), CountingGlue(), None, None, None, None
    m.emo_matrix, m.missing_glue = None, []
    m.gpt_cfg, m.stop_mel_token = CFG, CFG["stop_mel_token"]
    m.text_embedding = torch.randn(CFG["number_text_tokens"] + 1, D, generator=g)
    m.text_pos_embedding = torch.randn(CFG["max_text_tokens"] + 2, D, generator=g)
    m.speed_emb = torch.randn(2, D, generator=g)
    m.cache_spk_audio_prompt = m.cache_spk = m.cache_emo_audio_prompt = m.cache_emo_cond = None
    return m


def test_generation_args_defaults_and_leftovers(tts):
    g, rest = tts._generation_args({})
    assert vars(g) == dict(top_p=0.8, top_k=30, temperature=0.8, num_beams=3, length_penalty=0.0, repetition_penalty=10.0, max_mel_tokens=1500,
                           typical_mass=0.0, seed=0)
    assert rest == {}
    proc = object()
    given = dict(do_sample=False, top_k=5, num_beams=1, max_mel_tokens=40, seed=7, typical_sampling=True, typical_mass=0.7, logits_processor=proc)
    g, rest = tts._generation_args(given)
    assert (g.top_k, g.num_beams, g.max_mel_tokens, g.seed, g.typical_mass, g.top_p) == (5, 1, 40, 7, 0.7, 0.8)
    assert rest == dict(seed=7, typical_sampling=True, typical_mass=0.7, logits_processor=proc) and rest["logits_processor"] is proc
    assert tts._generation_args(dict(typical_mass=0.7))[0].typical_mass == 0.0  # only with typical_sampling
    assert tts._generation_args(dict(typical_sampling=True))[0].typical_mass == 0.9
    assert "top_k" in given  # the caller's dict is left alone


def test_resolve_emotion_truth_table(tts):
    R = tts._resolve_emotion
    vec = [0.5, 0, 0, 0, 0, 0, 0, 0.12345]
    assert R(None, 0.3, None) == (None, 1.0, None, True)  # no emotion prompt: the speaker prompt at alpha 1.0
    assert R("emo.wav", 0.3, None) == ("emo.wav", 0.3, None, False)
    assert R("emo.wav", 1.7, None) == ("emo.wav", 1.7, None, False)  # alpha is clamped for the vector only
    assert R("emo.wav", 1.0, vec) == (None, 1.0, vec, True)  # a vector replaces the emotion prompt
    assert R("emo.wav", 2.0, vec) == (None, 1.0, vec, True)  # clamped to 1.0: unscaled
    assert R(None, 0.5, vec) == (None, 1.0, [0.25, 0, 0, 0, 0, 0, 0, 0.0617], True)  # int(x * scale * 10000) / 10000 truncates
    assert R("emo.wav", -1.0, vec) == (None, 1.0, [0.0] * 8, True)


def test_prompt_caches(tts):
    glue = tts.glue
    spk, emo = tts._encode_prompts(b"speaker one", None)
    assert glue.calls["speaker"] == 1 and glue.calls["emotion"] == 1 and float(emo.mean()) == 10.0 + len(b"speaker one")
    # equal content in a fresh object hits both caches; a tuple with an array compares by content
    spk2, emo2 = tts._encode_prompts(bytes(bytearray(b"speaker one")), None)
    assert spk2 is spk and emo2 is emo and glue.calls["speaker"] == 1 and glue.calls["emotion"] == 1
    tts._encode_prompts(b"speaker one", "emo.wav")
    assert glue.calls["speaker"] == 1 and glue.calls["emotion"] == 2
    tts._encode_prompts((np.arange(4.0), 16000), "emo.wav")
    tts._encode_prompts((np.arange(4.0), 16000), "emo.wav")
    assert glue.calls["speaker"] == 2 and glue.calls["emotion"] == 2
    tts._encode_prompts((np.arange(4.0) + 1, 16000), "emo.wav")
    assert glue.calls["speaker"] == 3 and glue.calls["emotion"] == 2
    # a speaker that raises leaves no pair behind; the emotion pair is untouched, and the old prompt is encoded again afterwards
    with pytest.raises(ValueError):
        tts._encode_prompts("bad.wav", "emo.wav")
    assert (tts.cache_spk, tts.cache_spk_audio_prompt) == (None, None) and tts.cache_emo_audio_prompt == "emo.wav"
    with pytest.raises(ValueError):
        tts._encode_prompts("good.wav", "bad-emo.wav")
    assert (tts.cache_emo_cond, tts.cache_emo_audio_prompt) == (None, None) and tts.cache_spk_audio_prompt == "good.wav"
    n = glue.calls["emotion"]
    tts._encode_prompts("good.wav", "emo.wav")
    assert glue.calls["emotion"] == n + 1


def test_conds_latent_once_per_request(tts):
    spk, emo = tts._encode_prompts("spk.wav", "emo.wav")
    cl = tts._conds_latent(spk, emo, False, 0.5, None, False)
    base, e = float(len("spk.wav")), 10.0 + len("emo.wav")
    assert tts.glue.calls["merge_emovec"] == 1 and tts.glue.calls["get_conditioning"] == 1 and tts.glue.calls["emo_vector_mix"] == 0
    want = torch.arange(32 * D, dtype=torch.float32).reshape(32, D) + (base + 0.5 * (e - base))
    assert cl.shape == (34, D) and torch.equal(cl[:32], want) and torch.equal(cl[32], tts.speed_emb[1]) and torch.equal(cl[33], tts.speed_emb[0])
    assert torch.equal(cl, PL.conds_latent(tts.glue.get_conditioning(None), torch.full((D,), base + 0.5 * (e - base)), tts.speed_emb))
    # with a vector: emovec_mat + (1 - weight_sum) * emovec
    cl = tts._conds_latent(spk, emo, True, 1.0, [0.25, 0, 0, 0, 0, 0, 0, 0.25], False)
    assert tts.glue.calls["emo_vector_mix"] == 1
    assert torch.allclose(cl[0], torch.arange(D, dtype=torch.float32) + 0.5 + 0.5 * e)


def test_trim_codes(tts):
    stop = tts.stop_mel_token
    c = tts._trim_codes(np.array([5, 6, stop, 7, stop], dtype=np.int32))
    assert c.dtype == torch.int64 and c.shape == (1, 2) and c.tolist() == [[5, 6]]
    assert tts._trim_codes(np.array([5, 6, 7], dtype=np.int32)).tolist() == [[5, 6, 7]]
    assert tts._trim_codes(np.array([stop, 5], dtype=np.int32)).shape == (1, 0)
    assert tts._trim_codes(torch.tensor([[5, stop, 6]])).tolist() == [[5]]  # `infer` hands over the [1, n] tensor of gpt.generate


def test_segment_builder_agrees_with_prepare_gpt_inputs(tts):
    cl = torch.randn(34, D, generator=torch.Generator().manual_seed(4))
    ids = [7, CFG["start_text_token"], 9, 11, CFG["stop_text_token"], 13]  # two ids are dropped and made up for by left padding
    embeds, pad, P = PL.prepare_gpt_inputs(CFG, tts.text_embedding, tts.text_pos_embedding, cl, ids)
    assert pad == 2 and P == 34 + len(ids) + 2 + 1 and bool((embeds[:2] == 0).all())
    for max_seq, max_mel_tokens, want in ((192, 20, 20), (P + 2 + 5, 20, 5), (P, 20, 0), (10 ** 6, 10 ** 6, CFG["max_mel_tokens"] - 1)):
        seg = tts._segment(cl, ids, SimpleNamespace(max_seq=max_seq), max_mel_tokens, request=3, index=1, payload="p", stream=2)
        assert (seg.request, seg.index, seg.payload, seg.stream) == (3, 1, "p", 2)
        assert seg.n_left_pad == pad and seg.max_new == want and torch.equal(seg.embeds, embeds)
    seg = tts._segment(cl, ids, SimpleNamespace(max_seq=192), 20)
    assert (seg.request, seg.index, seg.payload, seg.stream) == (0, 0, None, None)
    # the latent prefix keeps the ids as they are: [conds; [start] ids [stop]]
    t = torch.tensor([CFG["start_text_token"]] + ids + [CFG["stop_text_token"]])
    want = torch.cat((cl, tts.text_embedding[t] + tts.text_pos_embedding[: t.numel()]), 0)
    assert torch.equal(PL.latent_prefix(CFG, tts.text_embedding, tts.text_pos_embedding, cl, ids), want)
