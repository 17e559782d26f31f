"""`IndexTTS2.infer_many` and `infer` run the latent forward of all their segments as ONE `GptEngine.latent_many` (IXTTS_LATENT_BATCH,
on by default): the PCM is exactly what the per-segment `latent` calls give, the packed call is made once, and when it raises the
segments are redone one by one.

The requests are pinned ones put together from the sentences of tests/test_gpu_infer_many_generation.py, under its settings, with at
most 16 codes per segment: no segment length that file has not already run (see tests/test_gpu_infer_many_vocoder.py on why that
matters)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tts_from_dir(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_latent"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM


def _spy(m, monkeypatch, fail_first=False):
    """count the latent calls of `GptEngine` (patched on the CLASS: a `latent` replaced on the engine object itself switches the packed
    path off, see the last test); `fail_first`: the first latent_many raises"""
    from voice_tts_amd.gpt_engine import GptEngine

    calls = dict(many=[], one=0)
    real_many, real_one = GptEngine.latent_many, GptEngine.latent

    def many(self, entries, **kw):
        entries = list(entries)
        calls["many"].append(len(entries))
        if fail_first and len(calls["many"]) == 1:
            raise RuntimeError("latent_many: patched to raise")
        return real_many(self, entries, **kw)

    def one(self, prefix, codes):
        calls["one"] += 1
        return real_one(self, prefix, codes)

    monkeypatch.setattr(GptEngine, "latent_many", many)
    monkeypatch.setattr(GptEngine, "latent", one)
    return calls


TWO = ["Hello world, this is a test. And then it says some more.",  # 19 + 15 tokens: two segments at 20 tokens per segment
       "A second voice says this. And then it says some more.",       # 16 + 15
       "A second voice says this. Hello world, this is a test."]      # 16 + 19


def _requests(SM):
    wav_a, wav_b = SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1)
    gens = [{"seed": 5}, {"temperature": 1.1, "top_k": 8, "length_penalty": 1.0}, {"num_beams": 1, "seed": 2}]
    reqs = [dict(spk_audio_prompt=w, text=t, generation=gen) for w, t, gen in zip((wav_a, wav_b, wav_a), TWO, gens)]
    return reqs, dict(decode_slots=8, max_mel_tokens=16, max_text_tokens_per_segment=20)


def _pcm(outs):
    assert all(isinstance(o, tuple) and o[0] == 22050 and o[1].dtype == np.int16 and o[1].shape[0] > 0 for o in outs), outs
    return [o[1] for o in outs]


def test_infer_many_runs_one_latent_many_and_gives_the_per_segment_pcm(tts_from_dir, monkeypatch):
    m, SM = tts_from_dir
    reqs, kw = _requests(SM)
    assert all(len(m._segments_of(r["text"], 20)) == 2 for r in reqs)
    monkeypatch.setattr(m, "latent_batch", False)
    calls = _spy(m, monkeypatch)
    off = _pcm(m.infer_many(reqs, **kw))
    assert calls == dict(many=[], one=6)  # switched off: the calls it always made
    monkeypatch.setattr(m, "latent_batch", True)
    calls = _spy(m, monkeypatch)
    on = _pcm(m.infer_many(reqs, **kw))
    assert calls == dict(many=[6], one=0)  # three requests of two segments in one call
    for a, b in zip(on, off):
        assert np.array_equal(a, b)
    # the packed call raises: every request still succeeds, segment by segment, with the same PCM
    calls = _spy(m, monkeypatch, fail_first=True)
    redo = _pcm(m.infer_many(reqs, **kw))
    assert calls == dict(many=[6], one=6)
    for a, b in zip(redo, off):
        assert np.array_equal(a, b)


def test_a_bad_code_fails_its_own_request_before_anything_is_packed(tts_from_dir, monkeypatch):
    m, SM = tts_from_dir
    reqs, kw = _requests(SM)
    monkeypatch.setattr(m, "latent_batch", True)
    good = _pcm(m.infer_many(reqs, **kw))
    real = m._trim_codes
    seen = []

    def trim(ids):  # the second request's first segment comes back with a code outside the codebook
        out = real(ids).clone()
        seen.append(1)
        if len(seen) == 3:
            out[0, 0] = 10 ** 6
        return out

    monkeypatch.setattr(m, "_trim_codes", trim)
    calls = _spy(m, monkeypatch)
    outs = m.infer_many(reqs, **kw)
    assert isinstance(outs[1], Exception) and calls == dict(many=[4], one=0)
    assert np.array_equal(outs[0][1], good[0]) and np.array_equal(outs[2][1], good[2])


def test_infer_on_two_segments_on_equals_off(tts_from_dir, monkeypatch):
    m, SM = tts_from_dir
    wav = SM.synthetic_wav_bytes(1.5, 24000)
    text = TWO[0]
    kw = dict(max_text_tokens_per_segment=20, num_beams=1, top_k=1, max_mel_tokens=16)
    import torch

    monkeypatch.setattr(m, "latent_batch", False)
    calls = _spy(m, monkeypatch)
    torch.manual_seed(1234)  # (the s2mel noise of an unpinned `infer` comes from the default generator)
    sr0, off = m.infer(wav, text, None, **kw)
    assert calls == dict(many=[], one=2)
    monkeypatch.setattr(m, "latent_batch", True)
    calls = _spy(m, monkeypatch)
    torch.manual_seed(1234)
    sr1, on = m.infer(wav, text, None, **kw)
    assert calls == dict(many=[2], one=0)
    assert sr0 == sr1 == 22050 and on.shape[0] > 0 and np.array_equal(on, off)
    # one segment: the per-segment path, switch or no switch
    calls = _spy(m, monkeypatch)
    m.infer(wav, "Hello world.", None, **kw)
    assert calls == dict(many=[], one=1)


def test_switch_is_resolved_once_and_reported(tts_from_dir, monkeypatch):
    from fastapi.testclient import TestClient

    from voice_tts_amd.scheduler import LATENT_BATCH_DEFAULT
    from voice_tts_amd.server import create_app

    m, SM = tts_from_dir
    assert m.latent_batch is LATENT_BATCH_DEFAULT or "IXTTS_LATENT_BATCH" in os.environ
    monkeypatch.setenv("IXTTS_WARMUP", "0")
    for want in (True, False):
        monkeypatch.setattr(m, "latent_batch", want)
        with TestClient(create_app(lambda: m)) as c:
            assert c.get("/debug/worker-info").json()["model_info"]["latent_batch"] is want


def test_a_latent_replaced_on_the_engine_object_keeps_its_per_segment_calls(tts_from_dir, monkeypatch):
    """a recorder around `m.gpt.latent` (tests/golden/make_golden_infer_parent.py installs one) sees every segment, switch or no switch"""
    m, SM = tts_from_dir
    reqs, kw = _requests(SM)
    monkeypatch.setattr(m, "latent_batch", True)
    want = _pcm(m.infer_many(reqs, **kw))
    seen, real = [], m.gpt.latent
    monkeypatch.setattr(m.gpt, "latent", lambda prefix, codes: (seen.append(int(codes.numel())), real(prefix, codes))[1])
    calls_many = []
    real_many = m.gpt.latent_many
    monkeypatch.setattr(m.gpt, "latent_many", lambda entries, **k: (calls_many.append(1), real_many(entries, **k))[1])
    got = _pcm(m.infer_many(reqs, **kw))
    assert len(seen) == 6 and not calls_many
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
