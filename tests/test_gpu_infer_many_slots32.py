"""`IndexTTS2.infer_many(decode_slots=32)` on a 16-bit model: twenty pinned requests, half without beams and half with three,
sound byte for byte as they do at `decode_slots=16` -- every wide engine (5..32 slots) gives a sequence the same bits -- while
the call really runs a 32-slot engine and ten beam groups.  An fp32 model asked for 32 slots is served on 16."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _model(tmp_path_factory, name, **kw):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp(name))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256, **kw)
    return m, SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1)


@pytest.fixture(scope="module")
def tts_bf16(tmp_path_factory):
    return _model(tmp_path_factory, "model_dir_slots32", use_fp16=True, gpt_dtype="bf16")


@pytest.fixture(scope="module")
def tts_f32(tmp_path_factory):
    return _model(tmp_path_factory, "model_dir_slots32_f32", use_fp16=False)


TEXTS = ["Hello world.", "Short.", "A second voice.", "This is a test.", "One more here.", "Say some more.", "And a last one.", "Numbers now.",
         "Speak up.", "Good night."]


def _requests(wav_a, wav_b):
    reqs = []
    for i in range(20):
        gen = {"seed": 100 + i, "num_beams": 1 if i % 2 == 0 else 3}
        if i % 4 == 0:
            gen.update(temperature=1.1, top_k=40)
        if i % 6 == 1:
            gen.update(length_penalty=1.0)
        reqs.append(dict(spk_audio_prompt=wav_a if i % 3 else wav_b, text=TEXTS[i % 10], generation=gen))
    return reqs


def test_twenty_pinned_requests_sound_the_same_at_32_and_at_16_slots(tts_bf16, monkeypatch):
    from voice_tts_amd import gpt_engine as GE
    from voice_tts_amd import scheduler as SCH

    m, wav_a, wav_b = tts_bf16
    assert m.gpt_dtype == "bf16"
    made, beam_runs, slot_runs = [], [], []
    real_init, real_beam, real_dec = GE.GptEngine.__init__, SCH.BeamGroupScheduler.run, SCH.DecodeScheduler.run

    def init_spy(self, *a, **kw):
        real_init(self, *a, **kw)
        made.append(self.max_batch)

    def beam_spy(self, segments, on_done, **kw):
        segments = list(segments)
        beam_runs.append((self.engine.max_batch, self.max_groups, len(segments)))
        return real_beam(self, segments, on_done, **kw)

    def dec_spy(self, segments, on_done, **kw):
        segments = list(segments)
        slot_runs.append((self.engine.max_batch, self.max_batch, len(segments)))
        return real_dec(self, segments, on_done, **kw)

    monkeypatch.setattr(GE.GptEngine, "__init__", init_spy)
    monkeypatch.setattr(SCH.BeamGroupScheduler, "run", beam_spy)
    monkeypatch.setattr(SCH.DecodeScheduler, "run", dec_spy)
    reqs = _requests(wav_a, wav_b)
    out32 = m.infer_many(reqs, decode_slots=32, max_mel_tokens=12)
    # the call really built and ran a 32-slot engine, and the beam class stepped ten groups of three
    assert 32 in made and 32 in m._engines and m._engines[32].max_batch == 32 and m._engines[32].dtype == "bf16"
    assert slot_runs == [(32, 32, 10)] and beam_runs == [(30, 10, 10)], (slot_runs, beam_runs)
    del slot_runs[:], beam_runs[:]
    out16 = m.infer_many(reqs, decode_slots=16, max_mel_tokens=12)
    assert slot_runs == [(16, 16, 10)] and beam_runs == [(15, 5, 10)], (slot_runs, beam_runs)
    assert len(out32) == len(out16) == 20
    for i, (a, b) in enumerate(zip(out32, out16)):
        assert isinstance(a, tuple) and isinstance(b, tuple), (i, a, b)
        assert a[0] == b[0] == 22050 and a[1].dtype == np.int16 and a[1].shape[0] > 0, i
        assert a[1].tobytes() == b[1].tobytes(), i  # the PCM of every request, byte for byte
    assert len({o[1].tobytes() for o in out32}) > 10  # (not twenty copies of one sound)


def test_an_fp32_model_asked_for_32_slots_is_served_on_16(tts_f32):
    m, wav_a, wav_b = tts_f32
    assert m.gpt_dtype == "f32"
    reqs = [dict(spk_audio_prompt=wav_a, text="Hello world."), dict(spk_audio_prompt=wav_b, text="Short."), dict(spk_audio_prompt=wav_a, text="One more here.")]
    outs = m.infer_many(reqs, decode_slots=32, num_beams=1, top_k=1, max_mel_tokens=12)
    assert 16 in m._engines and 32 not in m._engines and m._engines[16].max_batch == 16 and m._engines[16].dtype == "f32"
    assert len(outs) == 3
    for sr, pcm in outs:
        assert sr == 22050 and pcm.dtype == np.int16 and pcm.ndim == 2 and pcm.shape[0] > 0
