"""GPU: the emotion from text for several texts at once -- `QwenEmotion.inference_many` on the slots of the Qwen3 engine, and
`IndexTTS2.infer_many` requests that carry `use_emo_text` / `emo_text`."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qwen_twin as T  # noqa: E402
from test_gpu_qwen_emotion import GREEDY, RecordingEmotion, _tts  # noqa: E402

TEXTS = ["I am so happy today!", "what a gloomy afternoon", "so very angry", "I am so happy today!", "meh", "a much longer text about nothing at all"]


@pytest.fixture(scope="module")
def twin_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("qwen_many") / "qwen0.6bemo4-merge")
    T.write_twin(d, seed=5, layers=2)
    return d


@pytest.fixture(scope="module")
def qwen(twin_dir):
    from voice_tts_amd.qwen_emotion import QwenEmotion

    q = QwenEmotion(twin_dir, dtype="f32", device="cuda:0", max_seq=160)
    assert q.engine.slots == 4  # the default of IXTTS_QWEN_SLOTS
    return q


def test_inference_many_is_the_loop_over_inference(qwen, twin_dir, monkeypatch):
    from voice_tts_amd.qwen_emotion import QwenEmotion

    want = [qwen.inference(t) for t in TEXTS]
    groups = []
    real = qwen.engine.generate_many
    monkeypatch.setattr(qwen.engine, "generate_many", lambda prompts, *a, **k: (groups.append([len(p) for p in prompts]), real(prompts, *a, **k))[1])
    assert qwen.inference_many(TEXTS) == want
    # five different texts: a group of 4 and a group of 1, the longest prompts first
    assert [len(g) for g in groups] == [4, 1]
    flat = [n for g in groups for n in g]
    assert flat == sorted((len(qwen.prompt_ids(t)) for t in set(TEXTS)), reverse=True)
    assert qwen.inference_many([]) == []
    monkeypatch.setenv("IXTTS_QWEN_SLOTS", "1")
    q1 = QwenEmotion(twin_dir, dtype="f32", device="cuda:0", max_seq=160)
    assert q1.engine.slots == 1 and q1.inference_many(TEXTS) == want


def _sees_latent(glue):
    """FakeGlue's mel depends on the number of codes alone; this one also moves with the latent, so that a changed
    conditioning reaches the PCM."""
    real = glue.s2mel

    def s2mel(latent, codes, code_lens, speaker):
        mel = real(latent, codes, code_lens, speaker)
        mel[:, :, : latent.shape[1]] += 10.0 * latent.float().mean(dim=2).reshape(1, 1, -1)
        return mel.clamp(-11.5, 2)

    glue.s2mel = s2mel


def _requests(t1):
    return [dict(spk_audio_prompt="spk.wav", text="hello world", use_emo_text=True, emo_text=t1, emo_alpha=0.6),
            dict(spk_audio_prompt="spk.wav", text="what a gloomy afternoon", use_emo_text=True, emo_audio_prompt="angry.wav", emo_alpha=0.6),
            dict(spk_audio_prompt="spk.wav", text="hello world")]


def _with_vectors(reqs, emo):
    out = []
    for rq in reqs:
        rq = dict(rq)
        if rq.pop("use_emo_text", False):
            text = rq.pop("emo_text", None)
            rq["emo_vector"] = list(emo.inference(text if text is not None else rq["text"]).values())
            rq.pop("emo_audio_prompt", None)
        out.append(rq)
    return out


def test_infer_many_serves_the_emotion_from_text(qwen):
    m = _tts(qwen_emo=qwen)
    _sees_latent(m.glue)
    reqs = _requests("I am so happy today!")
    outs = m.infer_many(reqs, **GREEDY)
    refs = m.infer_many(_with_vectors(reqs, qwen), **GREEDY)
    for o, r in zip(outs, refs):
        assert isinstance(o, tuple) and o[0] == r[0] == 22050 and np.array_equal(o[1], r[1])
    # the emotion reached the audio: the same text without it sounds different
    assert outs[0][1].shape != outs[2][1].shape or not np.array_equal(outs[0][1], outs[2][1])


def test_infer_many_falls_back_to_inference_per_text():
    rec = RecordingEmotion()
    m = _tts(qwen_emo=rec)
    _sees_latent(m.glue)
    reqs = _requests("so very angry")
    outs = m.infer_many(reqs, **GREEDY)
    assert rec.calls == ["so very angry", "what a gloomy afternoon"]
    refs = m.infer_many(_with_vectors(reqs, RecordingEmotion()), **GREEDY)
    assert rec.calls == ["so very angry", "what a gloomy afternoon"]
    for o, r in zip(outs, refs):
        assert np.array_equal(o[1], r[1])
    assert not np.array_equal(outs[0][1], outs[2][1])


def test_infer_many_without_the_qwen_directory_fails_that_request_alone():
    m = _tts()
    assert m.qwen_emo is None
    plain = dict(spk_audio_prompt="spk.wav", text="hello world")
    reqs = [dict(plain, use_emo_text=True, emo_text="x", emo_alpha=0.6), plain, dict(plain, text="another plain one")]
    outs = m.infer_many(reqs, **GREEDY)
    with pytest.raises(NotImplementedError, match="qwen_emo_path"):
        raise outs[0]
    assert all(isinstance(o, tuple) and o[0] == 22050 and o[1].size for o in outs[1:])
    # the request with an emotion clip beside use_emo_text fails the same way, alone
    outs = m.infer_many(_requests("x"), **GREEDY)
    for o in outs[:2]:
        assert isinstance(o, NotImplementedError) and "qwen_emo_path" in str(o)
    assert isinstance(outs[2], tuple) and outs[2][1].size
