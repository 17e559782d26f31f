"""GPU: `IndexTTS2.infer(use_emo_text=True, ...)` with a Qwen3 twin as the emotion model (infer_v2.py:475-499)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qwen_twin as T  # noqa: E402
from test_gpu_infer_v2 import FakeGlue  # noqa: E402


def _tts(qwen_emo=None, model_dir="/nonexistent", cfg_path=None):
    import voice_tts_amd.weights as WR
    from indextts.infer_v2 import IndexTTS2

    gcfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    bcfg = WR.tiny_bigvgan_cfg(64)
    glue = FakeGlue(128, torch.device("cuda:0"))
    return IndexTTS2(cfg_path=cfg_path, model_dir=model_dir, device="cuda:0", glue=glue, gpt_state_dict=WR.make_gpt_weights(gcfg, seed=7),
                     bigvgan_state_dict=WR.make_bigvgan_weights(bcfg, seed=8), gpt_cfg=gcfg, bigvgan_cfg=bcfg, max_seq=192, max_frames=128,
                     qwen_emo=qwen_emo)


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    from voice_tts_amd.qwen_emotion import QwenEmotion

    d = str(tmp_path_factory.mktemp("qwen") / "qwen0.6bemo4-merge")
    T.write_twin(d, seed=5, layers=2)
    q = QwenEmotion(d, dtype="f32", device="cuda:0", max_seq=160)
    return _tts(qwen_emo=q), q


GREEDY = dict(num_beams=1, top_k=1, max_mel_tokens=12)


def test_emo_text_equals_its_emotion_vector(tts):
    m, q = tts
    T_ = "I am so happy today!"
    vec = list(q.inference(T_).values())
    assert len(vec) == 8
    a = m.infer("spk.wav", "hello world", None, use_emo_text=True, emo_text=T_, emo_alpha=0.6, **GREEDY)
    b = m.infer("spk.wav", "hello world", None, emo_vector=vec, emo_alpha=0.6, **GREEDY)
    assert a[0] == b[0] == 22050 and np.array_equal(a[1], b[1])
    assert m.last_timing["gpt_gen_time"] > 0


def test_emo_text_defaults_to_text_and_ignores_emotion_clip(tts):
    m, q = tts
    text = "what a gloomy afternoon"
    vec = list(q.inference(text).values())
    a = m.infer("spk.wav", text, None, use_emo_text=True, emo_alpha=0.6, **GREEDY)
    b = m.infer("spk.wav", text, None, emo_vector=vec, emo_alpha=0.6, **GREEDY)
    c = m.infer("spk.wav", text, None, emo_audio_prompt="angry.wav", use_emo_text=True, emo_alpha=0.6, **GREEDY)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[1], c[1])


def test_model_dir_loads_qwen_emo_path(tmp_path):
    from voice_tts_amd.qwen_emotion import QwenEmotion

    d = tmp_path / "md"
    T.write_twin(str(d / "qwen_emo"), seed=6, layers=1)
    (d / "config.yaml").write_text("qwen_emo_path: qwen_emo\n")
    m = _tts(model_dir=str(d), cfg_path=str(d / "config.yaml"))
    assert isinstance(m.qwen_emo, QwenEmotion) and m.qwen_emo.engine.dtype == "f16"


def test_without_qwen_dir_the_error_names_qwen_emo_path():
    m = _tts()
    assert m.qwen_emo is None
    with pytest.raises(NotImplementedError, match="qwen_emo_path"):
        m.infer("spk.wav", "hello", None, use_emo_text=True, **GREEDY)


class RecordingEmotion:
    """Stands where QwenEmotion stands: records the text it is asked about and answers a vector that depends on it."""

    def __init__(self):
        self.calls = []

    def inference(self, text):
        self.calls.append(text)
        v = [((len(text) * (i + 3)) % 7) / 10 for i in range(8)]
        return dict(zip(["happy", "angry", "sad", "afraid", "disgusted", "melancholic", "surprised", "calm"], v))


@pytest.fixture(scope="module")
def rec_tts():
    rec = RecordingEmotion()
    return _tts(qwen_emo=rec), rec


def test_the_emotion_text_is_what_reaches_the_model(rec_tts):
    m, rec = rec_tts
    a = m.infer("spk.wav", "hello world", None, use_emo_text=True, emo_text="so very angry", emo_alpha=0.6, **GREEDY)
    assert rec.calls == ["so very angry"]
    b = m.infer("spk.wav", "hello world", None, emo_vector=list(rec.inference("so very angry").values()), emo_alpha=0.6, **GREEDY)
    assert np.array_equal(a[1], b[1])
    # emo_text=None: the text itself; a given emotion clip is ignored
    rec.calls.clear()
    c = m.infer("spk.wav", "a different text", None, use_emo_text=True, emo_audio_prompt="angry.wav", emo_alpha=0.6, **GREEDY)
    assert rec.calls == ["a different text"]
    d = m.infer("spk.wav", "a different text", None, emo_vector=list(rec.inference("a different text").values()), emo_alpha=0.6, **GREEDY)
    assert np.array_equal(c[1], d[1])
