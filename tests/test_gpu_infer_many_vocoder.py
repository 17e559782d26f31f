"""`IndexTTS2.infer_many` sends the mels of all its requests through ONE batched vocoder pass (`pipeline.vocode_many` ->
`BigVGAN.forward_many`): the PCM is exactly what the per-segment passes give (IXTTS_BV_BATCH=0), and a request with a bad prompt
still fails alone.

The requests are pinned ones of tests/test_gpu_infer_many_generation.py, under its settings: their codes, and so their segment
lengths, are the ones that file has already run.  (The s2mel stage re-keys its tuned GEMM entries per segment length into
process-wide TunableOp state, first registration winning: a test that brings new lengths changes which library kernel a LATER
test's GEMMs get, and with it the last bits of that test's PCM.)"""
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

    root = str(tmp_path_factory.mktemp("model_dir_vocoder"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM


def test_infer_many_vocodes_all_requests_together(tts_from_dir, monkeypatch):
    m, SM = tts_from_dir
    monkeypatch.delenv("IXTTS_BV_BATCH", raising=False)
    wav_a, wav_b = SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1)
    reqs = [dict(spk_audio_prompt=wav_a, text="Hello world, this is a test.", generation={"num_beams": 1, "seed": 2}),
            dict(spk_audio_prompt=b"this is not audio at all", text="Broken prompt.", generation={"seed": 1}),
            dict(spk_audio_prompt=wav_b, text="A second voice says this.", generation={"temperature": 1.2, "top_k": 50, "seed": 3}),
            dict(spk_audio_prompt=wav_a, text="Short.", generation={"top_k": 1})]
    kw = dict(decode_slots=8, num_beams=1, max_mel_tokens=16)
    calls = []
    real = m.bigvgan.forward_varlen
    monkeypatch.setattr(m.bigvgan, "forward_varlen", lambda mel, frames, **k: (calls.append(list(frames)), real(mel, frames, **k))[1])
    outs = m.infer_many(reqs, **kw)
    assert isinstance(outs[1], Exception) and all(isinstance(outs[i], tuple) for i in (0, 2, 3))
    assert len(calls) == 1 and len(calls[0]) >= 3  # the segments of the three good requests in one pass
    monkeypatch.setenv("IXTTS_BV_BATCH", "0")
    outs0 = m.infer_many(reqs, **kw)
    assert len(calls) == 1  # switched off: one pass per segment
    assert isinstance(outs0[1], Exception) and type(outs0[1]) is type(outs[1])
    for i in (0, 2, 3):
        assert outs[i][0] == outs0[i][0] == 22050 and outs[i][1].dtype == np.int16 and outs[i][1].shape[0] > 0
        assert np.array_equal(outs[i][1], outs0[i][1]), i
