"""`IndexTTS2(..., use_fp16=True, gpt_dtype="f16")`: the served defaults with the GPT in IEEE half, the reference's own
precision under `use_fp16`.  A two-segment text takes the beam-group path (two groups of three beams on the wide engine), and
every engine the model creates has the resolved type."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tts_f16_from_dir(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_f16"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=True, gpt_dtype="f16", device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM


def test_infer_with_an_f16_gpt_under_the_served_defaults(tts_f16_from_dir, monkeypatch):
    from voice_tts_amd import scheduler as SCH

    m, SM = tts_f16_from_dir
    monkeypatch.delenv("IXTTS_BEAM_GROUPS", raising=False)
    assert m.use_fp16 and m.gpt_dtype == "f16" and m.gpt.dtype == "f16"
    runs = []
    real_run = SCH.BeamGroupScheduler.run

    def spy(self, segments, on_done, **kw):
        st = real_run(self, segments, on_done, **kw)
        runs.append((self.engine, len(segments)))
        return st

    monkeypatch.setattr(SCH.BeamGroupScheduler, "run", spy)
    wav = SM.synthetic_wav_bytes(1.5, 24000)
    sr, pcm = m.infer(wav, "Hello world, this is a test. 你好世界！", None, max_text_tokens_per_segment=20, max_mel_tokens=24, seed=4)
    assert sr == 22050 and pcm.dtype == np.int16 and pcm.ndim == 2 and pcm.shape[1] == 1
    assert np.isfinite(pcm.astype(np.float64)).all() and int(np.abs(pcm.astype(np.int32)).max()) <= 32767
    # two segments -> two beam groups stepping together on the wide engine, which is fp16 like the model's own
    assert len(runs) == 1 and runs[0][1] == 2, runs
    eng = runs[0][0]
    assert eng.dtype == "f16" and eng.max_batch >= 6 and eng is not m.gpt
    assert m._engines and all(e.dtype == "f16" for e in m._engines.values())
    # every segment yields between 1 and 24 codes -> frames; 200 ms of silence between the two segments
    sil = int(22050 * 0.2)
    assert sil + 2 * 256 <= pcm.shape[0] <= sil + 2 * int(24 * 1.72) * 256, pcm.shape
