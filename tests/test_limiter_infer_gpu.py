"""`output_limiter` / `output_peak_mode` through `infer` and `infer_many`, over the tiny model of tests/synthetic_model_dir.py (the request
and settings of tests/test_gpu_infer_loudness.py, so the segment lengths are ones the suite has already run).

(The file sorts behind every tests/test_gpu_*.py on purpose, as tests/test_speed_duration_gpu.py does: placed before
tests/test_gpu_infer_loudness.py it registered those lengths first, and tests/test_gpu_infer_parent.py then missed its recording by one
LSB in six samples -- see the note on TunableOp state in tests/test_gpu_infer_many_vocoder.py.)

`infer` and a pinned `infer_many` request do not synthesise the same samples (the s2mel noise of the one comes from torch's default
generator, of the other from the request's seed), so "the same bytes as `infer`" is held where it can be: the segments `infer_many`
hands to the output stage, put through `output.finish_pcm` with the keywords `infer` passes, give the bytes and the report
`infer_many` returned."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TEXT = "Hello world, this is a test. One more sentence follows here."
KW = dict(max_mel_tokens=16, max_text_tokens_per_segment=20)
CEILING = 32768.0 * 10.0 ** (-1.0 / 20.0)
OLD_KEYS = {"measured_lufs", "gain_db", "peak_dbfs_in", "target_met"}
NEW_KEYS = OLD_KEYS | {"peak_mode", "limited", "max_reduction_db", "limited_fraction", "delivered_lufs", "delivered_peak_dbfs"}


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_limiter"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM.synthetic_wav_bytes(1.5, 24000)


def _seeded(m, *a, **kw):
    """`infer` with torch's generators reseeded first (the s2mel noise of an unpinned request comes from the default generator)."""
    torch.manual_seed(11)
    return m.infer(*a, **kw)


def test_the_limiter_delivers_the_target_the_ceiling_used_to_cost(tts, monkeypatch):
    """8 kHz, -16 LUFS: the case DESIGN 4.3c reports as bound by its ceiling.  0.01 LU between the report and the twin's reading of the
    delivered int16 is 4.3c's bound for the truncation toward zero."""
    import loudness_ref as LR
    from voice_tts_amd import output as O

    m, wav_a = tts
    seen = []
    real = O.finish

    def spy(wav_lists, specs, interval_silence=200):
        seen.append(list(specs))
        return real(wav_lists, specs, interval_silence)

    monkeypatch.setattr(O, "finish", spy)
    kw = dict(output_sample_rate=8000, output_loudness=-16.0, seed=5, **KW)
    sr0, pcm0 = _seeded(m, wav_a, TEXT, None, **kw)
    old = m.last_loudness
    assert set(old) == OLD_KEYS and old["target_met"] is False and seen[-1][0].limits == ("sample", False)  # as it is today
    assert abs(int(np.abs(pcm0.astype(np.int32)).max()) - CEILING) <= 1.0
    sr, pcm = _seeded(m, wav_a, TEXT, None, output_limiter=True, **kw)
    rep = m.last_loudness
    assert len(seen[-1]) == 1 and seen[-1][0].limits == ("sample", True)
    got = LR.loudness(pcm[:, 0].astype(np.float64), sr)
    print(f"without the limiter: {old}\nwith it: {rep}\ndelivered {got:.4f} LUFS, peak {np.abs(pcm.astype(np.int32)).max()} (ceiling {CEILING:.1f})")
    assert sr == sr0 == 8000 and pcm.dtype == np.int16 and pcm.shape == pcm0.shape and set(rep) == NEW_KEYS
    assert abs(got + 16.0) <= O.LOUDNESS_TOLERANCE_LU and rep["target_met"] is True
    assert abs(rep["delivered_lufs"] - got) <= 0.01
    assert int(np.abs(pcm.astype(np.int32)).max()) <= math.floor(CEILING)
    assert rep["peak_mode"] == "sample" and rep["limited"] is True and rep["max_reduction_db"] < 0.0 and 0.0 < rep["limited_fraction"] < 1.0
    assert rep["measured_lufs"] == old["measured_lufs"] and rep["peak_dbfs_in"] == old["peak_dbfs_in"]
    assert abs(rep["measured_lufs"] + rep["gain_db"] + 16.0) < 1e-4 and rep["gain_db"] > old["gain_db"]  # the full gain: no give-way
    assert rep["delivered_peak_dbfs"] <= -1.0 + 1e-6
    # the same call without the limiter still is what it was
    sr1, pcm1 = _seeded(m, wav_a, TEXT, None, **kw)
    assert np.array_equal(pcm1, pcm0) and m.last_loudness == old


def test_a_true_peak_ceiling(tts):
    import limiter_ref as LM

    m, wav_a = tts
    kw = dict(output_sample_rate=8000, output_loudness=-16.0, output_peak=-1.0, seed=5, **KW)
    sr, pcm = _seeded(m, wav_a, TEXT, None, output_peak_mode="true", **kw)
    rep = m.last_loudness
    _seeded(m, wav_a, TEXT, None, output_peak_mode="sample", **kw)
    sample = m.last_loudness
    tp = LM.true_peak(pcm[:, 0].astype(np.float32))
    print(f"true mode: {rep}\nsample mode: {sample}\ntrue peak of the delivered int16: {tp:.2f} (ceiling {CEILING:.2f}), sample peak {np.abs(pcm.astype(np.int32)).max()}")
    assert set(rep) == NEW_KEYS and rep["peak_mode"] == "true" and rep["limited"] is False and set(sample) == OLD_KEYS
    assert tp <= CEILING + 1.0  # one LSB's worth for the truncation to int16
    assert rep["gain_db"] <= sample["gain_db"] and rep["peak_dbfs_in"] >= sample["peak_dbfs_in"] and rep["measured_lufs"] == sample["measured_lufs"]
    assert rep["target_met"] is False and abs(rep["delivered_peak_dbfs"] + 1.0) < 1e-4  # bound by the ceiling: the true peak sits on it


def test_infer_many_takes_the_keys_and_a_bad_value_fails_alone(tts, monkeypatch):
    from voice_tts_amd import output as O

    m, wav_a = tts
    P = dict(spk_audio_prompt=wav_a, text=TEXT, generation={"seed": 5})
    A = dict(P, sample_rate=8000, loudness=-16.0, limiter=True)
    B = dict(P, sample_rate=8000, loudness=-16.0, peak=-1.0, peak_mode="true")
    seen = []
    real, finish = O.finish_pcm_many, O.finish

    def spy(wav_lists, specs, interval_silence=200):
        seen.append(([[w.clone() for w in ws] for ws in wav_lists], list(specs), interval_silence))
        return finish(wav_lists, specs, interval_silence)

    monkeypatch.setattr(O, "finish", spy)
    outs = m.infer_many([A, B, dict(A, limiter="yes"), dict(P, sample_rate=8000, loudness=-16.0)], decode_slots=8, **KW)
    reps = m.last_loudness
    assert isinstance(outs[2], ValueError) and "limiter" in str(outs[2]) and all(isinstance(outs[k], tuple) for k in (0, 1, 3)), outs
    assert set(reps[0]) == NEW_KEYS and set(reps[1]) == NEW_KEYS and reps[2] is None and set(reps[3]) == OLD_KEYS
    lists, specs, _ = seen[-1]
    assert len(seen) == 1 and [s.limits for s in specs] == [("sample", True), ("true", False), ("sample", False)]
    # what `infer` does with such segments: `finish_pcm` under the keywords it passes
    for k, extra in ((0, dict(limiter=True, peak_mode="sample")), (1, dict(peak=-1.0, limiter=False, peak_mode="true"))):
        own = []
        sr, pcm = O.finish_pcm(lists[k], 8000, None, 200, loudness=-16.0, reports=own, **dict(dict(peak=-1.0), **extra))
        assert sr == outs[k][0] == 8000 and np.array_equal(pcm, outs[k][1]) and own[0] == reps[k], k
    # the request without a new control: the bytes of a call without the new arguments
    old = []
    sr, pcm = real([lists[2]], [8000], [None], 200, [-16.0], [-1.0], old)[0]
    assert np.array_equal(pcm, outs[3][1]) and old[0] == reps[3]
    # alone and in the batch: the same bytes
    alone = m.infer_many([A], decode_slots=8, **KW)
    assert np.array_equal(alone[0][1], outs[0][1]) and m.last_loudness[0] == reps[0]
    # call-wide defaults
    outs2 = m.infer_many([dict(P, sample_rate=8000, loudness=-16.0)], decode_slots=8, output_limiter=True, **KW)
    assert np.array_equal(outs2[0][1], outs[0][1]) and m.last_loudness[0] == reps[0]


def test_a_stream_refuses_both_before_any_work(tts, monkeypatch):
    m, wav_a = tts
    monkeypatch.setattr(m, "_prompt_stages", lambda *a, **k: pytest.fail("work was done"))
    for kw in (dict(output_limiter=True), dict(output_peak_mode="true", output_peak=-1.0), dict(output_peak_mode="sample")):
        with pytest.raises(ValueError, match="stream_return"):
            m.infer(wav_a, TEXT, None, stream_return=True, **kw, **KW)
    with pytest.raises(ValueError, match="ceiling"):
        m.infer(wav_a, TEXT, None, output_peak_mode="true", **KW)
    with pytest.raises(ValueError, match="limiter"):
        m.infer(wav_a, TEXT, None, output_limiter=1, **KW)
