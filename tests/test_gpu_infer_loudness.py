"""`output_loudness` / `output_peak` through `infer` and `infer_many`, over the tiny model of tests/synthetic_model_dir.py (the request
and settings of tests/test_gpu_infer_output_format.py, so the segment lengths are ones the suite has already run)."""
import math
import os
import sys
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TEXT = "Hello world, this is a test. One more sentence follows here."
KW = dict(max_mel_tokens=16, max_text_tokens_per_segment=20)
CEILING = 32768.0 * 10.0 ** (-1.0 / 20.0)  # the default ceiling beside a loudness target, -1 dBFS


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_loudness"))
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


def _blocks(pcm, sr):
    import loudness_ref as LR
    from voice_tts_amd import output as O

    z = LR.block_powers(LR.hop_energies(pcm.astype(np.float64), sr), O.hop_len(sr))
    with np.errstate(divide="ignore"):
        return z, -0.691 + 10.0 * np.log10(z)


@pytest.mark.parametrize("rate", [None, 8000])
@pytest.mark.parametrize("target", [-23.0, -16.0])
def test_the_delivered_audio_reads_the_target(tts, target, rate):
    """The twin reads the delivered int16 within 0.01 LU of the target: truncation toward zero biases a sample by at most 1 LSB and by
    0.5 LSB on average, against an RMS of thousands of LSB at these targets (-23 LUFS is an RMS of about 2300 LSB).  Where the report
    says the ceiling bound the gain, the delivered peak is the ceiling within 1 LSB instead."""
    import loudness_ref as LR

    m, wav_a = tts
    sr, pcm = _seeded(m, wav_a, TEXT, None, output_loudness=target, output_sample_rate=rate, seed=5, **KW)
    rep = m.last_loudness
    assert sr == (rate or 22050) and pcm.dtype == np.int16 and pcm.shape[1] == 1
    assert set(rep) == {"measured_lufs", "gain_db", "peak_dbfs_in", "target_met"} and rep["measured_lufs"] is not None
    got = LR.loudness(pcm[:, 0].astype(np.float64), sr)
    print(f"target {target} at {sr} Hz: report {rep}, delivered {got:.4f} LUFS, peak {np.abs(pcm.astype(np.int32)).max()}")
    # the condition on the input: the absolute gate is the one part that does not commute with a gain, so no block of the programme
    # may sit within |gain| + 1 dB of -70 LUFS, digital silence (and the filter's dying ring inside it) apart
    z, l = _blocks(pcm[:, 0], sr)
    near = (np.abs(l + 70.0) < abs(rep["gain_db"]) + 1.0) & (z > 1e-15)
    assert not near.any(), l[near]
    if rep["target_met"]:
        assert abs(got - target) <= 0.01, (got, target)
        assert abs(rep["measured_lufs"] + rep["gain_db"] - target) < 1e-4
        assert np.abs(pcm.astype(np.int32)).max() <= CEILING
    else:
        assert abs(np.abs(pcm.astype(np.int32)).max() - CEILING) <= 1.0 and got < target


def test_g711_of_a_levelled_request_is_g711_of_its_pcm(tts):
    from voice_tts_amd import output as O

    m, wav_a = tts
    kw = dict(output_loudness=-20.0, output_peak=-2.0, output_sample_rate=8000, seed=5, **KW)
    sr, pcm = _seeded(m, wav_a, TEXT, None, **kw)
    rep = m.last_loudness
    sr_u, ulaw = _seeded(m, wav_a, TEXT, None, output_encoding="mulaw", **kw)
    assert sr == sr_u == 8000 and ulaw.dtype == np.uint8 and m.last_loudness == rep
    assert np.array_equal(ulaw[:, 0], O.g711_encode(pcm[:, 0], "mulaw"))


def test_file_return_and_length_agree(tts, tmp_path):
    m, wav_a = tts
    out = str(tmp_path / "levelled.wav")
    assert _seeded(m, wav_a, TEXT, out, output_loudness=-23.0, seed=5, **KW) == out
    length, rep = m.last_timing["audio_length"], m.last_loudness
    with wave.open(out, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 22050)
        frames = w.readframes(w.getnframes())
    sr, pcm = _seeded(m, wav_a, TEXT, None, output_loudness=-23.0, seed=5, **KW)
    assert sr == 22050 and pcm.astype("<i2").tobytes() == frames and m.last_loudness == rep
    assert abs(length - pcm.shape[0] / 22050.0) < 1e-12 and abs(m.last_timing["audio_length"] - length) < 1e-12


def test_without_a_control_nothing_changes(tts, monkeypatch):
    from voice_tts_amd import output as O

    m, wav_a = tts
    real = O.finish
    entered = []

    def guard(*a, **kw):
        entered.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(O, "finish", guard)
    sr0, pcm0 = _seeded(m, wav_a, TEXT, None, seed=5, **KW)
    assert not entered and m.last_loudness is None and sr0 == 22050 and pcm0.dtype == np.int16  # the host path, as ever
    # a ceiling of 0 dBFS can never bind: the request goes through the device stage with a gain of exactly 1 and gives the same samples
    sr1, pcm1 = _seeded(m, wav_a, TEXT, None, output_peak=0.0, seed=5, **KW)
    assert len(entered) == 1 and sr1 == 22050 and np.array_equal(pcm1, pcm0)
    assert m.last_loudness["gain_db"] == 0.0 and m.last_loudness["target_met"] is True
    for kw in (dict(output_loudness=-23.0), dict(output_peak=-3.0)):
        with pytest.raises(ValueError, match="stream_return"):
            m.infer(wav_a, TEXT, None, stream_return=True, **kw, **KW)
    assert len(entered) == 1


def test_infer_many_levels_each_request_on_its_own(tts, monkeypatch):
    from voice_tts_amd import output as O

    m, wav_a = tts
    P = dict(spk_audio_prompt=wav_a, text=TEXT, generation={"seed": 5})
    A = dict(P, loudness=-23.0)
    seen = []
    real, finish = O.finish_pcm_many, O.finish

    def spy(wav_lists, specs, interval_silence=200):
        seen.append(([[w.clone() for w in ws] for ws in wav_lists], list(specs), interval_silence))
        return finish(wav_lists, specs, interval_silence)

    monkeypatch.setattr(O, "finish", spy)
    alone = m.infer_many([A], decode_slots=8, **KW)
    rep = m.last_loudness
    assert isinstance(alone[0], tuple) and alone[0][0] == 22050 and len(rep) == 1 and rep[0]["measured_lufs"] is not None
    outs = m.infer_many([dict(P, sample_rate=16000), A, dict(P, sample_rate=8000, encoding="mulaw", loudness=-16.0, peak=-6.0), dict(P, loudness=-3.0), P],
                        decode_slots=8, **KW)
    reps = m.last_loudness
    assert isinstance(outs[3], ValueError) and all(isinstance(outs[k], tuple) for k in (0, 1, 2, 4)), outs  # the bad value fails alone
    assert outs[1][0] == 22050 and np.array_equal(outs[1][1], alone[0][1]) and reps[1] == rep[0]  # alone and in the batch: the same bytes
    assert reps[0] is None and reps[3] is None and reps[4] is None and reps[2] is not None and outs[2][1].dtype == np.uint8
    # the request that asks for a rate and no level: its spec asks for the rate alone, its bytes are those of the list form without a level
    lists, specs, _ = seen[-1]
    assert len(seen) == 2 and [s.loudness for s in specs] == [None, -23.0, -16.0] and specs[0] == O.OutputSpec.of(sample_rate=16000)
    parent = real([lists[0]], [16000], [None], 200)[0]
    assert outs[0][0] == parent[0] == 16000 and np.array_equal(outs[0][1], parent[1])
    # a call-wide target holds for every request that does not bring its own
    outs = m.infer_many([P, dict(P, loudness=-30.0)], decode_slots=8, output_loudness=-20.0, **KW)
    a, b = m.last_loudness
    assert all(isinstance(o, tuple) for o in outs) and abs(a["measured_lufs"] - b["measured_lufs"]) < 1e-9
    if a["target_met"] and b["target_met"]:
        assert abs((a["gain_db"] - b["gain_db"]) - 10.0) < 1e-3
    # and a call without any level asks for the rate alone
    m.infer_many([dict(P, sample_rate=16000)], decode_slots=8, **KW)
    assert seen[-1][1] == [O.OutputSpec.of(sample_rate=16000)] and m.last_loudness == [None]
