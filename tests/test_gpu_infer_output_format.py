"""`output_sample_rate` / `output_encoding` through `infer`, `infer_generator` (streaming) and `infer_many`, over the tiny model of
tests/synthetic_model_dir.py.

The request is a pinned one of tests/test_gpu_infer_many_generation.py under that file's settings, so its segment lengths are ones
the suite has already run (see the note on TunableOp state in tests/test_gpu_infer_many_vocoder.py)."""
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


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_output_format"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM.synthetic_wav_bytes(1.5, 24000)


def test_infer_many_serves_a_pinned_request_in_three_formats(tts, monkeypatch):
    import output_ref as REF
    from voice_tts_amd import output as O

    m, wav_a = tts
    P = dict(spk_audio_prompt=wav_a, text=TEXT, generation={"seed": 5})
    reqs = [P, dict(P, sample_rate=16000), dict(P, sample_rate=8000, encoding="mulaw")]
    seen = []
    real, finish = O.finish_pcm_many, O.finish

    def spy(wav_lists, specs, interval_silence=200):
        seen.append(([[w.clone() for w in ws] for ws in wav_lists], list(specs), interval_silence))
        return finish(wav_lists, specs, interval_silence)

    monkeypatch.setattr(O, "finish", spy)
    outs = m.infer_many(reqs, decode_slots=8, **KW)
    assert all(isinstance(o, tuple) for o in outs), outs
    assert len(seen) == 1
    audio = m.last_timing["audio_length"]
    alone = m.infer_many([P], decode_slots=8, **KW)
    assert len(seen) == 1  # a call that asks for nothing never enters the output stage
    # the plain request: what the call without the other two gives -- existing behaviour is untouched
    assert outs[0][0] == alone[0][0] == 22050 and outs[0][1].dtype == np.int16 and np.array_equal(outs[0][1], alone[0][1])
    lists, specs, interval = seen[0]
    assert specs == [O.OutputSpec.of(sample_rate=16000), O.OutputSpec.of(sample_rate=8000, encoding="mulaw")] and interval == 200
    rates, encs = [16000, 8000], [None, "mulaw"]
    assert abs(audio - sum(o[1].shape[0] / o[0] for o in outs)) < 1e-9
    for ws, sr, enc, (got_sr, got) in zip(lists, rates, encs, outs[1:]):
        assert len(ws) >= 2 and all(w.dtype == torch.float32 and w.is_cuda and w.shape[0] == 1 for w in ws)
        one_sr, one = real([ws], [sr], [enc], interval)[0]  # `finish_pcm` of these segments, alone
        assert got_sr == one_sr == sr and got.dtype == one.dtype == (np.uint8 if enc == "mulaw" else np.int16)
        assert np.array_equal(got, one)
        lens = [O.resampled_len(w.shape[1], 22050, sr) for w in ws]
        gap = int(sr * interval / 1000.0)
        assert got.shape == (sum(lens) + gap * (len(ws) - 1), 1)
        # the resampled floats against fp64 on the same table, and the bytes as their conversion with the zero code in the gaps
        rows = O.Resampler(sr, ws[0].device).forward_many(ws)
        want, at = np.full(got.shape[0], O.ZERO_CODES["mulaw" if enc == "mulaw" else "pcm_s16le"], got.dtype), 0
        for w, r, n in zip(ws, rows, lens):
            y = r.cpu().numpy()[0].astype(np.float64)
            ref, bound = REF.resample_fp64(w.cpu().numpy()[0], sr)
            assert y.size == n and (np.abs(y - ref) <= bound).all()
            s16 = r.cpu().numpy()[0].astype(np.int16)  # truncation toward zero
            want[at:at + n] = O.g711_encode(s16, "mulaw") if enc == "mulaw" else s16
            at += n + gap
        assert np.array_equal(got[:, 0], want)
    # pinned: the three requests brought the same segments, and the plain result is their host-side cat and cast
    for a, b in zip(*lists):
        assert torch.equal(a, b)
    sil = torch.zeros(1, int(22050 * interval / 1000.0))
    parts = sum([[w.cpu(), sil] for w in lists[0]], [])[:-1]
    assert np.array_equal(outs[0][1], torch.cat(parts, dim=1).type(torch.int16).numpy().T)
    # a value outside the sets fails its request alone
    outs = m.infer_many([dict(P, sample_rate=12345), dict(P, encoding="alaw")], decode_slots=8, **KW)
    assert isinstance(outs[0], ValueError) and isinstance(outs[1], tuple) and outs[1][0] == 22050 and outs[1][1].dtype == np.uint8


def _seeded(m, *a, **kw):
    """`infer` with torch's generators reseeded first: outside a pinned `infer_many` request the s2mel noise comes from the default
    generator, so two calls compare only when both start from the same state (`seed=` covers the decode alone)."""
    torch.manual_seed(11)
    return m.infer(*a, **kw)


def test_infer_writes_the_file_at_the_requested_rate(tts, tmp_path):
    m, wav_a = tts
    out = str(tmp_path / "sub" / "out24k.wav")
    assert _seeded(m, wav_a, TEXT, out, output_sample_rate=24000, seed=5, **KW) == out
    length = m.last_timing["audio_length"]
    with wave.open(out, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 24000)
        frames = w.readframes(w.getnframes())
    sr, pcm = _seeded(m, wav_a, TEXT, None, output_sample_rate=24000, seed=5, **KW)
    assert sr == 24000 and pcm.dtype == np.int16 and pcm.shape[1] == 1 and pcm.astype("<i2").tobytes() == frames
    assert abs(length - pcm.shape[0] / 24000.0) < 1e-12 and abs(m.last_timing["audio_length"] - length) < 1e-12
    # an encoding alone: the plain call's samples, each through G.711
    sr0, pcm0 = _seeded(m, wav_a, TEXT, None, seed=5, **KW)
    assert sr0 == 22050 and pcm0.dtype == np.int16
    sr_a, alaw = _seeded(m, wav_a, TEXT, None, output_encoding="alaw", seed=5, **KW)
    from voice_tts_amd import output as O

    assert sr_a == 22050 and alaw.dtype == np.uint8 and np.array_equal(alaw[:, 0], O.g711_encode(pcm0[:, 0], "alaw"))


def test_stream_return_yields_segments_and_silences_of_the_new_lengths(tts):
    from voice_tts_amd import output as O

    m, wav_a = tts
    plain = list(_seeded(m, wav_a, TEXT, None, stream_return=True, seed=5, **KW))
    got = list(_seeded(m, wav_a, TEXT, None, stream_return=True, output_sample_rate=16000, seed=5, **KW))
    assert len(got) == len(plain) >= 4 and len(got) % 2 == 0
    for k, (a, b) in enumerate(zip(plain, got)):
        assert isinstance(b, torch.Tensor) and b.dtype == torch.float32 and not b.is_cuda and b.shape[0] == 1
        if k % 2 == 0:  # a segment: the resampled, clamped fp32 row
            assert b.shape[1] == O.resampled_len(a.shape[1], 22050, 16000)
            assert float(b.abs().max()) <= 32767.0
            assert torch.equal(b, O.Resampler(16000, "cuda:0").forward_many([a.to("cuda:0")])[0].cpu())
        else:  # the silence
            assert tuple(a.shape) == (1, 4410) and tuple(b.shape) == (1, 3200) and not b.any()
    with pytest.raises(ValueError, match="stream_return"):
        m.infer(wav_a, TEXT, None, stream_return=True, output_encoding="mulaw", **KW)
