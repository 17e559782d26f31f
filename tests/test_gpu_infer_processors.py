"""GPU: the processor keywords of HF `generate()` -- sequence_bias, bad_words_ids, forced_eos_token_id and the scalars -- through
`IndexTTS2.infer` (the `generate()` path of a one-segment text and the scheduler path of a two-segment text) and as keys of a
request's `generation` dict in `infer_many`, over the synthetic model directory."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_infer_constraints import ONE, TWO, _Decoded, _model, _run, wavs  # noqa: E402,F401  (fixtures and helpers of the sibling file)


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    return _model(str(tmp_path_factory.mktemp("model_dir_processors")))


def _decoded_ids(m, wav, text, **kw):
    """The ids of every segment (stop token included) as `infer` decodes them, on either path; the request ends there."""
    rows = []
    real_decode, real_generate = m._decode, m.gpt.generate

    def decode_spy(engine, todo, g):
        out = real_decode(engine, todo, g)
        rows.extend(np.asarray(out[k]).tolist() for k in sorted(out))
        return out

    def generate_spy(fake, *a, **k):
        out = real_generate(fake, *a, **k)
        rows.append(out[0, fake.shape[1]:].tolist())
        raise _Decoded()  # one segment: nothing else to decode

    def trim_spy(ids):
        raise _Decoded()

    m._decode, m.gpt.generate, m._trim_codes = decode_spy, generate_spy, trim_spy
    try:
        with pytest.raises(_Decoded):
            m.infer(wav, text, None, max_text_tokens_per_segment=20, num_beams=1, top_k=1, **kw)
    finally:
        del m._decode, m.gpt.generate, m._trim_codes
    return rows


@pytest.mark.parametrize("text,segments", [(ONE, 1), (TWO, 2)])
def test_infer_forced_eos_and_sequence_bias_on_the_generate_path_and_the_scheduler_path(tts, wavs, text, segments):
    m, wav = tts, wavs[0]
    stop = m.stop_mel_token
    cap = 12
    free = _decoded_ids(m, wav, text, max_mel_tokens=cap)
    assert (len(free) == 1) if segments == 1 else (len(free) >= 2)
    assert all(len(r) == cap and stop not in r for r in free)  # the synthetic model never stops by itself: every segment runs to its cap
    got = _decoded_ids(m, wav, text, max_mel_tokens=cap, forced_eos_token_id=stop)
    assert got == [r[:cap - 1] + [stop] for r in free], got  # the stop token is guaranteed at the cap
    # a bias on one code changes the codes from where that code stood
    code = free[0][3]
    at = free[0].index(code)
    biased = _decoded_ids(m, wav, text, max_mel_tokens=cap, sequence_bias={(code,): -1000.0})
    assert biased[0][:at] == free[0][:at] and biased[0][at] != code and code not in biased[0]
    # the same through a two-id bad word: only the continuation after its first id is banned
    if at > 0:
        word = [free[0][at - 1], code]
        banned = _decoded_ids(m, wav, text, max_mel_tokens=cap, bad_words_ids=[word])
        assert banned[0][:at] == free[0][:at] and banned[0][at] != code
    # to the end of the pipeline with every keyword set
    out = m.infer(wav, text, None, max_text_tokens_per_segment=20, num_beams=1, top_k=5, max_mel_tokens=cap, forced_eos_token_id=[stop],
                  sequence_bias=[[[code], -3.0]], bad_words_ids=[[1, 2]], exponential_decay_length_penalty=(4, 1.05), epsilon_cutoff=1e-4, eta_cutoff=1e-4,
                  renormalize_logits=True)
    assert out is not None and out[0] == 22050 and out[1].shape[0] > 0


def test_processor_keys_in_one_requests_generation_dict_leave_the_others_alone(tts, wavs):
    m, (wav_a, wav_b) = tts, wavs
    stop = m.stop_mel_token
    kw = dict(decode_slots=8, num_beams=1, max_mel_tokens=16)
    plain = _run(m, [dict(spk_audio_prompt=wav_a, text=ONE, generation={"seed": 2})], **kw)[0]
    assert isinstance(plain[0], bytes) and len(plain[1]) == 1 and stop not in plain[1][0]
    code = plain[1][0][2]
    gen = {"seed": 2, "forced_eos_token_id": stop, "sequence_bias": [[[code], -1000.0]], "bad_words_ids": [[plain[1][0][0], plain[1][0][1]]],
           "exponential_decay_length_penalty": [2, 1.01], "epsilon_cutoff": 1e-4, "renormalize_logits": True}
    C = dict(spk_audio_prompt=wav_a, text=ONE, generation=gen)
    U1 = dict(spk_audio_prompt=wav_b, text="A second voice says this.", generation={"seed": 1})
    U2 = dict(spk_audio_prompt=wav_a, text="Short.", generation={"top_k": 1})
    c_alone, u1_alone, u2_alone = (_run(m, [r], **kw)[0] for r in (C, U1, U2))
    for r in (c_alone, u1_alone, u2_alone):
        assert isinstance(r[0], bytes) and len(r[0]) > 0, r[0]
    codes = c_alone[1][0]
    assert codes[-1] == stop and len(codes) == 16 and code not in codes and codes[:2] != plain[1][0][:2] and codes != plain[1][0]
    assert _run(m, [C, U1, U2], **kw) == [c_alone, u1_alone, u2_alone]  # codes and PCM, byte for byte
    assert _run(m, [U2, C, U1], **kw) == [u2_alone, c_alone, u1_alone]
    assert _run(m, [U1, U2], **kw) == [u1_alone, u2_alone]  # and the others are what they are without it


def test_a_refused_processor_value_fails_its_request_only(tts, wavs):
    m, (wav_a, wav_b) = tts, wavs
    ok = dict(spk_audio_prompt=wav_a, text="Hello world.")
    for gen, word in (({"sequence_bias": {}}, "sequence_bias"), ({"bad_words_ids": [[10 ** 6]]}, "outside"), ({"epsilon_cutoff": 1.0}, "epsilon_cutoff"),
                      ({"sequence_bias": [[list(range(9)), 1.0]]}, "IXTTS_SEQ_BIAS_LEN"), ({"forced_eos_token_id": -3}, "forced_eos_token_id")):
        bad = dict(spk_audio_prompt=wav_a, text="Hello world.", generation=gen)
        outs = m.infer_many([ok, bad], decode_slots=4, num_beams=1, top_k=1, max_mel_tokens=8)
        assert isinstance(outs[1], ValueError) and word in str(outs[1]), (gen, outs[1])
        assert isinstance(outs[0], tuple) and outs[0][1].shape[0] > 0
