"""GPU: the constraint keywords of HF `generate()` through `IndexTTS2.infer` (the `generate()` path of a one-segment text and the
scheduler path of a two-segment text) and as keys of a request's `generation` dict in `infer_many` (the request is pinned: its
codes and PCM are a function of the request alone, with constraints set), over the synthetic model directory."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ONE = "Hello world, this is a test."
TWO = "Hello world, this is a test. One more sentence follows here."


def _model(root, stop_bias=0.0):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    cfg_path, cfg = SM.write_model_dir(root)
    if stop_bias:  # a GPT whose stop token wins every step it may be chosen at (the synthetic one never stops by itself)
        path = os.path.join(root, "gpt.pth")
        ck = torch.load(path)
        ck["model"]["mel_head.bias"] = ck["model"]["mel_head.bias"].clone()
        ck["model"]["mel_head.bias"][cfg["gpt"]["stop_mel_token"]] += stop_bias
        torch.save(ck, path)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    return IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=512)


@pytest.fixture(scope="module")
def wavs():
    import synthetic_model_dir as SM

    return SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1)


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    return _model(str(tmp_path_factory.mktemp("model_dir_constraints")))


@pytest.fixture(scope="module")
def tts_stops(tmp_path_factory):
    """The logits of this model span about -150..170: 400 on the stop token's bias lets it win wherever it is not -inf."""
    return _model(str(tmp_path_factory.mktemp("model_dir_constraints_stop")), stop_bias=400.0)


class _Decoded(Exception):
    pass


def _decoded_lengths(m, wav, text, **kw):
    """Codes per segment (stop token not counted) as `infer` decodes them, on either path; the request ends there."""
    stop = m.stop_mel_token
    counts = []
    real_decode, real_generate = m._decode, m.gpt.generate

    def decode_spy(engine, todo, g):
        out = real_decode(engine, todo, g)
        counts.extend(int((np.asarray(out[k]) != stop).sum()) for k in sorted(out))
        return out

    def generate_spy(fake, *a, **k):
        out = real_generate(fake, *a, **k)
        counts.append(int((out[0, fake.shape[1]:] != stop).sum()))
        raise _Decoded()  # one segment: nothing else to decode

    def trim_spy(ids):
        raise _Decoded()

    m._decode, m.gpt.generate, m._trim_codes = decode_spy, generate_spy, trim_spy
    try:
        with pytest.raises(_Decoded):
            m.infer(wav, text, None, max_text_tokens_per_segment=20, num_beams=1, top_k=1, **kw)
    finally:
        del m._decode, m.gpt.generate, m._trim_codes
    return counts


def _infer_code_counts(m, wav, text, **kw):
    """`infer` to the end -> the number of codes (stop token cut off) of every segment, as they reach the s2mel stage."""
    counts = []
    real = m._trim_codes

    def spy(ids):
        out = real(ids)
        counts.append(int(out.shape[1]))
        return out

    m._trim_codes = spy
    try:
        out = m.infer(wav, text, None, max_text_tokens_per_segment=20, num_beams=1, top_k=1, **kw)
    finally:
        del m._trim_codes
    assert out is not None and out[0] == 22050 and out[1].shape[0] > 0
    return counts


@pytest.mark.parametrize("text,segments", [(ONE, 1), (TWO, 2)])
def test_infer_min_new_tokens_on_the_generate_path_and_the_scheduler_path(tts_stops, wavs, text, segments):
    m, wav = tts_stops, wavs[0]
    free = _decoded_lengths(m, wav, text, max_mel_tokens=24)
    assert (len(free) == 1) if segments == 1 else (len(free) >= 2)
    assert free == [0] * len(free)  # unconstrained: the stop token at once, in every segment
    k = 12
    got = _infer_code_counts(m, wav, text, max_mel_tokens=24, min_new_tokens=k)
    assert got == [k] * len(free), got  # k codes, then the stop token
    # min_length counts the prompt's ids too (P = 34 conditioning rows + the text ids + start / stop text + start mel), per segment
    Ps = [34 + len(ids) + 3 for ids in m._segments_of(text, 20)]
    assert len(Ps) == len(free)
    L = max(Ps) + 5
    got = _infer_code_counts(m, wav, text, max_mel_tokens=L - min(Ps) + 6, min_length=L)
    assert got == [L - P for P in Ps], (Ps, L, got)
    # min_new_tokens wins over min_length
    assert _infer_code_counts(m, wav, text, max_mel_tokens=24, min_length=L, min_new_tokens=3) == [3] * len(free)


def _run(m, reqs, **kw):
    """-> per request (pcm bytes or the exception, [codes of each segment])."""
    decoded = {}
    real = m._decode

    def spy(engine, todo, g):
        out = real(engine, todo, g)
        decoded.update(out)
        return out

    m._decode = spy
    try:
        outs = m.infer_many(reqs, **kw)
    finally:
        del m._decode
    res = []
    for ri, o in enumerate(outs):
        codes = [np.asarray(decoded[k]).tolist() for k in sorted(k for k in decoded if k[0] == ri)]
        res.append((o[1].tobytes() if isinstance(o, tuple) else o, codes))
    return res


def test_a_pinned_request_with_constraints_sounds_the_same_in_any_company(tts, wavs):
    m, (wav_a, wav_b) = tts, wavs
    stop = m.stop_mel_token
    kw = dict(decode_slots=8, num_beams=1, max_mel_tokens=24)
    plain = _run(m, [dict(spk_audio_prompt=wav_a, text=ONE, generation={"seed": 2})], **kw)[0]
    assert isinstance(plain[0], bytes) and len(plain[1]) == 1
    banned = plain[1][0][:2]
    k = 20
    C = dict(spk_audio_prompt=wav_a, text=ONE, generation={"min_new_tokens": k, "no_repeat_ngram_size": 1, "suppress_tokens": banned, "seed": 2})
    U1 = dict(spk_audio_prompt=wav_b, text="A second voice says this.", generation={"seed": 1})
    U2 = dict(spk_audio_prompt=wav_a, text="Short.", generation={"top_k": 1})
    c_alone, u1_alone, u2_alone = (_run(m, [r], **kw)[0] for r in (C, U1, U2))
    for r in (c_alone, u1_alone, u2_alone):
        assert isinstance(r[0], bytes) and len(r[0]) > 0, r[0]
    codes = c_alone[1][0]
    assert stop not in codes[:k] and len(codes) >= k  # min_new_tokens
    body = [t for t in codes if t != stop]
    assert len(set(body)) == len(body) and 1 not in body  # no_repeat_ngram_size = 1: no id twice, none of the fake prompt's
    assert not set(banned) & set(codes) and codes != plain[1][0]  # suppress_tokens
    assert _run(m, [C, U1, U2], **kw) == [c_alone, u1_alone, u2_alone]  # codes and PCM, byte for byte
    assert _run(m, [U2, C, U1], **kw) == [u2_alone, c_alone, u1_alone]
    assert _run(m, [U1, U2], **kw) == [u1_alone, u2_alone]  # and the unconstrained ones are what they are without it


def test_a_refused_constraint_fails_its_request_only(tts, wavs):
    m, (wav_a, wav_b) = tts, wavs
    ok = dict(spk_audio_prompt=wav_a, text="Hello world.")
    bad = dict(spk_audio_prompt=wav_a, text="Hello world.", generation={"no_repeat_ngram_size": 99})
    outs = m.infer_many([ok, bad], decode_slots=4, num_beams=1, top_k=1, max_mel_tokens=8)
    assert isinstance(outs[1], ValueError) and "no_repeat_ngram_size" in str(outs[1])
    assert isinstance(outs[0], tuple) and outs[0][1].shape[0] > 0
