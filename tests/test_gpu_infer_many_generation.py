"""`IndexTTS2.infer_many` with per-request `generation` settings: a request that carries the key is pinned -- its codes and its
PCM are a function of the request alone, bit for bit, alone or in any batch and order (same `decode_slots`: one engine shape);
requests of different `num_beams` share a call; a bad key or a `num_beams` the engine cannot hold fails its request only."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_generation"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1)


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


def test_a_pinned_request_sounds_the_same_in_any_company(tts):
    m, wav_a, wav_b = tts
    kw = dict(decode_slots=8, num_beams=1, max_mel_tokens=16)
    A = dict(spk_audio_prompt=wav_a, text="Hello world, this is a test.")
    B = dict(spk_audio_prompt=wav_b, text="A second voice says this.", generation={"temperature": 1.2, "top_k": 50, "seed": 3})
    C = dict(spk_audio_prompt=wav_a, text="Short.", generation={"top_k": 1})
    abc = _run(m, [A, B, C], **kw)
    assert all(isinstance(r[0], bytes) and len(r[0]) > 0 for r in abc)
    b_alone, c_alone = _run(m, [B], **kw)[0], _run(m, [C], **kw)[0]
    assert abc[1][1] == b_alone[1] and abc[1][0] == b_alone[0]  # codes, then PCM byte for byte
    cba = _run(m, [C, B, A], **kw)
    assert cba[1] == b_alone
    assert abc[2] == c_alone and cba[0] == c_alone
    # the key is what B decodes under: without it, the call's settings and the slot's stream give other codes
    plain = _run(m, [{k: v for k, v in B.items() if k != "generation"}], **kw)[0]
    assert plain[1] != b_alone[1]


def test_pinned_beam_requests_of_two_segments_in_both_orders(tts):
    m, wav_a, wav_b = tts
    kw = dict(decode_slots=8, max_mel_tokens=16, max_text_tokens_per_segment=20)  # served default: 3 beams; two groups on six slots
    P = dict(spk_audio_prompt=wav_a, text="Hello world, this is a test. One more sentence follows here.", generation={"seed": 5})
    Q = dict(spk_audio_prompt=wav_b, text="A second voice says this. And then it says some more.", generation={"temperature": 1.1, "top_k": 8, "length_penalty": 1.0})
    p_alone, q_alone = _run(m, [P], **kw)[0], _run(m, [Q], **kw)[0]
    assert len(p_alone[1]) >= 2 and len(q_alone[1]) >= 2 and isinstance(p_alone[0], bytes) and isinstance(q_alone[0], bytes)
    assert _run(m, [P, Q], **kw) == [p_alone, q_alone]
    assert _run(m, [Q, P], **kw) == [q_alone, p_alone]


def test_requests_of_different_num_beams_share_a_call(tts):
    m, wav_a, wav_b = tts
    kw = dict(decode_slots=8, max_mel_tokens=16)
    one = dict(spk_audio_prompt=wav_a, text="Hello world, this is a test.", generation={"num_beams": 1, "seed": 2})
    three = dict(spk_audio_prompt=wav_b, text="A second voice says this.", generation={"num_beams": 3, "seed": 2})
    one_alone, three_alone = _run(m, [one], **kw)[0], _run(m, [three], **kw)[0]
    assert isinstance(one_alone[0], bytes) and isinstance(three_alone[0], bytes)
    assert _run(m, [one, three], **kw) == [one_alone, three_alone]
    assert _run(m, [three, one], num_beams=1, **kw) == [three_alone, one_alone]  # whatever the call's own num_beams


def test_a_bad_generation_dict_fails_its_request_only(tts):
    m, wav_a, wav_b = tts
    ok = dict(spk_audio_prompt=wav_a, text="Hello world.")
    typo = dict(spk_audio_prompt=wav_a, text="Hello world.", generation={"tempreture": 1})
    wide = dict(spk_audio_prompt=wav_b, text="Hello world.", generation={"num_beams": 4})  # one group of 4 on 4 slots: the 3-slot register engine
    outs = m.infer_many([ok, typo, wide, ok], decode_slots=4, num_beams=1, top_k=1, max_mel_tokens=8)
    assert isinstance(outs[1], ValueError) and "tempreture" in str(outs[1])
    assert isinstance(outs[2], NotImplementedError) and not isinstance(outs[2], AssertionError)
    for o in (outs[0], outs[3]):
        assert isinstance(o, tuple) and o[0] == 22050 and o[1].dtype == np.int16 and o[1].shape[0] > 0
