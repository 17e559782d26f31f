"""/tts with `sample_rate` / `encoding`: the fields reach the model only when the request sets them, the response's RIFF carries the
requested rate and format tag, a plain request produces the bytes it always produced, and a value outside the sets is a 422.
Stub models, no GPU."""
import io
import wave

import numpy as np
import pytest
from fastapi.testclient import TestClient

from voice_tts_amd import output as O
from voice_tts_amd.server import create_app

HEX = "00ff" * 60


class PcmTTS:
    """`infer(output_path=None)` -> (sr, pcm), as IndexTTS2; records the keywords it was called with."""
    device, use_fp16 = "cuda:0", True
    returns_pcm_without_path = True

    def __init__(self):
        self.kw = []

    @staticmethod
    def result(rate=None, encoding=None):
        sr = 22050 if rate is None else rate
        n = sr // 5 + 1  # odd for every rate of the set: the G.711 data chunk needs its pad byte
        if encoding in ("mulaw", "alaw"):
            return sr, (np.arange(n) % 251).astype(np.uint8).reshape(-1, 1)
        return sr, (np.arange(n) % 100).astype(np.int16).reshape(-1, 1)

    def infer(self, spk_audio_prompt, text, output_path, **kw):
        assert output_path is None
        self.kw.append(kw)
        return self.result(kw.get("output_sample_rate"), kw.get("output_encoding"))


def _plain_bytes(sr, pcm):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(pcm.astype("<i2").tobytes())
    return buf.getvalue()


def test_fields_reach_the_model_only_when_set_and_shape_the_riff():
    stub = PcmTTS()
    with TestClient(create_app(lambda: stub)) as c:
        r = c.post("/tts", json={"text": "plain", "spk_audio": HEX})
        assert r.status_code == 200
        assert "output_sample_rate" not in stub.kw[-1] and "output_encoding" not in stub.kw[-1]
        assert bytes.fromhex(r.json()["audio_hex"]) == _plain_bytes(*PcmTTS.result())  # the bytes a plain request always produced
        assert abs(r.json()["audio_length"] - 4411 / 22050) < 1e-12

        r = c.post("/tts", json={"text": "16k", "spk_audio": HEX, "sample_rate": 16000})
        assert r.status_code == 200 and stub.kw[-1]["output_sample_rate"] == 16000 and "output_encoding" not in stub.kw[-1]
        raw = bytes.fromhex(r.json()["audio_hex"])
        assert raw == _plain_bytes(*PcmTTS.result(16000))
        with wave.open(io.BytesIO(raw)) as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 16000, 3201)
        assert abs(r.json()["audio_length"] - 3201 / 16000) < 1e-12

        for law, tag in (("mulaw", 7), ("alaw", 6)):
            r = c.post("/tts", json={"text": law, "spk_audio": HEX, "sample_rate": 8000, "encoding": law})
            assert r.status_code == 200 and stub.kw[-1]["output_sample_rate"] == 8000 and stub.kw[-1]["output_encoding"] == law
            raw = bytes.fromhex(r.json()["audio_hex"])
            info = O.riff_info(raw)
            assert (info["tag"], info["channels"], info["rate"], info["bits"], info["cb_size"], info["fact"], info["frames"]) == (tag, 1, 8000, 8, 0, 1601, 1601)
            assert info["padded"] and len(raw) == 58 + 1601 + 1 and raw[58:58 + 1601] == PcmTTS.result(8000, law)[1].tobytes()
            assert abs(r.json()["audio_length"] - 1601 / 8000) < 1e-12

        r = c.post("/tts", json={"text": "enc only", "spk_audio": HEX, "encoding": "alaw"})
        assert r.status_code == 200 and stub.kw[-1]["output_encoding"] == "alaw" and "output_sample_rate" not in stub.kw[-1]
        assert O.riff_info(bytes.fromhex(r.json()["audio_hex"]))["rate"] == 22050


def test_values_outside_the_sets_are_a_422():
    stub = PcmTTS()
    with TestClient(create_app(lambda: stub)) as c:
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "sample_rate": 12345})
        assert r.status_code == 422 and "48000" in r.text
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "encoding": "mp3"})
        assert r.status_code == 422 and "alaw" in r.text
    assert stub.kw == []


def test_batcher_hands_the_fields_on_as_request_keys(monkeypatch):
    class BatchTTS(PcmTTS):
        def __init__(self):
            super().__init__()
            self.requests = []

        def infer_many(self, requests, decode_slots=8, **kw):
            self.requests += requests
            return [self.result(r.get("sample_rate"), r.get("encoding")) for r in requests]

    monkeypatch.setenv("IXTTS_BATCH_SLOTS", "2")
    monkeypatch.setenv("IXTTS_BATCH_WINDOW_MS", "1")
    stub = BatchTTS()
    with TestClient(create_app(lambda: stub)) as c:
        r = c.post("/tts", json={"text": "plain", "spk_audio": HEX})
        assert r.status_code == 200 and "sample_rate" not in stub.requests[-1] and "encoding" not in stub.requests[-1]
        assert bytes.fromhex(r.json()["audio_hex"]) == _plain_bytes(*PcmTTS.result())
        r = c.post("/tts", json={"text": "tel", "spk_audio": HEX, "sample_rate": 8000, "encoding": "mulaw"})
        assert r.status_code == 200 and stub.requests[-1]["sample_rate"] == 8000 and stub.requests[-1]["encoding"] == "mulaw"
        info = O.riff_info(bytes.fromhex(r.json()["audio_hex"]))
        assert (info["tag"], info["rate"], info["fact"]) == (7, 8000, 1601) and abs(r.json()["audio_length"] - 1601 / 8000) < 1e-12
    assert not stub.kw  # infer() never ran


def test_a_file_writing_model_gets_the_keywords_and_its_file_is_returned(tmp_path):
    class FileTTS:
        device, use_fp16 = "cuda:0", True

        def __init__(self):
            self.kw = []

        def infer(self, spk_audio_prompt, text, output_path, **kw):
            self.kw.append(kw)
            sr, pcm = PcmTTS.result(kw.get("output_sample_rate"), kw.get("output_encoding"))
            with open(output_path, "wb") as f:
                f.write(O.wav_bytes(sr, pcm, kw.get("output_encoding")))
            return output_path

    stub = FileTTS()
    with TestClient(create_app(lambda: stub)) as c:
        r = c.post("/tts", json={"text": "plain", "spk_audio": HEX})
        assert r.status_code == 200 and "output_sample_rate" not in stub.kw[-1] and "output_encoding" not in stub.kw[-1]
        assert bytes.fromhex(r.json()["audio_hex"]) == _plain_bytes(*PcmTTS.result())
        r = c.post("/tts", json={"text": "tel", "spk_audio": HEX, "sample_rate": 8000, "encoding": "alaw"})
        assert r.status_code == 200 and stub.kw[-1] == dict(emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None, verbose=False,
                                                            output_sample_rate=8000, output_encoding="alaw")
        assert O.riff_info(bytes.fromhex(r.json()["audio_hex"]))["tag"] == 6 and abs(r.json()["audio_length"] - 1601 / 8000) < 1e-12
        r = c.post("/tts", json={"text": "wide", "spk_audio": HEX, "sample_rate": 48000})
        assert r.status_code == 200 and abs(r.json()["audio_length"] - 9601 / 48000) < 1e-12
