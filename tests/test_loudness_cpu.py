"""The level control of the output stage, the parts that need no GPU: the K-weighting builder against the table of ITU-R BS.1770, the
fp64 twin (tests/loudness_ref.py) against the standard's own check and hand-computed gates, the gain rule, value validation, and
the two `/tts` fields."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as LR  # noqa: E402

from voice_tts_amd import output as O  # noqa: E402


def test_coefficients_at_48k_are_the_table_of_the_standard():
    b_s, a_s, b_h, a_h = O.k_weighting(48000)
    assert np.abs(b_s - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() < 1e-12
    assert np.abs(a_s - [1.0, -1.69065929318241, 0.73248077421585]).max() < 1e-12
    assert np.array_equal(b_h, [1.0, -2.0, 1.0])
    assert np.abs(a_h - [1.0, -1.99004745483398, 0.99007225036621]).max() < 1e-12
    for fs in O.SAMPLE_RATES:  # stable at every rate: both poles of either section inside the unit circle
        for a in O.k_weighting(fs)[1::2]:
            assert a.dtype == np.float64 and np.abs(np.roots(a)).max() < 1.0


def test_full_scale_997_hz_sine_reads_minus_3_01():
    t = np.arange(48000 * 5) / 48000.0
    L = LR.loudness(32768.0 * np.sin(2 * np.pi * 997.0 * t), 48000)
    assert abs(L - (-3.01)) <= 0.01, L


def test_hop_lengths():
    assert [O.hop_len(fs) for fs in O.SAMPLE_RATES] == [800, 1103, 1600, 2205, 2400, 3200, 4410, 4800]
    assert O.SAMPLE_RATES == (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)


def test_no_loudness_below_four_hops_and_for_silence():
    g = np.random.default_rng(1)
    x = g.standard_normal(4 * 800) * 3000
    assert LR.loudness(x, 8000) is not None
    assert LR.hop_energies(x, 8000).size == 4 and LR.hop_energies(x[:-1], 8000).size == 3
    assert LR.loudness(x[:-1], 8000) is None  # 3 hops and a partial one
    assert LR.loudness(np.zeros(0), 8000) is None
    assert LR.loudness(np.zeros(8000 * 2), 8000) is None  # all-zero: no block above -70
    assert LR.gain(None, 0.0, -23.0, -1.0) == (1.0, LR.NO_BLOCK)


def test_relative_gate_drops_passages_16_db_down():
    H = 800
    zl, zq = 10.0 ** ((-20.0 + 0.691) / 10.0), 10.0 ** ((-36.0 + 0.691) / 10.0)  # block powers of -20 and -36 LUFS
    e = np.array([zl * H] * 10 + [zq * H] * 10)
    # by hand: 7 loud blocks, 3 mixed ones (3+1, 2+2, 1+3 hops: -21.2, -22.9, -25.7 LUFS), 7 quiet ones.  All 17 pass the absolute
    # gate; their mean is (8.5 zl + 8.5 zq) / 17 = -22.9 LUFS, so the relative gate sits at -32.9 and the 7 quiet blocks leave.
    mean_all = (8.5 * zl + 8.5 * zq) / 17.0
    gamma = -0.691 + 10 * math.log10(mean_all) - 10.0
    assert -36.0 < gamma < -25.8
    want = -0.691 + 10 * math.log10((7 * zl + 1.5 * zl + 1.5 * zq) / 10.0)
    assert abs(LR.integrated(e, H) - want) < 1e-12
    assert abs(LR.integrated(e, H) - (-0.691 + 10 * math.log10(mean_all))) > 1.0  # (ungated it would read 1.6 LU lower)
    # the same through the filter: a 997 Hz tone, 2 s loud then 2 s 16 dB down, keeps 17 loud and 3 mixed
    # blocks of its 37: 18.5 loud and 1.5 quiet hops' worth over 20 blocks (0.01: the transient at the step)
    t = np.arange(8000 * 4) / 8000.0
    x = 8000.0 * np.sin(2 * np.pi * 997.0 * t) * np.where(t < 2.0, 1.0, 10.0 ** (-16.0 / 20.0))
    loud = LR.loudness(x[:16000], 8000)
    want = loud + 10 * math.log10((18.5 + 1.5 * 10.0 ** -1.6) / 20.0)
    assert abs(LR.loudness(x, 8000) - want) < 0.01


def test_gain_rule():
    g, flags = LR.gain(-30.0, 1000.0, -23.0, -1.0)
    assert abs(g - 10.0 ** (7.0 / 20.0)) < 1e-15 and flags == 0
    c = 32768.0 * 10.0 ** (-1.0 / 20.0)
    g, flags = LR.gain(-30.0, 20000.0, -23.0, -1.0)  # 2.24 x 20000 passes the ceiling: the gain gives way, the target is missed
    assert abs(g - c / 20000.0) < 1e-15 and flags == LR.CEILING_BOUND and g < 10.0 ** (7.0 / 20.0)
    g, flags = LR.gain(-30.0, 32767.0, None, -6.0)  # the ceiling alone
    assert abs(g - 32768.0 * 10.0 ** (-0.3) / 32767.0) < 1e-15 and flags == LR.CEILING_BOUND
    assert LR.gain(-30.0, 1000.0, None, -6.0) == (1.0, 0)  # under the ceiling: untouched
    assert LR.gain(-30.0, 30000.0, -40.0, None)[1] == 0 and LR.gain(None, 30000.0, -40.0, -20.0)[1] == LR.NO_BLOCK | LR.CEILING_BOUND
    assert LR.gain(-30.0, 0.0, -23.0, -1.0)[1] == 0  # a peak of 0 never binds


def test_values_are_validated():
    assert O.check_level() is None
    assert O.check_level(-23) == (-23.0, -1.0) and O.check_level(-23.0, -3) == (-23.0, -3.0) and O.check_level(None, 0) == (None, 0.0)
    assert O.check_level(-50, -20) == (-50.0, -20.0) and O.check_level(-5.0, 0.0) == (-5.0, 0.0)
    for bad in (-50.1, -4.9, 0, True, False, math.nan, "loud", math.inf):
        with pytest.raises(ValueError, match="loudness"):
            O.check_level(bad)
    for bad in (-20.5, 0.1, True, False, math.nan, "-1", -math.inf):
        with pytest.raises(ValueError, match="peak"):
            O.check_level(-23.0, bad)
        with pytest.raises(ValueError, match="peak"):
            O.check_level(None, bad)


def test_report_of_a_record():
    rec = np.zeros(1, O._RECORD)[0]
    rec["lufs"], rec["gain"], rec["peak"], rec["flags"] = -30.0, 2.0, 16384.0, 0
    assert O.level_report(rec, -24.0) == dict(measured_lufs=-30.0, gain_db=20 * math.log10(2.0), peak_dbfs_in=20 * math.log10(0.5), target_met=True)
    rec["flags"] = 1
    assert O.level_report(rec, -24.0)["target_met"] is False and O.level_report(rec, None)["target_met"] is True
    rec["flags"], rec["lufs"], rec["peak"] = 2, math.nan, 0.0
    r = O.level_report(rec, -24.0)
    assert r["measured_lufs"] is None and r["target_met"] is False and r["peak_dbfs_in"] == -math.inf


def test_stream_return_refuses_either_control_before_any_work():
    from voice_tts_amd.infer_v2 import IndexTTS2

    m = object.__new__(IndexTTS2)  # no model behind it: the refusal comes before anything is touched
    for kw in (dict(output_loudness=-23.0), dict(output_peak=-3.0)):
        with pytest.raises(ValueError, match="stream_return"):
            m.infer(b"", "text", None, stream_return=True, **kw)
    with pytest.raises(ValueError, match="loudness"):
        m.infer(b"", "text", None, output_loudness=-3.0)
    with pytest.raises(ValueError, match="peak"):
        m.infer(b"", "text", None, output_peak=1.0)


def test_tts_fields_reach_the_model_and_bad_values_are_a_422():
    from fastapi.testclient import TestClient

    from voice_tts_amd.server import create_app

    class Stub:
        device, use_fp16 = "cuda:0", True
        returns_pcm_without_path = True
        last_loudness = dict(measured_lufs=-30.0, gain_db=7.0, peak_dbfs_in=-12.0, target_met=True)

        def __init__(self):
            self.kw = []

        def infer(self, spk_audio_prompt, text, output_path, **kw):
            self.kw.append(kw)
            return kw.get("output_sample_rate") or 22050, np.zeros((100, 1), np.int16)

    stub, HEX = Stub(), "00ff" * 60
    with TestClient(create_app(lambda: stub)) as c:
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX})
        assert r.status_code == 200 and "output_loudness" not in stub.kw[-1] and "output_peak" not in stub.kw[-1]
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "loudness": -23})
        assert r.status_code == 200 and stub.kw[-1]["output_loudness"] == -23.0 and "output_peak" not in stub.kw[-1]
        assert set(r.json()) == {"audio_hex", "audio_length", "inference_time", "rtf", "text"}  # the response model is unchanged
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "peak": -3.0, "sample_rate": 8000})
        assert r.status_code == 200 and stub.kw[-1]["output_peak"] == -3.0 and "output_loudness" not in stub.kw[-1]
        n = len(stub.kw)
        for bad in ({"loudness": -4.0}, {"loudness": -51}, {"peak": 0.5}, {"peak": -21}, {"loudness": "loud"}, {"loudness": -23, "peak": 3}):
            r = c.post("/tts", json={"text": "x", "spk_audio": HEX, **bad})
            assert r.status_code == 422, (bad, r.text)
        assert len(stub.kw) == n
