"""The true peak and the limiter of the output stage on the CPU: the properties of the fp64 twin itself (tests/limiter_ref.py) -- the
algorithm holds what DESIGN 4.3d says it holds before any kernel is compared with it -- the interpolator's table, the validation of the
two controls, and the two `/tts` fields (stub model).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import limiter_ref as LM  # noqa: E402
import loudness_ref as LR  # noqa: E402
from voice_tts_amd import output as O  # noqa: E402

RATES = [8000, 22050, 48000]
CEILINGS = [-1.0, -2.0]


def _signals(fs):
    """The five programmes of the issue, about a third of a second each, fp32 on the +-32767 scale."""
    n = fs // 3 + 7
    t = np.arange(n)
    burst = np.zeros(n, np.float32)
    a, b = n // 4, n // 4 + fs // 8
    burst[a:b] = 32000.0 * np.sin(2 * np.pi * 180.0 * np.arange(b - a) / fs)
    click = np.zeros(n, np.float32)
    click[n // 2] = 32767.0
    return {
        "noise": LR.noise(n, fs, 5, rms=12000.0),
        "997 Hz sine": (30000.0 * np.sin(2 * np.pi * 997.0 * t / fs)).astype(np.float32),
        "fs/4 sine at 45 degrees": (30000.0 * np.sin(np.pi / 2 * t + np.pi / 4)).astype(np.float32),
        "180 Hz burst between silences": burst,
        "click": click,
    }


@pytest.mark.parametrize("fs", RATES)
def test_the_twin_holds_what_the_design_says(fs):
    W = O.lookaround(fs)
    assert W == {8000: 40, 22050: 110, 48000: 240}[fs]
    for peak in CEILINGS:
        c = O.ceiling(peak)
        assert abs(c - round(c)) > 0.3  # (29 204.6 / 26 028.5: neither near an integer)
        for name, y in _signals(fs).items():
            for mode in O.PEAK_MODES:
                got = LM.limit(y, fs, peak, mode)
                r, a, out = got["r"], got["a"], got["out"]
                assert (a <= r + 1e-12).all(), (fs, peak, name, mode, float((a - r).max()))  # the first and last W samples included
                assert (got["a32"].astype(np.float64) <= r).all()
                near = np.convolve((r < 1.0).astype(np.float64), np.ones(4 * W + 1), "same") > 0.5  # an r < 1 within 2W
                assert (a[~near] == 1.0).all() and (got["a32"][~near] == 1.0).all(), (fs, peak, name, mode)
                assert float(np.abs(out).max()) <= c * (1.0 + 2.0 ** -23), (fs, peak, name, mode, float(np.abs(out).max()), c)
                if mode == "true":
                    tp = LM.true_peak(out)
                    assert tp <= c * (1.0 + 1e-4), (fs, peak, name, tp / c - 1.0)
                if name != "fs/4 sine at 45 degrees":
                    assert got["count"] > 0, (fs, peak, name, mode)  # (the programme does reach its ceiling)
        # sample mode leaves the inter-sample peaks of the fs/4 sine alone: that is the point of the other mode.  Its samples are
        # +-21 213, under both ceilings, so nothing is limited and the true peak stays where it was: 30 000 less 0.033 dB inside the
        # sine (29 886 / 26 028.5 = +1.20 dB over the ceiling of -2 dBFS, +0.20 dB over that of -1 dBFS), and 0.6 dB more at its
        # cut-off ends -- measured here: +1.81 dB and +0.81 dB at every rate.  "More than 1 dB over c" can hold at -2 dBFS only: at
        # -1 dBFS a signal of amplitude 30 000 is 0.23 dB over c to begin with, so there the test asks that it stays over c.
        y = _signals(fs)["fs/4 sine at 45 degrees"]
        got = LM.limit(y, fs, peak, "sample")
        over = 20.0 * np.log10(LM.true_peak(got["out"]) / c)
        print(f"{fs} Hz, ceiling {peak} dBFS, sample mode: the fs/4 sine's true peak stays {over:+.3f} dB over c")
        assert got["count"] == 0 and over > (1.0 if peak == -2.0 else 0.0), (fs, peak, over)
        assert LM.limit(y, fs, peak, "true")["count"] > 0


def test_the_interpolator():
    h = O.true_peak_taps()
    assert h.shape == (49,) and h[24] == 1.0 and h[0] == 0.0 and h[48] == 0.0 and np.array_equal(h, h[::-1])
    assert np.abs(h[np.arange(0, 49, 4)[np.arange(0, 49, 4) != 24]]).max() < 1e-15  # phase 0 is the identity
    y = LR.noise(300, 8000, 3)
    z = LM.interpolate(y)
    assert np.array_equal(z[:, 0], y.astype(np.float64))
    # every phase has twelve taps, j = -5 .. 6
    for k in (1, 2, 3):
        assert [j for j in range(-8, 9) if abs(k - 4 * j) <= 24 and h[k - 4 * j + 24] != 0.0] == list(range(-5, 7))
    n = np.arange(4000)
    sine = (30000.0 * np.sin(np.pi / 2 * n + np.pi / 4)).astype(np.float32)
    inner = np.abs(LM.interpolate(sine))[100:-100]  # (away from the cut-off ends)
    db = 20.0 * np.log10(inner.max() / 30000.0)
    assert abs(db) < 0.05 and abs(20.0 * np.log10(np.abs(sine).max() / 30000.0) + 3.0103) < 1e-3, db
    dc = np.abs(LM.interpolate(np.full(400, 10000.0, np.float32)))[100:-100].max() / 10000.0
    assert 1.0 <= dc and 20.0 * np.log10(dc) < 0.01, dc
    sums = [sum(h[k - 4 * j + 24] for j in range(-5, 7)) for k in (1, 2, 3)]
    assert abs(sums[0] - 1.0005) < 1e-4 and abs(sums[1] - 1.0009) < 1e-4 and abs(sums[2] - sums[0]) < 1e-12, sums


def test_window_and_lookaround():
    for fs, W in ((8000, 40), (22050, 110), (44100, 221), (48000, 240)):
        w = O.limiter_window(fs)
        assert O.lookaround(fs) == W and w.shape == (2 * W + 1,) and (w > 0).all() and abs(w.sum() - 1.0) < 1e-15 and np.allclose(w, w[::-1], atol=1e-18)


def test_check_limit():
    assert O.PEAK_MODES == ("sample", "true") and O.LOUDNESS_TOLERANCE_LU == 0.5
    assert O.check_limit(None, None, None) == (None, "sample", False)
    assert O.check_limit("sample", False, (-16.0, -1.0)) == ((-16.0, -1.0), "sample", False)
    assert O.check_limit("true", None, (None, -3.0)) == ((None, -3.0), "true", False)
    assert O.check_limit(None, True, None) == ((None, O.DEFAULT_PEAK), "sample", True)  # the limiter brings its own ceiling
    assert O.check_limit("true", True, None) == ((None, O.DEFAULT_PEAK), "true", True)
    assert O.check_limit(None, True, O.check_level(-16.0, None)) == ((-16.0, -1.0), "sample", True)
    assert O.check_limit(None, True, O.check_level(None, -2.0)) == ((None, -2.0), "sample", True)
    with pytest.raises(ValueError, match="ceiling"):
        O.check_limit("true", None, None)  # nothing for the mode to qualify
    with pytest.raises(ValueError, match="ceiling"):
        O.check_limit("true", False, None)
    for bad in ("rms", "TRUE", 1, True, 0.5, ["true"]):
        with pytest.raises(ValueError, match="peak mode"):
            O.check_limit(bad, None, (None, -1.0))
    for bad in ("yes", 1, 0, 1.0, "true", [True]):
        with pytest.raises(ValueError, match="limiter"):
            O.check_limit(None, bad, (None, -1.0))
    # `check_level` is what it was
    assert O.check_level(None, None) is None and O.check_level(-16.0, None) == (-16.0, -1.0)


def test_reports_keep_todays_keys_without_the_new_controls():
    rec = np.zeros(1, O._RECORD)[0]
    rec["lufs"], rec["gain"], rec["peak"] = -30.0, 2.0, 1000.0
    assert list(O.level_report(rec, -24.0)) == ["measured_lufs", "gain_db", "peak_dbfs_in", "target_met"]
    rep = O.level_report_limit(rec, -24.0, "true", False)
    assert list(rep)[:4] == list(O.level_report(rec, -24.0)) and {k: rep[k] for k in list(rep)[:4]} == O.level_report(rec, -24.0)
    assert list(rep)[4:] == ["peak_mode", "limited", "max_reduction_db", "limited_fraction", "delivered_lufs", "delivered_peak_dbfs"]
    assert rep["peak_mode"] == "true" and rep["limited"] is False and rep["max_reduction_db"] == 0.0 and rep["limited_fraction"] == 0.0
    assert abs(rep["delivered_lufs"] - (-30.0 + 20.0 * np.log10(2.0))) < 1e-12
    second = np.zeros(1, O._RECORD)[0]
    second["lufs"], second["peak"] = -24.3, 29000.0
    rep = O.level_report_limit(rec, -24.0, "sample", True, 1000, (np.float32(0.5), 10), second)
    assert rep["limited"] is True and abs(rep["max_reduction_db"] + 6.0206) < 1e-3 and rep["limited_fraction"] == 0.01
    assert rep["delivered_lufs"] == -24.3 and rep["target_met"] is True and set(rep) == set(O.level_report_limit(rec, -24.0, "true", False))
    second["lufs"] = -24.6
    assert O.level_report_limit(rec, -24.0, "sample", True, 1000, (np.float32(0.5), 10), second)["target_met"] is False
    assert O.level_report_limit(rec, None, "sample", True, 1000, (np.float32(1.0), 0), second)["limited"] is False


# --------------------------------------------------------------------------------------------------------------------------- /tts
HEX = "00ff" * 60


class PcmTTS:
    """`infer(output_path=None)` -> (sr, pcm), as IndexTTS2; records the keywords it was called with."""
    device, use_fp16 = "cuda:0", True
    returns_pcm_without_path = True
    last_loudness = None

    def __init__(self):
        self.kw = []

    def infer(self, spk_audio_prompt, text, output_path, **kw):
        assert output_path is None
        self.kw.append(kw)
        return 22050, (np.arange(4411) % 100).astype(np.int16).reshape(-1, 1)


def test_the_two_fields_reach_infer_and_bad_values_are_a_422():
    from fastapi.testclient import TestClient

    from voice_tts_amd.server import create_app

    stub = PcmTTS()
    with TestClient(create_app(lambda: stub)) as c:
        r = c.post("/tts", json={"text": "plain", "spk_audio": HEX})
        assert r.status_code == 200 and "output_peak_mode" not in stub.kw[-1] and "output_limiter" not in stub.kw[-1]
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "loudness": -16, "limiter": True})
        assert r.status_code == 200 and stub.kw[-1]["output_limiter"] is True and stub.kw[-1]["output_loudness"] == -16 and "output_peak_mode" not in stub.kw[-1]
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "peak": -1, "peak_mode": "true"})
        assert r.status_code == 200 and stub.kw[-1]["output_peak_mode"] == "true" and stub.kw[-1]["output_peak"] == -1 and "output_limiter" not in stub.kw[-1]
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "peak_mode": "true", "limiter": True})
        assert r.status_code == 200 and stub.kw[-1]["output_peak_mode"] == "true" and stub.kw[-1]["output_limiter"] is True
        n = len(stub.kw)
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "peak": -1, "peak_mode": "rms"})
        assert r.status_code == 422 and "true" in r.text
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "peak": -1, "limiter": "yes"})
        assert r.status_code == 422
        r = c.post("/tts", json={"text": "x", "spk_audio": HEX, "peak_mode": "true"})
        assert r.status_code == 422 and "ceiling" in r.text
    assert len(stub.kw) == n
