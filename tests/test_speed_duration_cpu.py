"""Speaking rate and target duration without a GPU: the one definition of the frame count, `S2Mel` at other frame counts against the
reference's own regulator and CFM (tests/golden/s2mel_rate.npz), the duration fit as a pure function, and the server's 422s."""
import math
import random

import numpy as np
import pytest
import torch

import voice_tts_amd.s2mel as S2
from voice_tts_amd import output as O

HD64 = dict(hidden_dim=128, num_heads=2, wavenet_hidden=128, depth=3)


def test_target_frames_is_the_expression_it_replaces():
    for n in range(1, 4097):
        assert S2.target_frames(n) == int((torch.tensor([n]) * 1.72).long()), n
    lens = torch.arange(1, 4097)
    assert torch.equal(S2.target_frames(lens), (lens * 1.72).long())  # a tensor of lengths: the tensor `__call__` hands the regulator
    assert S2.target_frames(1, 2.0) == 1 and int((torch.tensor([1]) * 1.72 / 2.0).long()) == 0  # truncates to 0: 1 is delivered
    for speed in (0.5, 0.8, 1.0, 1.25, 1.999, 2.0):
        got = S2.target_frames(lens, speed)
        assert int(got.min()) >= 1
        assert torch.equal(got, (lens * 1.72 / speed).long().clamp(min=1))
    assert torch.equal(S2.target_frames(lens, 1.0), S2.target_frames(lens))


@pytest.mark.parametrize("bad", [True, float("nan"), 0.49, 2.01, "1.0", float("inf"), -1.0])
def test_speed_outside_the_range_is_refused(bad):
    with pytest.raises(ValueError, match="speed"):
        S2.check_speed(bad)
    assert S2.check_speed(None) is None and S2.check_speed(0.5) == 0.5 and S2.check_speed(2) == 2.0 and S2.SPEED_RANGE == (0.5, 2.0)


def test_audio_seconds_follows_the_speed():
    from voice_tts_amd.pipeline import audio_seconds

    codes = [90, 1, 423]
    assert audio_seconds(codes) == sum(int(n * 1.72) * 256 / 22050 for n in codes) + 2 * 0.2
    assert audio_seconds(codes, speed=2.0) == sum(S2.target_frames(n, 2.0) * 256 / 22050 for n in codes) + 2 * 0.2


def _model(g, device="cpu"):
    cfg = S2.tiny_s2mel_cfg(gpt_dim=1280, semantic_dim=1024, lr_in_channels=1024, codebook_size=8194, **HD64)
    return S2.S2Mel(S2.make_s2mel_weights(cfg, seed=int(g["seed"])), cfg, device=device), cfg


def _t(g, k):
    return torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k])


def test_s2mel_at_each_speed_vs_reference(golden):
    """`cond` and `mel` within the bounds tests/test_s2mel_golden.py applies to the same tensors on the CPU (cond: allclose at 2e-5;
    mel: 5e-5 * max(1, max|ref|))."""
    g = golden("s2mel_rate.npz")
    m, cfg = _model(g)
    n, Tp = g["codes"].shape[1], g["ref_mel"].shape[-1]
    S = m.vq2emb(_t(g, "codes")) + m.gpt_layer(_t(g, "latent"))
    for k, speed in enumerate(g["speeds"]):
        F = S2.target_frames(n, float(speed))
        assert F == int(g["frames"][k])
        cond = m.length_regulator(S, torch.tensor([F]))
        ref = _t(g, f"cond_{k}")
        assert cond.shape == ref.shape and torch.allclose(cond, ref, atol=2e-5), (speed, float((cond - ref).abs().max()))
        noise = torch.cat([torch.zeros(1, 80, Tp), _t(g, f"noise_{k}")], -1)  # (the solve zeroes the prompt's frames of the noise)
        mel = m(_t(g, "latent"), _t(g, "codes"), torch.tensor([n]), _t(g, "prompt_condition"), _t(g, "ref_mel"), _t(g, "style"),
                n_timesteps=int(g["n_steps"]), inference_cfg_rate=0.7, noise=noise, frames=F)
        ref = _t(g, f"mel_{k}")
        err = (mel - ref).abs().max().item()
        print(f"speed {speed}: {F} frames, mel max|err| {err:.2e}")
        assert mel.shape == ref.shape == (1, 80, F)
        assert err <= 5e-5 * max(1.0, ref.abs().max().item())


def test_regulator_sweep_vs_reference(golden):
    g = golden("s2mel_rate.npz")
    m, cfg = _model(g)
    S = m.vq2emb(_t(g, "codes")) + m.gpt_layer(_t(g, "latent"))
    rows = set()
    for j, (n, speed, F) in enumerate(zip(g["sweep_n"], g["sweep_speed"], g["sweep_frames"])):
        assert S2.target_frames(int(n), float(speed)) == int(F)
        rows.add(int(g["sweep_tp"]) + int(F))
        cond = m.length_regulator(S[:, :int(n)], torch.tensor([int(F)]))
        ref = _t(g, f"sweep_cond_{j}")
        assert cond.shape == ref.shape and torch.allclose(cond, ref, atol=2e-5), (n, speed)
    assert rows >= {63, 64, 65}


def test_solve_many_with_mixed_frames_equals_each_call_on_the_cpu():
    cfg = S2.tiny_s2mel_cfg()
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=3), cfg, "cpu")
    g = torch.Generator().manual_seed(4)
    items, noises, frames = [], [], []
    for n, Tp, speed in [(20, 9, 0.5), (13, 5, None), (31, 9, 2.0), (2, 4, None)]:
        items.append((torch.randn(1, n, cfg["gpt_dim"], generator=g), torch.randint(0, cfg["codebook_size"], (1, n), generator=g),
                      torch.randn(1, Tp, cfg["content_dim"], generator=g), torch.randn(1, 80, Tp, generator=g), torch.randn(1, cfg["style_dim"], generator=g)))
        frames.append(None if speed is None else S2.target_frames(n, speed))
        noises.append(torch.randn(1, 80, Tp + (frames[-1] or S2.target_frames(n)), generator=g))
    outs = m.solve_many(items, n_timesteps=2, noises=noises, frames=frames)
    for it, z, f, out in zip(items, noises, frames, outs):
        ref = m(it[0], it[1], torch.tensor([it[1].shape[1]]), it[2], it[3], it[4], n_timesteps=2, noise=z, frames=f)
        assert out.shape == ref.shape == (1, 80, f or S2.target_frames(it[1].shape[1]))
        assert (out - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
    plain = m.solve_many(items[1::2], n_timesteps=2, noises=noises[1::2])
    for a, b in zip(plain, m.solve_many(items[1::2], n_timesteps=2, noises=noises[1::2], frames=[None, None])):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------------------- the duration fit
def _share_bound(natural, frames):
    S, total = sum(natural), sum(frames)
    return max(abs(f - a * total / S) for f, a in zip(frames, natural))


def test_fit_over_random_code_counts_rates_and_gaps():
    """Delivered length exactly N; the pad below one frame's worth of delivered samples plus one sample per segment; every count at
    least 1 and within 1 of its share (a 1-frame segment -- one code -- may hold its one frame against a share below 1: then the
    others give it up, and the bound is checked for programmes without such a segment); DurationError exactly when the largest
    total that fits implies a speed outside the range (found here by trying every total)."""
    rnd = random.Random(7)
    refused = met = 0
    for trial in range(600):
        n = rnd.randint(1, 6)
        codes = [rnd.choice([1, 2, 3, rnd.randint(4, 60), rnd.randint(4, 600)]) for _ in range(n)]
        natural = [S2.target_frames(c) for c in codes]
        rate, gap = rnd.choice(O.SAMPLE_RATES), rnd.choice([0, 200, 137])
        nat_s = O.delivered_len(natural, rate, gap) / rate
        duration = nat_s * rnd.choice([rnd.uniform(0.3, 0.6), rnd.uniform(0.6, 1.9), rnd.uniform(1.9, 2.4), 0.5, 1.0, 2.0])
        N = int(duration * rate + 0.5)
        S = sum(natural)
        fits = [t for t in range(n, 2 * S + 8) if O.delivered_len(O.share_frames(natural, t), rate, gap) <= N]
        best = max(fits) if fits else 0
        feasible = best >= n and 0.5 <= S / best <= 2.0
        if not feasible:
            with pytest.raises(O.DurationError) as e:
                O.fit_frames(natural, duration, rate, gap)
            assert isinstance(e.value, ValueError) and abs(e.value.natural_s - nat_s) < 1e-12 and e.value.min_s <= e.value.natural_s <= e.value.max_s
            for d in (e.value.min_s, e.value.max_s):  # both ends of the interval it carries can be asked for
                fr, N2, pad = O.fit_frames(natural, d, rate, gap)
                assert pad == 0 and N2 == O.delivered_len(fr, rate, gap)
            refused += 1
            continue
        frames, N1, pad = O.fit_frames(natural, duration, rate, gap)
        met += 1
        assert N1 == N and sum(frames) == best and min(frames) >= 1
        assert O.delivered_len(frames, rate, gap) + pad == N and pad >= 0
        orig, new = O.resample_ratio(22050, rate)
        assert pad < 256 * new / orig + n, (pad, natural, rate)
        if min(natural) >= 2:
            assert _share_bound(natural, frames) < 1.0, (natural, frames)
    assert refused > 50 and met > 200, (refused, met)


def test_fit_refuses_bad_durations_and_keeps_proportions():
    for bad in (0, -1.0, float("nan"), float("inf"), True, "2"):
        with pytest.raises(ValueError, match="duration"):
            O.fit_frames([10, 20], bad)
    frames, N, pad = O.fit_frames([100, 200, 50], 350 * 256 / 22050 * 1.5 + 0.4)
    assert sum(frames) == 525 and frames == [150, 300, 75] and N - pad == 525 * 256 + 2 * 4410


# --------------------------------------------------------------------------------------------------------- the server
HEX = "00ff" * 60


class PcmTTS:
    device, use_fp16 = "cuda:0", True
    returns_pcm_without_path = True

    def __init__(self):
        self.kw, self.requests = [], []

    def _result(self, kw):
        if kw.get("duration") is not None and kw["duration"] > 5:
            raise O.DurationError(kw["duration"], 1.5, 0.8, 2.9)
        return 22050, np.zeros((int((kw.get("duration") or 0.2) * 22050 + 0.5), 1), np.int16)

    def infer(self, spk_audio_prompt, text, output_path, **kw):
        self.kw.append(kw)
        return self._result(kw)

    def infer_many(self, requests, decode_slots=8, **kw):
        self.requests += requests
        out = []
        for r in requests:
            try:
                out.append(self._result(r))
            except Exception as e:
                out.append(e)
        return out


@pytest.mark.parametrize("batched", [False, True])
def test_server_fields_and_422s(batched, monkeypatch):
    from fastapi.testclient import TestClient

    from voice_tts_amd.server import create_app

    if batched:
        monkeypatch.setenv("IXTTS_BATCH_SLOTS", "2")
        monkeypatch.setenv("IXTTS_BATCH_WINDOW_MS", "1")
    stub = PcmTTS()
    seen = (lambda: stub.requests) if batched else (lambda: stub.kw)
    with TestClient(create_app(lambda: stub)) as c:
        base = {"text": "x", "spk_audio": HEX}
        r = c.post("/tts", json=base)
        assert r.status_code == 200 and "speed" not in seen()[-1] and "duration" not in seen()[-1]
        calls = len(seen())
        for body, word in (({"speed": 3}, "speed"), ({"speed": 0.4}, "speed"), ({"speed": 1.2, "duration": 2.0}, "combined"), ({"duration": 0}, "duration"),
                           ({"duration": -2.0}, "duration")):
            r = c.post("/tts", json={**base, **body})
            assert r.status_code == 422 and word in r.text, (body, r.text)
        assert len(seen()) == calls  # refused before inference
        r = c.post("/tts", json={**base, "speed": 1.25})
        assert r.status_code == 200 and seen()[-1]["speed"] == 1.25 and "duration" not in seen()[-1]
        r = c.post("/tts", json={**base, "duration": 2.0})
        assert r.status_code == 200 and seen()[-1]["duration"] == 2.0 and "speed" not in seen()[-1]
        assert abs(r.json()["audio_length"] - 2.0) < 1e-12
        r = c.post("/tts", json={**base, "duration": 9.0})  # the model finds it cannot be met
        assert r.status_code == 422, r.text
        detail = r.json()["detail"]
        assert detail["natural_s"] == 1.5 and detail["min_s"] == 0.8 and detail["max_s"] == 2.9 and "9.0" in detail["error"]


def test_fit_pad_is_what_finish_pcm_lays_out_as_silence():
    """`finish_pcm_many(totals=...)` on the CPU side of its contract: a total shorter than the segments is refused before any launch."""
    w = [torch.zeros(1, 100)]
    with pytest.raises(ValueError, match="do not fit"):
        O.finish_pcm_many([w], [None], [None], 200, totals=[99])
    assert math.isclose(O.delivered_len([1, 1], 22050, 200), 2 * 256 + 4410)


def test_an_injected_s2mel_stage_refuses_a_pace():
    """`Glue.s2mel(latent, codes, code_lens, speaker)` has no frame count to set: a speed or a duration names the built-in stage."""
    from indextts.infer_v2 import IndexTTS2

    m = IndexTTS2.__new__(IndexTTS2)
    m.s2mel = None
    assert m._rate_control(None, None) == (None, None)
    for kw in (dict(speed=1.2, duration=None), dict(speed=None, duration=3.0)):
        with pytest.raises(NotImplementedError, match="built-in s2mel"):
            m._rate_control(**kw)
    with pytest.raises(ValueError, match="combined"):
        m._rate_control(1.2, 3.0)
    with pytest.raises(ValueError, match="stream_return"):
        m._rate_control(None, 3.0, stream_return=True)
    m.s2mel = object()
    assert m._rate_control(2, None) == (2.0, None) and m._rate_control(None, 3) == (None, 3.0)
