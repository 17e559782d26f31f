"""Speaking rate and target duration on the device: `S2Mel` at other frame counts against the reference's own regulator and CFM
(tests/golden/s2mel_rate.npz), alone and packed, and `speed=` / `duration=` through `infer`, its stream and `infer_many` over the tiny
model of tests/synthetic_model_dir.py.

(This file brings segment lengths no other file has: it sorts behind every tests/test_gpu_*.py on purpose -- see the note on
TunableOp state in tests/test_gpu_infer_many_vocoder.py.)"""
import os
import sys
import wave

import numpy as np
import pytest
import torch

import voice_tts_amd.s2mel as S2
from voice_tts_amd import output as O

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DEV = torch.device("cuda:0")
HD64 = dict(hidden_dim=128, num_heads=2, wavenet_hidden=128, depth=3)
TEXT = "Hello world, this is a test. One more sentence follows here."
KW = dict(max_mel_tokens=16, max_text_tokens_per_segment=20)
GREEDY = dict(num_beams=1, top_k=1, **KW)
GAP = int(22050 * 0.2)


# ------------------------------------------------------------------------------------------- S2Mel against the reference's classes
@pytest.fixture(scope="module")
def twin(golden):
    g = golden("s2mel_rate.npz")
    cfg = S2.tiny_s2mel_cfg(gpt_dim=1280, semantic_dim=1024, lr_in_channels=1024, codebook_size=8194, **HD64)
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=int(g["seed"])), cfg, device=DEV)
    t = lambda k: torch.from_numpy(g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]).to(DEV)  # noqa: E731
    return g, cfg, m, t


def _close(got, ref, bound=2e-4):
    """The bound tests/test_gpu_s2mel.py holds the device to against the reference fixture."""
    err = (got - ref).abs().max().item()
    assert got.shape == ref.shape and err <= bound * max(1.0, ref.abs().max().item()), err
    return err


def test_s2mel_on_gpu_at_each_speed_vs_reference(twin, monkeypatch):
    g, cfg, m, t = twin
    calls = []
    real = S2.attn_full
    monkeypatch.setattr(S2, "attn_full", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    n, Tp = g["codes"].shape[1], g["ref_mel"].shape[-1]
    S = m.vq2emb(t("codes")) + m.gpt_layer(t("latent"))
    for k, speed in enumerate(g["speeds"]):
        F = S2.target_frames(n, float(speed))
        assert F == int(g["frames"][k])
        e_cond = _close(m.length_regulator(S, torch.tensor([F], device=DEV)), t(f"cond_{k}"))
        noise = torch.cat([torch.zeros(1, 80, Tp, device=DEV), t(f"noise_{k}")], -1)
        del calls[:]
        mel = m(t("latent"), t("codes"), torch.tensor([n], device=DEV), t("prompt_condition"), t("ref_mel"), t("style"),
                n_timesteps=int(g["n_steps"]), inference_cfg_rate=0.7, noise=noise, frames=F)
        e_mel = _close(mel, t(f"mel_{k}"))
        print(f"speed {speed}: {F} frames, cond max|err| {e_cond:.2e}, mel max|err| {e_mel:.2e}")
        assert len(calls) == int(g["n_steps"]) * cfg["depth"]  # the HIP attention ran, as in test_s2mel_on_gpu_vs_reference_fixture


def test_regulator_sweep_and_its_packed_solve_across_a_tile_edge(twin):
    """The short targets of the fixture (Tp + F = 63, 64, 65 rows and their neighbours): `cond` against the reference's regulator, and
    the packed solve of all of them against each one's own `__call__`."""
    g, cfg, m, t = twin
    Tp = int(g["sweep_tp"])
    S = m.vq2emb(t("codes")) + m.gpt_layer(t("latent"))
    items, frames, noises = [], [], []
    gen = torch.Generator().manual_seed(5)
    for j, (n, F) in enumerate(zip(g["sweep_n"], g["sweep_frames"])):
        n, F = int(n), int(F)
        _close(m.length_regulator(S[:, :n], torch.tensor([F], device=DEV)), t(f"sweep_cond_{j}"))
        items.append((t("latent")[:, :n], t("codes")[:, :n], t("prompt_condition")[:, :Tp], t("ref_mel")[:, :, :Tp], t("style")))
        frames.append(F)
        noises.append(torch.randn(1, 80, Tp + F, generator=gen).to(DEV))
    assert {Tp + F for F in frames} >= {63, 64, 65} and all(m.packable(Tp + F, Tp) for F in frames)
    outs = m.solve_many(items, n_timesteps=2, noises=noises, frames=frames)
    for it, z, F, out in zip(items, noises, frames, outs):
        ref = m(it[0], it[1], torch.tensor([it[1].shape[1]], device=DEV), it[2], it[3], it[4], n_timesteps=2, noise=z, frames=F)
        assert out.shape == (1, 80, F)
        _close(out, ref, 1e-5)


def test_solve_many_with_mixed_frames_equals_each_call(twin):
    """One item at speed 0.5, one at its natural count, one at 2.0, of unequal lengths, and one too short to be packed -- each against
    its own `__call__` within the bound tests/test_gpu_s2mel_batch.py asserts for the uniform case (1e-5 of max(1, max|ref|)); with
    `frames` None everywhere the bytes are those of the call without the keyword."""
    g, cfg, m, t = twin
    gen = torch.Generator().manual_seed(23)
    items, frames, noises = [], [], []
    for n, Tp, speed in [(40, 30, 0.5), (23, 20, None), (60, 30, 2.0), (4, 4, None)]:
        items.append((t("latent")[:, :n] * 1.0, torch.randint(0, 8192, (1, n), generator=gen).to(DEV), torch.randn(1, Tp, cfg["content_dim"], generator=gen).to(DEV),
                      (torch.randn(1, 80, Tp, generator=gen) * 2 - 4).to(DEV), torch.randn(1, cfg["style_dim"], generator=gen).to(DEV)))
        frames.append(None if speed is None else S2.target_frames(n, speed))
        noises.append(torch.randn(1, 80, Tp + (frames[-1] or S2.target_frames(n)), generator=gen).to(DEV))
    Ts = [it[2].shape[1] + (f or S2.target_frames(it[1].shape[1])) for it, f in zip(items, frames)]
    assert [m.packable(T, it[2].shape[1]) for T, it in zip(Ts, items)] == [True, True, True, False] and len(set(Ts)) == 4
    outs = m.solve_many(items, n_timesteps=2, noises=noises, frames=frames)
    worst = 0.0
    for it, z, f, out in zip(items, noises, frames, outs):
        ref = m(it[0], it[1], torch.tensor([it[1].shape[1]], device=DEV), it[2], it[3], it[4], n_timesteps=2, noise=z, frames=f)
        assert out.shape == (1, 80, f or S2.target_frames(it[1].shape[1]))
        worst = max(worst, _close(out, ref, 1e-5))
    print(f"solve_many, mixed frames: worst max|err| {worst:.2e}")
    nat = [torch.randn(1, 80, it[2].shape[1] + S2.target_frames(it[1].shape[1]), generator=gen).to(DEV) for it in items]
    a = m.solve_many(items, n_timesteps=2, noises=nat)
    b = m.solve_many(items, n_timesteps=2, noises=nat, frames=[None] * len(items))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------- the request paths
@pytest.fixture(scope="module")
def tts(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_speed_duration"))
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


def _with_codes(m, fn):
    """fn() -> (its result, the codes every segment handed to the latent pass)."""
    log, real = [], m._trim_codes

    def spy(ids):
        out = real(ids)
        log.append(out[0].tolist())
        return out

    m._trim_codes = spy
    try:
        return fn(), log
    finally:
        del m._trim_codes


@pytest.fixture(scope="module")
def natural(tts):
    """The plain greedy call: (pcm, code count per segment)."""
    m, wav = tts
    (sr, pcm), codes = _with_codes(m, lambda: _seeded(m, wav, TEXT, None, **GREEDY))
    assert sr == 22050 and m.last_duration is None and len(codes) >= 2
    return pcm, [len(c) for c in codes], codes


def test_speed_changes_the_frames_and_not_the_codes(tts, natural):
    m, wav = tts
    pcm0, ns, codes0 = natural
    gaps = GAP * (len(ns) - 1)
    assert pcm0.shape[0] == sum(S2.target_frames(n) for n in ns) * 256 + gaps
    sr, pcm = _seeded(m, wav, TEXT, None, speed=None, **GREEDY)
    assert sr == 22050 and pcm.dtype == pcm0.dtype and pcm.tobytes() == pcm0.tobytes() and m.last_duration is None
    for speed in (1.0, 1.25):
        (sr, pcm), codes = _with_codes(m, lambda: _seeded(m, wav, TEXT, None, speed=speed, **GREEDY))
        assert codes == codes0  # the decode does not see the speed
        frames = [S2.target_frames(n, speed) for n in ns]
        assert sr == 22050 and pcm.dtype == np.int16 and pcm.shape == (sum(frames) * 256 + gaps, 1) and np.abs(pcm).max() > 0
        rep = m.last_duration
        assert rep == dict(natural_s=pcm0.shape[0] / 22050.0, delivered_s=pcm.shape[0] / 22050.0,
                           speed=sum(S2.target_frames(n) for n in ns) / float(sum(frames)), pad_samples=0)
    assert pcm.shape[0] < pcm0.shape[0]
    chunks = list(_seeded(m, wav, TEXT, None, stream_return=True, speed=1.25, **GREEDY))
    assert [c.shape[1] for c in chunks[0::2]] == [f * 256 for f in frames] and all(tuple(c.shape) == (1, GAP) for c in chunks[1::2])
    assert m.last_duration["pad_samples"] == 0 and m.last_duration["delivered_s"] == (sum(frames) * 256 + gaps) / 22050.0


def test_bad_values_are_refused_before_any_work(tts, monkeypatch):
    m, wav = tts
    monkeypatch.setattr(m, "_encode_prompts", lambda *a, **k: pytest.fail("work began"))
    for kw in (dict(speed=True), dict(speed=float("nan")), dict(speed=0.3), dict(speed=2.5), dict(duration=0.0), dict(duration=float("nan")),
               dict(speed=1.0, duration=2.0), dict(duration=2.0, stream_return=True)):
        with pytest.raises(ValueError, match="speed|duration"):
            m.infer(wav, TEXT, None, **kw, **GREEDY)


@pytest.mark.parametrize("loud", [None, -23.0])
@pytest.mark.parametrize("rate,enc", [(None, None), (8000, "mulaw"), (44100, None)])
def test_duration_delivers_exactly_the_samples_asked_for(tts, natural, rate, enc, loud):
    m, wav = tts
    pcm0, ns, _ = natural
    sr = rate or 22050
    nat_s = pcm0.shape[0] / 22050.0
    nat = [S2.target_frames(n) for n in ns]
    orig, new = O.resample_ratio(22050, sr)
    zero = O.ZERO_CODES[enc or "pcm_s16le"]
    for factor in (0.8, 1.0, 1.3):
        D = nat_s * factor
        N = int(D * sr + 0.5)
        got_sr, pcm = _seeded(m, wav, TEXT, None, duration=D, output_sample_rate=rate, output_encoding=enc, output_loudness=loud, **GREEDY)
        rep = m.last_duration
        print(f"{sr} Hz {enc} loudness {loud} x{factor}: N {N}, report {rep}")
        assert got_sr == sr and pcm.shape == (N, 1) and pcm.dtype == (np.uint8 if enc == "mulaw" else np.int16)
        assert rep["delivered_s"] == N / float(sr) and abs(m.last_timing["audio_length"] - N / float(sr)) < 1e-12
        assert abs(rep["natural_s"] - O.delivered_len(nat, sr, 200) / float(sr)) < 1e-12
        frames, N1, pad = O.fit_frames(nat, D, sr, 200)
        assert N1 == N and rep["pad_samples"] == pad and rep["speed"] == sum(nat) / float(sum(frames))
        assert 0 <= pad < 256.0 * new / orig + len(ns)  # less than one frame's worth of delivered samples plus one per segment
        assert (pcm[N - pad:] == zero).all()
        assert (rep["speed"] > 1.0) == (factor < 1.0) or factor == 1.0  # (the gaps keep their length: the speech alone takes up the change)
        assert (m.last_loudness is not None) == (loud is not None)
        if factor == 1.0 and rate is None and loud is None:
            assert frames == nat and pad == 0 and np.array_equal(pcm, pcm0)  # the natural programme, through the output stage


def test_duration_file_header_and_the_unmeetable(tts, natural, tmp_path):
    m, wav = tts
    pcm0, ns, _ = natural
    nat_s = pcm0.shape[0] / 22050.0
    out = str(tmp_path / "fit.wav")
    assert _seeded(m, wav, TEXT, out, duration=nat_s * 1.3, output_sample_rate=8000, output_encoding="mulaw", **GREEDY) == out
    N = int(nat_s * 1.3 * 8000 + 0.5)
    info = O.riff_info(open(out, "rb").read())
    assert (info["tag"], info["rate"], info["frames"], info["fact"]) == (7, 8000, N, N) and m.last_timing["audio_length"] == N / 8000.0
    out = str(tmp_path / "fit16.wav")
    _seeded(m, wav, TEXT, out, duration=nat_s * 0.8, **GREEDY)
    with wave.open(out, "rb") as w:
        assert (w.getframerate(), w.getsampwidth(), w.getnframes()) == (22050, 2, int(nat_s * 0.8 * 22050 + 0.5))
    with pytest.raises(O.DurationError) as e:
        _seeded(m, wav, TEXT, None, duration=nat_s * 3, **GREEDY)
    err = e.value
    assert isinstance(err, ValueError) and abs(err.natural_s - nat_s) < 1e-12 and err.min_s < nat_s < err.max_s < nat_s * 3
    sr, pcm = _seeded(m, wav, TEXT, None, duration=err.max_s, **GREEDY)  # the end of the interval it carries can be asked for
    assert pcm.shape[0] == int(err.max_s * 22050 + 0.5) and m.last_duration["speed"] == 0.5 and m.last_duration["pad_samples"] == 0


def test_infer_many_pinned_request_with_a_speed_is_a_function_of_the_request(tts, monkeypatch):
    m, wav = tts
    P0 = dict(spk_audio_prompt=wav, text=TEXT, generation={"seed": 5})
    P = dict(P0, speed=0.8)
    Q = dict(spk_audio_prompt=wav, text="Another request. It is shorter.", generation={"seed": 9})
    R = dict(spk_audio_prompt=wav, text=TEXT)
    for env in ("0", "1"):
        monkeypatch.setenv("IXTTS_S2MEL_BATCH", env)
        alone = m.infer_many([P], decode_slots=8, **KW)
        rep = m.last_duration
        assert isinstance(alone[0], tuple) and len(rep) == 1 and rep[0]["pad_samples"] == 0 and rep[0]["speed"] < 1.0
        company = m.infer_many([Q, P, R], decode_slots=8, **KW)
        assert all(isinstance(o, tuple) for o in company) and m.last_duration == [None, rep[0], None]
        reordered = m.infer_many([R, dict(Q, speed=1.5), P], decode_slots=8, **KW)
        assert m.last_duration[0] is None and m.last_duration[1] is not None and m.last_duration[2] == rep[0]
        assert alone[0][1].tobytes() == company[1][1].tobytes() == reordered[2][1].tobytes(), env
        plain = m.infer_many([P0], decode_slots=8, **KW)
        assert m.last_duration == [None] and alone[0][1].shape[0] > plain[0][1].shape[0]
        assert abs(rep[0]["natural_s"] - plain[0][1].shape[0] / 22050.0) < 1e-12  # the same codes at the natural pace
    monkeypatch.setenv("IXTTS_S2MEL_BATCH", "0")
    plain = m.infer_many([P0], decode_slots=8, **KW)  # (segment after segment, as the calls below)
    # a bad value, and a duration that cannot be met, fail their own request only
    n0 = plain[0][1].shape[0] / 22050.0
    outs = m.infer_many([dict(P0, speed=3.0), P0, dict(P0, duration=n0 * 3), dict(P0, speed=1.2, duration=n0), dict(P0, duration=n0 * 1.2, sample_rate=16000)],
                        decode_slots=8, **KW)
    assert isinstance(outs[0], ValueError) and isinstance(outs[2], O.DurationError) and isinstance(outs[3], ValueError)
    assert abs(outs[2].natural_s - n0) < 1e-12 and outs[2].min_s < n0 < outs[2].max_s
    assert np.array_equal(outs[1][1], plain[0][1])
    assert outs[4][0] == 16000 and outs[4][1].shape[0] == int(n0 * 1.2 * 16000 + 0.5)
    rep = m.last_duration
    assert rep[:4] == [None] * 4 and rep[4]["delivered_s"] == outs[4][1].shape[0] / 16000.0 and rep[4]["speed"] < 1.0
    # a call-wide speed holds for every request that does not bring its own
    outs = m.infer_many([P0, dict(P0, speed=2.0)], decode_slots=8, speed=0.5, **KW)
    assert outs[0][1].shape[0] > plain[0][1].shape[0] > outs[1][1].shape[0]
    assert m.last_duration[0]["speed"] < 0.6 and m.last_duration[1]["speed"] > 1.7
