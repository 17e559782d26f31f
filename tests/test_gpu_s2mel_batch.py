"""Row N1 on the device, many segments in ONE CFM solve: the packed (ragged) HIP entries (csrc/attn_full_x3.hip varlen attention,
csrc/dit_ops.hip *_varlen row ops, csrc/gemm_x6.hip gate epilogue over packed sequences) against fp64 / their torch forms, and
`S2Mel.solve_many` at production width against per-segment `__call__`s, down to `IndexTTS2.infer` / `infer_many`."""
import numpy as np
import pytest
import torch

import voice_tts_amd.s2mel as S2
from voice_tts_amd import gemm as G

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def test_varlen_attention_matches_fp64_per_sequence():
    """Queries of sequence s see the keys of sequence s only; lengths 1, 63, 64, 65, 301, 2322 and more, 16 sequences x 8 heads, on
    strided views of one packed wqkv output."""
    lens = [1, 63, 64, 65, 301, 2322, 5, 128, 129, 700, 2, 1000, 33, 256, 17, 420]
    H = 8
    pk = S2.RowPack(lens, DEV)
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(pk.rows, 3, H, 64, generator=g)
    qkv[:, 0] *= 2.0  # sharper softmax
    qd = qkv.to(DEV)
    out = S2.attn_full_packed(qd[:, 0], qd[:, 1], qd[:, 2], pk).cpu().double()
    worst = 0.0
    for s in range(pk.n):
        a, b = pk.span(s)
        q, k, v = (qkv[a:b, i].double().transpose(0, 1) for i in range(3))
        ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).transpose(0, 1)
        err = (out[a:b] - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        worst = max(worst, err)
        assert err <= 2e-5, (lens[s], err)
    print(f"varlen attention, {pk.n} sequences x {H} heads: worst rel err {worst:.2e}")


def test_packed_row_ops_match_their_torch_forms():
    lens, H, hd = [1, 70, 5, 300, 64, 2], 512, 64
    pk = S2.RowPack(lens, DEV)
    pkc = S2.RowPack(lens, "cpu")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(pk.rows, H, generator=g)
    wb, gg = torch.randn(pk.n, 2 * H, generator=g), 1 + 0.1 * torch.randn(H, generator=g)
    close = lambda a, b: (a.cpu() - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())  # noqa: E731
    assert close(S2.adaln_rmsnorm_packed(x.to(DEV), wb.to(DEV), gg.to(DEV), pk), S2.adaln_rmsnorm_packed(x, wb, gg, pkc))
    assert close(S2.ln_modulate_packed(x.to(DEV), wb.to(DEV), pk), S2.ln_modulate_packed(x, wb, pkc))
    qkv = torch.randn(pk.rows, 3 * H, generator=g)
    ang = torch.outer(torch.arange(400).float(), 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd)))
    fc = torch.polar(torch.ones_like(ang), ang)
    qd = qkv.to(DEV)
    S2.rope_qk_packed(qd, fc.to(DEV), pk, hd)
    assert close(qd, S2.rope_qk_packed(qkv, fc, pkc, hd))
    # the WaveNet pack: each sequence with its own k - 1 halo rows
    pp, ppc = S2.RowPack([t + 4 for t in lens if t > 2], DEV), S2.RowPack([t + 4 for t in lens if t > 2], "cpu")
    P = torch.randn(pp.rows, 128, generator=g)
    Pd = P.to(DEV)
    S2.reflect_halo_rows_packed(Pd, pp, 2, 2)
    assert torch.equal(Pd.cpu(), S2.reflect_halo_rows_packed(P.clone(), ppc, 2, 2))
    C = 128
    acc = torch.randn(pp.rows - 4, 2 * C, generator=g)
    gate = torch.randn(pp.n, 3 * 2 * C, generator=g)
    assert close(S2.wn_gate_rows_packed(acc.to(DEV), gate.to(DEV), 2 * C, C, pp), S2.wn_gate_rows_packed(acc, gate, 2 * C, C, ppc))


@pytest.mark.parametrize("lens,C,k", [([1909, 450, 30, 1000], 512, 5), ([203, 7, 90], 64, 5), ([90, 12, 40], 128, 3)])
def test_ragged_tap_gate_epilogue_matches_fp64(lens, C, k):
    """k taps over row-shifted windows of ONE split of a padded pack + bias + the gate biases of each row's own sequence, with the
    error bound of test_gpu_s2mel_gemm.test_tap_gate_epilogue_matches_fp64."""
    g = torch.Generator().manual_seed(sum(lens) + C)
    pp = S2.RowPack([t + k - 1 for t in lens], DEV)
    P = torch.randn(pp.rows, C, generator=g)
    taps = torch.randn(2 * C, C, k, generator=g) / (C * k) ** 0.5
    bias = 0.1 * torch.randn(2 * C, generator=g)
    nl = 3
    gate = torch.randn(pp.n, 2 * C * nl, generator=g)
    off = 2 * C
    M = pp.rows - (k - 1)
    Pd = P.double()
    acc = bias.double() + sum(Pd[j:j + M] @ taps[:, :, j].double().t() for j in range(k))
    bidx = torch.repeat_interleave(torch.arange(pp.n), torch.tensor(pp.lens))[:M]
    xg = acc + gate.double()[bidx, off:off + 2 * C]
    ref = torch.tanh(xg[:, :C]) * torch.sigmoid(xg[:, C:])
    wcat = torch.cat([taps[:, :, j] for j in range(k)], 1)
    pl = G.PackedLinear(G.interleave_halves(wcat[:C], wcat[C:]).to(DEV), G.interleave_halves(bias[:C], bias[C:]).to(DEV))
    out = G.pair_linear(G.split(P.to(DEV)), pl, G.GATE, taps=k, gate=gate.to(DEV), gate_off=off, seq_off=pp).cpu().double()
    Pg = P.to(DEV)
    la = torch.addmm(bias.to(DEV), Pg[:M], taps[:, :, 0].t().to(DEV))
    for j in range(1, k):
        la.addmm_(Pg[j:j + M], taps[:, :, j].t().to(DEV))
    lib = S2.wn_gate_rows_packed(la, gate.to(DEV), off, C, pp).cpu().double()
    scale = xg.abs().max()
    e_x6, e_lib = float((out - ref).abs().max() / scale), float((lib - ref).abs().max() / scale)
    rms = lambda d: float((d ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())  # noqa: E731
    print(f"ragged taps+gate {lens} C={C} k={k}: max err {e_x6:.2e} (library {e_lib:.2e})")
    assert e_x6 <= 2e-6 and rms(out - ref) <= max(2e-7, 2.0 * rms(lib - ref))
    assert e_lib <= 2e-6


@pytest.fixture(scope="module")
def prod():
    cfg = S2.S2MEL_CFG
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=1234), cfg, device=DEV)
    g = torch.Generator().manual_seed(21)
    items, noises = [], []
    for n, Tp in [(150, 430), (423, 200), (1100, 430)]:
        items.append((torch.randn(1, n, cfg["gpt_dim"], generator=g).to(DEV), torch.randint(0, cfg["codebook_size"], (1, n), generator=g).to(DEV),
                      torch.randn(1, Tp, cfg["content_dim"], generator=g).to(DEV), (torch.randn(1, 80, Tp, generator=g) * 2 - 5).to(DEV),
                      torch.randn(1, cfg["style_dim"], generator=g).to(DEV)))
        noises.append(torch.randn(1, 80, Tp + int(n * 1.72), generator=g).to(DEV))
    return m, items, noises


@pytest.mark.parametrize("env", [{}, {"IXTTS_S2MEL_GEMM": "library"}, {"IXTTS_ATTN_FULL": "f32"}])
def test_solve_many_production_width_equals_per_segment_calls(prod, env, monkeypatch):
    m, items, noises = prod
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    outs = m.solve_many(items, n_timesteps=3, noises=noises)
    worst = 0.0
    for it, z, out in zip(items, noises, outs):
        ref = m(it[0], it[1], torch.tensor([it[1].shape[1]], device=DEV), it[2], it[3], it[4], n_timesteps=3, noise=z)
        assert out.shape == ref.shape
        err = (out - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        worst = max(worst, err)
    print(f"solve_many {env}: worst rel err {worst:.2e}")
    assert worst <= 1e-5


def test_packed_step_launches_do_not_grow_with_segments(prod, monkeypatch):
    """One Euler step of the packed solve issues as many HIP launches (row ops, attention, split-product GEMMs) for 4 segments as
    for 1."""
    m, items, noises = prod
    counts = []
    real_call, real_attn, real_pair, real_split = S2._hip_call, S2.attn_full_packed, G.pair_linear, G.split
    log, on = [], [False]
    spy = lambda name, fn: lambda *a, **k: ((log.append(name) if on[0] else None), fn(*a, **k))[1]  # noqa: E731
    monkeypatch.setattr(S2, "_hip_call", lambda *a: ((log.append(a[0]) if on[0] else None), real_call(*a))[1])
    monkeypatch.setattr(S2, "attn_full_packed", spy("attn", real_attn))
    monkeypatch.setattr(G, "pair_linear", spy("pair", real_pair))
    monkeypatch.setattr(G, "split", spy("split", real_split))
    real_solve = m._cfm_packed

    def solve(*a):  # the packed solve only (the per-item length regulators before it are not part of the step)
        on[0] = True
        try:
            return real_solve(*a)
        finally:
            on[0] = False

    monkeypatch.setattr(m, "_cfm_packed", solve)
    for n in (1, 4):
        log.clear()
        m.solve_many([items[i % 2] for i in range(n)], n_timesteps=1, noises=[noises[i % 2] for i in range(n)])
        counts.append(len(log))
    print(f"HIP launches per packed step: {counts}")
    assert counts[0] == counts[1] and counts[0] > 0


@pytest.fixture(scope="module")
def tts_from_dir(tmp_path_factory):
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM


def test_infer_packs_the_segments_into_one_solve(tts_from_dir, monkeypatch):
    """With IXTTS_S2MEL_BATCH=1 a multi-segment `infer` makes ONE solve_many call; its PCM equals the default's (segment after
    segment, IXTTS_S2MEL_BATCH=0) within 2 LSB."""
    m, SM = tts_from_dir
    wav = SM.synthetic_wav_bytes(1.5, 24000)
    text = "Hello world, this is a test. Another sentence here. And a third one, a little longer than the others."
    calls = []
    real = m.s2mel.solve_many
    monkeypatch.setattr(m.s2mel, "solve_many", lambda items, **kw: (calls.append(len(items)), real(items, **kw))[1])
    kw = dict(num_beams=1, top_k=1, max_mel_tokens=24, max_text_tokens_per_segment=12)
    m.infer(wav, "Warm.", None, num_beams=1, top_k=1, max_mel_tokens=4)  # the prompt caches filled before the seeded runs
    monkeypatch.setenv("IXTTS_S2MEL_BATCH", "1")
    torch.manual_seed(7)
    sr, pcm = m.infer(wav, text, None, **kw)
    assert len(calls) == 1 and calls[0] > 1 and m.last_timing["s2mel_time"] > 0
    monkeypatch.setenv("IXTTS_S2MEL_BATCH", "0")
    torch.manual_seed(7)
    sr0, pcm0 = m.infer(wav, text, None, **kw)
    assert len(calls) == 1
    assert pcm.shape == pcm0.shape and int(np.abs(pcm.astype(np.int32) - pcm0.astype(np.int32)).max()) <= 2


def test_infer_many_packs_every_request_and_fails_requests_alone(tts_from_dir, monkeypatch):
    m, SM = tts_from_dir
    wav_a, wav_b = SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1)
    reqs = [dict(spk_audio_prompt=wav_a, text="Hello world, this is a test. A second one."),
            dict(spk_audio_prompt=b"this is not audio at all", text="Broken prompt."),
            dict(spk_audio_prompt=wav_b, text="Short.")]
    calls = []
    real = m.s2mel.solve_many
    monkeypatch.setattr(m.s2mel, "solve_many", lambda items, **kw: (calls.append(len(items)), real(items, **kw))[1])
    kw = dict(decode_slots=4, num_beams=1, top_k=1, max_mel_tokens=20, max_text_tokens_per_segment=8)
    m.infer_many(reqs, **kw)  # the prompt caches in the state the seeded runs find them
    assert calls == []  # off by default
    monkeypatch.setenv("IXTTS_S2MEL_BATCH", "1")
    torch.manual_seed(3)
    outs = m.infer_many(reqs, **kw)
    assert isinstance(outs[1], Exception) and isinstance(outs[0], tuple) and isinstance(outs[2], tuple)
    assert len(calls) == 1 and calls[0] >= 3  # both speakers' segments in one pack
    monkeypatch.setenv("IXTTS_S2MEL_BATCH", "0")
    torch.manual_seed(3)
    outs0 = m.infer_many(reqs, **kw)
    for a, b in ((outs[0], outs0[0]), (outs[2], outs0[2])):
        assert a[1].shape == b[1].shape and int(np.abs(a[1].astype(np.int32) - b[1].astype(np.int32)).max()) <= 2
