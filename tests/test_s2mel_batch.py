"""Row N1, many segments in ONE CFM solve (`S2Mel.solve_many`): the packed (ragged) rows against per-segment `__call__`s, on the
CPU leg (the torch forms of the packed row ops: row -> sequence index gathers).  The device forms are in test_gpu_s2mel_batch.py."""
import pytest
import torch

import voice_tts_amd.s2mel as S2

CFGS = {"tiny": {}, "hd64": dict(hidden_dim=128, num_heads=2, wavenet_hidden=128, depth=3)}


def _model(name, seed=5):
    cfg = S2.tiny_s2mel_cfg(gpt_dim=1280, semantic_dim=1024, lr_in_channels=1024, codebook_size=8194, **CFGS[name])
    return S2.S2Mel(S2.make_s2mel_weights(cfg, seed=seed), cfg), cfg


def _item(cfg, g, n_codes, Tp):
    return (torch.randn(1, n_codes, cfg["gpt_dim"], generator=g), torch.randint(0, cfg["codebook_size"], (1, n_codes), generator=g),
            torch.randn(1, Tp, cfg["content_dim"], generator=g), torch.randn(1, 80, Tp, generator=g) * 2 - 4,
            torch.randn(1, cfg["style_dim"], generator=g))


def _call(m, it, **kw):
    return m(it[0], it[1], torch.tensor([it[1].shape[1]]), it[2], it[3], it[4], **kw)


def _frames(it):
    return it[2].shape[1] + int(it[1].shape[1] * 1.72)


# (codes, prompt frames): T = Tp + floor(1.72 n) covers T mod 4 = 0..3; two prompt lengths; (1, 4) is shorter than the WaveNet halo
SHAPES = {1: [(9, 12)], 2: [(7, 12), (12, 20)], 5: [(7, 12), (9, 20), (3, 12), (20, 20), (1, 4)]}


@pytest.mark.parametrize("name", list(CFGS))
@pytest.mark.parametrize("n", [1, 2, 5])
def test_solve_many_equals_per_segment_calls(name, n):
    m, cfg = _model(name)
    g = torch.Generator().manual_seed(100 + n)
    items = [_item(cfg, g, nc, Tp) for nc, Tp in SHAPES[n]]
    if n == 5:
        assert sorted(_frames(it) % 4 for it in items[:4]) == [0, 1, 2, 3] and _frames(items[4]) < m._halo()
    noises = [torch.randn(1, 80, _frames(it), generator=g) for it in items]
    outs = m.solve_many(items, n_timesteps=3, noises=noises)
    assert len(outs) == n
    for it, z, out in zip(items, noises, outs):
        ref = _call(m, it, n_timesteps=3, noise=z)
        assert out.shape == ref.shape == (1, 80, int(it[1].shape[1] * 1.72))
        assert (out - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


def test_solve_many_without_cfg_and_over_several_packs(monkeypatch):
    """inference_cfg_rate 0 (no null branch), and a frame budget that splits the request into several packs grouped by length."""
    m, cfg = _model("tiny")
    g = torch.Generator().manual_seed(7)
    items = [_item(cfg, g, nc, Tp) for nc, Tp in [(7, 12), (30, 20), (4, 12), (12, 8)]]
    noises = [torch.randn(1, 80, _frames(it), generator=g) for it in items]
    monkeypatch.setenv("IXTTS_S2MEL_BATCH_FRAMES", "40")
    calls = []
    real = m._cfm_packed
    monkeypatch.setattr(m, "_cfm_packed", lambda segs, *a: (calls.append([s["mu"].shape[1] for s in segs]), real(segs, *a))[1])
    for rate in (0.0, 0.7):
        calls.clear()
        outs = m.solve_many(items, n_timesteps=2, inference_cfg_rate=rate, noises=noises)
        for it, z, out in zip(items, noises, outs):
            ref = _call(m, it, n_timesteps=2, inference_cfg_rate=rate, noise=z)
            assert (out - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
        assert [t for c in calls for t in c] == sorted(_frames(it) for it in items)
        assert all(sum(c) <= 40 or len(c) == 1 for c in calls) and len(calls) > 1


def test_reference_fixture_second_in_a_pack(golden):
    """tests/golden/s2mel_tiny.npz (the reference's MyModel / CFM), solved second in a pack beside another segment, reproduces the
    fixture's mel within test_s2mel_golden's tolerance."""
    g = golden("s2mel_tiny.npz")
    cfg = S2.tiny_s2mel_cfg(gpt_dim=1280, semantic_dim=1024, lr_in_channels=1024, codebook_size=8194)
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=int(g["seed"])), cfg)
    t = lambda k: torch.from_numpy(g[k])  # noqa: E731
    fx = (t("latent"), t("codes"), t("prompt_condition"), t("ref_mel"), t("style"))
    gen = torch.Generator().manual_seed(3)
    other = _item(cfg, gen, 11, 17)
    outs = m.solve_many([other, fx], n_timesteps=int(g["n_steps"]), noises=[torch.randn(1, 80, _frames(other), generator=gen), t("noise")])
    ref = t("mel")
    assert outs[1].shape == ref.shape
    assert (outs[1] - ref).abs().max().item() <= 5e-5 * max(1.0, ref.abs().max().item())


def test_seeded_noise_matches_successive_calls():
    """noises=None: each item's noise is drawn from the default generator in item order, as n successive `__call__`s draw it."""
    m, cfg = _model("tiny")
    g = torch.Generator().manual_seed(9)
    items = [_item(cfg, g, nc, Tp) for nc, Tp in [(12, 20), (5, 12), (8, 12)]]
    torch.manual_seed(1234)
    outs = m.solve_many(items, n_timesteps=2)
    torch.manual_seed(1234)
    refs = [_call(m, it, n_timesteps=2) for it in items]
    for out, ref in zip(outs, refs):
        assert (out - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


def test_packed_row_ops_torch_forms():
    """The CPU forms of the packed row ops equal the single-sequence ops applied sequence by sequence."""
    g = torch.Generator().manual_seed(2)
    lens, H = [5, 1, 9, 4], 16
    pk = S2.RowPack(lens, "cpu")
    x = torch.randn(pk.rows, H, generator=g)
    wb, gg = torch.randn(len(lens), 2 * H, generator=g), torch.randn(H, generator=g)
    a = S2.adaln_rmsnorm_packed(x, wb, gg, pk)
    b = S2.ln_modulate_packed(x, wb, pk)
    for s in range(pk.n):
        lo, hi = pk.span(s)
        assert torch.allclose(a[lo:hi], S2.adaln_rmsnorm(x[None, lo:hi], wb[s:s + 1], gg)[0], atol=1e-6)
        assert torch.allclose(b[lo:hi], S2.ln_modulate(x[None, lo:hi], wb[s:s + 1])[0], atol=1e-6)
    # RoPE restarts at each sequence
    hd = 8
    qkv = torch.randn(pk.rows, 3 * H, generator=g)
    ang = torch.outer(torch.arange(16).float(), 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd)))
    fc = torch.polar(torch.ones_like(ang), ang)
    r = S2.rope_qk_packed(qkv, fc, pk, hd)
    for s in range(pk.n):
        lo, hi = pk.span(s)
        q = S2.S2Mel._rotary(qkv[None, lo:hi, :H].reshape(1, hi - lo, H // hd, hd), fc[:hi - lo]).reshape(hi - lo, H)
        assert torch.allclose(r[lo:hi, :H], q, atol=1e-6) and torch.equal(r[:, 2 * H:], qkv[:, 2 * H:])
    # reflect halo per sequence (torch's reflect padding; zero-extended as encodec's pad1d below the pad length)
    left = right = 2
    pp = S2.RowPack([t + 4 for t in lens], "cpu")
    P = torch.randn(pp.rows, 3, generator=g)
    S2.reflect_halo_rows_packed(P, pp, left, right)
    for s in range(pp.n):
        lo, hi = pp.span(s)
        inner = P[lo + left:hi - right].t()[None]
        assert torch.equal(P[lo:hi].t()[None], S2._pad_reflect(inner, left, right))
    # the gate takes the biases of the row's sequence (rows past the end: the last one)
    C = 4
    acc = torch.randn(pp.rows - 4, 2 * C, generator=g)
    gate = torch.randn(pp.n, 3 * 2 * C, generator=g)
    out = S2.wn_gate_rows_packed(acc, gate, 2 * C, C, pp)
    seq = torch.repeat_interleave(torch.arange(pp.n), torch.tensor(pp.lens))[:acc.shape[0]]
    xg = acc + gate[seq, 2 * C:4 * C]
    assert torch.allclose(out, torch.tanh(xg[:, :C]) * torch.sigmoid(xg[:, C:]))
