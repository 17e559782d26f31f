"""The s2mel DiT / WaveNet GEMMs with fused epilogues (csrc/gemm_x6.hip `ixtts_gemm_x6_pair_f32`): [w1; w3] with the SwiGLU in its
epilogue and the WaveNet's k taps as one GEMM with the gate in its epilogue, against fp64 at the production shapes (the criterion of
test_gpu_gemm_x6.py), the DiT with them against the library GEMMs (IXTTS_S2MEL_GEMM=library), and that the device path takes them."""
import os

import pytest
import torch

from voice_tts_amd import _lib
from voice_tts_amd import gemm as G


def _errors(out, ref, lib, scale=None):
    scale = ref.abs().max() if scale is None else scale
    e_x6, e_lib = float((out - ref).abs().max() / scale), float((lib - ref).abs().max() / scale)
    rms = lambda d: float((d ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())  # noqa: E731
    return e_x6, e_lib, rms(out - ref), rms(lib - ref)


def test_interleave_halves_and_argument_checks():
    """CPU: the packing order the pair epilogues read, and the entry point refuses bad shapes before touching a device."""
    a, b = torch.arange(64 * 3).reshape(64, 3), -torch.arange(64 * 3).reshape(64, 3)
    w = G.interleave_halves(a, b)
    assert torch.equal(w[:32], a[:32]) and torch.equal(w[32:64], b[:32]) and torch.equal(w[64:96], a[32:]) and torch.equal(w[96:], b[32:])
    if not os.path.exists(_lib.LIB_PATH):
        from voice_tts_amd import build
        build.build(verbose=False)
    L = _lib.lib()
    assert L.ixtts_gemm_x6_pair_f32(None, 100, 0, 1, None, None, None, 0, 1, 1, None, 64, 100, 128, 512, 1, 0, None) != 0
    assert L.ixtts_gemm_x6_pair_f32(1, 100, 0, 3, 1, None, None, 0, 1, 1, 1, 64, 100, 128, 512, 1, 0, None) != 0  # K not taps x 64k
    assert L.ixtts_gemm_x6_pair_f32(1, 100, 0, 1, 1, None, None, 0, 1, 1, 1, 64, 100, 96, 512, 1, 0, None) != 0  # N % 64
    assert L.ixtts_gemm_x6_pair_f32(1, 100, 0, 1, 1, None, None, 0, 1, 1, 1, 64, 100, 128, 512, 2, 0, None) != 0  # gate without biases


@pytest.mark.gpu
@pytest.mark.parametrize("M,Fd,K,tile", [(4644, 1536, 512, 0), (4644, 1536, 512, 3), (300, 128, 64, 2), (257, 96, 192, 3)])
def test_swiglu_epilogue_matches_fp64(M, Fd, K, tile):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + Fd)
    x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    w1, w3 = torch.randn(Fd, K, generator=g) / K ** 0.5, torch.randn(Fd, K, generator=g) / K ** 0.5
    xd = x.double()
    a, b = xd @ w1.double().t(), xd @ w3.double().t()
    ref = a * torch.sigmoid(a) * b
    pl = G.PackedLinear(G.interleave_halves(w1, w3).to(dev))
    out = G.pair_linear(x.to(dev), pl, G.SWIGLU, tile=tile).cpu().double()
    u = torch.nn.functional.linear(x.to(dev), torch.cat([w1, w3]).to(dev))
    lib = (torch.nn.functional.silu(u[:, :Fd]) * u[:, Fd:]).cpu().double()
    e_x6, e_lib, rms_x6, rms_lib = _errors(out, ref, lib)
    print(f"swiglu {M}x{2 * Fd}x{K} tile {tile}: max err {e_x6:.2e} (library {e_lib:.2e}), rms {rms_x6:.2e} (library {rms_lib:.2e})")
    assert e_x6 <= 2e-6 and rms_x6 <= max(2e-7, 2.0 * rms_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,C,k", [(2, 1909, 512, 5), (2, 203, 64, 5), (3, 90, 128, 3)])
def test_tap_gate_epilogue_matches_fp64(B, T, C, k):
    """k taps over row-shifted windows of ONE split of a padded row buffer [B * (T + k - 1), C] + bias + per-batch gate biases.  The
    error is taken relative to the GEMM's own scale, max |a + g|: the gate maps a GEMM error e to at most 1.25 e (|d/da| <= 1,
    |d/db| <= 1/4), while its output is bounded by 1 -- against that, the library's own error at K = 5 x 512 is at the 2e-6 bar."""
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(T + C)
    Tp = T + k - 1
    P = torch.randn(B * Tp, C, generator=g)
    taps = torch.randn(2 * C, C, k, generator=g) / (C * k) ** 0.5
    bias = 0.1 * torch.randn(2 * C, generator=g)
    nl = 3
    gate = torch.randn(B, 2 * C * nl, generator=g)
    off = 2 * C  # layer 1's gate biases
    M = B * Tp - (k - 1)
    Pd = P.double()
    acc = bias.double() + sum(Pd[j:j + M] @ taps[:, :, j].double().t() for j in range(k))
    bidx = (torch.arange(M) // Tp).clamp(max=B - 1)
    xg = acc + gate.double()[bidx, off:off + 2 * C]
    ref = torch.tanh(xg[:, :C]) * torch.sigmoid(xg[:, C:])
    wcat = torch.cat([taps[:, :, j] for j in range(k)], 1)
    pl = G.PackedLinear(G.interleave_halves(wcat[:C], wcat[C:]).to(dev), G.interleave_halves(bias[:C], bias[C:]).to(dev))
    out = G.pair_linear(G.split(P.to(dev)), pl, G.GATE, taps=k, gate=gate.to(dev), gate_off=off, rows_per_batch=Tp).cpu().double()
    assert out.shape == (M, C)
    from voice_tts_amd.s2mel import wn_gate_rows

    Pg = P.to(dev)
    la = torch.addmm(bias.to(dev), Pg[:M], taps[:, :, 0].t().to(dev))
    for j in range(1, k):
        la.addmm_(Pg[j:j + M], taps[:, :, j].t().to(dev))
    lib = wn_gate_rows(la, gate.to(dev), off, C, Tp).cpu().double()
    e_x6, e_lib, rms_x6, rms_lib = _errors(out, ref, lib, scale=xg.abs().max())
    print(f"taps+gate B={B} T={T} C={C} k={k}: max err {e_x6:.2e} (library {e_lib:.2e}), rms {rms_x6:.2e} (library {rms_lib:.2e})")
    assert e_x6 <= 2e-6 and rms_x6 <= max(2e-7, 2.0 * rms_lib)


@pytest.mark.gpu
def test_dit_on_fused_gemms_matches_library_and_takes_them(monkeypatch):
    """Production width, 3 Euler steps of the CFM (CFG batch of 2): the fused-epilogue GEMMs against IXTTS_S2MEL_GEMM=library within
    1e-5 of scale; and every [w1; w3] and WaveNet in_layer of a DiT step goes through them on the device."""
    import voice_tts_amd.s2mel as S2

    dev = torch.device("cuda:0")
    cfg = S2.S2MEL_CFG
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=1234), cfg, device=dev)
    g = torch.Generator().manual_seed(11)
    T, Tp = 900, 300
    mu = torch.randn(1, T, cfg["content_dim"], generator=g).to(dev)
    prompt = (torch.randn(1, 80, Tp, generator=g) * 2 - 5).to(dev)
    style = torch.randn(1, cfg["style_dim"], generator=g).to(dev)
    noise = torch.randn(1, 80, T, generator=g)
    lens = torch.tensor([T], device=dev)

    calls = []
    real = G.pair_linear
    monkeypatch.setattr(G, "pair_linear", lambda *a, **kw: (calls.append(a[2]), real(*a, **kw))[1])
    monkeypatch.setenv("IXTTS_S2MEL_GEMM", "library")
    lib = m.cfm_inference(mu, lens, prompt, style, n_timesteps=3, noise=noise)
    assert calls == []
    monkeypatch.delenv("IXTTS_S2MEL_GEMM")
    x6 = m.cfm_inference(mu, lens, prompt, style, n_timesteps=3, noise=noise)
    per_step = [G.SWIGLU] * cfg["depth"] + [G.GATE] * cfg["wavenet_layers"]
    assert calls == per_step * 3
    err = float((x6 - lib).abs().max()) / max(1.0, float(lib.abs().max()))
    print(f"cfm 3 steps, fused GEMMs vs library: rel err {err:.2e}")
    assert err <= 1e-5
