"""The fp64 twin of the s2mel stage (`S2Mel(W, cfg, dtype=torch.float64)`, CPU): the high-precision reference the device paths are
measured against in test_gpu_s2mel_fp64.py.  Here: the twin is fp64 throughout, it reproduces the reference program's fixtures (so it
is not only a copy of this project's own reading of the model), the default dtype is untouched, and the fp32 CPU leg's distance from
the twin -- the arithmetic's own noise, the yardstick of the device tests -- is printed and held below the fixtures' bar."""
import pytest
import torch

import s2mel_budget as SB
import voice_tts_amd.s2mel as S2

FIXTURES = {"s2mel_tiny.npz": {}, "s2mel_hd64.npz": dict(hidden_dim=128, num_heads=2, wavenet_hidden=128, depth=3)}


@pytest.fixture(scope="module", params=list(SB.CONFIGS))
def legs(request):
    cfg, cpu, twin = SB.models(request.param)
    return request.param, cfg, cpu, twin, SB.inputs(cfg)


def _all_tensors(x, seen=None):
    seen = set() if seen is None else seen
    if id(x) in seen:
        return
    seen.add(id(x))
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, dict):
        for v in x.values():
            yield from _all_tensors(v, seen)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _all_tensors(v, seen)
    elif hasattr(x, "__dict__"):  # PackedLinear and the like
        yield from _all_tensors(vars(x), seen)


def test_twin_holds_and_returns_fp64_only(legs):
    name, cfg, cpu, twin, inp = legs
    twin._rope_cache(70)
    held = list(_all_tensors(vars(twin)))
    assert len(held) > len(twin.W) > 50
    for t in held:
        assert t.dtype in (torch.float64, torch.complex128), t.dtype
    i = SB._to(twin, inp)
    ctx, x, tp = SB._cfg_context(twin, i["seg"])
    for t in _all_tensors(ctx):
        assert t.dtype in (torch.float64, torch.bool), t.dtype
    t1 = twin._t_embed(torch.tensor([SB.T_EVAL]), "cfm.estimator.t_embedder")
    assert t1.dtype == torch.float64
    outs = [twin.dit_step(ctx, x, torch.full((2,), SB.T_EVAL), out_from=tp), twin._attention(i["qkv150"].clone(), 2, 150, None),
            twin._transformer(i["tr_x"], i["tr_c"], None), twin._wavenet_rows(i["wn_h"], i["wn_g"]),
            twin.cfm_inference(i["seg"]["mu"], torch.tensor([SB.T]), i["seg"]["prompt"], i["seg"]["style"], 1, SB.CFG_RATE, noise=i["seg"]["z"])]
    outs += twin._cfm_packed(i["pack"][:2], 1, SB.CFG_RATE)
    for o in outs:
        assert o.dtype == torch.float64


def test_what_precedes_the_activations_is_the_fp32_models(legs):
    """t_freqs, the timestep sinusoids and the RoPE table are computed in fp32 as the default leg computes them, then widened: the
    twin's tables equal the fp32 leg's bit for bit, so the two differ by rounding of the arithmetic alone."""
    name, cfg, cpu, twin, inp = legs
    assert torch.equal(twin.t_freqs, cpu.t_freqs.double())
    assert torch.equal(twin._rope_cache(300), cpu._rope_cache(300).to(torch.complex128))
    for k, w in cpu.W.items():
        assert torch.equal(twin.W[k], w.double()), k
    seen = []
    real = torch.nn.functional.linear
    try:
        torch.nn.functional.linear = lambda x, *a, **k: (seen.append(x), real(x, *a, **k))[1]
        t = torch.tensor([SB.T_EVAL, 0.0, 1.0])
        cpu._t_embed(t, "cfm.estimator.t_embedder")
        twin._t_embed(t, "cfm.estimator.t_embedder")
    finally:
        torch.nn.functional.linear = real
    assert seen[0].dtype == torch.float32 and seen[2].dtype == torch.float64 and torch.equal(seen[2], seen[0].double())
    # the length regulator's nearest-neighbour stretch picks the frames the fp32 op picks (90 -> 154 frames differs in fp64 arithmetic)
    x = torch.randn(1, 90, cfg["lr_in_channels"], generator=torch.Generator().manual_seed(2))
    a, b = cpu.length_regulator(x, torch.tensor([154])), twin.length_regulator(x.double(), torch.tensor([154]))
    assert b.dtype == torch.float64 and (a - b).abs().max().item() <= 2e-5 * max(1.0, b.abs().max().item())


def test_device_twin_and_other_dtypes_are_refused():
    cfg = SB.CONFIGS["hd64"]()
    W = S2.make_s2mel_weights(cfg, seed=1)
    with pytest.raises(ValueError):
        S2.S2Mel(W, cfg, device="cuda", dtype=torch.float64)
    with pytest.raises(ValueError):
        S2.S2Mel(W, cfg, dtype=torch.float16)
    assert S2.S2Mel(W, cfg).dtype == torch.float32 and all(w.dtype == torch.float32 for w in S2.S2Mel(W, cfg).W.values())


@pytest.mark.parametrize("fx", list(FIXTURES))
def test_twin_vs_reference_fixtures(golden, fx):
    """The twin against the reference program's own outputs, at the bar the fp32 stage has there on the device (2e-4 x max)."""
    g = golden(fx)
    cfg = S2.tiny_s2mel_cfg(gpt_dim=1280, semantic_dim=1024, lr_in_channels=1024, codebook_size=8194, **FIXTURES[fx])
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=int(g["seed"])), cfg, dtype=torch.float64)
    f = lambda k: torch.from_numpy(g[k]).double()  # noqa: E731
    n = g["codes"].shape[1]
    mel = m(f("latent"), torch.from_numpy(g["codes"]), torch.tensor([n]), f("prompt_condition"), f("ref_mel"), f("style"),
            n_timesteps=int(g["n_steps"]), inference_cfg_rate=0.7, noise=f("noise"))
    ref = f("mel")
    assert mel.dtype == torch.float64 and mel.shape == ref.shape
    err = (mel - ref).abs().max().item()
    print(f"twin vs {fx}: max|err| {err:.3e} (|ref|max {ref.abs().max().item():.3f})")
    assert err <= 2e-4 * max(1.0, ref.abs().max().item())
    # one DiT evaluation too
    cat = torch.cat([f("prompt_condition"), f("cond")], dim=1)
    T = cat.shape[1]
    one = m.dit(f("noise"), torch.zeros(1, 80, T, dtype=torch.float64), torch.tensor([T]), torch.tensor([0.3]), f("style"), cat)
    ref1 = f("dit_one")
    assert (one - ref1).abs().max().item() <= 2e-4 * max(1.0, ref1.abs().max().item())


@pytest.mark.parametrize("case", SB.CPU_CASES)
def test_fp32_cpu_leg_against_the_twin(legs, case, record_property):
    """The fp32 arithmetic's own noise: one velocity evaluation at t = 0.37, a 3-step solve, a 3-step packed solve.  Measured
    (max, rms; relative to the twin's max and rms): hd64 4.1e-7..5.8e-7, production width at T = 200 7.0e-7..8.0e-7 -- more than two
    orders of magnitude below the 2e-4 fixture bar asserted here.  The numbers are the yardstick of test_gpu_s2mel_fp64.py."""
    name, cfg, cpu, twin, inp = legs
    ref = SB.run(twin, case, inp)
    got = SB.run(cpu, case, inp)
    assert ref.dtype == torch.float64 and got.shape == ref.shape
    e_max, e_rms = SB.rel_err(got, ref)
    print(f"fp32 CPU leg vs twin, {name} {case}: max {e_max:.3e} rms {e_rms:.3e}")
    record_property("e_max", e_max)
    record_property("e_rms", e_rms)
    assert 0.0 < e_max < 2e-4 and 0.0 < e_rms < 2e-4, (e_max, e_rms)
