"""The GPT's third weight type, IEEE half (`dtype="f16"`): fp16 matrices and K/V cache, fp32 activations and accumulation.

Every bound here is the bf16 bound of the same comparison (tests/test_gpu_gpt.py, test_gpu_wide.py, test_gpu_fullsize.py)
divided by 4: fp16 rounds an operand to 11 significant bits where bf16 keeps 8, a factor 8, which leaves a factor 2 of
headroom.  The weight-rounding share alone, measured with the CPU oracle (max logit error / logit scale against fp32), is
7.4e-4 at 24 x 1280 (bf16: 6.1e-3) and 3.2e-4 on the tiny twin (bf16: 2.3e-3).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MATS = ("c_attn.weight", "c_proj.weight", "c_fc.weight", "mel_head.weight")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rounded(W, to):
    return {k: (v.to(to).to(torch.float32) if k.endswith(MATS) else v) for k, v in W.items()}


@pytest.fixture(scope="module")
def tiny(golden):
    """The tiny twin of tests/golden/gpt_tiny.npz: its weights, the fp32 oracle and the oracle on fp16-rounded matrices."""
    import voice_tts_amd.weights as WR
    from oracle import gpt as OG

    g = golden("gpt_tiny.npz")
    cfg = WR.tiny_gpt_cfg(model_dim=int(g["model_dim"]), layers=int(g["layers"]), heads=int(g["heads"]))
    W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=50.0)
    orc = OG.GptOracle(W, cfg["layers"], cfg["heads"])
    orc16 = OG.GptOracle(_rounded(W, torch.float16), cfg["layers"], cfg["heads"])
    return g, cfg, W, orc, orc16


def test_f16_engine_against_the_f16_rounded_oracle(tiny, dev):
    """Same checker as the bf16 twin test (oracle on the SAME rounded matrices, K/V unrounded in the checker): prefill logits
    within 2.5e-3 of max|logit| (bf16: 1e-2), free-running greedy tokens equal up to the first oracle near-tie (top-2 margin
    below 5e-3 of the logit scale), the first 4 at least."""
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    g, cfg, W, orc, orc16 = tiny
    embeds, mask = torch.from_numpy(g["embeds_plain"]), torch.from_numpy(g["mask_plain"])
    ids, margins, logits = OG.generate_greedy(orc16, embeds, mask, 24, return_logits=True)
    eng = GptEngine(cfg, dtype="f16", max_seq=256, max_batch=1, device=dev).load_state_dict(W)
    assert eng.dtype == "f16"
    eng.prefill(0, embeds, 0)
    got0 = eng.read_logits(0)
    ref0 = logits[0].numpy()
    rel = np.abs(got0 - ref0).max() / np.abs(ref0).max()
    print(f"f16 tiny twin: prefill logits rel err {rel:.2e}")
    assert rel <= 2.5e-3, rel
    eng.decode(1, 24, repetition_penalty=10.0)
    out = eng.read(0)[0].tolist()
    scale = float(logits.abs().max())
    upto = next((k for k, m in enumerate(margins) if m < 5e-3 * scale), len(ids))
    print(f"f16 tiny twin: tokens compared up to step {upto} of {len(ids)}, equal over all: {out == ids}")
    assert out[:upto] == ids[:upto], (upto, out, ids)
    assert out[:4] == ids[:4]


def test_f16_register_engines_of_1_to_4_slots_do_not_depend_on_company(tiny, dev):
    """B is a template parameter of the register GEMVs: on engines of 1, 2, 3 and 4 slots every slot's tokens and final
    logits are, bit for bit, what the same prompt gives alone on the 1-slot engine.  One slot carries the padded prompt."""
    from voice_tts_amd.gpt_engine import GptEngine

    g, cfg, W, orc, orc16 = tiny
    gen = torch.Generator().manual_seed(41)
    prompts = [(torch.from_numpy(g["embeds_plain"]), 0), (torch.from_numpy(g["embeds_padded"]), 3),
               (torch.randn(23, cfg["model_dim"], generator=gen) * 0.5, 0), (torch.randn(11, cfg["model_dim"], generator=gen) * 0.5, 0)]
    n = 40
    one = GptEngine(cfg, dtype="f16", max_seq=256, max_batch=1, device=dev).load_state_dict(W)
    alone = []
    for e, pad in prompts:
        one.prefill(0, e, pad)
        one.decode(1, n, repetition_penalty=10.0, suppress_stop=True)
        alone.append((one.read(0)[0][:n].tolist(), one.read_logits(0).copy()))
    assert len({tuple(a[0]) for a in alone}) == 4  # four different sequences
    for B in (2, 3, 4):
        eng = GptEngine(cfg, dtype="f16", max_seq=256, max_batch=B, device=dev).load_state_dict(W)
        for b in range(B):
            eng.prefill(b, *prompts[b])
        eng.decode(B, n, repetition_penalty=10.0, suppress_stop=True)
        for b in range(B):
            assert eng.read(b)[0][:n].tolist() == alone[b][0], (B, b)
            assert np.array_equal(eng.read_logits(b), alone[b][1]), (B, b)


def test_f16_split_attention_across_context_buckets(tiny, dev, monkeypatch):
    """The 200-row and 150-row prompts of test_split_attention_across_context_buckets through 700 steps on the fp16 cache:
    the split-S instantiations (one per 256-key bucket) and the any-length kernel (IXTTS_ATTN=legacy) give the same tokens."""
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    g = tiny[0]
    cfg = WR.tiny_gpt_cfg(model_dim=int(g["model_dim"]), layers=int(g["layers"]), heads=int(g["heads"]), max_mel_tokens=800)
    W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=50.0)
    emb = torch.randn(200, cfg["model_dim"], generator=torch.Generator().manual_seed(77)) * 0.5
    n = 700

    def run(legacy):
        if legacy:
            monkeypatch.setenv("IXTTS_ATTN", "legacy")
        else:
            monkeypatch.delenv("IXTTS_ATTN", raising=False)
        eng = GptEngine(cfg, dtype="f16", max_seq=1024, max_batch=2, device=dev).load_state_dict(W)
        eng.prefill(0, emb, 0)
        eng.prefill(1, emb[:150], 0)
        eng.decode(2, n, repetition_penalty=10.0, suppress_stop=True)
        return eng.read(0)[0][:n].tolist(), eng.read(1)[0][:n].tolist()

    a0, a1 = run(False)
    b0, b1 = run(True)
    assert len(a0) == n and len(a1) == n
    assert a0 == b0 and a1 == b1


def test_f16_rows_flash_attention_on_a_long_left_padded_prompt(tiny, dev):
    """Prefill of a 205-row prompt with 5 left-padding rows (two 128-row workgroups of the causal flash kernel, fp16 rows and
    cache): last-row logits against the fp32 oracle's masked prefill within 1.25e-2 max(1, max|ref|) (bf16: 5e-2)."""
    from voice_tts_amd.gpt_engine import GptEngine

    g, cfg, W, orc, orc16 = tiny
    gen = torch.Generator().manual_seed(5)
    prompt = torch.cat([torch.zeros(5, cfg["model_dim"]), torch.randn(200, cfg["model_dim"], generator=gen) * 0.5])
    mask = torch.cat([torch.zeros(5, dtype=torch.long), torch.ones(201, dtype=torch.long)])
    ref = orc.prefill(prompt, mask, 8192)[0].numpy()
    eng = GptEngine(cfg, dtype="f16", max_seq=512, max_batch=1, device=dev).load_state_dict(W)
    eng.prefill(0, prompt, 5)
    got = eng.read_logits(0)
    err = np.abs(got - ref).max()
    print(f"f16 flash prefill: max|err| {err:.3e}, max|ref| {np.abs(ref).max():.3f}")
    assert np.isfinite(got).all()
    assert err <= 1.25e-2 * max(1.0, np.abs(ref).max()), err


def test_f16_latent_pass_with_a_ragged_second_tile(tiny, dev):
    """Latent pass over T = 130 code rows (one full 128-row tile of the rows GEMM plus a ragged one) against `latent_pass` of
    the oracle on the fp16-rounded matrices.  The tests hold no bf16 latent bound to divide by 4, so the bf16 engine runs here
    too, against the oracle on ITS rounded matrices: the fp16 error must be no larger than bf16's, by either yardstick (own
    rounded oracle, fp32 oracle)."""
    import voice_tts_amd.weights as WR
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    g = tiny[0]
    cfg = WR.tiny_gpt_cfg(model_dim=int(g["model_dim"]), layers=int(g["layers"]), heads=int(g["heads"]), max_mel_tokens=160)
    W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=50.0)
    conds = torch.from_numpy(g["conds_latent"])
    text = torch.from_numpy(g["text_plain"]).long()
    codes = torch.randint(0, 8192, (130,), generator=torch.Generator().manual_seed(13))
    t = torch.cat((torch.tensor([0]), text, torch.tensor([1])))
    prefix = torch.cat((conds, W["text_embedding.weight"][t] + W["text_pos_embedding.emb.weight"][: t.numel()]), 0)
    ref32 = OG.GptOracle(W, cfg["layers"], cfg["heads"]).latent_pass(conds, text, codes)
    err = {}
    for dtype, to in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        ref = OG.GptOracle(_rounded(W, to), cfg["layers"], cfg["heads"]).latent_pass(conds, text, codes)
        eng = GptEngine(cfg, dtype=dtype, max_seq=256, max_batch=1, device=dev).load_state_dict(W)
        lat = eng.latent(prefix, codes).cpu()
        assert lat.shape == ref.shape == (130, cfg["model_dim"]) and bool(torch.isfinite(lat).all())
        err[dtype] = ((lat - ref).abs().max().item(), (lat - ref32).abs().max().item())
    print(f"latent T=130, max|ref| {ref32.abs().max().item():.3f}: f16 max|err| {err['f16'][0]:.3e} (own oracle) {err['f16'][1]:.3e} (fp32 oracle); "
          f"bf16 {err['bf16'][0]:.3e} / {err['bf16'][1]:.3e}")
    assert err["f16"][0] <= err["bf16"][0] and err["f16"][1] <= err["bf16"][1], err


def _prompts(n, D, seed=31):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        rows, pad = 9 + 5 * i, (i % 3)
        e = torch.randn(rows, D, generator=g) * 0.5
        e[:pad] = 0
        out.append((e, pad))
    return out


def _tiny7():
    import voice_tts_amd.weights as WR

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    return cfg, WR.make_gpt_weights(cfg, seed=7, head_scale=50.0)


def test_f16_wide_tokens_and_logits_do_not_depend_on_company(dev):
    """test_wide_tokens_and_logits_do_not_depend_on_company on v_mfma_f32_16x16x32_f16: engines of 8 and of 16 slots, 40 steps,
    every sequence bit for bit what it is alone."""
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny7()
    P = _prompts(8, 128)
    eng = GptEngine(cfg, dtype="f16", max_seq=160, max_batch=8, device=dev).load_state_dict(W)
    n = 40
    alone = []
    for e, pad in P:
        eng.prefill(0, e, pad)
        first = eng.read_logits(0).copy()
        eng.decode(1, n, repetition_penalty=10.0, suppress_stop=True)
        alone.append((first, eng.read(0)[0][:n].tolist(), eng.read_logits(0).copy()))
    for B in (8, 5):
        for b in range(B):
            eng.prefill(b, *P[b])
        firsts = [eng.read_logits(b).copy() for b in range(B)]
        eng.decode(B, n, repetition_penalty=10.0, suppress_stop=True)
        for b in range(B):
            assert np.array_equal(firsts[b], alone[b][0]), (B, b)
            assert eng.read(b)[0][:n].tolist() == alone[b][1], (B, b)
            assert np.array_equal(eng.read_logits(b), alone[b][2]), (B, b)
    big = GptEngine(cfg, dtype="f16", max_seq=160, max_batch=16, device=dev).load_state_dict(W)
    for b in range(16):
        big.prefill(b, *P[b % 8])
    big.decode(16, n, repetition_penalty=10.0, suppress_stop=True)
    for b in range(16):
        assert big.read(b)[0][:n].tolist() == alone[b % 8][1], b
        assert np.array_equal(big.read_logits(b), alone[b % 8][2]), b


@pytest.mark.parametrize("slots", [8, 16])
def test_f16_wide_agrees_with_the_register_gemvs(dev, slots):
    """Same fp16 weights through a 3-slot register engine and a wide engine: prefill logits within 1e-5 of the scale (the head
    GEMV's hi + lo split of the fp32 activations must be fp32-faithful: dropping the lo parts, or losing the small ones to
    fp16's exponent range, costs ~2.5e-4), tokens equal, final logits within 1e-3 of the scale after 32 steps (the ff
    activations travel as fp16 in the wide engine; bf16: 4e-3)."""
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny7()
    P = _prompts(3, 128, seed=5)
    narrow = GptEngine(cfg, dtype="f16", max_seq=160, max_batch=3, device=dev).load_state_dict(W)
    wide = GptEngine(cfg, dtype="f16", max_seq=160, max_batch=slots, device=dev).load_state_dict(W)
    n = 32
    outs = []
    for eng in (narrow, wide):
        for b, (e, pad) in enumerate(P):
            eng.prefill(b, e, pad)
        l0 = [eng.read_logits(b).copy() for b in range(3)]
        eng.decode(3, n, repetition_penalty=10.0, suppress_stop=True)
        outs.append((l0, [eng.read(b)[0][:n].tolist() for b in range(3)], [eng.read_logits(b).copy() for b in range(3)]))
    scale = max(float(np.abs(x).max()) for x in outs[0][0])
    for b in range(3):
        e0 = np.abs(outs[0][0][b] - outs[1][0][b]).max() / scale
        e1 = np.abs(outs[0][2][b] - outs[1][2][b]).max() / scale
        print(f"f16 wide({slots}) vs register, slot {b}: prefill logits {e0:.2e}, final logits {e1:.2e} of the scale {scale:.2f}")
        assert e0 <= 1e-5, (b, e0)
        assert outs[0][1][b] == outs[1][1][b], b
        assert e1 <= 1e-3, (b, e1)


def test_f16_beam_sample_kv_reorder_full_and_shared_prefix_agree(tiny, dev, monkeypatch):
    """3-beam beam-sample on the fp16 register engine: the K/V reorder (gpt_beam.hip) moves bytes, `esize` per element.  The
    same seed on an engine that moves every row (IXTTS_BEAM_REORDER=full) and on the default (shared leading rows stay) gives
    identical ids and an identical score, and the beams did swap ancestors."""
    from voice_tts_amd.gpt_engine import GptEngine

    g, cfg, W, orc, orc16 = tiny
    embeds = torch.from_numpy(g["embeds_plain"])
    monkeypatch.setenv("IXTTS_BEAM_REORDER", "full")
    full = GptEngine(cfg, dtype="f16", max_seq=128, max_batch=3, device=dev).load_state_dict(W)
    monkeypatch.delenv("IXTTS_BEAM_REORDER")
    eng = GptEngine(cfg, dtype="f16", max_seq=128, max_batch=3, device=dev).load_state_dict(W)
    patterns = set()
    for seed in (1, 2):
        res = []
        for e in (eng, full):
            e.prefill(0, embeds, 0)
            e.beam_begin(3)
            for _ in range(5):  # (temperature 3: flat enough that the beams keep swapping ancestors)
                e.beam_decode(8, repetition_penalty=10.0, temperature=3.0, top_k=30, top_p=0.95, suppress_stop=True, seed=seed)
                ids, done, score, bs, lt, src = e.beam_read(64)
                if e is eng:
                    patterns.add(tuple(src.tolist()))
            res.append((ids.tolist(), score))
        assert len(res[0][0]) > 0
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1], (seed, res)
    assert len(patterns) >= 2, patterns


# ---------------------------------------------------------------------------------------------------------------------------------
# Production width, 24 x 1280: the `gpt_full` recipe of tests/test_gpu_fullsize.py (seed 1234, P = 57, 24 greedy steps).
@pytest.fixture(scope="module")
def gpt_full():
    import voice_tts_amd.weights as WR
    from oracle import gpt as OG

    W = WR.make_gpt_weights(WR.GPT_CFG, seed=1234)
    orc = OG.GptOracle(W, WR.GPT_CFG["layers"], WR.GPT_CFG["heads"])
    g = torch.Generator().manual_seed(2)
    conds = torch.randn(34, 1280, generator=g) * 0.5
    text = torch.randint(2, 12000, (20,), generator=g)  # config 1: 20-token text -> P = 57
    fake, embeds, mask = orc.prepare_gpt_inputs(conds, text)
    n = 24
    ids, margins, logits = OG.generate_greedy(orc, embeds, mask, n, return_logits=True, suppress_stop=True)
    return W, embeds, ids, margins, logits


@pytest.fixture(scope="module")
def full_f16_engine(gpt_full, dev):
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    return GptEngine(WR.GPT_CFG, dtype="f16", max_seq=256, max_batch=1, device=dev).load_state_dict(gpt_full[0])


def test_f16_production_width_vs_fp32_oracle_and_bf16(gpt_full, full_f16_engine, dev):
    """B = 1 at 24 x 1280 against the fp32 oracle: first logits within 3.75e-3 of the scale (bf16 is held to 1.5e-2 at this
    width) and strictly closer than the bf16 engine's in the same run; free-running greedy tokens are the oracle's at every
    step whose oracle margin exceeds 7.5e-3 of the scale (the histories are the same up to the first differing token, which
    therefore has to sit at a near-tie; beyond it the two runs are not comparable step by step)."""
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    W, embeds, ids, margins, logits = gpt_full
    ref0 = logits[0].numpy()
    scale = float(logits.abs().max())
    rel = {}
    outs = {}
    for dtype in ("f16", "bf16"):
        eng = full_f16_engine if dtype == "f16" else GptEngine(WR.GPT_CFG, dtype="bf16", max_seq=256, max_batch=1, device=dev).load_state_dict(W)
        eng.prefill(0, embeds, 0)
        rel[dtype] = float(np.abs(eng.read_logits(0) - ref0).max()) / scale
        eng.decode(1, len(ids), repetition_penalty=10.0, suppress_stop=True)
        outs[dtype] = eng.read(0)[0].tolist()
    agree = {k: int(np.sum(np.array(v) == np.array(ids))) for k, v in outs.items()}
    print(f"24 x 1280 first-logit err / scale: f16 {rel['f16']:.2e}, bf16 {rel['bf16']:.2e}; tokens equal to the fp32 oracle's: "
          f"f16 {agree['f16']}/{len(ids)}, bf16 {agree['bf16']}/{len(ids)}")
    assert rel["f16"] <= 3.75e-3, rel
    assert rel["f16"] < rel["bf16"], rel
    out = outs["f16"]
    first = next((k for k in range(len(ids)) if out[k] != ids[k]), len(ids))
    assert all(out[k] == ids[k] for k in range(first))
    assert first == len(ids) or margins[first] <= 7.5e-3 * scale, (first, margins[first], scale, out, ids)


def test_f16_wide_engine_of_6_slots_at_production_width(gpt_full, full_f16_engine, dev):
    """The D = 1280 row splits of the wide kernels (15 / 5 / 16 + 4 / 5 / 16 + 16 rows per workgroup): six prompts of different
    lengths on a 6-slot fp16 wide engine (reading the register engine's arena) against each prompt alone on the register
    engine -- tokens equal, first and final logits within 1e-3 of the scale."""
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    W, embeds, ids, margins, logits = gpt_full
    reg = full_f16_engine
    n = 24
    prompts = [embeds[: embeds.shape[0] - 3 * b] for b in range(6)]
    alone = []
    for e in prompts:
        reg.prefill(0, e, 0)
        first = reg.read_logits(0).copy()
        reg.decode(1, n, repetition_penalty=10.0, suppress_stop=True)
        alone.append((first, reg.read(0)[0][:n].tolist(), reg.read_logits(0).copy()))
    wide = GptEngine(WR.GPT_CFG, dtype="f16", max_seq=256, max_batch=6, device=dev).share_arena(reg)
    for b, e in enumerate(prompts):
        wide.prefill(b, e, 0)
    firsts = [wide.read_logits(b).copy() for b in range(6)]
    wide.decode(6, n, repetition_penalty=10.0, suppress_stop=True)
    scale = max(float(np.abs(a[0]).max()) for a in alone)
    for b in range(6):
        e0 = np.abs(firsts[b] - alone[b][0]).max() / scale
        e1 = np.abs(wide.read_logits(b) - alone[b][2]).max() / scale
        print(f"f16 wide(6) vs register at 24 x 1280, slot {b}: first logits {e0:.2e}, final logits {e1:.2e} of the scale {scale:.2f}")
        assert wide.read(b)[0][:n].tolist() == alone[b][1], b
        assert e0 <= 1e-3 and e1 <= 1e-3, (b, e0, e1)


def test_f16_errors(tiny, dev):
    """An unknown type is a ValueError that lists the accepted names; a folded weight beyond fp16's range is refused at finalize
    (never stored as inf); engines of different weight types do not share an arena.  None of it faults the device: the last
    engine still decodes."""
    from voice_tts_amd._lib import IxttsError
    from voice_tts_amd.gpt_engine import GptEngine

    g, cfg, W, orc, orc16 = tiny
    with pytest.raises(ValueError) as ei:
        GptEngine(cfg, dtype="f8", max_seq=64, max_batch=1, device=dev)
    assert all(name in str(ei.value) for name in ("f32", "bf16", "f16"))
    big = dict(W)
    big["gpt.h.0.mlp.c_fc.weight"] = W["gpt.h.0.mlp.c_fc.weight"].clone()
    big["gpt.h.0.mlp.c_fc.weight"][3, 5] = 1e6
    e1 = GptEngine(cfg, dtype="f16", max_seq=64, max_batch=1, device=dev)
    with pytest.raises(IxttsError) as ei:
        e1.load_state_dict(big)
    assert "fp16 overflow" in str(ei.value)
    with pytest.raises(IxttsError):
        e1.decode(1, 1)  # not finalized
    GptEngine(cfg, dtype="bf16", max_seq=64, max_batch=1, device=dev).load_state_dict(big)  # the same weights are fine in bf16
    owner = GptEngine(cfg, dtype="bf16", max_seq=64, max_batch=1, device=dev).load_state_dict(W)
    e2 = GptEngine(cfg, dtype="f16", max_seq=64, max_batch=2, device=dev)
    with pytest.raises(IxttsError):
        e2.share_arena(owner)
    e3 = GptEngine(cfg, dtype="f16", max_seq=64, max_batch=1, device=dev).load_state_dict(W)
    e4 = GptEngine(cfg, dtype="f16", max_seq=64, max_batch=2, device=dev).share_arena(e3)  # same type: accepted
    e4.prefill(0, torch.from_numpy(g["embeds_plain"]), 0)
    e4.decode(1, 4, repetition_penalty=10.0)
    assert len(e4.read(0)[0]) == 4
    torch.cuda.synchronize()


def test_f16_arena_travels_as_bytes_and_is_adopted(dev):
    """Load-time weight distribution with an fp16 GPT: the packed arena is a uint8 tensor over the raw device pointer, goes
    through `dist.broadcast` on a one-rank group unchanged, is copied into a second handle (the receiving rank's side) and
    adopted there: same greedy tokens as the engine that loaded the state dict."""
    import socket

    import torch.distributed as dist

    import voice_tts_amd.weights as WR
    from voice_tts_amd.pipeline import HotPath

    gcfg, bcfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2), WR.tiny_bigvgan_cfg(64)
    Wg, Wb = WR.make_gpt_weights(gcfg, seed=7), WR.make_bigvgan_weights(bcfg, seed=8)
    a = HotPath(gcfg, bcfg, dtype="f16", device=dev, max_batch=1, max_seq=96, max_frames=16).load(Wg, Wb)
    b = HotPath(gcfg, bcfg, dtype="f16", device=dev, max_batch=1, max_seq=96, max_frames=16)
    bf = HotPath(gcfg, bcfg, dtype="bf16", device=dev, max_batch=1, max_seq=96, max_frames=16)
    src, dst = a.broadcast_tensors(), b.broadcast_tensors()
    assert src[0].dtype == torch.uint8 and src[0].numel() == bf.broadcast_tensors()[0].numel()  # same bytes as a bf16 arena
    before = [t.clone() for t in src]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        for t in src:
            dist.broadcast(t, src=0)
        dist.barrier()
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    assert all(torch.equal(x, y) for x, y in zip(before, a.broadcast_tensors()))
    for x, y in zip(src, dst):
        y.copy_(x)
    b.adopt()
    assert b.gpt.dtype == "f16"
    emb = torch.randn(20, 128, generator=torch.Generator().manual_seed(1))
    assert a.generate([(emb, 0)], 12)[0].tolist() == b.generate([(emb, 0)], 12)[0].tolist()
