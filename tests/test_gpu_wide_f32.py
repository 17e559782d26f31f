"""Wide engines in the parity mode (fp32 weights, max_batch 5..16): the decode GEMVs on the fp32 matrix cores
(gemv_wide_f32_kernel, csrc/gpt_wide.h).  Creation; a sequence's arithmetic independent of its company and slot, bit for bit;
the reference fixtures and the CPU oracle at the register engine's own fp32 bounds; beam groups stepping together; and the
product surface (`infer_many`, the served default of `infer`) routing an fp32 model to the wide engine."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NB = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tiny(seed=7):
    import voice_tts_amd.weights as WR

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    return cfg, WR.make_gpt_weights(cfg, seed=seed, head_scale=50.0)


def _prompts(n, D, seed=31):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        rows, pad = 9 + 5 * i, (i % 3)
        e = torch.randn(rows, D, generator=g) * 0.5
        e[:pad] = 0
        out.append((e, pad))
    return out


# ------------------------------------------------------------------------------------------------------------- 1. creation
def test_fp32_engines_of_8_and_16_slots_construct_and_load(dev):
    from voice_tts_amd._lib import IxttsError
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny()
    D, L, V, S = 128, 2, cfg["number_mel_codes"], 64
    mats = L * 12 * D * D + V * D                      # QKV + out-proj + FC + MLP-out per layer, head
    vecs = L * 13 * D + 4 * D + V                      # biases and LayerNorm vectors (always fp32)
    for mb in (8, 16):
        eng = GptEngine(cfg, dtype="f32", max_seq=96, max_batch=mb, device=dev).load_state_dict(W)
        assert eng.max_batch == mb
        # 4-byte weights and K/V (read S rows, append one), fp32 vectors and two embedding rows per sequence
        want = mats * 4 + vecs * 4 + mb * 2 * L * (S + 1) * D * 4 + mb * 2 * D * 4
        assert eng.step_bytes(mb, S) == want, (eng.step_bytes(mb, S), want)
    with pytest.raises(IxttsError):
        GptEngine(cfg, dtype="f32", max_seq=96, max_batch=17, device=dev)


# ------------------------------------------------------------------------------------------- 2. company independence, bit for bit
def test_fp32_wide_tokens_and_logits_do_not_depend_on_company(dev):
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny()
    P = _prompts(8, 128)
    eng = GptEngine(cfg, dtype="f32", max_seq=160, max_batch=8, device=dev).load_state_dict(W)
    n = 40
    alone = []
    for e, pad in P:
        eng.prefill(0, e, pad)
        first = eng.read_logits(0).copy()
        eng.decode(1, n, repetition_penalty=10.0, suppress_stop=True)
        alone.append((first, eng.read(0)[0][:n].tolist(), eng.read_logits(0).copy()))
    assert len({tuple(a[1]) for a in alone}) == 8
    for B in (8, 5):
        for b in range(B):
            eng.prefill(b, *P[b])
        firsts = [eng.read_logits(b).copy() for b in range(B)]
        eng.decode(B, n, repetition_penalty=10.0, suppress_stop=True)
        for b in range(B):
            assert np.array_equal(firsts[b], alone[b][0]), (B, b)
            assert eng.read(b)[0][:n].tolist() == alone[b][1], (B, b)
            assert np.array_equal(eng.read_logits(b), alone[b][2]), (B, b)
    for b in range(8):  # reversed slot order: the slot index is not part of the arithmetic
        eng.prefill(b, *P[7 - b])
    firsts = [eng.read_logits(b).copy() for b in range(8)]
    eng.decode(8, n, repetition_penalty=10.0, suppress_stop=True)
    for b in range(8):
        assert np.array_equal(firsts[b], alone[7 - b][0]), b
        assert eng.read(b)[0][:n].tolist() == alone[7 - b][1], b
        assert np.array_equal(eng.read_logits(b), alone[7 - b][2]), b
    big = GptEngine(cfg, dtype="f32", max_seq=160, max_batch=16, device=dev).load_state_dict(W)  # all 16 MFMA columns: each prompt twice
    for b in range(16):
        big.prefill(b, *P[b % 8])
    firsts = [big.read_logits(b).copy() for b in range(16)]
    big.decode(16, n, repetition_penalty=10.0, suppress_stop=True)
    for b in range(16):
        assert np.array_equal(firsts[b], alone[b % 8][0]), b
        assert big.read(b)[0][:n].tolist() == alone[b % 8][1], b
        assert np.array_equal(big.read_logits(b), alone[b % 8][2]), b


# -------------------------------------------------------------------------------------------- 3. twin vs the reference fixtures
@pytest.fixture(scope="module")
def tiny8(golden, dev):
    import voice_tts_amd.weights as WR
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_tiny.npz")
    cfg = WR.tiny_gpt_cfg(model_dim=int(g["model_dim"]), layers=int(g["layers"]), heads=int(g["heads"]))
    W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=50.0)
    eng = GptEngine(cfg, dtype="f32", max_seq=256, max_batch=8, device=dev).load_state_dict(W)
    return g, OG.GptOracle(W, cfg["layers"], cfg["heads"]), eng


SLOT = 3


def _fill_company(eng, D):
    for b, (e, pad) in enumerate(_prompts(8, D, seed=13)):
        if b != SLOT:
            eng.prefill(b, e, pad)


@pytest.mark.parametrize("tag", ["plain", "padded"])
def test_fp32_wide_greedy_ids_match_reference_in_slot_3_of_8(tiny8, tag):
    """test_tiny_greedy_ids_match_reference of test_gpu_gpt.py, same bounds, among 7 other sequences."""
    g, orc, eng = tiny8
    embeds = torch.from_numpy(g[f"embeds_{tag}"])
    n_pad = int((g[f"mask_{tag}"] == 0).sum())
    ref_ids, ref_l = g[f"ids_{tag}"], g[f"logits_{tag}"]
    n = len(ref_ids)
    _fill_company(eng, embeds.shape[1])
    eng.prefill(SLOT, embeds, n_pad)
    l0 = eng.read_logits(SLOT)
    print(f"{tag}: first logits rel err {np.abs(l0 - ref_l[0]).max() / np.abs(ref_l[0]).max():.2e}")
    assert np.abs(l0 - ref_l[0]).max() <= 2e-4 * np.abs(ref_l[0]).max()
    eng.decode(8, n, repetition_penalty=10.0)
    assert eng.read(SLOT)[0].tolist() == ref_ids.tolist()
    _fill_company(eng, embeds.shape[1])
    eng.prefill(SLOT, embeds, n_pad)
    eng.decode(8, 1, repetition_penalty=10.0)
    l1 = eng.read_logits(SLOT)
    assert np.abs(l1 - ref_l[1]).max() <= 2e-4 * np.abs(ref_l[1]).max()


def test_fp32_wide_teacher_forced_logits_vs_oracle_in_slot_3_of_8(tiny8):
    from oracle import gpt as OG

    g, orc, eng = tiny8
    embeds = torch.from_numpy(g["embeds_plain"])
    mask = torch.from_numpy(g["mask_plain"])
    forced = [7, 8193 - 5, 4000, 17, 17, 256, 8191, 3]
    ids, margins, logits = OG.generate_greedy(orc, embeds, mask, len(forced), return_logits=True, forced=forced)
    _fill_company(eng, embeds.shape[1])
    eng.prefill(SLOT, embeds, 0)
    worst = 0.0
    for k, tok in enumerate(forced):
        got = eng.read_logits(SLOT)
        ref = logits[k].numpy()
        worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
        assert np.abs(got - ref).max() <= 2e-4 * np.abs(ref).max(), k
        eng.force_next(SLOT, tok)
        eng.decode(8, 1, repetition_penalty=10.0)
    print(f"teacher-forced logits rel err {worst:.2e}")
    assert eng.read(SLOT)[0].tolist() == forced


# ------------------------------------------------------------------------------------------- 4. production width vs the oracle
def test_fp32_wide_production_width_two_layers_vs_oracle(dev):
    """D = 1280, 20 heads, K = 1280 and 5120, the production vocabulary (the head's row tail and every rows-per-workgroup shape
    live), 2 layers; 8 slots of unequal prompts, 64 free-running greedy steps; two slots against ONE causal oracle pass each at
    the fp32 bounds of test_bench_shape_fp32_1100_steps_vs_oracle."""
    import voice_tts_amd.weights as WR
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    cfg = dict(WR.GPT_CFG, layers=2)
    W = WR.make_gpt_weights(cfg, seed=1234)
    orc = OG.GptOracle(W, cfg["layers"], cfg["heads"])
    g = torch.Generator().manual_seed(100)
    prompts = []
    for i in range(8):
        rows, pad = 41 + 8 * i, {2: 3, 5: 1}.get(i, 0)
        e = torch.randn(rows, 1280, generator=g) * 0.5
        e[:pad] = 0
        mask = torch.ones(rows + 1, dtype=torch.long)
        mask[:pad] = 0
        prompts.append((e, mask, pad))
    N = 64
    eng = GptEngine(cfg, dtype="f32", max_seq=256, max_batch=8, device=dev).load_state_dict(W)
    for b, (e, mask, pad) in enumerate(prompts):
        eng.prefill(b, e, pad)
    checked = [2, 7]  # a padded prompt and the longest one
    got = {0: [eng.read_logits(b).copy() for b in checked]}
    done = 0
    for k in (1, 2, 32, N):
        eng.decode(8, k - done, repetition_penalty=10.0, suppress_stop=True)
        done = k
        got[k] = [eng.read_logits(b).copy() for b in checked]
    for j, b in enumerate(checked):
        ids = eng.read(b)[0][:N]
        assert len(ids) == N
        e, mask, pad = prompts[b]
        rows = OG.teacher_forced_logits(orc, e, mask, ids.tolist())
        picks, margins = OG.greedy_choices(rows, len(mask), ids.tolist(), theta=10.0, suppress_stop=True)
        scale = float(rows.abs().max())
        worst = max(np.abs(got[k][j] - rows[k].numpy()).max() for k in got) / scale
        close = [k for k in range(N) if margins[k] < 1e-4 * scale]
        differ = [k for k in range(N) if picks[k] != int(ids[k])]
        wrong = [k for k in differ if margins[k] >= 1e-4 * scale]
        print(f"fp32 wide slot {b}: logits rel err {worst:.2e} over {len(got)} read points, {len(close)} near-tie steps, "
              f"{len(differ)} differing tokens, {len(wrong)} of them outside near-ties")
        assert worst <= 3e-4, (b, worst)
        assert not wrong, (b, wrong[:5])
        assert len(differ) <= len(close)


# ---------------------------------------------------------------------------------------------------- 5. beam groups in fp32
def _snap(eng, max_new, group):
    ids, done, score, bs, lt, src = eng.beam_read(max_new, group=group)
    return ids.tolist(), done, score, bs.tolist(), lt.tolist(), src.tolist()


def test_fp32_groups_together_equal_groups_alone_free_running(dev):
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    W = WR.make_gpt_weights(cfg, seed=5, head_scale=50.0)
    W["mel_head.bias"] = W["mel_head.bias"].clone()
    W["mel_head.bias"][8193] += 24.0  # eos reachable: some groups collect hypotheses and finish early
    eng = GptEngine(cfg, dtype="f32", max_seq=160, max_batch=9, device=dev).load_state_dict(W)
    g = torch.Generator().manual_seed(77)
    prompts = []
    for rows, pad in ((20, 0), (33, 2), (9, 0)):
        e = torch.randn(rows, 128, generator=g) * 0.5
        e[:pad] = 0
        prompts.append((e.to(dev), pad))
    n, chunk = 48, 8
    alone = []
    for i in range(3):
        eng.prefill(0, *prompts[i])
        eng.beam_begin(NB, group=0, rng_stream=i)
        tr = []
        for _ in range(0, n, chunk):
            eng.beam_decode(chunk, groups=1, seed=11)
            tr.append(_snap(eng, n, 0))
        alone.append(tr)
    print("done flags per chunk:", [[int(c[1]) for c in a] for a in alone], "final lengths:", [len(a[-1][0]) for a in alone])
    assert len({tuple(a[-1][0]) for a in alone}) == 3
    for order in ([0, 1, 2], [2, 0, 1]):  # segment order[g] lands in group g
        for gi, i in enumerate(order):
            eng.prefill(gi * NB, *prompts[i])
            eng.beam_begin(NB, group=gi, rng_stream=i)
        for c in range(n // chunk):
            eng.beam_decode(chunk, groups=3, seed=11)
            for gi, i in enumerate(order):
                assert _snap(eng, n, gi) == alone[i][c], (order, gi, i, c)


BEAM_TAGS = ["noeos", "mid", "mid2", "eos", "eos2", "lp1", "lpneg", "lp2noeos"]


@pytest.mark.parametrize("tag", BEAM_TAGS)
def test_fp32_beam_sample_replays_reference_trace_in_group_1_of_3(golden, dev, tag):
    """test_beam_sample_replays_reference_trace of test_gpu_gpt.py (same bounds), in group 1 of a 9-slot fp32 engine while
    groups 0 and 2 draw freely on other prompts."""
    import voice_tts_amd.weights as WR
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_beam.npz")
    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=50.0)
    W["mel_head.bias"] = W["mel_head.bias"].clone()
    W["mel_head.bias"][8193] += float(g[f"{tag}_stop_bias"])
    orc = OG.GptOracle(W, cfg["layers"], cfg["heads"])
    eng = GptEngine(cfg, dtype="f32", max_seq=128, max_batch=9, device=dev).load_state_dict(W)
    fake, embeds, mask = orc.prepare_gpt_inputs(torch.from_numpy(g[f"{tag}_conds_latent"]), g[f"{tag}_text"])
    picks = g[f"{tag}_picks"]
    max_new = int(g[f"{tag}_max_new"])
    lp = float(g[f"{tag}_length_penalty"]) if f"{tag}_length_penalty" in g.files else 0.0
    others = _prompts(2, 128, seed=3)
    eng.prefill(0, *others[0])
    eng.prefill(NB, embeds, 0)
    eng.prefill(2 * NB, *others[1])
    for grp in range(3):
        eng.beam_begin(NB, group=grp, rng_stream=grp)
    kw = dict(repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, length_penalty=lp, groups=3, seed=11)
    for step in range(picks.shape[0]):
        eng.beam_force(picks[step], group=1)
        eng.beam_decode(1, **kw)
        ids, done, score, bs, lt, src = eng.beam_read(max_new, group=1)
        assert lt.tolist() == g[f"{tag}_next_tokens"][step].tolist(), step
        assert src.tolist() == g[f"{tag}_next_indices"][step].tolist(), step
        assert np.allclose(bs, g[f"{tag}_next_scores"][step], rtol=1e-4, atol=2e-3), step
    assert done == bool(g[f"{tag}_done"])
    assert ids.tolist() == g[f"{tag}_sequence"].tolist()
    assert abs(score - float(g[f"{tag}_sequence_score"][0])) <= 2e-3 * max(1.0, abs(score))
    if done:  # once done, further steps change nothing (HF leaves the loop)
        eng.beam_decode(3, **kw)
        ids2, done2 = eng.beam_read(max_new, group=1)[:2]
        assert done2 and ids2.tolist() == ids.tolist()


# -------------------------------------------------------------------------------------------------------- 6. product surface
@pytest.fixture(scope="module")
def tts_f32_from_dir(tmp_path_factory):
    """`IndexTTS2(cfg_path, model_dir)` from a synthetic model_dir with the reference's default precision (use_fp16=False)."""
    import synthetic_model_dir as SM
    from indextts.infer_v2 import IndexTTS2
    from voice_tts_amd.front import TextNormalizer, TextTokenizer

    root = str(tmp_path_factory.mktemp("model_dir_wide_f32"))
    cfg_path, cfg = SM.write_model_dir(root)

    class Same:
        def normalize(self, s):
            return s

    tok = TextTokenizer(root + "/bpe.model", TextNormalizer(Same(), Same()))
    m = IndexTTS2(cfg_path=cfg_path, model_dir=root, use_fp16=False, device="cuda:0", tokenizer=tok, max_seq=256, max_frames=256)
    return m, SM


def test_fp32_infer_many_takes_8_decode_slots(tts_f32_from_dir):
    m, SM = tts_f32_from_dir
    wav_a, wav_b = SM.synthetic_wav_bytes(1.5, 24000), SM.synthetic_wav_bytes(1.0, 16000, seed=1)
    reqs = [dict(spk_audio_prompt=wav_a, text="Hello world, this is a test. 你好世界！"),
            dict(spk_audio_prompt=wav_b, text="Short."),
            dict(spk_audio_prompt=wav_a, text="Vector.", emo_vector=[0.3, 0, 0, 0, 0, 0, 0.2, 0.1])]
    outs = m.infer_many(reqs, decode_slots=8, num_beams=1, top_k=1, max_mel_tokens=20)
    assert 8 in m._engines and m._engines[8].max_batch == 8 and m._engines[8].dtype == "f32"
    assert len(outs) == 3
    for rq, (sr, pcm) in zip(reqs, outs):
        assert sr == 22050 and pcm.dtype == np.int16 and pcm.ndim == 2 and pcm.shape[1] == 1
        kw = {k: rq[k] for k in ("emo_vector",) if k in rq}
        ref_sr, ref = m.infer(rq["spk_audio_prompt"], rq["text"], None, num_beams=1, top_k=1, max_mel_tokens=20, **kw)
        assert ref.shape == pcm.shape, (rq["text"], ref.shape, pcm.shape)


def test_fp32_served_default_decodes_the_segments_beam_groups_together(tts_f32_from_dir, monkeypatch):
    from voice_tts_amd import scheduler as SCH

    m, SM = tts_f32_from_dir
    wav = SM.synthetic_wav_bytes(1.5, 24000)
    text = "Hello world, this is a test. 你好世界！ One more sentence follows here. And a last one."
    runs = []
    real_run = SCH.BeamGroupScheduler.run

    def spy(self, segments, on_done, **kw):
        st = real_run(self, segments, on_done, **kw)
        runs.append((self.engine.max_batch, self.max_groups, len(segments), self.engine.dtype, dict(st)))
        return st

    monkeypatch.setattr(SCH.BeamGroupScheduler, "run", spy)
    monkeypatch.delenv("IXTTS_BEAM_GROUPS", raising=False)
    m.infer(wav, text, None, max_text_tokens_per_segment=20, max_mel_tokens=24, seed=4)
    assert not runs  # an fp32 model joins the groups only when the variable is set explicitly
    monkeypatch.setenv("IXTTS_BEAM_GROUPS", "5")
    sr, pcm = m.infer(wav, text, None, max_text_tokens_per_segment=20, max_mel_tokens=24, seed=4)
    assert sr == 22050 and pcm.dtype == np.int16 and pcm.shape[1] == 1 and pcm.shape[0] > 0
    assert len(runs) == 1 and runs[0][0] == 15 and runs[0][2] >= 3 and runs[0][3] == "f32", runs  # one run, wide fp32 engine, all segments
    assert runs[0][4]["busy_group_steps"] > runs[0][4]["decode_calls"] * 8, runs  # several groups per step
    monkeypatch.setenv("IXTTS_BEAM_GROUPS", "1")
    sr2, pcm2 = m.infer(wav, text, None, max_text_tokens_per_segment=20, max_mel_tokens=24, seed=4)
    assert len(runs) == 1 and sr2 == 22050 and pcm2.shape[0] > 0
