"""bf16 / fp16 engines of 17..32 slots (csrc/gpt_wide.h, NB == 2: two blocks of 16 columns served from one weight stream).  The
arithmetic of a column is the one-block kernel's, so every comparison here is bit for bit (`==` on ids, `array_equal` on logits)
against the 16-slot engine, whose kernels are the ones it always had: limits, company and slot independence, partial blocks,
per-slot sampler state above slot 15, beam groups, the decode scheduler, and the production width."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
N_STEPS = 40
GREEDY = dict(repetition_penalty=10.0, suppress_stop=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tiny(seed=7):
    import voice_tts_amd.weights as WR

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    return cfg, WR.make_gpt_weights(cfg, seed=seed, head_scale=50.0)


def _prompts(n, D, seed=31, rows0=9, step=3):
    """n distinct prompts of unequal length, every third and every third-plus-one left-padded."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        rows, pad = rows0 + step * i, (i % 3)
        e = torch.randn(rows, D, generator=g) * 0.5
        e[:pad] = 0
        out.append((e, pad))
    return out


@pytest.fixture(scope="module", params=DTYPES)
def twin(request, dev):
    """Per weight type: the 16-slot and the 32-slot engine over one set of device weights, 32 prompts, and every prompt decoded
    alone in slot 0 of the 16-slot engine (first-step logits, 40 greedy ids, the logits after them): computed once, never changed."""
    from voice_tts_amd.gpt_engine import GptEngine

    dt = request.param
    cfg, W = _tiny()
    e16 = GptEngine(cfg, dtype=dt, max_seq=192, max_batch=16, device=dev).load_state_dict(W)
    e32 = GptEngine(cfg, dtype=dt, max_seq=192, max_batch=32, device=dev).share_arena(e16)
    P = _prompts(32, 128)
    solo = []
    for e, pad in P:
        e16.prefill(0, e, pad)
        first = e16.read_logits(0).copy()
        e16.decode(1, N_STEPS, **GREEDY)
        solo.append((first, e16.read(0)[0][:N_STEPS].tolist(), e16.read_logits(0).copy()))
    assert len({tuple(s[1]) for s in solo}) == 32
    return dt, cfg, W, e16, e32, P, solo


# ------------------------------------------------------------------------------------------------------------------ 1. limits
@pytest.mark.parametrize("dt", DTYPES)
def test_limits_of_the_16_bit_engines(dev, dt):
    from voice_tts_amd import _lib
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny()
    for mb in (17, 24, 32):
        eng = GptEngine(cfg, dtype=dt, max_seq=96, max_batch=mb, device=dev)
        assert eng.max_batch == mb
    with pytest.raises(_lib.IxttsError, match="1..32"):
        GptEngine(cfg, dtype=dt, max_seq=96, max_batch=33, device=dev)
    eng = GptEngine(cfg, dtype=dt, max_seq=96, max_batch=32, device=dev).load_state_dict(W)
    D, L, V, S = 128, 2, cfg["number_mel_codes"], 64
    mats = L * 12 * D * D + V * D                      # QKV + out-proj + FC + MLP-out per layer, head: read ONCE for all 32
    vecs = L * 13 * D + 4 * D + V                      # biases and LayerNorm vectors (always fp32)
    want = mats * 2 + vecs * 4 + 32 * 2 * L * (S + 1) * D * 2 + 32 * 2 * D * 4
    assert eng.step_bytes(32, S) == want, (eng.step_bytes(32, S), want)
    assert _lib.max_batch() == 16
    assert [_lib.max_batch_for(t) for t in ("bf16", "f16", "f32")] == [32, 32, 16]


# ------------------------------------------------------------------------------------------- 2. company and slot independence
def test_32_sequences_each_as_alone_on_the_16_slot_engine(twin):
    dt, cfg, W, e16, e32, P, solo = twin
    for b in range(32):
        e32.prefill(b, *P[b])
    firsts = [e32.read_logits(b).copy() for b in range(32)]
    e32.decode(32, N_STEPS, **GREEDY)
    for b in range(32):
        assert np.array_equal(firsts[b], solo[b][0]), b
        assert e32.read(b)[0][:N_STEPS].tolist() == solo[b][1], b
        assert np.array_equal(e32.read_logits(b), solo[b][2]), b
    # one prompt in a column of block 0 and in a column of block 1, among the others
    for b in range(32):
        e32.prefill(b, *P[5 if b in (3, 19) else b])
    e32.decode(32, N_STEPS, **GREEDY)
    assert e32.read(3)[0][:N_STEPS].tolist() == e32.read(19)[0][:N_STEPS].tolist() == solo[5][1]
    assert np.array_equal(e32.read_logits(3), e32.read_logits(19)) and np.array_equal(e32.read_logits(3), solo[5][2])


# ------------------------------------------------------------------------------------------------------------ 3. partial blocks
@pytest.mark.parametrize("n_active", [1, 5, 16, 17, 31, 32])
def test_partial_blocks(twin, n_active):
    """17 and 31 run block 1 with repeated columns (which store nothing); 1, 5 and 16 take the one-block kernels."""
    dt, cfg, W, e16, e32, P, solo = twin
    for b in range(n_active):
        e32.prefill(b, *P[31 - b])
    firsts = [e32.read_logits(b).copy() for b in range(n_active)]
    e32.decode(n_active, N_STEPS, **GREEDY)
    for b in range(n_active):
        assert np.array_equal(firsts[b], solo[31 - b][0]), b
        assert e32.read(b)[0][:N_STEPS].tolist() == solo[31 - b][1], b
        assert np.array_equal(e32.read_logits(b), solo[31 - b][2]), b


# ------------------------------------------------------------------------------------------- 4. per-slot state above slot 15
def test_per_slot_cfg_and_stream_above_slot_15(twin):
    dt, cfg, W, e16, e32, P, solo = twin
    kinds = [dict(repetition_penalty=10.0),
             dict(repetition_penalty=10.0, do_sample=True, temperature=0.8, top_k=30, top_p=0.8, seed=11),
             dict(repetition_penalty=10.0, do_sample=True, temperature=1.2, seed=5)]
    cfgs = [dict(kinds[b % 3], suppress_stop=True) for b in range(32)]
    streams = [100 + 7 * b for b in range(32)]
    n = 24
    for b in range(32):
        e32.prefill(b, *P[b])
    e32.decode_slots(n, cfgs, streams)
    got = [e32.read(b)[0][:n].tolist() for b in range(32)]
    for j in range(16):  # the same segment, cfg and stream in slot j of the 16-slot engine
        e16.prefill(j, *P[16 + j])
    e16.decode_slots(n, cfgs[16:], streams[16:])
    for j in range(16):
        assert got[16 + j] == e16.read(j)[0][:n].tolist(), 16 + j
    assert len({tuple(g) for g in got[16:]}) == 16


def test_bans_and_processors_on_slot_25(twin):
    dt, cfg, W, e16, e32, P, solo = twin
    t0 = solo[25][1][0]  # what slot 25 would say first

    def run(table):
        for b in range(32):
            e32.prefill(b, *P[b])
        e32.set_bans(25, [t0])
        if table:
            e32.set_processors(25, dict(table=table, forced_eos=()))
        e32.decode(32, N_STEPS, **GREEDY)
        return [e32.read(b)[0][:N_STEPS].tolist() for b in (24, 25, 26)]

    left, mid, right = run(None)
    assert t0 not in mid and mid != solo[25][1]
    assert left == solo[24][1] and right == solo[26][1]  # the neighbours know nothing of it
    first, y = mid[0], (mid[1] + 1000) % 8000            # the ban's first token, and an id that did not follow it
    assert y not in (t0, first)
    left, mid2, right = run([((first, y), 3e4)])          # ... now follows it: the bias of the pair lands on y after `first`
    assert mid2[0] == first and mid2[1] == y and t0 not in mid2
    assert left == solo[24][1] and right == solo[26][1]


# ------------------------------------------------------------------------------------------------------------- 5. beam groups
@pytest.fixture(scope="module")
def beam_twin(dev):
    import voice_tts_amd.weights as WR

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    W = WR.make_gpt_weights(cfg, seed=5, head_scale=50.0)
    W["mel_head.bias"] = W["mel_head.bias"].clone()
    W["mel_head.bias"][8193] += 24.0  # eos reachable: some groups collect hypotheses and finish early
    g = torch.Generator().manual_seed(77)
    segs = []
    for i in range(18):
        rows, pad, n = 9 + (7 * i) % 31, i % 4, 8 + (11 * i) % 37
        e = torch.randn(rows, 128, generator=g) * 0.5
        e[:pad] = 0
        segs.append((e.to(dev), pad, n))
    return cfg, W, segs


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nb,groups,n_segs", [(3, 10, 13), (4, 8, 10), (2, 16, 18)])
def test_beam_groups_on_32_slots_equal_one_group_at_a_time(beam_twin, dev, dt, nb, groups, n_segs):
    """tests/test_gpu_beam_groups.py::test_scheduler_refills_and_parks_groups_same_tokens on 32 slots: ids AND scores."""
    from voice_tts_amd.gpt_engine import GptEngine
    from voice_tts_amd.scheduler import BeamGroupScheduler, Segment

    cfg, W, segs = beam_twin
    segs = segs[:n_segs]
    e16 = GptEngine(cfg, dtype=dt, max_seq=160, max_batch=16, device=dev).load_state_dict(W)
    e32 = GptEngine(cfg, dtype=dt, max_seq=160, max_batch=32, device=dev).share_arena(e16)

    def run(eng, max_groups):
        out = [None] * len(segs)
        sch = BeamGroupScheduler(eng, nb, max_groups=max_groups, sync_every=8)
        st = sch.run([Segment(0, i, e, p, n) for i, (e, p, n) in enumerate(segs)],
                     lambda seg, ids, sc: out.__setitem__(seg.index, (np.asarray(ids).tolist(), float(sc))), seed=5)
        return out, sch.max_groups, st

    turn, one, _ = run(e16, 1)  # the 16-slot engine, segment after segment (the reference's order)
    stepped, real = [], e32.beam_decode
    e32.beam_decode = lambda steps, groups=1, **kw: (stepped.append(groups), real(steps, groups=groups, **kw))[1]
    together, got_groups, st = run(e32, None)
    assert one == 1 and got_groups == groups and max(stepped) == groups  # every group of the engine stepped in one launch
    assert st["refills"] == n_segs - groups > 0
    assert together == turn
    assert len({tuple(t[0]) for t in turn}) == n_segs and all(len(t[0]) <= n + 1 for t, (_, _, n) in zip(turn, segs))


# ---------------------------------------------------------------------------------------------------------------- 6. scheduler
def test_decode_scheduler_40_segments_on_32_slots(twin, dev):
    from voice_tts_amd.scheduler import DecodeScheduler, Segment

    dt, cfg, W, e16, e32, P, solo = twin
    g = torch.Generator().manual_seed(91)
    segs = []
    for i in range(40):
        rows, pad, n = 8 + (7 * i) % 31, i % 4, 6 + (11 * i) % 37
        e = torch.randn(rows, 128, generator=g) * 0.5
        e[:pad] = 0
        segs.append(Segment(0, i, e.to(dev), pad, n))
    stop = cfg["stop_mel_token"]
    for fixed in (True, False):
        alone = {}
        for s in segs:
            DecodeScheduler(e16, 1, stop, sync_every=8).run([s], lambda seg, ids: alone.__setitem__(seg.index, np.asarray(ids).tolist()), fixed_length=fixed,
                                                          repetition_penalty=10.0)
        got = {}
        sch = DecodeScheduler(e32, 32, stop, sync_every=8)
        st = sch.run(segs, lambda seg, ids: got.__setitem__(seg.index, np.asarray(ids).tolist()), fixed_length=fixed, repetition_penalty=10.0)
        assert st["refills"] > 0 and st["refills"] >= len(segs) - 32
        assert got == alone
        if fixed:
            assert all(len(got[s.index]) == s.max_new for s in segs)


# ---------------------------------------------------------------------------------------------------------- 7. production width
@pytest.mark.parametrize("dt", DTYPES)
def test_production_width_32_slots_equal_two_batches_of_16(dev, dt):
    """D = 1280, 20 heads: NI = 10 k-steps per wave, the MLP-out K = 5120 path, the production vocabulary -- the shapes at which
    the two-block kernels hold the most registers, which the tiny twin cannot see."""
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    cfg = WR.tiny_gpt_cfg(model_dim=1280, layers=2, heads=20)
    W = WR.make_gpt_weights(cfg, seed=1234)
    e16 = GptEngine(cfg, dtype=dt, max_seq=128, max_batch=16, device=dev).load_state_dict(W)
    e32 = GptEngine(cfg, dtype=dt, max_seq=128, max_batch=32, device=dev).share_arena(e16)
    P = _prompts(32, 1280, seed=100, rows0=12, step=2)
    n = 12
    want = []
    for half in (0, 16):
        for j in range(16):
            e16.prefill(j, *P[half + j])
        firsts = [e16.read_logits(j).copy() for j in range(16)]
        e16.decode(16, n, **GREEDY)
        want += [(firsts[j], e16.read(j)[0][:n].tolist(), e16.read_logits(j).copy()) for j in range(16)]
    for b in range(32):
        e32.prefill(b, *P[b])
    firsts = [e32.read_logits(b).copy() for b in range(32)]
    e32.decode(32, n, **GREEDY)
    for b in range(32):
        assert np.array_equal(firsts[b], want[b][0]), b
        assert e32.read(b)[0][:n].tolist() == want[b][1], b
        assert np.array_equal(e32.read_logits(b), want[b][2]), b
    assert len({tuple(w[1]) for w in want}) == 32
