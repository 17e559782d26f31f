"""Sampler settings and random streams per SEQUENCE (`decode_slots`, `beam_decode_groups`): a slot's tokens under its own
cfg and stream are, bit for bit, the ones the uniform call (`decode`, `beam_decode`: one cfg for all, stream = slot index)
gives it; the stream, not the slot, selects the draws; the processed probabilities match the oracle per slot; a cfg may change
between calls and a refilled slot keeps nothing of its previous occupant; beam groups carry their own cfg and length penalty.

Register engines pick their GEMV kernels by the number of active slots, so every comparison on one keeps that number equal on
both sides; wide engines run the same kernels whatever it is (tests/test_gpu_wide.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GREEDY = dict(repetition_penalty=10.0)
S_SERVED = dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.8, seed=11)
S_SHARP = dict(do_sample=True, temperature=1.3, top_k=5, top_p=0.5, seed=12)
S_OPEN = dict(do_sample=True, temperature=0.8, top_k=0, top_p=1.0, seed=13)
S_TYPICAL = dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.8, typical_mass=0.9, seed=14)
NO_PENALTY = dict(repetition_penalty=1.0)
CFGS = [GREEDY, S_SERVED, S_SHARP, S_OPEN, S_TYPICAL, NO_PENALTY]
S_HOT = dict(do_sample=True, temperature=1.3, top_k=0, top_p=1.0, seed=7)
STEPS = (8, 3)  # the 8-step graph, then the single-step graph three times


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny(golden, dev):
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_tiny.npz")
    cfg = WR.tiny_gpt_cfg(model_dim=int(g["model_dim"]), layers=int(g["layers"]), heads=int(g["heads"]))
    assert cfg["number_mel_codes"] == 8194
    prompts = [(torch.from_numpy(g["embeds_plain"]), 0), (torch.from_numpy(g["embeds_padded"]), int((g["mask_padded"] == 0).sum()))]
    engines = {}

    def engine(name):
        # head_scale 50 is the fixture's: a peaked head, most warped supports hold one token; "wide_soft" flattens it so that the
        # sampling cfgs really part ways
        if name not in engines:
            dtype, slots, head_scale = {"reg": ("f32", 3, 50.0), "wide": ("f32", 6, 50.0), "wide_bf16": ("bf16", 6, 50.0), "wide_soft": ("f32", 6, 5.0)}[name]
            W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=head_scale)
            engines[name] = GptEngine(cfg, dtype=dtype, max_seq=256, max_batch=slots, device=dev).load_state_dict(W)
        return engines[name]

    return prompts, engine


def _prefill(eng, prompts, n, which=None):
    for b in range(n):
        eng.prefill(b, *prompts[(b if which is None else which[b]) % 2])


def _ids(eng, n):
    return [eng.read(b)[0].tolist() for b in range(n)]


@pytest.mark.parametrize("name,n", [("reg", 2), ("reg", 3), ("wide", 4), ("wide", 6), ("wide_bf16", 4), ("wide_bf16", 6), ("wide_soft", 6)])
def test_per_slot_equals_uniform(tiny, name, n):
    prompts, engine = tiny
    eng = engine(name)
    _prefill(eng, prompts, n)
    for k in STEPS:
        eng.decode_slots(k, CFGS[:n])
    got = _ids(eng, n)
    assert all(1 <= len(x) <= sum(STEPS) for x in got)
    if name == "wide_soft":  # the four sampling cfgs gave four different sequences
        assert len({tuple(got[i]) for i in (1, 2, 3, 4)}) == 4, got
    for i in range(n):
        _prefill(eng, prompts, n)
        eng.decode(n, sum(STEPS), **CFGS[i])  # 11 steps: the same two graphs
        assert eng.read(i)[0].tolist() == got[i], (name, n, i)


@pytest.mark.parametrize("name", ["reg", "wide"])
def test_the_stream_selects_the_draws_not_the_slot(tiny, name):
    prompts, engine = tiny
    eng = engine(name)
    same = [0, 0, 0]  # one prompt in three slots

    def run(streams):
        _prefill(eng, prompts, 3, same)
        for k in STEPS:
            eng.decode_slots(k, [S_HOT] * 3, streams)
        return _ids(eng, 3)

    a = run([5, 9, 5])
    assert a[0] == a[2]          # stream 5 in slot 0 and in slot 2
    assert a[0] != a[1]          # streams 5 and 9 of one seed part ways within 11 steps
    b = run([2, 9, 5])
    assert b[2] == a[2] and b[1] == a[1] and b[0] != a[0]
    _prefill(eng, prompts, 3, same)
    eng.decode(3, sum(STEPS), **S_HOT)  # the uniform call: stream = slot index
    old = _ids(eng, 3)
    assert b[0] == old[2]        # stream 2 == what slot 2 always drew
    assert run(None) == old      # no streams given: the slot index


@pytest.mark.parametrize("name", ["reg", "wide"])
def test_processed_probabilities_per_slot_vs_oracle(tiny, name):
    """The bound the uniform path is held to (tests/test_gpu_gpt.py::test_sampling_distribution_vs_oracle): max-abs <= 1e-5,
    equal support."""
    from oracle import gpt as OG

    prompts, engine = tiny
    eng = engine(name)
    tkp = [(0.8, 30, 0.8), (1.3, 5, 0.5), (0.8, 128, 1.0), (0.7, 1, 0.9)][: min(4, eng.max_batch)]
    n = len(tkp)
    forced = [11, 4097, 256]
    _prefill(eng, prompts, n, [0] * n)
    for tok in forced:
        for b in range(n):
            eng.force_next(b, tok)
        eng.decode(n, 1, repetition_penalty=10.0)
    logits = [torch.from_numpy(eng.read_logits(b)) for b in range(n)]
    P = prompts[0][0].shape[0] + 1
    hist = [1] * (P - 1) + [8192] + forced
    eng.decode_slots(1, [dict(repetition_penalty=10.0, do_sample=True, temperature=T, top_k=k, top_p=p, seed=1000 + b) for b, (T, k, p) in enumerate(tkp)])
    for b, (T, k, p) in enumerate(tkp):
        ref = torch.softmax(OG.process_logits(logits[b], hist, 10.0, T, k, p, 1), -1).numpy()
        probs = eng.read_probs(b)
        err = float(np.abs(probs - ref).max())
        print(name, "slot", b, (T, k, p), "max|dp|", err, "support", int((probs > 0).sum()), int((ref > 0).sum()))
        assert err <= 1e-5, (b, T, k, p, err)
        assert (probs > 0).sum() == (ref > 0).sum()
        assert ref[int(eng.read(b)[0][len(forced)])] > 0


@pytest.mark.parametrize("name", ["reg", "wide"])
def test_cfg_changes_between_calls_and_a_refilled_slot_starts_clean(tiny, name):
    from oracle import gpt as OG

    prompts, engine = tiny
    eng = engine(name)
    # sampling -> greedy for slot 1 between two calls
    _prefill(eng, prompts, 2)
    eng.decode_slots(4, [S_SERVED, S_OPEN], [3, 4])
    so_far = eng.read(1)[0].tolist()
    assert len(so_far) == 4
    logits = torch.from_numpy(eng.read_logits(1))
    P = prompts[1][0].shape[0] + 1
    want = int(torch.argmax(OG.process_logits(logits, [1] * (P - 1) + [8192] + so_far, 10.0)))
    eng.decode_slots(1, [S_SERVED, GREEDY], [3, 4])
    assert eng.read(1)[0].tolist() == so_far + [want]

    # slot 0 is refilled mid-run (another prompt, cfg and stream); slot 1 goes on
    def run(refill):
        _prefill(eng, prompts, 2)
        eng.decode_slots(5, [S_SERVED, S_HOT], [3, 4])
        if refill:
            eng.prefill(0, *prompts[1])
        eng.decode_slots(6, [S_SHARP if refill else S_SERVED, S_HOT], [9 if refill else 3, 4])
        return _ids(eng, 2)

    calm, stirred = run(False), run(True)
    assert stirred[1] == calm[1] and len(calm[1]) == 11
    # the newcomer alone: same prompt, cfg and stream from a fresh slot 0 (a register engine keeps two slots active: its
    # kernels are chosen by that number; the companion is a different one)
    if eng.max_batch > 4:
        eng.prefill(0, *prompts[1])
        eng.decode_slots(6, [S_SHARP], [9])
    else:
        _prefill(eng, prompts, 2, [1, 0])
        eng.decode_slots(6, [S_SHARP, GREEDY], [9, 0])
    assert eng.read(0)[0].tolist() == stirred[0] and len(stirred[0]) == 6


NB = 3
G_A = dict(temperature=0.8, top_k=30, top_p=0.8, repetition_penalty=10.0, length_penalty=0.0, seed=11)
G_B = dict(temperature=1.1, top_k=8, top_p=1.0, repetition_penalty=2.0, length_penalty=1.0, seed=11)
G_SEARCH = dict(do_sample=False, repetition_penalty=10.0, length_penalty=1.0, seed=11)


def _snap(eng, max_new, group):
    ids, done, score, bs, lt, src = eng.beam_read(max_new, group=group)
    return ids.tolist(), done, score, bs.tolist(), lt.tolist(), src.tolist()


@pytest.mark.parametrize("pair", [(G_A, G_B), (G_SEARCH, G_A)], ids=["two-samplers", "search-beside-sample"])
def test_beam_groups_carry_their_own_cfg(tiny, pair):
    prompts, engine = tiny
    eng = engine("wide")
    streams, n = (4, 9), 16
    alone = []
    for g in range(2):  # one group at a time through the uniform call
        eng.prefill(0, *prompts[g])
        eng.beam_begin(NB, group=0, rng_stream=streams[g])
        tr = []
        for k in STEPS + (5,):
            eng.beam_decode(k, groups=1, **pair[g])
            tr.append(_snap(eng, n, 0))
        alone.append(tr)
    assert alone[0][-1][2:4] != alone[1][-1][2:4]  # (the head is peaked: the cfgs may agree on the ids, never on the scores)
    for g in range(2):
        eng.prefill(g * NB, *prompts[g])
        eng.beam_begin(NB, group=g, rng_stream=streams[g])
    for c, k in enumerate(STEPS + (5,)):
        eng.beam_decode_groups(k, list(pair))
        for g in range(2):
            assert _snap(eng, n, g) == alone[g][c], (g, c)


def test_a_bad_entry_is_refused_by_name_and_the_engine_goes_on(tiny):
    from voice_tts_amd._lib import IxttsError

    prompts, engine = tiny
    eng = engine("wide")
    _prefill(eng, prompts, 3)
    with pytest.raises(IxttsError, match=r"code -1: .*slot 1\b"):
        eng.decode_slots(1, [GREEDY, dict(S_SERVED, temperature=0.0), GREEDY])
    eng.decode_slots(2, [GREEDY, S_SERVED, GREEDY])
    assert all(len(x) >= 1 for x in _ids(eng, 3))
    for g in range(2):
        eng.prefill(g * NB, *prompts[g])
        eng.beam_begin(NB, group=g, rng_stream=g)
    with pytest.raises(IxttsError, match=r"code -1: .*group 1\b"):
        eng.beam_decode_groups(1, [G_A, dict(G_A, top_k=129)])
    eng.beam_decode_groups(2, [G_A, dict(G_SEARCH, top_k=129)])  # (the warpers' settings are not looked at without sampling)
    assert len(eng.beam_read(8, group=1)[0]) >= 2
