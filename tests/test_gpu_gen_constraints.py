"""GPU: the constraints HF `generate()` builds from plain keywords -- no_repeat_ngram_size, min_new_tokens / min_length,
suppress_tokens, begin_suppress_tokens, min_p -- in the HIP sampler and the beam step, against the restatement of the reference's
processor classes (tests/gen_constraints_ref.py, pinned to the recorded classes by tests/test_gen_constraints.py).

Method of test_gpu_gpt.py::test_sampling_distribution_vs_oracle: force a history, read the logits, take one sampled step, compare
the probability vector the step drew from with the restatement applied to the DEVICE's own logits: max-abs <= 1e-5, equal support.
FLAT (no penalty, temperature 4, no top-k / top-p) gives every id positive mass in the unconstrained vector -- on the CPU oracle
this model's logits span -50..45, so the smallest probability is about e^-24, a normal fp32 number -- and every case asserts that
the unconstrained device vector gives the ids in question positive mass: that is what makes the zero meaningful."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FLAT = dict(repetition_penalty=1.0, temperature=4.0, top_k=0, top_p=1.0, do_sample=True)
START, STOP = 8192, 8193


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _weights(g, stop_bias=0.0):
    import voice_tts_amd.weights as WR

    cfg = WR.tiny_gpt_cfg(model_dim=int(g["model_dim"]), layers=int(g["layers"]), heads=int(g["heads"]))
    W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=50.0)
    if stop_bias:
        W["mel_head.bias"] = W["mel_head.bias"].clone()
        W["mel_head.bias"][STOP] += stop_bias
    return cfg, W


@pytest.fixture(scope="module")
def tiny(golden, dev):
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_tiny.npz")
    cfg, W = _weights(g)
    eng = GptEngine(cfg, dtype="f32", max_seq=256, max_batch=2, device=dev).load_state_dict(W)
    embeds = torch.from_numpy(g["embeds_plain"])
    P = embeds.shape[0] + 1
    assert P == 49
    return g, eng, embeds, P


def _step(eng, embeds, forced, bans=None, **kw):
    """Slot 0: prefill, (bans,) the forced history, then ONE step under `kw` -> (the logits that step saw, the probabilities it drew from)."""
    eng.prefill(0, embeds, 0)
    if bans is not None:
        eng.set_bans(0, *bans)
    for tok in forced:
        eng.force_next(0, tok)
        eng.decode(1, 1, repetition_penalty=1.0)
    logits = torch.from_numpy(eng.read_logits(0))
    eng.decode(1, 1, seed=5, **kw)
    return logits, eng.read_probs(0)


def _ref_probs(logits, P, forced, sampler, **cons):
    import gen_constraints_ref as R

    s = R.process(logits, R.history_of(P, forced), P, stop=STOP, theta=sampler["repetition_penalty"], sampling=True, temperature=sampler["temperature"],
                  top_k=sampler["top_k"], top_p=sampler["top_p"], **cons)
    return torch.softmax(s, -1).numpy()


def _check(probs, ref, what):
    err = float(np.abs(probs - ref).max())
    print(what, "max-abs", err, "support", int((probs > 0).sum()), int((ref > 0).sum()))
    assert err <= 1e-5, (what, err)
    assert (probs > 0).sum() == (ref > 0).sum(), what


@pytest.mark.parametrize("forced,n,banned", [
    ([11, 4097, 256, 11, 4097], 3, {256}),
    ([11, 4097, 256, 11, 4097], 2, {256}),
    ([7, 7, 7], 2, {7}),                       # the window overlaps the suffix
    ([1, 1], 3, {1, START}),                   # both come from the fake prefix [1] * (P - 1) + [start]
    ([11, 4097, 256, 11, 4097], 1, {1, START, 11, 4097, 256}),
    ([11, 4097, 256, 12, 4097], 3, set()),
    ([], 8, set()),
    ([1, 1, 1, 1, 1, 1, 1], 8, {1, START}),    # the largest n, its suffix wholly inside the ones
])
def test_ngram_ban_on_forced_histories(tiny, forced, n, banned):
    g, eng, embeds, P = tiny
    logits, free = _step(eng, embeds, forced, **FLAT)
    assert (free > 0).all()  # the unconstrained vector gives every id positive mass
    logits2, probs = _step(eng, embeds, forced, no_repeat_ngram_size=n, **FLAT)
    assert torch.equal(logits, logits2)
    ref = _ref_probs(logits, P, forced, FLAT, no_repeat_ngram_size=n)
    assert set(np.nonzero(ref == 0)[0].tolist()) == banned
    assert set(np.nonzero(probs == 0)[0].tolist()) == banned
    _check(probs, ref, ("ngram", forced, n))


def test_ngram_ban_on_the_survivor_path(tiny):
    """top_k = 30 (the sorted-survivor path of the sampler) with n = 1 and a history that holds the unconstrained top-3 ids."""
    g, eng, embeds, P = tiny
    forced = [3765, 6143, 7680]  # a fixed point on the CPU oracle: after this history these three are the three largest logits
    top30 = dict(FLAT, top_k=30)
    logits, free = _step(eng, embeds, forced, **top30)
    assert set(np.argsort(-free)[:3].tolist()) == set(forced) and (free[forced] > 0).all()
    _, probs = _step(eng, embeds, forced, no_repeat_ngram_size=1, **top30)
    assert (probs[forced] == 0).all() and (probs > 0).sum() == 30
    _check(probs, _ref_probs(logits, P, forced, top30, no_repeat_ngram_size=1), "ngram survivor path")


def test_ngram_ban_free_running_greedy(tiny):
    import gen_constraints_ref as R

    g, eng, embeds, P = tiny
    eng.prefill(0, embeds, 0)
    eng.decode(1, 16, repetition_penalty=1.0, suppress_stop=True)
    plain = eng.read(0)[0].tolist()
    assert plain[11] == 1089 and plain[2] == 1089  # the unconstrained run repeats a token: the ban below is known to act
    eng.prefill(0, embeds, 0)
    got = []
    for k in range(16):
        logits = torch.from_numpy(eng.read_logits(0))
        s = R.process(logits, R.history_of(P, got), P, stop=STOP, theta=1.0, no_repeat_ngram_size=1, suppress_stop=True)
        eng.decode(1, 1, repetition_penalty=1.0, suppress_stop=True, no_repeat_ngram_size=1)
        got = eng.read(0)[0].tolist()
        assert len(got) == k + 1 and got[-1] == int(s.argmax()), k
    assert len(set(got)) == 16 and got[:11] == plain[:11] and got[11] != 1089


def test_ngram_scan_past_1024_and_past_2048_generated_tokens(golden, dev):
    """The scan's second round (windows 1024.. of the generated tokens) and its reads beyond the 2048 tokens it keeps on chip: each
    time the only earlier occurrence of the suffix lies in that range, so the ban can come from nowhere else."""
    import gen_constraints_ref as R
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_tiny.npz")
    cfg, W = _weights(g)
    eng = GptEngine(cfg, dtype="f32", max_seq=2304, max_batch=1, device=dev).load_state_dict(W)
    embeds = torch.from_numpy(g["embeds_plain"])
    P = embeds.shape[0] + 1
    greedy = dict(repetition_penalty=1.0, suppress_stop=True)
    eng.prefill(0, embeds, 0)
    for free_steps, (a, b, c) in ((1040, (8001, 8002, 8003)), (1000, (8011, 8012, 8013))):
        eng.decode(1, free_steps, **greedy)
        for tok in (a, b, c):
            eng.force_next(0, tok)
            eng.decode(1, 1, **greedy)
        eng.decode(1, 20, **greedy)
        for tok in (a, b):
            eng.force_next(0, tok)
            eng.decode(1, 1, **greedy)
        hist = eng.read(0)[0].tolist()
        where = [i for i, t in enumerate(hist) if t == c]
        assert len(where) == 1 and hist.count(a) == 2 and hist.count(b) == 2  # the free-running stretches never emit them
        assert where[0] >= (1024 if a == 8001 else 2048)
        logits = torch.from_numpy(eng.read_logits(0))
        eng.decode(1, 1, seed=3, no_repeat_ngram_size=3, suppress_stop=True, **FLAT)  # (no stop token: the sequence goes on below)
        probs = eng.read_probs(0)
        ref = _ref_probs(logits, P, hist, FLAT, no_repeat_ngram_size=3, suppress_stop=True)
        assert ref[c] == 0 and probs[c] == 0
        _check(probs, ref, ("ngram long", len(hist)))


@pytest.fixture(scope="module")
def stop_biased(golden, dev):
    """An engine whose stop token wins the first greedy step (mel_head.bias[stop] raised)."""
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_tiny.npz")
    cfg, W = _weights(g, stop_bias=60.0)
    return GptEngine(cfg, dtype="f32", max_seq=256, max_batch=2, device=dev).load_state_dict(W)


def test_min_new_tokens(tiny, stop_biased, dev):
    g, _, embeds, P = tiny
    eng = stop_biased
    eng.prefill(0, embeds, 0)
    eng.decode(1, 8, repetition_penalty=1.0)
    ids, fin = eng.read(0)
    assert fin and ids.tolist() == [STOP]  # unconstrained: the stop token at once
    eng.prefill(0, embeds, 0)
    eng.decode(1, 8, repetition_penalty=1.0, min_new_tokens=5)
    ids, fin = eng.read(0)
    assert fin and len(ids) == 6 and ids[-1] == STOP and STOP not in ids[:5].tolist()
    five = ids[:5].tolist()
    # the mass of the stop token at gen_count 4 and 5
    for forced, zero in ((five[:4], True), (five, False)):
        logits, probs = _step(eng, embeds, forced, min_new_tokens=5, **FLAT)
        _, free = _step(eng, embeds, forced, **FLAT)
        assert free[STOP] > 0
        assert (probs[STOP] == 0) == zero
        _check(probs, _ref_probs(logits, P, forced, FLAT, min_new_tokens=5), ("min_new", len(forced)))
    # min_length through generate(); min_new_tokens wins when both are given
    fake = torch.ones(1, P, dtype=torch.long, device=dev)
    fake[0, -1] = START
    eng.store_mel_emb(embeds.unsqueeze(0).to(dev))
    kw = dict(max_length=P + 12, do_sample=False, num_beams=1, repetition_penalty=1.0)
    assert eng.generate(fake, **kw)[0, P:].tolist() == [STOP]
    assert eng.generate(fake, min_length=P + 5, **kw)[0, P:].tolist() == five + [STOP]
    assert eng.generate(fake, min_new_tokens=5, **kw)[0, P:].tolist() == five + [STOP]
    assert eng.generate(fake, min_length=P + 5, min_new_tokens=3, **kw)[0, P:].tolist() == five[:3] + [STOP]
    assert eng.generate(fake, min_length=P - 2, **kw)[0, P:].tolist() == [STOP]
    # more than can be generated is no error: the sequence runs to its cap without a stop token
    out = eng.generate(fake, min_new_tokens=500, max_length=P + 7, do_sample=False, num_beams=1, repetition_penalty=1.0)
    assert out.shape[1] == P + 7 and STOP not in out[0, P:].tolist()
    # num_return_sequences > 1: every row under the constraint
    out = eng.generate(fake, min_new_tokens=4, max_length=P + 9, do_sample=True, top_k=30, temperature=1.0, num_beams=1, repetition_penalty=1.0,
                       num_return_sequences=2, seed=4)
    for row in out[:, P:].tolist():
        assert STOP not in row[:4]


def test_suppress_and_begin_suppress_tokens(tiny):
    from voice_tts_amd._lib import IxttsError

    g, eng, embeds, P = tiny
    logits0, free0 = _step(eng, embeds, [], **FLAT)
    a, b = [int(i) for i in np.argsort(-free0)[:2]]  # the unconstrained argmax and runner-up
    assert free0[a] > 0 and free0[b] > 0
    bans = ((a,), (b,))
    _, probs0 = _step(eng, embeds, [], bans=bans, **FLAT)
    assert probs0[a] == 0 and probs0[b] == 0  # first generated token: both lists act
    _check(probs0, _ref_probs(logits0, P, [], FLAT, suppress_tokens=[a], begin_suppress_tokens=[b]), "bans step 0")
    logits1, free1 = _step(eng, embeds, [11], **FLAT)
    assert free1[a] > 0 and free1[b] > 0
    _, probs1 = _step(eng, embeds, [11], bans=bans, **FLAT)
    assert probs1[a] == 0 and probs1[b] > 0  # second token: the begin list is through
    _check(probs1, _ref_probs(logits1, P, [11], FLAT, suppress_tokens=[a], begin_suppress_tokens=[b]), "bans step 1")
    # greedy decoding honours them too
    eng.prefill(0, embeds, 0)
    eng.set_bans(0, [a], [b])
    eng.decode(1, 1, repetition_penalty=1.0)
    assert eng.read(0)[0].tolist() not in ([a], [b])
    # a prefill of the slot without set_bans: the mass is back
    _, again = _step(eng, embeds, [], **FLAT)
    assert again[a] > 0 and again[b] > 0 and np.array_equal(again, free0)
    # set_bans replaces the slot's lists
    eng.prefill(0, embeds, 0)
    eng.set_bans(0, [a], [b])
    eng.set_bans(0, [b])
    eng.decode(1, 1, seed=5, **FLAT)
    p = eng.read_probs(0)
    assert p[a] > 0 and p[b] == 0
    for bad in ([8194], [-1]):
        with pytest.raises(IxttsError):
            eng.set_bans(0, bad)
        with pytest.raises(IxttsError):
            eng.set_bans(0, (), bad)
    with pytest.raises(IxttsError):
        eng.set_bans(2, [1])  # slot out of range


def test_min_p_on_both_sampler_paths(tiny, golden):
    """The fixture's min_p settings without beams (min_tokens_to_keep = 1): top_k = 0 (whole-vocabulary path) and top_k = 30
    (sorted survivors).  A setting whose reference vector on the device's logits has a probability within 1e-5 (relative) of the
    threshold is skipped -- rounding would decide membership -- and at most one may be."""
    import gen_constraints_ref as R

    g, eng, embeds, P = tiny
    fx = golden("gen_constraints.npz")
    forced = [11, 4097, 256]
    names = [n for n in fx["min_p_cases"].tolist() if int(fx[f"{n}_min_keep"]) == 1]
    assert {int(fx[f"{n}_top_k"]) for n in names} == {0, 30}
    skipped = 0
    for n in names:
        sampler = dict(repetition_penalty=1.0, temperature=float(fx[f"{n}_temperature"]), top_k=int(fx[f"{n}_top_k"]), top_p=float(fx[f"{n}_top_p"]), do_sample=True)
        mp = float(fx[f"{n}_min_p"])
        logits, free = _step(eng, embeds, forced, **sampler)
        before = R.process(logits, R.history_of(P, forced), P, theta=1.0, sampling=True, temperature=sampler["temperature"], top_k=sampler["top_k"],
                           top_p=sampler["top_p"])
        if mp < 1.0:
            margin = R.min_p_margin(before, mp)
        else:  # min_p = 1 keeps what ties with the largest: how far the runner-up is from it
            top2 = torch.topk(torch.softmax(before.double(), -1), 2).values
            margin = float((top2[0] - top2[1]) / top2[0])
        print(n, "margin", margin)
        if margin <= 1e-5:
            skipped += 1
            continue
        _, probs = _step(eng, embeds, forced, min_p=mp, **sampler)
        ref = _ref_probs(logits, P, forced, sampler, min_p=mp)
        assert (ref > 0).sum() < (free > 0).sum() and (free[ref == 0] > 0).any()  # MinP removes ids the unconstrained vector holds
        _check(probs, ref, n)
    assert skipped <= 1
    # greedy decoding does not run the warper
    eng.prefill(0, embeds, 0)
    eng.decode(1, 4, repetition_penalty=1.0, suppress_stop=True)
    plain = eng.read(0)[0].tolist()
    eng.prefill(0, embeds, 0)
    eng.decode(1, 4, repetition_penalty=1.0, suppress_stop=True, min_p=0.9)
    assert eng.read(0)[0].tolist() == plain


def test_constraints_belong_to_the_slot(tiny):
    g, eng, embeds, P = tiny
    other = torch.from_numpy(g["embeds_padded"])
    plain = dict(repetition_penalty=1.0, suppress_stop=True)
    hard = dict(plain, no_repeat_ngram_size=1, min_new_tokens=3)
    eng.prefill(0, embeds, 0)
    eng.decode(1, 16, **plain)
    free0 = eng.read(0)[0].tolist()
    bans = (free0[:2], [free0[2]])
    eng.prefill(0, other, 3)
    eng.decode(1, 16, **plain)
    solo1 = eng.read(0)[0].tolist()
    eng.prefill(0, embeds, 0)
    eng.set_bans(0, *bans)
    eng.decode_slots(16, [hard])
    solo0 = eng.read(0)[0].tolist()
    assert solo0 != free0 and not set(free0[:2]) & set(solo0) and solo0[0] != free0[2] and len(set(solo0)) == 16
    eng.prefill(0, embeds, 0)
    eng.set_bans(0, *bans)
    eng.prefill(1, other, 3)
    eng.decode_slots(16, [hard, plain])
    assert eng.read(0)[0].tolist() == solo0  # bit for bit its solo constrained run
    assert eng.read(1)[0].tolist() == solo1  # and the plain neighbour its solo unconstrained run
    # the other way round: the constrained sequence in slot 1
    eng.prefill(0, other, 3)
    eng.prefill(1, embeds, 0)
    eng.set_bans(1, *bans)
    eng.decode_slots(16, [plain, hard])
    assert eng.read(0)[0].tolist() == solo1 and eng.read(1)[0].tolist() == solo0


def test_argument_errors_name_the_slot(tiny):
    from voice_tts_amd import _lib
    from voice_tts_amd._lib import IxttsError

    g, eng, embeds, P = tiny
    eng.prefill(0, embeds, 0)
    eng.prefill(1, embeds, 0)
    ok = dict(repetition_penalty=1.0)
    for bad in (dict(no_repeat_ngram_size=_lib.NGRAM_MAX + 1), dict(min_p=1.5), dict(min_new_tokens=-1), dict(min_p=-0.1), dict(no_repeat_ngram_size=-1)):
        with pytest.raises(IxttsError, match="slot 1"):
            eng.decode_slots(1, [ok, dict(ok, **bad)])
        with pytest.raises(IxttsError, match="slot 0"):
            eng.decode_slots(1, [dict(ok, **bad), ok])
        with pytest.raises(IxttsError):
            eng.decode(1, 1, **bad)
    eng.decode_slots(1, [dict(ok, no_repeat_ngram_size=_lib.NGRAM_MAX, min_p=1.0), dict(ok, min_p=0.0)])  # the range's ends are fine


# ------------------------------------------------------------------------------------------------ beams
def _beam_engine(golden, dev, tag):
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    fx = golden("gen_constraints.npz")
    cfg, W = _weights(dict(model_dim=128, layers=2, heads=2, seed=int(fx["beam_seed"])), stop_bias=float(fx[f"beam_{tag}_stop_bias"]))
    orc = OG.GptOracle(W, cfg["layers"], cfg["heads"])
    eng = GptEngine(cfg, dtype="f32", max_seq=128, max_batch=3, device=dev).load_state_dict(W)
    fake, embeds, mask = orc.prepare_gpt_inputs(torch.from_numpy(fx[f"beam_{tag}_conds_latent"]), fx[f"beam_{tag}_text"])
    return fx, eng, embeds


@pytest.mark.parametrize("tag", ["min_new", "ngram1", "suppress"])
def test_beam_search_with_constraints_walks_the_reference_trace(golden, dev, tag):
    """Beam search proper (3 beams) under min_new_tokens (the stop token would win step 0), no_repeat_ngram_size = 1 (each beam's
    own reordered history) and suppress_tokens (the unconstrained trace's first tokens): the trace the reference's scorer, model
    forward and processor classes recorded, step by step; then the same through `generate()`."""
    fx, eng, embeds = _beam_engine(golden, dev, tag)
    p = f"beam_{tag}_"
    max_new, theta = int(fx[p + "max_new"]), float(fx[p + "theta"])
    cons = {}
    if int(fx[p + "n"]):
        cons["no_repeat_ngram_size"] = int(fx[p + "n"])
    if int(fx[p + "min_new"]):
        cons["min_new_tokens"] = int(fx[p + "min_new"])
    suppress = fx[p + "suppress"].tolist()
    assert cons or suppress
    eng.prefill(0, embeds, 0)
    if suppress:
        eng.set_bans(0, suppress)
    eng.beam_begin(3)
    for step in range(fx[p + "picks"].shape[0]):
        eng.beam_decode(1, repetition_penalty=theta, length_penalty=0.0, do_sample=False, **cons)
        ids, done, score, bs, lt, src = eng.beam_read(max_new)
        assert lt.tolist() == fx[p + "next_tokens"][step].tolist(), step
        assert src.tolist() == fx[p + "next_indices"][step].tolist(), step
        assert np.allclose(bs, fx[p + "next_scores"][step], rtol=1e-4, atol=2e-3), step
    assert done == bool(fx[p + "done"])
    assert ids.tolist() == fx[p + "sequence"].tolist()
    assert abs(score - float(fx[p + "sequence_score"][0])) <= 2e-3 * max(1.0, abs(score))
    eng.store_mel_emb(embeds.unsqueeze(0))
    P = embeds.shape[0] + 1
    out = eng.generate(torch.ones(1, P, dtype=torch.long), max_length=P + max_new, do_sample=False, num_beams=3, repetition_penalty=theta, length_penalty=0.0,
                       suppress_tokens=suppress or None, **cons)
    assert out[0, P:].tolist() == fx[p + "sequence"].tolist()


def test_beam_sample_step_with_min_p(golden, dev):
    """One beam-sample step under min_p (min_tokens_to_keep = 2), through the forced-draw hook: a forced candidate outside the
    survivors scores -inf, so the scores of six forced draws show which of them lie in the support -- two ids MinP keeps, four that
    TopK keeps and MinP removes."""
    import gen_constraints_ref as R

    fx, eng, embeds = _beam_engine(golden, dev, "ngram1")
    P = embeds.shape[0] + 1
    sampler = dict(repetition_penalty=1.0, temperature=4.0, top_k=30, top_p=1.0)
    eng.prefill(0, embeds, 0)
    ls = torch.log_softmax(torch.from_numpy(eng.read_logits(0)), -1)
    hist = R.history_of(P, [])
    before = R.process(ls, hist, P, theta=1.0, sampling=True, min_keep=2, **{k: v for k, v in sampler.items() if k != "repetition_penalty"})
    order = torch.argsort(before, descending=True)[:30].tolist()
    ratios = torch.softmax(before, -1)[order] / torch.softmax(before, -1)[order[0]]
    n_in = 4
    mp = float((ratios[n_in - 1] * ratios[n_in]).sqrt())  # between the 4th and the 5th survivor's probability ratio
    assert R.min_p_margin(before, mp) > 1e-3 and 0 < mp < 1
    after = R.process(ls, hist, P, theta=1.0, sampling=True, min_keep=2, min_p=mp, **{k: v for k, v in sampler.items() if k != "repetition_penalty"})
    support = set(torch.nonzero(~torch.isinf(after)).flatten().tolist())
    assert support == set(order[:n_in])
    picks = [order[0], order[3], order[4], order[9], order[20], order[29]]  # beam 0: flat pick = token
    eng.beam_begin(3)
    eng.beam_force(picks)
    eng.beam_decode(1, seed=1, min_p=mp, **sampler)
    ids, done, score, bs, lt, src = eng.beam_read(12)
    assert lt.tolist()[:2] == [order[0], order[3]] and src.tolist() == [0, 0, 0]
    assert np.allclose(bs[:2], [float(after[order[0]]), float(after[order[3]])], rtol=1e-4, atol=2e-3)
    assert bs[2] == -np.inf  # the third beam had to come from a candidate MinP removed
    # the same draws without min_p: all six are survivors of TopK
    eng.prefill(0, embeds, 0)
    eng.beam_begin(3)
    eng.beam_force(picks)
    eng.beam_decode(1, seed=1, **sampler)
    bs0, lt0 = eng.beam_read(12)[3:5]
    assert lt0.tolist() == [order[0], order[3], order[4]] and np.isfinite(bs0).all()
    # free running: every new beam's token lies in the reference support
    for seed in range(4):
        eng.prefill(0, embeds, 0)
        eng.beam_begin(3)
        eng.beam_decode(1, seed=seed, min_p=mp, **sampler)
        bs1, lt1 = eng.beam_read(12)[3:5]
        live = [int(t) for t, s in zip(lt1, bs1) if s > -1e8]
        assert len(live) == 3 and set(live) <= support, (seed, live)
