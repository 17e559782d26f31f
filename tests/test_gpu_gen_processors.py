"""GPU: the other half of the processor keywords of HF `generate()` -- sequence_bias, bad_words_ids, forced_eos_token_id,
exponential_decay_length_penalty, epsilon_cutoff, eta_cutoff, renormalize_logits -- in the HIP sampler and the beam step, against
the restatement of the reference's processor classes (tests/gen_processors_ref.py, pinned to the recorded classes by
tests/test_gen_processors.py).

The method of test_gpu_gen_constraints.py: force a history, read the logits, take one sampled step, compare the probability
vector the step drew from with the restatement applied to the DEVICE's own logits: max-abs <= 1e-5, equal support.  FLAT (no
penalty, temperature 4, no top-k / top-p) gives every id positive mass in the unconstrained vector."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_gen_constraints import FLAT, START, STOP, _check, _weights, dev, stop_biased, tiny  # noqa: E402,F401  (fixtures and helpers of the sibling file)

NEG = float("-inf")
V = 8194


def _step(eng, embeds, forced, table=None, forced_eos=None, bans=None, free=0, **kw):
    """Slot 0: prefill, (the slot state,) `free` greedy steps, the forced history, then ONE step under `kw` -> (the history, the logits
    that step saw, the probabilities it drew from)."""
    eng.prefill(0, embeds, 0)
    if bans is not None:
        eng.set_bans(0, *bans)
    if table is not None:
        eng.set_sequence_bias(0, table)
    if forced_eos is not None:
        eng.set_forced_eos(0, forced_eos)
    if free:
        eng.decode(1, free, repetition_penalty=1.0, suppress_stop=True)
    for tok in forced:
        eng.force_next(0, tok)
        eng.decode(1, 1, repetition_penalty=1.0)
    hist = eng.read(0)[0].tolist() if (free or forced) else []
    logits = torch.from_numpy(eng.read_logits(0))
    eng.decode(1, 1, seed=5, **kw)
    return hist, logits, eng.read_probs(0)


def _ref(logits, P, hist, sampler, min_keep=1, **cons):
    import gen_processors_ref as R

    s = R.process(logits, R.history_of(P, hist), P, stop=STOP, theta=sampler["repetition_penalty"], sampling=True, temperature=sampler["temperature"],
                  top_k=sampler["top_k"], top_p=sampler["top_p"], min_keep=min_keep, **cons)
    return torch.softmax(s, -1).numpy()


HIST = [11, 4097, 256]


def test_sequence_bias_full_table_every_register_and_two_on_one_id(tiny):
    g, eng, embeds, P = tiny
    # 64 entries that all match after HIST: one-id entries on an id of every per-thread register (0, 1023, 1024, ..., V - 1), two-id
    # and three-id entries whose leading ids are the history's tail, two of them on an id a one-id entry biases too
    ones = [0, 1023, 1024, 2053, 3079, 4097, 5120, 6147, 7177, V - 1] + [100 + i for i in range(22)]
    table = [((t,), (-3.0 if i % 2 else 2.5) + 0.01 * i) for i, t in enumerate(ones)]
    table += [((256, 200 + i), 1.0 + 0.1 * i) for i in range(15)] + [((256, 1024), -1.5)]
    table += [((4097, 256, 300 + i), -2.0 + 0.2 * i) for i in range(15)] + [((4097, 256, 0), 4.0)]
    assert len(table) == 64
    _, logits, free = _step(eng, embeds, HIST, **FLAT)
    assert (free > 0).all()
    _, logits2, probs = _step(eng, embeds, HIST, table=table, **FLAT)
    assert torch.equal(logits, logits2) and not np.array_equal(probs, free)
    ref = _ref(logits, P, HIST, FLAT, sequence_bias_table=table)
    _check(probs, ref, "full table")
    for t in (0, 1024, 1023, V - 1, 214, 314):  # the biased ids moved as the reference moves them
        assert abs(np.log(probs[t] / free[t]) - np.log(ref[t] / torch.softmax(logits / 4.0, -1).numpy()[t])) < 1e-3, t
    # entries that do not match leave the vector alone, bit for bit
    miss = [((255, 200), 5.0), ((4097, 255, 300), 5.0), ((11, 4097, 257, 301), 5.0)]
    _, _, same = _step(eng, embeds, HIST, table=miss, **FLAT)
    assert np.array_equal(same, free)


def test_sequence_bias_lands_before_the_repetition_penalty(tiny):
    g, eng, embeds, P = tiny
    hot = dict(FLAT, repetition_penalty=10.0)
    _, logits, free = _step(eng, embeds, HIST, **hot)
    raw = float(logits[4097])
    assert raw != 0.0
    bias = float(np.float32(-raw + (3.0 if raw < 0 else -3.0)))  # the biased score changes sign: the penalty divides where it would have multiplied
    table = [((4097,), bias)]
    _, _, probs = _step(eng, embeds, HIST, table=table, **hot)
    ref = _ref(logits, P, HIST, hot, sequence_bias_table=table)
    _check(probs, ref, ("bias before penalty", raw, bias))
    wrong = logits.clone()
    import gen_processors_ref as R
    from oracle import gpt as OG

    wrong = OG.repetition_penalty(wrong, R.history_of(P, HIST), 10.0)
    wrong[4097] += bias
    wrong = torch.softmax(wrong / 4.0, -1).numpy()
    assert abs(wrong[4097] - ref[4097]) > 1e-3 * max(wrong[4097], ref[4097]) and abs(probs[4097] - wrong[4097]) > abs(probs[4097] - ref[4097])


def test_sequence_bias_entry_longer_than_the_history(tiny):
    """A prefill of ONE row: P = 2.  The 3-id entry (1, start, x) equals the whole history plus x but is longer than it: ignored,
    as HF ignores it; one step later (start, 11, y) matches."""
    g, eng, embeds, P = tiny
    one = embeds[:1]
    table = [((1, START, 500), 5.0), ((START, 11, 501), 5.0)]
    _, logits0, free0 = _step(eng, one, [], **FLAT)
    _, _, probs0 = _step(eng, one, [], table=table, **FLAT)
    assert np.array_equal(probs0, free0)
    _, logits1, free1 = _step(eng, one, [11], **FLAT)
    _, _, probs1 = _step(eng, one, [11], table=table, **FLAT)
    ref = _ref(logits1, 2, [11], FLAT, sequence_bias_table=table)
    assert probs1[501] > free1[501] * 2 and free1[501] > 0
    _check(probs1, ref, "P = 2, one step later")


def test_sequence_bias_past_1024_and_past_2048_generated_tokens(golden, dev):
    """An 8-id entry whose seven leading ids end the history when 1024 and when 2049 tokens have been generated."""
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_tiny.npz")
    cfg, W = _weights(g)
    eng = GptEngine(cfg, dtype="f32", max_seq=2304, max_batch=1, device=dev).load_state_dict(W)
    embeds = torch.from_numpy(g["embeds_plain"])
    P = embeds.shape[0] + 1
    lead = [8001, 8002, 8003, 8004, 8005, 8006, 8007]
    table = [(tuple(lead) + (600,), 6.0), (tuple(lead[1:]) + (8100, 601), 6.0)]
    greedy = dict(repetition_penalty=1.0, suppress_stop=True)
    eng.prefill(0, embeds, 0)
    eng.set_sequence_bias(0, table)
    count = 0
    for target in (1024, 2049):
        eng.decode(1, target - 7 - count, **greedy)
        for tok in lead:
            eng.force_next(0, tok)
            eng.decode(1, 1, **greedy)
        hist = eng.read(0)[0].tolist()
        assert len(hist) == target and hist[-7:] == lead
        logits = torch.from_numpy(eng.read_logits(0))
        eng.decode(1, 1, seed=3, suppress_stop=True, **FLAT)
        probs = eng.read_probs(0)
        count = target + 1
        ref = _ref(logits, P, hist, FLAT, sequence_bias_table=table, suppress_stop=True)
        plain = _ref(logits, P, hist, FLAT, suppress_stop=True)
        assert ref[600] > 2 * plain[600] and probs[600] > 2 * plain[600] and abs(probs[601] - plain[601]) <= 1e-5
        _check(probs, ref, ("bias long", target))


def test_bad_words_with_and_without_a_match(tiny):
    g, eng, embeds, P = tiny
    import gen_processors_ref as R

    words = [[256, 300], [4097, 301], [302], [11, 4097, 256, 303], [12, 4097, 256, 304], [STOP]]
    _, logits, free = _step(eng, embeds, HIST, **FLAT)
    assert (free[[300, 301, 302, 303, 304, STOP]] > 0).all()
    eng.prefill(0, embeds, 0)
    eng.set_sequence_bias(0, None, words)  # as generate() takes them; [stop] is dropped
    for tok in HIST:
        eng.force_next(0, tok)
        eng.decode(1, 1, repetition_penalty=1.0)
    eng.decode(1, 1, seed=5, **FLAT)
    probs = eng.read_probs(0)
    assert set(np.nonzero(probs == 0)[0].tolist()) == {300, 302, 303}
    _check(probs, _ref(logits, P, HIST, FLAT, bad_words=R.bad_words_table(words, STOP)), "bad words")
    # greedy decoding honours them: the unconstrained argmax as a one-id bad word
    top = int(logits.argmax())
    eng.prefill(0, embeds, 0)
    eng.set_sequence_bias(0, None, [[top]])
    for tok in HIST:
        eng.force_next(0, tok)
        eng.decode(1, 1, repetition_penalty=1.0)
    eng.decode(1, 1, repetition_penalty=1.0)
    assert eng.read(0)[0].tolist()[-1] == int(torch.topk(logits, 2).indices[1])


@pytest.mark.parametrize("top_k", [0, 30])
def test_forced_eos_on_both_sampler_paths(tiny, top_k):
    g, eng, embeds, P = tiny
    sampler = dict(FLAT, top_k=top_k)
    forced = HIST[:2]
    _, logits, free = _step(eng, embeds, forced, **sampler)
    assert 0 <= free[STOP] < 0.5
    # the step before: nothing
    _, _, before = _step(eng, embeds, forced, forced_eos=[STOP], forced_eos_step=4, **sampler)
    assert np.array_equal(before, free)
    # its step (the third generated token): one-hot, also under min_new_tokens beyond it, which sits in front of it
    for extra in ({}, dict(min_new_tokens=50)):
        _, _, at = _step(eng, embeds, forced, forced_eos=[STOP], forced_eos_step=3, **sampler, **extra)
        assert at[STOP] == 1.0 and (at > 0).sum() == 1
        _check(at, _ref(logits, P, forced, sampler, forced_eos_ids=[STOP], max_length=P + 3, min_new_tokens=extra.get("min_new_tokens", 0)), ("forced", top_k))
        assert eng.read(0)[0].tolist() == forced + [STOP] and eng.read(0)[1]
    # two forced ids share the mass; SuppressTokens, behind it in the chain, still takes one away
    _, _, two = _step(eng, embeds, forced, forced_eos=[STOP, 17], forced_eos_step=3, **sampler)
    assert two[STOP] == 0.5 and two[17] == 0.5
    _, _, sup = _step(eng, embeds, forced, forced_eos=[STOP, 17], bans=([17], []), forced_eos_step=3, **sampler)
    assert sup[STOP] == 1.0 and sup[17] == 0
    _check(sup, _ref(logits, P, forced, sampler, forced_eos_ids=[STOP, 17], max_length=P + 3, suppress_tokens=[17]), "forced + suppress")
    # set_bans and set_forced_eos leave each other's flags alone, in either order
    eng.prefill(0, embeds, 0)
    eng.set_forced_eos(0, [STOP, 17])
    eng.set_bans(0, [17])
    for tok in forced:
        eng.force_next(0, tok)
        eng.decode(1, 1, repetition_penalty=1.0)
    eng.decode(1, 1, seed=5, forced_eos_step=3, **sampler)
    assert np.array_equal(eng.read_probs(0), sup)


def test_forced_eos_greedy_and_through_generate(tiny, dev):
    g, eng, embeds, P = tiny
    plain = dict(repetition_penalty=1.0, suppress_stop=True)
    eng.prefill(0, embeds, 0)
    eng.decode(1, 8, **plain)
    free = eng.read(0)[0].tolist()
    assert len(free) == 8 and STOP not in free
    eng.prefill(0, embeds, 0)
    eng.set_forced_eos(0, STOP)
    eng.decode(1, 8, forced_eos_step=6, **plain)
    ids, fin = eng.read(0)
    assert fin and ids.tolist() == free[:5] + [STOP]
    # generate() at a cap the sequence would otherwise overrun ends in the stop token
    fake = torch.ones(1, P, dtype=torch.long, device=dev)
    fake[0, -1] = START
    eng.store_mel_emb(embeds.unsqueeze(0).to(dev))
    kw = dict(max_length=P + 6, do_sample=False, num_beams=1, repetition_penalty=1.0, suppress_stop=True)
    assert eng.generate(fake, **kw)[0, P:].tolist() == free[:6]
    assert eng.generate(fake, forced_eos_token_id=STOP, **kw)[0, P:].tolist() == free[:5] + [STOP]
    assert eng.generate(fake, forced_eos_token_id=[STOP], min_new_tokens=40, **kw)[0, P:].tolist() == free[:5] + [STOP]
    out = eng.generate(fake, forced_eos_token_id=STOP, max_length=P + 4, do_sample=True, top_k=30, temperature=1.0, num_beams=1, repetition_penalty=1.0,
                       num_return_sequences=2, seed=4, suppress_stop=True)
    assert out.shape == (2, P + 4) and out[:, -1].tolist() == [STOP, STOP]


@pytest.mark.parametrize("which,start,factor,count", [
    ("tiny", 3, 1.5, 3), ("tiny", 3, 1.5, 4), ("tiny", 3, 1.03, 150),
    ("stop_biased", 3, 1.02, 3), ("stop_biased", 3, 1.02, 4), ("stop_biased", 3, 1.002, 150),
])
def test_exponential_decay_at_its_start_one_past_it_and_far_behind_it(tiny, stop_biased, which, start, factor, count):
    """generated == start_index: nothing yet; start_index + 1; far behind it -- on a negative stop score (the plain engine) and a
    positive one (the stop-biased engine).  The power is fp64 on the device as in HF, the rest fp32 in HF's order: the bound of
    the other cases, 1e-5, holds here too."""
    g, _, embeds, P = tiny
    eng = tiny[1] if which == "tiny" else stop_biased
    hist, logits, free = _step(eng, embeds, [], free=count, **FLAT)
    assert len(hist) == count
    assert (logits[STOP] > 0) if which == "stop_biased" else (logits[STOP] != 0)
    print(which, "stop logit", float(logits[STOP]), "factor ** n", factor ** max(count - start, 0))
    _, logits2, probs = _step(eng, embeds, [], free=count, exp_decay_start=start, exp_decay_factor=factor, **FLAT)
    assert torch.equal(logits, logits2)
    ref = _ref(logits, P, hist, FLAT, exp_decay_penalty=(start, factor))
    if count == start:
        assert np.array_equal(probs, free)
    else:
        assert not np.array_equal(ref, _ref(logits, P, hist, FLAT)) and not np.array_equal(probs, free)
    _check(probs, ref, ("decay", which, count))


def _neighbour_threshold(before, ranks):
    """The geometric mean of two neighbouring probabilities of `before`'s softmax, at the rank (of `ranks`) with the widest gap."""
    p = torch.sort(torch.softmax(before.double(), -1), descending=True).values
    j = max(ranks, key=lambda r: float(p[r] / p[r + 1]))
    return float((p[j] * p[j + 1]).sqrt()), j + 1


@pytest.mark.parametrize("top_k", [0, 30])
def test_epsilon_and_eta_cutoff_on_both_sampler_paths(tiny, top_k):
    import gen_processors_ref as R

    g, eng, embeds, P = tiny
    sampler = dict(repetition_penalty=1.0, temperature=4.0, top_k=top_k, top_p=1.0, do_sample=True)
    _, logits, free = _step(eng, embeds, HIST, **sampler)
    hist = R.history_of(P, HIST)
    before = R.process(logits, hist, P, stop=STOP, theta=1.0, sampling=True, temperature=4.0, top_k=top_k)
    # epsilon: between two neighbouring probabilities
    eps, n_keep = _neighbour_threshold(before, (3, 5, 8, 12, 20))
    assert 0 < eps < 1 and R.cut_margin(before, eps) > 1e-3
    _, _, probs = _step(eng, embeds, HIST, epsilon_cutoff=eps, **sampler)
    ref = _ref(logits, P, HIST, sampler, epsilon_cutoff=eps)
    assert (ref > 0).sum() == n_keep < (free > 0).sum() and (free[ref == 0] > 0).any()  # it removes ids the uncut vector holds
    _check(probs, ref, ("epsilon", top_k, eps))
    # eta: of a fixed list the value whose threshold lies farthest from any probability
    cands = []
    for eta in (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0.6, 0.9):
        thr = float(R.eta_threshold(before, eta))
        kept = int((torch.softmax(before, -1) >= thr).sum())
        if 1 < kept < int((free > 0).sum()):
            cands.append((R.cut_margin(before, thr), eta, kept))
    assert cands
    margin, eta, kept = max(cands)
    print("eta", eta, "margin", margin, "keeps", kept)
    assert margin > 1e-3
    _, _, probs = _step(eng, embeds, HIST, eta_cutoff=eta, **sampler)
    ref = _ref(logits, P, HIST, sampler, eta_cutoff=eta)
    assert (ref > 0).sum() == kept and (free[ref == 0] > 0).any()
    _check(probs, ref, ("eta", top_k, eta))
    # both, eta looking at what epsilon left: of the same list the value whose threshold on THAT row lies farthest from any probability
    after_eps = R.process(logits, hist, P, stop=STOP, theta=1.0, sampling=True, temperature=4.0, top_k=top_k, epsilon_cutoff=eps)
    pool = []
    for e in (1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0.6, 0.9):
        thr = float(R.eta_threshold(after_eps, e))
        pool.append((1 < int((torch.softmax(after_eps, -1) >= thr).sum()) < n_keep, R.cut_margin(after_eps, thr), e))  # one that cuts again, if any does
    cuts, margin2, eta2 = max(pool)
    print("eta after epsilon", eta2, "margin", margin2, "cuts again", cuts)
    assert margin2 > 1e-3
    _, _, probs = _step(eng, embeds, HIST, epsilon_cutoff=eps, eta_cutoff=eta2, **sampler)
    _check(probs, _ref(logits, P, HIST, sampler, epsilon_cutoff=eps, eta_cutoff=eta2), ("epsilon + eta", top_k, eta2))


def test_greedy_ignores_the_cutoffs_and_renormalisation_changes_nothing_without_beams(tiny):
    g, eng, embeds, P = tiny
    plain = dict(repetition_penalty=1.0, suppress_stop=True)
    eng.prefill(0, embeds, 0)
    eng.decode(1, 6, **plain)
    free = eng.read(0)[0].tolist()
    for extra in (dict(epsilon_cutoff=0.9, eta_cutoff=0.9), dict(renormalize_logits=True)):
        eng.prefill(0, embeds, 0)
        eng.decode(1, 6, **plain, **extra)
        assert eng.read(0)[0].tolist() == free, extra
    for sampler in (FLAT, dict(FLAT, top_k=30, top_p=0.8)):
        _, _, a = _step(eng, embeds, HIST, **sampler)
        _, _, b = _step(eng, embeds, HIST, renormalize_logits=True, **sampler)
        assert np.array_equal(a, b)
        eng.prefill(0, embeds, 0)
        eng.decode(1, 5, seed=9, **sampler)
        t0 = eng.read(0)[0].tolist()
        eng.prefill(0, embeds, 0)
        eng.decode(1, 5, seed=9, renormalize_logits=True, **sampler)
        assert eng.read(0)[0].tolist() == t0


def test_slot_state_belongs_to_the_slot_and_a_prefill_clears_it(tiny):
    g, eng, embeds, P = tiny
    other = torch.from_numpy(g["embeds_padded"])
    eng.prefill(0, embeds, 0)
    eng.prefill(1, other, 3)
    eng.decode_slots(1, [FLAT, FLAT])
    free0, free1 = eng.read_probs(0), eng.read_probs(1)
    table = [((t,), -5.0) for t in range(0, 6400, 100)]
    assert len(table) == 64
    eng.prefill(0, embeds, 0)
    eng.set_sequence_bias(0, table)
    eng.prefill(1, other, 3)
    eng.decode_slots(1, [dict(FLAT, epsilon_cutoff=1e-3), FLAT])
    assert np.array_equal(eng.read_probs(1), free1) and not np.array_equal(eng.read_probs(0), free0)  # the neighbour: bit for bit unconstrained
    # the other way round, with forced ids too
    eng.prefill(0, other, 3)
    eng.prefill(1, embeds, 0)
    eng.set_sequence_bias(1, table)
    eng.set_forced_eos(1, [STOP])
    eng.decode_slots(1, [FLAT, dict(FLAT, forced_eos_step=1)])
    assert np.array_equal(eng.read_probs(0), free1)
    p1 = eng.read_probs(1)
    assert p1[STOP] == 1.0 and (p1 > 0).sum() == 1
    # a prefill clears the table ...
    eng.prefill(1, embeds, 0)
    eng.prefill(0, other, 3)
    eng.decode_slots(1, [FLAT, FLAT])
    assert np.array_equal(eng.read_probs(1), free0) and np.array_equal(eng.read_probs(0), free1)
    # ... and the forced ids: at the forced step nothing is left to force (every score -inf: argmax gives id 0, not the stop token)
    eng.prefill(1, embeds, 0)
    eng.set_bans(1, [5])
    eng.decode_slots(1, [dict(repetition_penalty=1.0), dict(repetition_penalty=1.0, forced_eos_step=1)])
    assert eng.read(1)[0].tolist() == [0]
    # set_sequence_bias replaces the slot's table; an empty one switches it off
    eng.prefill(0, embeds, 0)
    eng.set_sequence_bias(0, table)
    eng.set_sequence_bias(0, [])
    eng.decode(1, 1, seed=0, **FLAT)
    assert np.array_equal(eng.read_probs(0), free0)


def test_argument_errors_name_the_slot_or_the_group(tiny, golden, dev):
    import ctypes as C

    from voice_tts_amd import _lib
    from voice_tts_amd._lib import IxttsError
    from voice_tts_amd.gpt_engine import GptEngine

    g, _, embeds, P = tiny
    eng = GptEngine(_weights(g)[0], dtype="f32", max_seq=128, max_batch=2, device=dev).load_state_dict(_weights(g)[1])  # (its own: it ends in beam mode)
    eng.prefill(0, embeds, 0)
    eng.prefill(1, embeds, 0)
    ok = dict(repetition_penalty=1.0)
    for bad in (dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.1), dict(eta_cutoff=1.0), dict(eta_cutoff=-1e-3), dict(exp_decay_factor=-1.0),
                dict(exp_decay_start=-1, exp_decay_factor=1.1), dict(exp_decay_factor=float("inf")), dict(forced_eos_step=-1)):
        with pytest.raises(IxttsError, match="slot 1"):
            eng.decode_slots(1, [ok, dict(ok, **bad)])
        with pytest.raises(IxttsError, match="slot 0"):
            eng.decode_slots(1, [dict(ok, **bad), ok])
        with pytest.raises(IxttsError):
            eng.decode(1, 1, **bad)
    eng.decode_slots(1, [dict(ok, epsilon_cutoff=0.0, eta_cutoff=0.999, exp_decay_start=0, exp_decay_factor=1e-3), ok])  # the ranges' ends are fine
    eng.beam_begin(2)
    with pytest.raises(IxttsError, match="group 0"):
        eng.beam_decode_groups(1, [dict(epsilon_cutoff=1.0)])
    # the table: the wrapper refuses in Python and names the slot, the library refuses on its own
    with pytest.raises(ValueError, match="slot 1.*IXTTS_SEQ_BIAS_MAX = 64"):
        eng.set_sequence_bias(1, {(i,): 1.0 for i in range(65)})
    with pytest.raises(ValueError, match="slot 1.*IXTTS_SEQ_BIAS_LEN = 8"):
        eng.set_sequence_bias(1, None, [list(range(9))])
    with pytest.raises(ValueError, match="slot 0"):
        eng.set_sequence_bias(0, {(V,): 1.0})
    with pytest.raises(ValueError, match="slot 0"):
        eng.set_forced_eos(0, [V])
    ids = (C.c_int32 * 65)(*range(65))
    lens = (C.c_int32 * 65)(*([1] * 65))
    bias = (C.c_float * 65)(*([1.0] * 65))
    call = _lib.lib().ixtts_gpt_set_sequence_bias
    with pytest.raises(IxttsError, match="slot 1.*IXTTS_SEQ_BIAS_MAX"):
        _lib.check(call(eng._h, 1, ids, lens, bias, 65, eng._stream()), "ixtts_gpt_set_sequence_bias")
    lens[0] = 9
    with pytest.raises(IxttsError, match="slot 1.*IXTTS_SEQ_BIAS_LEN"):
        _lib.check(call(eng._h, 1, ids, lens, bias, 4, eng._stream()), "ixtts_gpt_set_sequence_bias")
    lens[0] = 1
    ids[2] = V
    with pytest.raises(IxttsError, match="slot 1"):
        _lib.check(call(eng._h, 1, ids, lens, bias, 4, eng._stream()), "ixtts_gpt_set_sequence_bias")
    with pytest.raises(IxttsError):
        _lib.check(call(eng._h, 2, ids, lens, bias, 1, eng._stream()), "ixtts_gpt_set_sequence_bias")  # slot out of range
    with pytest.raises(IxttsError, match="slot 1"):
        _lib.check(_lib.lib().ixtts_gpt_set_forced_eos(eng._h, 1, ids, 4, eng._stream()), "ixtts_gpt_set_forced_eos")


# ------------------------------------------------------------------------------------------------ beams
def _beam_engine(golden, dev, tag):
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    fx = golden("gen_processors.npz")
    cfg, W = _weights(dict(model_dim=128, layers=2, heads=2, seed=int(fx["beam_seed"])), stop_bias=float(fx[f"beam_{tag}_stop_bias"]))
    orc = OG.GptOracle(W, cfg["layers"], cfg["heads"])
    eng = GptEngine(cfg, dtype="f32", max_seq=128, max_batch=3, device=dev).load_state_dict(W)
    fake, embeds, mask = orc.prepare_gpt_inputs(torch.from_numpy(fx[f"beam_{tag}_conds_latent"]), fx[f"beam_{tag}_text"])
    return fx, eng, embeds


@pytest.mark.parametrize("tag", ["bias_bad_words", "forced_eos", "renorm"])
def test_beam_search_with_processors_walks_the_reference_trace(golden, dev, tag):
    """Beam search proper (3 beams) under sequence_bias + bad_words_ids (each beam's own reordered history), forced_eos_token_id at
    a cap the free trace overruns, and renormalize_logits: the trace the reference's scorer, model forward and processor classes
    recorded, step by step; then the same through `generate()`.  At the forced step every candidate but the stop token scores
    -inf, so the beams that go on are arbitrary ids at -inf: there the scores are compared, tokens and sources where they are
    finite."""
    fx, eng, embeds = _beam_engine(golden, dev, tag)
    p = f"beam_{tag}_"
    cfg = json.loads(str(fx[p + "cfg"]))
    max_new, theta = int(fx[p + "max_new"]), float(cfg["theta"])
    table = {tuple(ids): float(b) for ids, b in cfg.get("table", [])} or None
    words = cfg.get("bad_words")
    forced = cfg.get("forced")
    cons = {}
    if cfg.get("renorm"):
        cons["renormalize_logits"] = True
    assert table or words or forced or cons
    eng.prefill(0, embeds, 0)
    if table or words:
        eng.set_sequence_bias(0, table, words)
    if forced:
        eng.set_forced_eos(0, forced)
    eng.beam_begin(3)
    step_cons = dict(cons, forced_eos_step=max_new) if forced else cons
    for step in range(fx[p + "picks"].shape[0]):
        eng.beam_decode(1, repetition_penalty=theta, length_penalty=0.0, do_sample=False, **step_cons)
        ids, done, score, bs, lt, src = eng.beam_read(max_new)
        want = fx[p + "next_scores"][step]
        live = np.isfinite(want) & (want > -1e8)
        assert np.array_equal(np.isfinite(bs) & (bs > -1e8), live), step
        assert lt[live].tolist() == fx[p + "next_tokens"][step][live].tolist(), step
        assert src[live].tolist() == fx[p + "next_indices"][step][live].tolist(), step
        assert np.allclose(bs[live], want[live], rtol=1e-4, atol=2e-3), step
    assert done == bool(fx[p + "done"])
    assert ids.tolist() == fx[p + "sequence"].tolist()
    assert abs(score - float(fx[p + "sequence_score"][0])) <= 2e-3 * max(1.0, abs(score))
    eng.store_mel_emb(embeds.unsqueeze(0))
    P = embeds.shape[0] + 1
    out = eng.generate(torch.ones(1, P, dtype=torch.long), max_length=P + max_new, do_sample=False, num_beams=3, repetition_penalty=theta, length_penalty=0.0,
                       sequence_bias=table, bad_words_ids=words, forced_eos_token_id=forced, **cons)
    assert out[0, P:].tolist() == fx[p + "sequence"].tolist()


def test_beam_sample_step_with_epsilon_cutoff_and_with_renormalisation(golden, dev):
    """One beam-sample step (min_tokens_to_keep = 2) through the forced-draw hook: a forced candidate outside the survivors scores
    -inf, kept ones score as the reference does -- under epsilon_cutoff, and under renormalize_logits, where the kept scores are
    the reference's renormalised ones."""
    import gen_processors_ref as R

    fx, eng, embeds = _beam_engine(golden, dev, "renorm")
    P = embeds.shape[0] + 1
    sampler = dict(repetition_penalty=1.0, temperature=4.0, top_k=30, top_p=1.0)
    warp = {k: v for k, v in sampler.items() if k != "repetition_penalty"}
    eng.prefill(0, embeds, 0)
    ls = torch.log_softmax(torch.from_numpy(eng.read_logits(0)), -1)
    hist = R.history_of(P, [])
    before = R.process(ls, hist, P, theta=1.0, sampling=True, min_keep=2, **warp)
    order = torch.argsort(before, descending=True)[:30].tolist()
    pr = torch.softmax(before, -1)[order]
    n_in = 4
    eps = float((pr[n_in - 1] * pr[n_in]).sqrt())  # between the 4th and the 5th survivor's probability
    assert R.cut_margin(before, eps) > 1e-3 and 0 < eps < 1
    after = R.process(ls, hist, P, theta=1.0, sampling=True, min_keep=2, epsilon_cutoff=eps, **warp)
    assert set(torch.nonzero(~torch.isinf(after)).flatten().tolist()) == set(order[:n_in])
    picks = [order[0], order[3], order[4], order[9], order[20], order[29]]  # beam 0: flat pick = token
    eng.beam_begin(3)
    eng.beam_force(picks)
    eng.beam_decode(1, seed=1, epsilon_cutoff=eps, **sampler)
    ids, done, score, bs, lt, src = eng.beam_read(12)
    assert lt.tolist()[:2] == [order[0], order[3]] and src.tolist() == [0, 0, 0]
    assert np.allclose(bs[:2], [float(after[order[0]]), float(after[order[3]])], rtol=1e-4, atol=2e-3)
    assert bs[2] == -np.inf  # the third beam had to come from a candidate the cutoff removed
    # renormalisation: all six are survivors of TopK; their scores are log-probabilities over the 30
    renorm = R.process(ls, hist, P, theta=1.0, sampling=True, min_keep=2, renormalize_logits=True, **warp)
    assert abs(float(torch.exp(renorm[order].double()).sum()) - 1.0) < 1e-5 and float((renorm[order[0]] - before[order[0]]).abs()) > 1e-2
    eng.prefill(0, embeds, 0)
    eng.beam_begin(3)
    eng.beam_force(picks)
    eng.beam_decode(1, seed=1, renormalize_logits=True, **sampler)
    bs0, lt0 = eng.beam_read(12)[3:5]
    assert lt0.tolist() == [order[0], order[3], order[4]]
    assert np.allclose(bs0, [float(renorm[t]) for t in lt0.tolist()], rtol=1e-4, atol=2e-3)
    # both: the logsumexp runs over what the cutoff left
    both = R.process(ls, hist, P, theta=1.0, sampling=True, min_keep=2, epsilon_cutoff=eps, renormalize_logits=True, **warp)
    eng.prefill(0, embeds, 0)
    eng.beam_begin(3)
    eng.beam_force(picks)
    eng.beam_decode(1, seed=1, epsilon_cutoff=eps, renormalize_logits=True, **sampler)
    bs1 = eng.beam_read(12)[3]
    assert np.allclose(bs1[:2], [float(both[order[0]]), float(both[order[3]])], rtol=1e-4, atol=2e-3) and bs1[2] == -np.inf
