"""CPU: the constraint keywords of HF `generate()` -- min_new_tokens / min_length, no_repeat_ngram_size, suppress_tokens,
begin_suppress_tokens, min_p.  The restatement the GPU tests compare against (tests/gen_constraints_ref.py) equals what the
reference's own processor classes recorded (tests/golden/gen_constraints.npz); the keyword parsing; the schedulers' host logic
(set_bans between a slot's prefill and its next decode call, the scalars in that slot's cfg only) against recording engines."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_constraints_ref as R  # noqa: E402
from voice_tts_amd.gpt_engine import generation_constraints, resolve_min_length  # noqa: E402
from voice_tts_amd.scheduler import BeamGroupScheduler, DecodeScheduler, Segment  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden):
    return golden("gen_constraints.npz")


def test_the_fixture_holds_the_cases_the_kernel_can_get_wrong(fx):
    names = set(fx["cases"].tolist())
    assert {"ngram3_ones_prefix", "ngram1", "ngram2_overlap", "begin_first", "begin_later"} <= names
    keeps = {int(fx[f"{n}_min_keep"]) for n in fx["min_p_cases"].tolist()}
    assert keeps == {1, 2}
    assert set(fx["beam_cases"].tolist()) == {"min_new", "ngram1", "suppress"}
    # what the special cases are about
    start = int(fx["start"])
    banned = lambda n: set(np.nonzero(np.isinf(fx[f"{n}_scores"]))[0].tolist())  # noqa: E731
    assert banned("ngram3_ones_prefix") == {1, start}
    assert banned("ngram1") == set(fx["ngram1_history"].tolist()) and {1, start} <= banned("ngram1")
    assert banned("ngram2_overlap") == {7} and banned("ngram3_repeat") == {256} and banned("ngram2_repeat") == {256}
    assert banned("begin_first") == {17, 18} and banned("begin_later") == set() and banned("ngram8_short") == set()


def test_restatement_of_the_processors_equals_the_reference_classes(fx):
    stop = int(fx["stop"])
    for n in fx["cases"].tolist():
        got = R.constrain(torch.from_numpy(fx[f"{n}_logits"]), fx[f"{n}_history"].tolist(), int(fx[f"{n}_P"]), stop, int(fx[f"{n}_n"]),
                          int(fx[f"{n}_min_new"]), fx[f"{n}_suppress"].tolist(), fx[f"{n}_begin"].tolist()).numpy()
        assert np.array_equal(got, fx[f"{n}_scores"]), n  # -inf in the same places, everything else untouched


def test_restatement_of_min_p_equals_the_reference_warper(fx):
    for n in fx["min_p_cases"].tolist():
        T, k, p, mp, keep = float(fx[f"{n}_temperature"]), int(fx[f"{n}_top_k"]), float(fx[f"{n}_top_p"]), float(fx[f"{n}_min_p"]), int(fx[f"{n}_min_keep"])
        logits = torch.from_numpy(fx[f"{n}_logits"])
        got = R.process(logits, [1, int(fx["start"])], 2, stop=int(fx["stop"]), theta=1.0, sampling=True, temperature=T, top_k=k, top_p=p, min_p=mp,
                        min_keep=keep).numpy()
        ref = fx[f"{n}_scores"]
        assert np.array_equal(np.isinf(got), np.isinf(ref)), n  # the kept mask
        assert (~np.isinf(ref)).sum() >= keep
        live = ~np.isinf(ref)
        assert np.allclose(got[live], ref[live], rtol=1e-6, atol=0), n
        if mp < 1.0:  # the generator's guard: rounding cannot decide membership
            before = R.process(logits, [1, int(fx["start"])], 2, theta=1.0, sampling=True, temperature=T, top_k=k, top_p=p, min_keep=keep)
            assert R.min_p_margin(before, mp) > 1e-5, n


def test_ngram_ban_in_closed_form_over_the_fake_prefix():
    """What the kernel computes -- windows ending at e >= -2 relative to the first generated token, e = -2 standing for every window
    inside the ones -- equals the plain scan over the full history, for every n, prompt length and a few histories."""
    def closed(P, gen, n, start):
        G = len(gen)
        if P + G < n:
            return set()
        hist = lambda k: 1 if k < -1 else start if k == -1 else gen[k]  # noqa: E731
        out = set()
        for e in range(max(n - 1 - P, -2), G):
            if all(hist(e - n + 1 + i) == hist(G - n + 1 + i) for i in range(n - 1)):
                out.add(hist(e))
        return out

    rng = np.random.RandomState(5)
    gens = [[], [1], [1, 1], [1, 1, 1, 1], [8192], [1, 8192], [1, 1, 8192, 1, 1], [7, 7, 7], [11, 4097, 256, 11, 4097]]
    gens += [rng.randint(0, 3, size=m).tolist() for m in (5, 9, 17)] + [[1 if x else 8192 for x in rng.randint(0, 2, size=12)]]
    for P in (2, 3, 4, 9, 49):
        for gen in gens:
            for n in range(1, 9):
                assert closed(P, gen, n, 8192) == R.ngram_banned(R.history_of(P, gen), n), (P, gen, n)


def test_keyword_parsing():
    assert generation_constraints({}, 49) == ({}, None)
    kw = dict(min_length=54, seed=3)
    assert generation_constraints(kw, 49) == (dict(min_new_tokens=5), None) and kw == dict(seed=3)  # popped, the rest left alone
    assert generation_constraints(dict(min_length=40), 49) == ({}, None)  # max(0, L - P)
    assert generation_constraints(dict(min_length=54, min_new_tokens=3), 49) == (dict(min_new_tokens=3), None)  # min_new_tokens wins
    assert generation_constraints(dict(min_length=54, min_new_tokens=None), 49) == (dict(min_new_tokens=5), None)  # None: not given
    cfg, bans = generation_constraints(dict(no_repeat_ngram_size=4, min_p=0.1, suppress_tokens=[5, 6], begin_suppress_tokens=np.array([7])), 49)
    assert cfg == dict(no_repeat_ngram_size=4, min_p=0.1) and bans == ((5, 6), (7,))
    assert generation_constraints(dict(no_repeat_ngram_size=0, min_p=0.0, min_new_tokens=0, suppress_tokens=[], begin_suppress_tokens=None), 49) == ({}, None)
    assert generation_constraints(dict(begin_suppress_tokens=[9]), 49) == ({}, ((), (9,)))
    # a caller whose segments differ in prompt length resolves min_length per segment
    cfg, _ = generation_constraints(dict(min_length=60, no_repeat_ngram_size=2))
    assert cfg == dict(min_length=60, no_repeat_ngram_size=2)
    assert resolve_min_length(cfg, 50) == dict(min_new_tokens=10, no_repeat_ngram_size=2)
    assert resolve_min_length(cfg, 70) == dict(no_repeat_ngram_size=2)
    assert resolve_min_length(dict(min_p=0.5), 70) == dict(min_p=0.5)


def _bare_tts():
    from voice_tts_amd.infer_v2 import IndexTTS2
    from voice_tts_amd.weights import tiny_gpt_cfg

    m = IndexTTS2.__new__(IndexTTS2)
    m.gpt_cfg = tiny_gpt_cfg(model_dim=16, layers=1, heads=2)
    m.device = torch.device("cpu")
    g = torch.Generator().manual_seed(3)
    m.text_embedding = torch.randn(m.gpt_cfg["number_text_tokens"] + 1, 16, generator=g)
    m.text_pos_embedding = torch.randn(m.gpt_cfg["max_text_tokens"] + 2, 16, generator=g)
    return m


def test_infer_helper_and_generation_keys():
    from types import SimpleNamespace

    from voice_tts_amd.infer_v2 import IndexTTS2

    m = _bare_tts()
    for k in ("min_new_tokens", "min_length", "no_repeat_ngram_size", "suppress_tokens", "begin_suppress_tokens", "min_p"):
        assert k in IndexTTS2.GENERATION_KEYS
    given = dict(top_k=5, min_new_tokens=4, min_p=0.2, suppress_tokens=[3], seed=1)
    g, rest = m._generation_args(given)
    assert rest == dict(min_new_tokens=4, min_p=0.2, suppress_tokens=[3], seed=1)  # the new keywords stay among the leftovers
    assert m._generation_constraints(rest) == (dict(min_new_tokens=4, min_p=0.2), ((3,), ()))
    assert rest == dict(min_new_tokens=4, min_p=0.2, suppress_tokens=[3], seed=1)  # left alone for gpt.generate
    assert m._generation_constraints({}) is None and m._generation_constraints(dict(seed=2)) is None
    assert m._generation_constraints(dict(min_length=60)) == (dict(min_length=60), None)
    assert m._generation_constraints(dict(min_length=60, min_new_tokens=2)) == (dict(min_new_tokens=2), None)
    for bad in (dict(min_new_tokens=-1), dict(no_repeat_ngram_size=9), dict(min_p=1.5), dict(suppress_tokens=[m.gpt_cfg["number_mel_codes"]]), dict(begin_suppress_tokens=[-1])):
        with pytest.raises(ValueError):
            m._generation_constraints(bad)
    # a request's `generation` dict: the keys are accepted, the request is pinned, an unknown key is still refused
    gcall, _ = m._generation_args({})
    gr, pinned, cons = m._request_generation(dict(generation=dict(min_new_tokens=7, suppress_tokens=[4, 5])), {}, gcall)
    assert pinned and cons == (dict(min_new_tokens=7), ((4, 5), ()))
    gr, pinned, cons = m._request_generation({}, dict(no_repeat_ngram_size=3), gcall)
    assert not pinned and gr is gcall and cons == (dict(no_repeat_ngram_size=3), None)
    assert m._request_generation({}, {}, gcall) == (gcall, False, None)
    with pytest.raises(ValueError):
        m._request_generation(dict(generation=dict(min_new_token=7)), {}, gcall)
    # the segment builder: scalars into the sampler (min_length against the segment's own prompt), lists into bans; nothing set: as before
    cl = torch.randn(34, 16, generator=torch.Generator().manual_seed(4))
    ids = [7, 9, 11]
    eng = SimpleNamespace(max_seq=192)
    P = 34 + len(ids) + 2 + 1
    seg = m._segment(cl, ids, eng, 20, constraints=(dict(min_length=P + 6, min_p=0.3), ((5,), ())), sampler=dict(top_k=7))
    assert seg.sampler == dict(top_k=7, min_new_tokens=6, min_p=0.3) and seg.bans == ((5,), ())
    seg = m._segment(cl, ids, eng, 20, constraints=(dict(min_length=P - 1), None))
    assert seg.sampler is None and seg.bans is None
    seg = m._segment(cl, ids, eng, 20)
    assert seg.sampler is None and seg.bans is None


# ------------------------------------------------------------------------------------------------ schedulers, recording engines
STOP = 99
RUN = dict(repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, seed=0, typical_mass=0.0)


class Recorder:
    """Slot b emits its key at every step; every call is written down with its arguments."""

    def __init__(self, max_batch, max_seq=200):
        self.max_batch, self.max_seq = max_batch, max_seq
        self.seq, self.calls = [None] * max_batch, []

    def prefill(self, b, embeds, pad):
        self.seq[b] = dict(key=int(embeds[0, 0]), out=[])
        self.calls.append(("prefill", b, self.seq[b]["key"]))

    def set_bans(self, b, suppress_tokens=(), begin_suppress_tokens=()):
        self.calls.append(("set_bans", b, tuple(suppress_tokens), tuple(begin_suppress_tokens)))

    def decode(self, n_active, n_steps, **kw):
        self.calls.append(("decode", n_active, n_steps, kw))
        for b in range(n_active):
            self.seq[b]["out"] += [self.seq[b]["key"]] * n_steps

    def decode_slots(self, n_steps, cfgs, streams=None):
        self.calls.append(("decode_slots", n_steps, [dict(c) for c in cfgs], [self.seq[b]["key"] for b in range(len(cfgs))]))
        for b in range(len(cfgs)):
            self.seq[b]["out"] += [self.seq[b]["key"]] * n_steps

    def read(self, b):
        return np.asarray(self.seq[b]["out"], np.int32), False


def _seg(key, max_new, **kw):
    e = torch.zeros(5, 4)
    e[0, 0] = key
    return Segment(request=key // 10, index=key % 10, embeds=e, n_left_pad=0, max_new=max_new, **kw)


def test_segment_has_an_optional_bans_field():
    assert _seg(10, 4).bans is None
    assert _seg(10, 4, bans=((1,), (2,))).bans == ((1,), (2,))


def test_decode_scheduler_sets_bans_after_the_prefill_and_again_after_a_refill():
    cons = dict(min_new_tokens=3, no_repeat_ngram_size=2)
    # longest cap first: 30 takes slot 0, 20 slot 1, 40 refills slot 1 when 20 is through
    segs = [_seg(20, 4, sampler=cons, bans=((5, 6), (7,))), _seg(30, 12), _seg(40, 3, bans=((), (8,)))]
    eng = Recorder(2)
    DecodeScheduler(eng, 2, STOP, sync_every=4).run(segs, lambda s, ids: None, do_sample=True, **RUN)
    calls = eng.calls
    assert [c for c in calls if c[0] == "set_bans"] == [("set_bans", 1, (5, 6), (7,)), ("set_bans", 1, (), (8,))]
    for i, c in enumerate(calls):
        if c[0] == "set_bans":  # right after that slot's prefill, before the next decode call
            assert calls[i - 1][0] == "prefill" and calls[i - 1][1] == c[1] and calls[i + 1][0] in ("decode_slots", "prefill")
    assert [c[2] for c in calls if c[0] == "prefill" and c[1] == 1] == [20, 40]  # the refill of slot 1
    base = dict(RUN, do_sample=True, suppress_stop=False)
    seen = set()
    for c in [c for c in calls if c[0] == "decode_slots"]:
        for cfg, key in zip(c[2], c[3]):
            assert cfg == (dict(base, **cons) if key == 20 and 20 not in seen_done(calls, c) else base), (key, cfg)
            seen.add(key)
    assert seen == {20, 30, 40}
    assert not any(c[0] == "decode" for c in calls)


def seen_done(calls, upto):
    """Keys whose slot was prefilled anew before call `upto` (their segment is through)."""
    done, held = set(), {}
    for c in calls:
        if c is upto:
            break
        if c[0] == "prefill":
            if c[1] in held:
                done.add(held[c[1]])
            held[c[1]] = c[2]
    return done


def test_decode_scheduler_without_bans_never_calls_set_bans():
    eng = Recorder(2)
    eng.set_bans = None  # any call would fail
    DecodeScheduler(eng, 2, STOP, sync_every=4).run([_seg(10, 4), _seg(20, 6)], lambda s, ids: None, do_sample=True, **RUN)
    assert all(c[0] in ("prefill", "decode") for c in eng.calls)
    assert all(c[3] == dict(RUN, do_sample=True, suppress_stop=False) for c in eng.calls if c[0] == "decode")


class BeamRecorder:
    def __init__(self, max_batch):
        self.max_batch, self.calls, self.steps = max_batch, [], {}

    def prefill(self, b, embeds, pad):
        self.calls.append(("prefill", b, int(embeds[0, 0])))

    def set_bans(self, b, suppress_tokens=(), begin_suppress_tokens=()):
        self.calls.append(("set_bans", b, tuple(suppress_tokens), tuple(begin_suppress_tokens)))

    def beam_begin(self, nb, group=0, rng_stream=0):
        self.calls.append(("begin", group))
        self.steps[group] = 0

    def beam_park(self, group):
        self.calls.append(("park", group))

    def beam_decode(self, n_steps, groups=1, **kw):
        self.calls.append(("beam_decode", n_steps, groups, kw))
        for g in range(groups):
            self.steps[g] = self.steps.get(g, 0) + n_steps

    def beam_decode_groups(self, n_steps, cfgs):
        self.calls.append(("beam_decode_groups", n_steps, [dict(c) for c in cfgs]))
        for g in range(len(cfgs)):
            self.steps[g] = self.steps.get(g, 0) + n_steps

    def beam_read(self, max_new, group=0):
        return np.zeros(min(self.steps[group], max_new), np.int32), False, 0.0


def test_beam_scheduler_sets_bans_on_the_groups_first_slot():
    cons = dict(min_new_tokens=2, min_p=0.1)
    segs = [_seg(10, 8, sampler=cons, bans=((3,), ())), _seg(20, 4), _seg(30, 3, bans=((), (4,)))]
    eng = BeamRecorder(6)
    BeamGroupScheduler(eng, 3, sync_every=4).run(segs, lambda s, ids, score: None, length_penalty=0.0, **RUN)
    calls = eng.calls
    # group 0 <- 10 (slot 0), group 1 <- 20 (slot 3), then 30 refills group 1
    assert [c for c in calls if c[0] == "set_bans"] == [("set_bans", 0, (3,), ()), ("set_bans", 3, (), (4,))]
    for i, c in enumerate(calls):
        if c[0] == "set_bans":
            assert calls[i - 1][0] == "prefill" and calls[i - 1][1] == c[1] and calls[i + 1][0] == "begin"
    base = dict(RUN, length_penalty=0.0, suppress_stop=False)
    groups = [c for c in calls if c[0] == "beam_decode_groups"]
    assert groups and not any(c[0] == "beam_decode" for c in calls)
    assert all(c[2][0] == dict(base, **cons) for c in groups)       # group 0 holds segment 10 throughout
    assert all(cfg == base for c in groups for cfg in c[2][1:])     # the scalars in that group's cfg only
