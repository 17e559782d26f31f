"""CPU: the other half of the processor keywords of HF `generate()` -- sequence_bias, bad_words_ids, forced_eos_token_id,
exponential_decay_length_penalty, epsilon_cutoff, eta_cutoff, renormalize_logits.  The restatement the GPU tests compare against
(tests/gen_processors_ref.py) equals what the reference's own processor classes recorded (tests/golden/gen_processors.npz): masks
equal, scores within 1e-6 relative; the keyword parsing; the request path's helpers; the schedulers' host logic against recording
engines."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gen_processors_ref as R  # noqa: E402
from voice_tts_amd import _lib  # noqa: E402
from voice_tts_amd.gpt_engine import PROCESSOR_KEYS, generation_processors, sequence_bias_table  # noqa: E402
from voice_tts_amd.scheduler import BeamGroupScheduler, DecodeScheduler, Segment  # noqa: E402

NEG = float("-inf")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("gen_processors.npz")


def _same(got, ref, what):
    assert np.array_equal(np.isinf(got), np.isinf(ref)), what  # the kept mask
    assert not np.isnan(got).any(), what
    live = ~np.isinf(ref)
    assert np.allclose(got[live], ref[live], rtol=1e-6, atol=0), (what, float(np.abs(got[live] - ref[live]).max()))


def ref_kwargs(cfg, stop):
    """A fixture case's settings (the generator's names) -> keyword arguments of `gen_processors_ref.process`."""
    kw = dict(theta=cfg.get("theta", 1.0), sequence_bias_table=[(tuple(ids), b) for ids, b in cfg.get("table", [])],
              bad_words=R.bad_words_table(cfg.get("bad_words", []), stop), no_repeat_ngram_size=cfg.get("n", 0), min_new_tokens=cfg.get("min_new", 0),
              forced_eos_ids=cfg.get("forced", ()), max_length=cfg.get("max_length"), exp_decay_penalty=cfg.get("decay"),
              suppress_tokens=cfg.get("suppress", ()))
    if cfg.get("sampling"):
        kw.update(sampling=True, temperature=cfg["temperature"], top_k=cfg["top_k"], top_p=cfg["top_p"], min_p=cfg["min_p"], epsilon_cutoff=cfg["epsilon"],
                  eta_cutoff=cfg["eta"])
    kw["renormalize_logits"] = bool(cfg.get("renorm"))
    return kw


def _case_logits(fx, n):
    logits = torch.from_numpy(fx["row_logits"]).clone()
    for t, v in json.loads(str(fx[f"{n}_fix"])).items():
        logits[int(t)] = v
    return logits


def test_the_fixture_holds_the_cases_the_kernel_can_get_wrong(fx):
    names = set(fx["cases"].tolist())
    assert {"bias_one_id", "bias_8_ids_match", "bias_prefix_in_fake_prompt", "bias_longer_than_history", "bias_two_on_one_id", "bias_before_penalty",
            "bad_word_eos_dropped", "bad_word_then_forced_eos", "bad_word_not_yet_forced", "forced_eos_over_min_new", "decay_at_start",
            "decay_start_plus_1_positive", "decay_start_plus_1_negative", "decay_far_positive", "decay_far_negative"} <= names
    stop, start = int(fx["stop"]), int(fx["start"])
    sc = lambda n: fx[f"{n}_scores"]  # noqa: E731
    lg = lambda n: _case_logits(fx, n).numpy()  # noqa: E731
    assert int(fx["bias_longer_than_history_P"]) == 2 and sc("bias_longer_than_history")[7] == lg("bias_longer_than_history")[7]
    assert fx["bias_prefix_in_fake_prompt_history"].tolist()[-3:] == [1, start, 40]
    assert len(json.loads(str(fx["bias_8_ids_match_cfg"]))["table"][0][0]) == 8 and sc("bias_8_ids_match")[700] == lg("bias_8_ids_match")[700] + 4.0
    # the sign flip that proves the order: (-2 + 5) / 10, not -2 * 10 + 5
    assert lg("bias_before_penalty")[77] == -2.0 and abs(sc("bias_before_penalty")[77] - 0.3) < 1e-6
    assert np.isfinite(sc("bad_word_eos_dropped")[stop]) and sc("bad_word_eos_dropped")[4] == NEG
    assert sc("bad_word_then_forced_eos")[stop] == 0 and np.isfinite(sc("bad_word_then_forced_eos")).sum() == 1
    assert sc("bad_word_not_yet_forced")[stop] == NEG and np.isfinite(sc("bad_word_not_yet_forced")).sum() == int(fx["V"]) - 1
    assert sc("forced_eos_over_min_new")[stop] == 0
    assert np.array_equal(sc("decay_at_start"), lg("decay_at_start"))
    assert sc("decay_start_plus_1_positive")[stop] == 3.0 and sc("decay_start_plus_1_negative")[stop] == -1.0
    assert lg("decay_far_positive")[stop] > 0 > lg("decay_far_negative")[stop]
    w = fx["warper_cases"].tolist()
    combos = {(int(json.loads(str(fx[f"{n}_cfg"]))["top_k"]), int(fx[f"{n}_min_keep"]), "eps" if json.loads(str(fx[f"{n}_cfg"]))["epsilon"] else "eta")
              for n in w if n.startswith(("eps_k", "eta_k"))}
    assert combos == {(k, keep, kind) for k in (0, 30) for keep in (1, 2) for kind in ("eps", "eta")}
    assert "renorm_after_warpers" in w
    assert set(fx["beam_cases"].tolist()) == {"bias_bad_words", "forced_eos", "renorm"}
    assert fx["beam_forced_eos_sequence"].tolist()[-1] == 8193 and int(fx["beam_forced_eos_max_new"]) == len(fx["beam_forced_eos_sequence"])
    for tag in fx["beam_cases"].tolist():
        assert fx[f"beam_{tag}_picks"].shape[0] <= 12 and fx[f"beam_{tag}_next_tokens"].shape[1] == 3


def test_restatement_of_the_processors_equals_the_reference_classes(fx):
    stop = int(fx["stop"])
    for n in fx["cases"].tolist():
        cfg = json.loads(str(fx[f"{n}_cfg"]))
        got = R.process(_case_logits(fx, n), fx[f"{n}_history"].tolist(), int(fx[f"{n}_P"]), stop=stop, **ref_kwargs(cfg, stop)).numpy()
        _same(got, fx[f"{n}_scores"], n)


def test_restatement_of_the_cutoffs_equals_the_reference_warpers(fx):
    stop, start = int(fx["stop"]), int(fx["start"])
    for n in fx["warper_cases"].tolist():
        cfg = json.loads(str(fx[f"{n}_cfg"]))
        keep = int(fx[f"{n}_min_keep"])
        logits = torch.from_numpy(fx[f"{n}_logits"])
        kw = ref_kwargs(cfg, stop)
        got = R.process(logits, [1, start], 2, stop=stop, min_keep=keep, **kw).numpy()
        _same(got, fx[f"{n}_scores"], n)
        assert (~np.isinf(got)).sum() >= keep
        # the generator's guard: rounding cannot decide membership; and which term of eta's threshold is the smaller
        before = R.process(logits, [1, start], 2, stop=stop, min_keep=keep, **dict(kw, epsilon_cutoff=0.0, eta_cutoff=0.0, renormalize_logits=False))
        if cfg["epsilon"]:
            assert R.cut_margin(before, cfg["epsilon"]) > 1e-5, n
            before = R.process(logits, [1, start], 2, stop=stop, min_keep=keep, **dict(kw, eta_cutoff=0.0, renormalize_logits=False))
        if cfg["eta"]:
            thr = float(R.eta_threshold(before, cfg["eta"]))
            assert R.cut_margin(before, thr) > 1e-5, n
            if n.endswith("_peaked"):
                assert thr == np.float32(cfg["eta"]), n
            if n.endswith("_flat"):
                assert thr < np.float32(cfg["eta"]), n
        if cfg["renorm"]:
            live = ~np.isinf(got)
            assert abs(float(np.exp(got[live].astype(np.float64)).sum()) - 1.0) < 1e-5


def test_renormalisation_changes_no_probability_without_beams(fx):
    stop, start = int(fx["stop"]), int(fx["start"])
    n = "renorm_after_warpers"
    kw = ref_kwargs(json.loads(str(fx[f"{n}_cfg"])), stop)
    a = R.process(torch.from_numpy(fx[f"{n}_logits"]), [1, start], 2, stop=stop, **kw)
    b = R.process(torch.from_numpy(fx[f"{n}_logits"]), [1, start], 2, stop=stop, **dict(kw, renormalize_logits=False))
    assert not torch.equal(a, b) and int(a.argmax()) == int(b.argmax())
    assert np.allclose(torch.softmax(a, -1).numpy(), torch.softmax(b, -1).numpy(), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ the parser
def test_parser_takes_both_forms_of_sequence_bias():
    as_dict = {(52,): -4.0, (7, 8, 9): 2.5}
    as_list = [[[52], -4.0], [[7, 8, 9], 2.5]]
    want = [((52,), -4.0), ((7, 8, 9), 2.5)]
    for form in (as_dict, as_list, json.loads(json.dumps(as_list))):
        kw = dict(sequence_bias=form, seed=3)
        cfg, state = generation_processors(kw, 8193, 8194)
        assert cfg == {} and state == dict(table=want, forced_eos=()) and kw == dict(seed=3)  # popped, the rest left alone
    assert sequence_bias_table(as_dict, [[5, 6], [8193], [5, 6]], 8193, 8194) == want + [((5, 6), NEG)]  # [eos] dropped, a repeated word once
    assert sequence_bias_table(None, [[8193]], 8193, 8194) == []
    assert sequence_bias_table(None, [[8193]], None, 8194) == [((8193,), NEG)]


def test_parser_scalars_and_none():
    kw = dict(forced_eos_token_id=8193, exponential_decay_length_penalty=(40, 1.02), epsilon_cutoff=3e-4, eta_cutoff=2e-3, renormalize_logits=True,
              bad_words_ids=[[3, 4]], top_k=5)
    cfg, state = generation_processors(kw, 8193, 8194)
    assert cfg == dict(exp_decay_start=40, exp_decay_factor=1.02, epsilon_cutoff=3e-4, eta_cutoff=2e-3, renormalize_logits=True)
    assert state == dict(table=[((3, 4), NEG)], forced_eos=(8193,)) and kw == dict(top_k=5)
    assert generation_processors(dict(forced_eos_token_id=[8193, 7]), 8193, 8194)[1] == dict(table=[], forced_eos=(8193, 7))
    assert generation_processors(dict(exponential_decay_length_penalty=[0, 2]), 8193)[0] == dict(exp_decay_start=0, exp_decay_factor=2.0)
    # None = not given; 0 = off; renormalize_logits only when it is True
    none = {k: None for k in PROCESSOR_KEYS}
    assert generation_processors(dict(none), 8193, 8194) == ({}, None)
    assert generation_processors(dict(epsilon_cutoff=0.0, eta_cutoff=0, renormalize_logits=False), 8193, 8194) == ({}, None)
    assert generation_processors({}, 8193, 8194) == ({}, None)
    assert set(PROCESSOR_KEYS) == {"sequence_bias", "bad_words_ids", "forced_eos_token_id", "exponential_decay_length_penalty", "epsilon_cutoff",
                                   "eta_cutoff", "renormalize_logits"}


@pytest.mark.parametrize("bad", [
    dict(sequence_bias={}), dict(sequence_bias=[]), dict(sequence_bias="x"), dict(sequence_bias={(): 1.0}), dict(sequence_bias={(3, -1): 1.0}),
    dict(sequence_bias={(3,): 1}), dict(sequence_bias={3: 1.0}), dict(sequence_bias=[[[3], 1]]), dict(sequence_bias=[[[], 1.0]]),
    dict(sequence_bias=[[[3.5], 1.0]]), dict(sequence_bias={(8194,): 1.0}), dict(sequence_bias={(3,): float("nan")}),
    dict(bad_words_ids=[]), dict(bad_words_ids=[[]]), dict(bad_words_ids=[3]), dict(bad_words_ids=[[3, -2]]), dict(bad_words_ids=((3,),)),
    dict(bad_words_ids=[[8194]]),
    dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-0.1), dict(eta_cutoff=1.0), dict(eta_cutoff=-1e-3),
    dict(exponential_decay_length_penalty=(-1, 1.1)), dict(exponential_decay_length_penalty=(3, 0.0)), dict(exponential_decay_length_penalty=(3, -2.0)),
    dict(exponential_decay_length_penalty=(3,)), dict(exponential_decay_length_penalty=(1.5, 1.1)), dict(exponential_decay_length_penalty=(3, float("inf"))),
    dict(forced_eos_token_id=-1), dict(forced_eos_token_id=8194), dict(forced_eos_token_id=[]), dict(forced_eos_token_id=[3, 8194]),
])
def test_parser_refuses_what_hf_refuses(bad):
    with pytest.raises(ValueError):
        generation_processors(dict(bad), 8193, 8194)


def test_parser_names_the_limits_of_the_table():
    assert _lib.SEQ_BIAS_MAX == 64 and _lib.SEQ_BIAS_LEN == 8
    full = {(i, i + 1): 1.0 for i in range(40)}
    words = [[100 + i] for i in range(24)]
    assert len(generation_processors(dict(sequence_bias=dict(full), bad_words_ids=list(words)), 8193, 8194)[1]["table"]) == 64
    with pytest.raises(ValueError, match="IXTTS_SEQ_BIAS_MAX = 64"):
        generation_processors(dict(sequence_bias=dict(full), bad_words_ids=words + [[999]]), 8193, 8194)  # the two share the table
    assert generation_processors(dict(bad_words_ids=[list(range(8))]), 8193, 8194)[1]["table"] == [(tuple(range(8)), NEG)]
    with pytest.raises(ValueError, match="IXTTS_SEQ_BIAS_LEN = 8"):
        generation_processors(dict(bad_words_ids=[list(range(9))]), 8193, 8194)
    with pytest.raises(ValueError, match="IXTTS_SEQ_BIAS_LEN = 8"):
        generation_processors(dict(sequence_bias={tuple(range(9)): 1.0}), 8193, 8194)


def test_sampler_cfg_follows_the_header():
    import ctypes as C

    names = [f[0] for f in _lib.SamplerCfg._fields_]
    assert names[-7:] == ["exp_decay_start", "exp_decay_factor", "epsilon_cutoff", "eta_cutoff", "renormalize_logits", "forced_eos_step", "n_seq_bias"]
    assert names[names.index("min_p") + 1] == "exp_decay_start"  # appended behind min_p
    assert dict(_lib.SamplerCfg._fields_)["exp_decay_factor"] is C.c_double
    here = os.path.dirname(os.path.abspath(__file__))
    header = open(os.path.join(here, "..", "include", "ixtts_hip.h")).read()
    body = header[header.index("typedef struct ixtts_sampler_cfg {"):header.index("} ixtts_sampler_cfg;")]
    order = [body.index(f" {n};") for n in names]
    assert order == sorted(order)  # the same fields in the same order
    assert "#define IXTTS_SEQ_BIAS_MAX 64" in header and "#define IXTTS_SEQ_BIAS_LEN 8" in header
    for sym in ("ixtts_gpt_set_sequence_bias", "ixtts_gpt_set_forced_eos"):
        assert sym in _lib.SYMBOLS and f"int {sym}(" in header
    z = _lib.SamplerCfg()  # a caller that zero-fills the new fields has every new stage off
    assert (z.exp_decay_factor, z.epsilon_cutoff, z.eta_cutoff, z.renormalize_logits, z.forced_eos_step, z.n_seq_bias) == (0.0, 0.0, 0.0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------ the request path's helpers
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


def test_generation_dict_takes_the_new_keys_and_still_refuses_a_misspelt_one():
    from types import SimpleNamespace

    from voice_tts_amd.infer_v2 import IndexTTS2

    m = _bare_tts()
    stop = m.gpt_cfg["stop_mel_token"]
    for k in PROCESSOR_KEYS:
        assert k in IndexTTS2.GENERATION_KEYS
    gcall, _ = m._generation_args({})
    gen = dict(sequence_bias=[[[52], -4.0]], bad_words_ids=[[3, 4]], forced_eos_token_id=stop, exponential_decay_length_penalty=[30, 1.05],
               epsilon_cutoff=3e-4, eta_cutoff=1e-3, renormalize_logits=True)
    gr, pinned, cons = m._request_generation(dict(generation=dict(gen)), {}, gcall)
    assert pinned and cons is None  # accepted; none of them is one of the older constraints
    for wrong in ("sequence_biases", "bad_word_ids", "forced_eos", "epsilon_cut_off", "renormalise_logits"):
        with pytest.raises(ValueError, match="unknown key"):
            m._request_generation(dict(generation={wrong: 1}), {}, gcall)
    # the leftovers of _generation_args carry them on to gpt.generate; the helper leaves them alone
    g, rest = m._generation_args(dict(top_k=5, **gen))
    assert rest == gen
    cfg, state = m._generation_processors(rest)
    assert rest == gen
    assert cfg == dict(exp_decay_start=30, exp_decay_factor=1.05, epsilon_cutoff=3e-4, eta_cutoff=1e-3, renormalize_logits=True)
    assert state == dict(table=[((52,), -4.0), ((3, 4), NEG)], forced_eos=(stop,))
    assert m._generation_processors({}) is None and m._generation_processors(dict(seed=2, min_p=0.1)) is None
    for bad in (dict(sequence_bias={}), dict(bad_words_ids=[[m.gpt_cfg["number_mel_codes"]]]), dict(epsilon_cutoff=1.0), dict(forced_eos_token_id=-1),
                dict(exponential_decay_length_penalty=(2, 0.0))):
        with pytest.raises(ValueError):
            m._generation_processors(bad)
    # the segment builder: scalars into the sampler, the forced step = the segment's own max_new, the slot state into Segment.processors
    cl = torch.randn(34, 16, generator=torch.Generator().manual_seed(4))
    eng = SimpleNamespace(max_seq=192)
    seg = m._segment(cl, [7, 9, 11], eng, 20, processors=(cfg, state), sampler=dict(top_k=7))
    assert seg.max_new == 20 and seg.sampler == dict(top_k=7, forced_eos_step=20, **cfg) and seg.processors == state and seg.bans is None
    seg = m._segment(cl, [7, 9, 11], eng, 500, processors=({}, dict(table=[], forced_eos=(stop,))))
    cap = min(192 - (34 + 3 + 2 + 1) - 2, m.gpt_cfg["max_mel_tokens"] - 1)  # what the engine and the position table leave of the 500
    assert cap < 500 and seg.max_new == cap and seg.sampler == dict(forced_eos_step=cap)
    seg = m._segment(cl, [7, 9, 11], eng, 20, processors=(dict(epsilon_cutoff=0.1), None))
    assert seg.sampler == dict(epsilon_cutoff=0.1) and seg.processors is None
    seg = m._segment(cl, [7, 9, 11], eng, 20)
    assert seg.sampler is None and seg.processors is None and seg.bans is None


# ------------------------------------------------------------------------------------------------ schedulers, recording engines
STOP = 99
RUN = dict(repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, seed=0, typical_mass=0.0)


class Recorder:
    def __init__(self, max_batch, max_seq=200):
        self.max_batch, self.max_seq = max_batch, max_seq
        self.seq, self.calls = [None] * max_batch, []

    def prefill(self, b, embeds, pad):
        self.seq[b] = dict(key=int(embeds[0, 0]), out=[])
        self.calls.append(("prefill", b, self.seq[b]["key"]))

    def set_bans(self, b, suppress_tokens=(), begin_suppress_tokens=()):
        self.calls.append(("set_bans", b))

    def set_processors(self, b, state):
        self.calls.append(("set_processors", b, state))

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


def test_segment_has_an_optional_processors_field():
    assert _seg(10, 4).processors is None and _seg(10, 4).bans is None
    st = dict(table=[((1,), 2.0)], forced_eos=())
    assert _seg(10, 4, processors=st).processors is st


def test_decode_scheduler_installs_the_slot_state_after_the_prefill_and_again_after_a_refill():
    a, b = dict(table=[((5,), -1.0)], forced_eos=(STOP,)), dict(table=[], forced_eos=(STOP,))
    segs = [_seg(20, 4, sampler=dict(forced_eos_step=4), processors=a, bans=((1,), ())), _seg(30, 12), _seg(40, 3, processors=b)]
    eng = Recorder(2)
    DecodeScheduler(eng, 2, STOP, sync_every=4).run(segs, lambda s, ids: None, do_sample=True, **RUN)
    calls = eng.calls
    assert [c for c in calls if c[0] == "set_processors"] == [("set_processors", 1, a), ("set_processors", 1, b)]
    for i, c in enumerate(calls):
        if c[0] == "set_processors":  # after that slot's prefill (and its set_bans), before the next decode call
            assert calls[i - 1][:2] in (("prefill", c[1]), ("set_bans", c[1])) and calls[i + 1][0] in ("decode_slots", "prefill")
    first = [c for c in calls if c[0] == "decode_slots"][0]
    assert [cfg.get("forced_eos_step", 0) for cfg in first[2]] == [0, 4]  # in that slot's cfg only


def test_schedulers_without_slot_state_never_call_set_processors():
    eng = Recorder(2)
    eng.set_processors = None  # any call would fail
    DecodeScheduler(eng, 2, STOP, sync_every=4).run([_seg(10, 4), _seg(20, 6, bans=((1,), ()))], lambda s, ids: None, do_sample=True, **RUN)
    assert {c[0] for c in eng.calls} <= {"prefill", "decode", "decode_slots", "set_bans"}


class BeamRecorder:
    def __init__(self, max_batch):
        self.max_batch, self.calls, self.steps = max_batch, [], {}

    def prefill(self, b, embeds, pad):
        self.calls.append(("prefill", b, int(embeds[0, 0])))

    def set_processors(self, b, state):
        self.calls.append(("set_processors", b, state))

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


def test_beam_scheduler_installs_the_slot_state_on_the_groups_first_slot():
    a, b = dict(table=[((5, 6), NEG)], forced_eos=()), dict(table=[], forced_eos=(STOP,))
    segs = [_seg(10, 8, sampler=dict(renormalize_logits=True), processors=a), _seg(20, 4), _seg(30, 3, sampler=dict(forced_eos_step=3), processors=b)]
    eng = BeamRecorder(6)
    BeamGroupScheduler(eng, 3, sync_every=4).run(segs, lambda s, ids, score: None, length_penalty=0.0, **RUN)
    calls = eng.calls
    # group 0 <- 10 (slot 0), group 1 <- 20 (slot 3), then 30 refills group 1
    assert [c for c in calls if c[0] == "set_processors"] == [("set_processors", 0, a), ("set_processors", 3, b)]
    for i, c in enumerate(calls):
        if c[0] == "set_processors":
            assert calls[i - 1][:2] == ("prefill", c[1]) and calls[i + 1][0] == "begin"
    groups = [c for c in calls if c[0] == "beam_decode_groups"]
    assert groups and all(c[2][0].get("renormalize_logits") is True for c in groups)
    assert any(c[2][1].get("forced_eos_step") == 3 for c in groups) and not any("forced_eos_step" in c[2][0] for c in groups)
