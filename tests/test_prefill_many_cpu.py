"""CPU side of the batched prefill: the pass rule (`ixtts_gpt_prefill_plan`, pure host arithmetic) and the schedulers' refill
rounds over fake engines that record their calls."""
import numpy as np
import pytest
import torch

from voice_tts_amd.gpt_engine import GptEngine
from voice_tts_amd.scheduler import BeamGroupScheduler, DecodeScheduler, Segment, resolve_batch_prefill

STOP = 8193


# --------------------------------------------------------------------------------------------------------------------- the plan
def test_plan_closes_a_pass_when_the_next_sequence_does_not_fit():
    assert GptEngine.prefill_plan([136, 136, 136], [0, 0, 0], 300) == ([0, 0, 1], 2)  # T = 137 each
    assert GptEngine.prefill_plan([136, 136, 136], [0, 0, 0], 411) == ([0, 0, 0], 1)
    assert GptEngine.prefill_plan([136, 136, 136], [0, 0, 0], 410) == ([0, 0, 1], 2)


def test_plan_subtracts_padding_before_the_cap():
    assert GptEngine.prefill_plan([136, 136, 136], [0, 111, 0], 300) == ([0, 0, 0], 1)  # 137 + 26 + 137 = 300
    assert GptEngine.prefill_plan([136, 136, 136], [0, 110, 0], 300) == ([0, 0, 1], 2)


def test_plan_gives_a_sequence_of_the_whole_cap_a_pass_of_its_own():
    assert GptEngine.prefill_plan([9, 99, 9], [0, 0, 0], 100) == ([0, 1, 2], 3)
    assert GptEngine.prefill_plan([99], [0], 100) == ([0], 1)


def test_plan_keeps_the_order_and_returns_the_pass_count():
    rows = [50, 10, 60, 5, 5, 80, 1]
    passes, n = GptEngine.prefill_plan(rows, [0] * 7, 100)  # T: 51 11 61 6 6 81 2
    assert passes == [0, 0, 1, 1, 1, 2, 2] and n == 3
    assert passes == sorted(passes)  # a later entry never lands in an earlier pass: nothing is re-ordered to fill one up
    assert GptEngine.prefill_plan([], [], 100) == ([], 0)


def test_plan_of_the_gpu_tests_edges_case_is_two_passes():
    """tests/test_gpu_prefill_many.py, EDGES at max_seq 640: 727 packed rows, so the default plan has to cut the call in two"""
    edges = [(1, 0), (63, 0), (64, 0), (127, 0), (128, 0), (200, 0), (40, 3), (100, 70), (130, 64), (9, 8)]
    assert sum(r + 1 - p for r, p in edges) == 727 > 640
    passes, n = GptEngine.prefill_plan([r for r, _ in edges], [p for _, p in edges], 640)
    assert n == 2 and passes == [0] * 7 + [1] * 3  # 2 + 64 + 65 + 128 + 129 + 201 + 38 = 627; 31 more would make 658


# --------------------------------------------------------------------------------------------------------------- the schedulers
def _seg(tag, max_new, pad=0, **kw):
    return Segment(0, tag, torch.full((4 + tag % 3, 2), float(tag)), pad, max_new, **kw)


class Fake:
    """Records every call; a sequence's ids are zeros (nothing ever stops early)."""

    def __init__(self, max_batch):
        self.max_batch, self.calls, self.steps = max_batch, [], {}

    def prefill(self, b, embeds, pad):
        self.calls.append(("prefill", b, int(embeds[0, 0])))
        self.steps[b] = 0

    def set_bans(self, b, suppress_tokens=(), begin_suppress_tokens=()):
        self.calls.append(("set_bans", b))

    def set_processors(self, b, state):
        self.calls.append(("set_processors", b))

    def decode(self, n_active, n_steps, **kw):
        self.calls.append(("decode", n_active, n_steps))
        for b in range(n_active):
            self.steps[b] = self.steps.get(b, 0) + n_steps

    def read(self, b):
        return np.zeros(self.steps[b], np.int32), False

    def beam_begin(self, nb, group=0, rng_stream=0):
        self.calls.append(("begin", group, rng_stream))
        self.gsteps = getattr(self, "gsteps", {})
        self.gsteps[group] = 0

    def beam_park(self, group):
        self.calls.append(("park", group))

    def beam_decode(self, n_steps, groups=1, **kw):
        self.calls.append(("beam_decode", n_steps, groups))
        for g in range(groups):
            self.gsteps[g] = self.gsteps.get(g, 0) + n_steps

    def beam_read(self, max_new, group=0):
        return np.zeros(min(self.gsteps[group], max_new), np.int32), False, 0.0


class FakeMany(Fake):
    def prefill_many(self, entries, rows_max=0):
        self.calls.append(("prefill_many", [(b, int(e[0, 0]), pad) for b, e, pad in entries]))
        for b, _, _ in entries:
            self.steps[b] = 0


def _rounds(calls):
    """the per-slot prefill calls grouped into refill rounds (a round ends at the next decode call)"""
    out, cur = [], []
    for c in calls:
        if c[0] == "prefill":
            cur.append((c[1], c[2]))
        elif c[0] in ("decode", "beam_decode") and cur:
            out.append(cur)
            cur = []
    return out


SEGS = [(10, 9), (11, 3), (12, 6), (13, 3), (14, 5), (15, 2), (16, 7)]


def _decode_segs():
    return [_seg(t, n, pad=t % 2, bans=((3,), ()) if t % 2 else None, processors=dict(table=(), forced_eos=(5,)) if t % 3 == 0 else None) for t, n in SEGS]


def test_decode_scheduler_one_prefill_many_per_round_holds_what_the_loop_would_fill():
    serial, many = Fake(3), FakeMany(3)
    st_s = DecodeScheduler(serial, 3, STOP, sync_every=4, batch_prefill=False).run(_decode_segs(), lambda s, ids: None)
    st_m = DecodeScheduler(many, 3, STOP, sync_every=4, batch_prefill=True).run(_decode_segs(), lambda s, ids: None)
    rounds = _rounds(serial.calls)
    got = [c[1] for c in many.calls if c[0] == "prefill_many"]
    assert [[(b, tag) for b, tag, _ in r] for r in got] == rounds and len(rounds) > 2 and len(rounds[0]) == 3
    assert all(pad == tag % 2 for r in got for _, tag, pad in r)
    assert all([b for b, _, _ in r] == sorted(b for b, _, _ in r) for r in got)  # slot order
    assert not any(c[0] == "prefill" for c in many.calls)
    # the slot-state calls of a round come after its prefill_many, in slot order, and are the serial run's
    state = lambda calls: [c for c in calls if c[0] in ("set_bans", "set_processors")]
    assert state(many.calls) == state(serial.calls) and len(state(serial.calls)) >= 5
    last = None
    for c in many.calls:
        if c[0] == "prefill_many":
            last = {b for b, _, _ in c[1]}
        elif c[0] in ("set_bans", "set_processors"):
            assert last is not None and c[1] in last
        elif c[0] == "decode":
            last = None
    assert [c for c in many.calls if c[0] == "decode"] == [c for c in serial.calls if c[0] == "decode"]
    assert st_s["prefill_seqs"] == st_m["prefill_seqs"] == len(SEGS)
    assert st_s["prefill_calls"] == len(SEGS) and st_m["prefill_calls"] == len(got) < len(SEGS)
    assert {k: v for k, v in st_s.items() if k != "prefill_calls"} == {k: v for k, v in st_m.items() if k != "prefill_calls"}


def test_beam_scheduler_one_prefill_many_per_round_then_bans_and_begin():
    serial, many = Fake(9), FakeMany(9)
    mk = lambda: [_seg(t, n, bans=((3,), ()) if t % 2 else None) for t, n in SEGS]
    st_s = BeamGroupScheduler(serial, 3, sync_every=4, batch_prefill=False).run(mk(), lambda s, ids, sc: None)
    st_m = BeamGroupScheduler(many, 3, sync_every=4, batch_prefill=True).run(mk(), lambda s, ids, sc: None)
    rounds = _rounds(serial.calls)
    got = [c[1] for c in many.calls if c[0] == "prefill_many"]
    assert [[(b, tag) for b, tag, _ in r] for r in got] == rounds and len(rounds[0]) == 3
    assert all(b % 3 == 0 for r in got for b, _, _ in r)  # the groups' first slots
    pick = lambda calls: [c for c in calls if c[0] in ("set_bans", "begin", "park", "beam_decode")]
    assert pick(many.calls) == pick(serial.calls)
    pending = []
    for c in many.calls:
        if c[0] == "prefill_many":
            assert not pending
            pending = [b // 3 for b, _, _ in c[1]]
        elif c[0] == "begin":
            assert pending and c[1] == pending.pop(0)  # every begin follows its round's prefill_many, in group order
        elif c[0] == "beam_decode":
            assert not pending
    assert st_s["prefill_seqs"] == st_m["prefill_seqs"] == len(SEGS)
    assert st_m["prefill_calls"] == len(got) < st_s["prefill_calls"] == len(SEGS)


def test_an_engine_without_prefill_many_gets_the_per_slot_calls():
    runs = []
    for eng, batch in ((Fake(3), True), (Fake(3), False), (FakeMany(3), False)):
        st = DecodeScheduler(eng, 3, STOP, sync_every=4, batch_prefill=batch).run(_decode_segs(), lambda s, ids: None)
        assert not any(c[0] == "prefill_many" for c in eng.calls)
        assert st["prefill_calls"] == st["prefill_seqs"] == len(SEGS)
        runs.append(eng.calls)
    assert runs[0] == runs[1] == runs[2]
    # ... a slot's state calls directly behind its own prefill, as ever
    for i, c in enumerate(runs[0]):
        if c[0] == "set_bans":
            assert runs[0][i - 1] [0] == "prefill" and runs[0][i - 1][1] == c[1]
    beam = []
    for eng, batch in ((Fake(9), True), (FakeMany(9), False)):
        BeamGroupScheduler(eng, 3, sync_every=4, batch_prefill=batch).run([_seg(t, n) for t, n in SEGS], lambda s, ids, sc: None)
        beam.append(eng.calls)
    assert beam[0] == beam[1] and beam[0][0][0] == "prefill" and beam[0][1][0] == "begin"


def test_switch_resolution(monkeypatch):
    from voice_tts_amd import scheduler

    monkeypatch.delenv("IXTTS_PREFILL_BATCH", raising=False)
    assert resolve_batch_prefill() is scheduler.BATCH_PREFILL_DEFAULT
    assert DecodeScheduler(Fake(2), 2, STOP).batch_prefill is scheduler.BATCH_PREFILL_DEFAULT
    for env, want in (("1", True), ("0", False)):
        monkeypatch.setenv("IXTTS_PREFILL_BATCH", env)
        assert resolve_batch_prefill() is want
        assert DecodeScheduler(Fake(2), 2, STOP).batch_prefill is want
        assert BeamGroupScheduler(Fake(6), 3).batch_prefill is want
        # the keyword wins over the variable
        assert DecodeScheduler(Fake(2), 2, STOP, batch_prefill=not want).batch_prefill is (not want)
        assert BeamGroupScheduler(Fake(6), 3, batch_prefill=not want).batch_prefill is (not want)
    monkeypatch.setenv("IXTTS_PREFILL_BATCH", "yes")
    with pytest.raises(ValueError, match="IXTTS_PREFILL_BATCH"):
        resolve_batch_prefill()
