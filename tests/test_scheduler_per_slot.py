"""Host logic of per-segment sampler settings and random streams in the two schedulers, against recording engines (no GPU):
without overrides the uniform calls and nothing else; with them one cfg and one stream per slot / one cfg per group with every
decode call, across refills, with the run's defaults under idle slots and parked groups."""
import numpy as np
import torch

from voice_tts_amd.scheduler import BeamGroupScheduler, DecodeScheduler, Segment

STOP = 99
RUN = dict(repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, seed=0, typical_mass=0.0)


class Recorder:
    """Slot b emits its key at every step, STOP after `stop_after[key]` tokens; every call is written down with its arguments."""

    def __init__(self, max_batch, stop_after=None, max_seq=200):
        self.max_batch, self.max_seq, self.stop_after = max_batch, max_seq, stop_after or {}
        self.seq, self.calls = [None] * max_batch, []

    def prefill(self, b, embeds, pad):
        self.seq[b] = dict(key=int(embeds[0, 0]), out=[])
        self.calls.append(("prefill", b, self.seq[b]["key"]))

    def _step(self, n_active, n_steps):
        for b in range(n_active):
            s = self.seq[b]
            for _ in range(n_steps):
                s["out"].append(STOP if len(s["out"]) >= self.stop_after.get(s["key"], 10 ** 6) else s["key"])

    def decode(self, n_active, n_steps, **kw):
        self.calls.append(("decode", n_active, n_steps, kw))
        self._step(n_active, n_steps)

    def decode_slots(self, n_steps, cfgs, streams=None):
        assert streams is None or len(streams) == len(cfgs)
        self.calls.append(("decode_slots", n_steps, [dict(c) for c in cfgs], None if streams is None else list(streams),
                           [self.seq[b]["key"] for b in range(len(cfgs))]))
        self._step(len(cfgs), n_steps)

    def read(self, b):
        out = np.asarray(self.seq[b]["out"], np.int32)
        return out, bool((out == STOP).any())


class OldRecorder(Recorder):
    decode_slots = None  # an engine from before: any call would fail


def _seg(key, max_new, rows=5, **kw):
    e = torch.zeros(rows, 4)
    e[0, 0] = key
    return Segment(request=key // 10, index=key % 10, embeds=e, n_left_pad=0, max_new=max_new, **kw)


def test_without_overrides_only_the_uniform_call_is_made():
    eng = OldRecorder(2, stop_after={11: 3})
    got = {}
    DecodeScheduler(eng, 2, STOP, sync_every=4).run([_seg(11, 10), _seg(12, 6), _seg(21, 5)], lambda s, ids: got.__setitem__(s.index + 10 * s.request, ids.tolist()),
                                                    do_sample=True, **RUN)
    assert got == {11: [11] * 3 + [STOP], 12: [12] * 6, 21: [21] * 5}
    decodes = [c for c in eng.calls if c[0] != "prefill"]
    assert decodes and all(c[0] == "decode" and c[3] == dict(RUN, do_sample=True, suppress_stop=False) for c in decodes)


def test_per_slot_lists_across_a_refill_with_defaults_under_idle_slots():
    hot = dict(temperature=1.2, top_k=50, seed=3, do_sample=True)
    greedy = dict(top_k=1, do_sample=False)
    # longest cap first: 30 takes slot 0, 20 slot 1 (no stream of its own: the slot's), 10 slot 2; 40 refills the slot 10 frees
    segs = [_seg(10, 7, sampler=hot, stream=0), _seg(20, 9), _seg(30, 12, sampler=greedy, stream=5), _seg(40, 5, stream=8)]
    eng = Recorder(3)
    got = {}
    st = DecodeScheduler(eng, 3, STOP, sync_every=4).run(segs, lambda s, ids: got.__setitem__(s.request, ids.tolist()), do_sample=True, **RUN)
    assert got == {1: [10] * 7, 2: [20] * 9, 3: [30] * 12, 4: [40] * 5}  # every cap honoured, unequal as they are
    assert not any(c[0] == "decode" for c in eng.calls)
    base = dict(RUN, do_sample=True, suppress_stop=False)
    want_cfg = {10: dict(base, **hot), 20: base, 30: dict(base, **greedy), 40: base}
    seen_idle = False
    occupant_done = {}
    for c in [c for c in eng.calls if c[0] == "decode_slots"]:
        _, steps, cfgs, streams, keys = c
        for b, key in enumerate(keys):
            live = occupant_done.get(key, 0) < {10: 7, 20: 9, 30: 12, 40: 5}[key]
            if live:
                assert cfgs[b] == want_cfg[key], (key, cfgs[b])
                assert streams[b] == {10: 0, 20: b, 30: 5, 40: 8}[key]
            else:  # its segment was handed back and nothing queued: the run's settings, the slot's own stream
                assert cfgs[b] == base and streams[b] == b
                seen_idle = True
            occupant_done[key] = occupant_done.get(key, 0) + steps
    assert seen_idle and st["refills"] == 1
    # the refill: slot 2 held segment 10 (its own cfg, stream 0), then segment 40 under the run's cfg and stream 8 from its first step
    slot2 = [(c[4][2], c[2][2], c[3][2]) for c in eng.calls if c[0] == "decode_slots" and len(c[4]) > 2]
    assert slot2[0] == (10, dict(base, **hot), 0)
    first40 = next(i for i, x in enumerate(slot2) if x[0] == 40)
    assert first40 == 2 and all(x == (40, base, 8) for x in slot2[first40:])
    assert st["decode_calls"] == len([c for c in eng.calls if c[0] == "decode_slots"])


def test_a_stream_alone_is_an_override_and_fixed_length_reaches_every_entry():
    eng = Recorder(2)
    DecodeScheduler(eng, 2, STOP, sync_every=8).run([_seg(10, 3, stream=7)], lambda s, ids: None, fixed_length=True, **RUN)
    calls = [c for c in eng.calls if c[0] == "decode_slots"]
    assert len(calls) == 1 and calls[0][3] == [7] and calls[0][2] == [dict(RUN, suppress_stop=True)]


class BeamRecorder:
    def __init__(self, max_batch, done_after=None):
        self.max_batch, self.max_seq, self.done_after = max_batch, 200, done_after or {}
        self.slot_key, self.groups, self.calls = {}, {}, []

    def prefill(self, b, embeds, pad):
        self.slot_key[b] = int(embeds[0, 0])

    def beam_begin(self, num_beams, group=0, rng_stream=0):
        self.groups[group] = dict(key=self.slot_key[group * num_beams], n=0, parked=False)
        self.calls.append(("begin", group, self.groups[group]["key"], rng_stream))

    def beam_park(self, group):
        self.groups[group]["parked"] = True

    def _step(self, n_groups, n_steps):
        for g in range(n_groups):
            if not self.groups[g]["parked"]:
                self.groups[g]["n"] += n_steps

    def beam_decode(self, n_steps, groups=1, **kw):
        self.calls.append(("decode", groups, n_steps, kw))
        self._step(groups, n_steps)

    def beam_decode_groups(self, n_steps, cfgs):
        self.calls.append(("decode_groups", n_steps, [dict(c) for c in cfgs], [(self.groups[g]["key"], self.groups[g]["parked"]) for g in range(len(cfgs))]))
        self._step(len(cfgs), n_steps)

    def beam_read(self, max_new, group=0):
        s = self.groups[group]
        n = min(s["n"], self.done_after.get(s["key"], 10 ** 6), max_new)
        return np.full(n, s["key"], np.int32), s["n"] >= self.done_after.get(s["key"], 10 ** 6), -1.0


def test_beam_groups_uniform_without_overrides_per_group_with_them():
    run = dict(RUN, length_penalty=0.0)
    eng = BeamRecorder(6)
    eng.beam_decode_groups = None
    BeamGroupScheduler(eng, 3, sync_every=4).run([_seg(10, 6), _seg(20, 6, stream=9)], lambda s, ids, sc: None, **run)
    assert all(c[3] == dict(run, suppress_stop=False) for c in eng.calls if c[0] == "decode")
    assert [(c[2], c[3]) for c in eng.calls if c[0] == "begin"] == [(10, 0), (20, 9)]  # streams go through beam_begin, as ever

    mine = dict(temperature=1.1, top_k=8, length_penalty=1.0, seed=4)
    eng = BeamRecorder(6, done_after={20: 3})
    got = {}
    BeamGroupScheduler(eng, 3, sync_every=4).run([_seg(10, 10, sampler=mine, stream=2), _seg(20, 9), _seg(30, 12, sampler=dict(do_sample=False))],
                                                 lambda s, ids, sc: got.__setitem__(s.request, len(ids)), **run)
    assert got == {1: 10, 2: 3, 3: 12}
    assert not any(c[0] == "decode" for c in eng.calls)
    assert [(c[2], c[3]) for c in eng.calls if c[0] == "begin"] == [(30, 2), (10, 2), (20, 1)]  # 20 refills group 1 after 10
    base = dict(run, suppress_stop=False)
    want = {10: dict(base, **mine), 20: base, 30: dict(base, do_sample=False)}
    parked_seen = False
    for _, steps, cfgs, who in [c for c in eng.calls if c[0] == "decode_groups"]:
        for cfg, (key, parked) in zip(cfgs, who):
            assert cfg == (base if parked else want[key]), (key, parked, cfg)
            parked_seen |= parked
    assert parked_seen  # group 0 ran out of work while group 1 went on: the run's defaults
