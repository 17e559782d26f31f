"""The two schedulers with their refill rounds as one `prefill_many` (`batch_prefill=True`) against one `prefill` per slot
(`False`) on the 32-slot tiny bf16 engine: every segment's ids identical, fewer prefill calls."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def e32(dev):
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    W = WR.make_gpt_weights(cfg, seed=5, head_scale=50.0)
    W["mel_head.bias"] = W["mel_head.bias"].clone()
    W["mel_head.bias"][8193] += 24.0  # eos reachable: some sequences finish early and their slots are refilled out of step
    return cfg, GptEngine(cfg, dtype="bf16", max_seq=192, max_batch=32, device=dev).load_state_dict(W)


def _segments(n, dev):
    from voice_tts_amd.scheduler import Segment

    g = torch.Generator().manual_seed(91)
    segs = []
    for i in range(n):
        rows, pad, new = 8 + (7 * i) % 31, i % 4, 6 + (11 * i) % 37
        e = torch.randn(rows, 128, generator=g) * 0.5
        e[:pad] = 0
        segs.append(Segment(0, i, e.to(dev), pad, new))
    return segs


def test_decode_scheduler_40_segments_batched_refills_same_ids(e32, dev):
    from voice_tts_amd.scheduler import DecodeScheduler

    cfg, eng = e32
    segs = _segments(40, dev)
    out, stats = {}, {}
    for batch in (False, True):
        got = {}
        sch = DecodeScheduler(eng, 32, cfg["stop_mel_token"], sync_every=8, batch_prefill=batch)
        stats[batch] = dict(sch.run(segs, lambda seg, ids: got.__setitem__(seg.index, np.asarray(ids).tolist()), repetition_penalty=10.0))
        out[batch] = got
    assert out[True] == out[False] and len(out[False]) == 40
    assert len({tuple(v) for v in out[False].values()}) > 30
    assert stats[True]["prefill_seqs"] == stats[False]["prefill_seqs"] == 40
    assert stats[True]["prefill_calls"] < stats[False]["prefill_calls"] == 40
    assert stats[True]["refills"] == stats[False]["refills"] >= 8


def test_beam_scheduler_13_segments_on_10_groups_batched_refills_same_ids(e32, dev):
    from voice_tts_amd.scheduler import BeamGroupScheduler

    cfg, eng = e32
    segs = _segments(13, dev)
    out, stats = {}, {}
    for batch in (False, True):
        got = {}
        sch = BeamGroupScheduler(eng, 3, sync_every=8, batch_prefill=batch)
        assert sch.max_groups == 10
        stats[batch] = dict(sch.run(segs, lambda seg, ids, sc: got.__setitem__(seg.index, (np.asarray(ids).tolist(), float(sc))), seed=5))
        out[batch] = got
    assert out[True] == out[False] and len(out[False]) == 13
    assert stats[True]["prefill_seqs"] == stats[False]["prefill_seqs"] == 13
    assert stats[True]["prefill_calls"] < stats[False]["prefill_calls"] == 13
