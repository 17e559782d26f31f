"""CPU: how the batched vocoder pass groups its rows (`plan_vocoder_batches`) and how `pipeline.vocode_many` drives a vocoder --
one `forward_many` call per group, the per-mel loop for a vocoder without one, and a failure confined to the mel that caused it."""
import random

import pytest
import torch

from voice_tts_amd.bigvgan import plan_vocoder_batches
from voice_tts_amd.pipeline import vocode, vocode_many


@pytest.mark.parametrize("seed", range(6))
def test_plan_covers_every_row_once_within_the_cap(seed):
    rng = random.Random(seed)
    n = rng.randint(0, 40)
    frames = [rng.choice([0, 1, 86, 258, 258, 700, 1892, 5000]) + rng.randint(0, 3) for _ in range(n)]
    cap = rng.choice([1, 300, 2048, 4096])
    groups = plan_vocoder_batches(frames, cap)
    assert sorted(i for g in groups for i in g) == list(range(n))  # every index exactly once
    assert all(g for g in groups)
    for g in groups:
        if len(g) > 1:
            assert len(g) * max(frames[i] for i in g) <= cap, (g, cap)
    for i, f in enumerate(frames):  # an over-long row stands alone
        if f > cap:
            assert [i] in groups
    flat = [frames[i] for g in groups for i in g]
    assert flat == sorted(frames)  # rows sorted by length, so a group pads little


def test_plan_examples():
    assert plan_vocoder_batches([], 100) == []
    assert plan_vocoder_batches([258] * 16, 4096) == [list(range(15)), [15]]  # 15 x 258 = 3870 <= 4096 < 16 x 258
    assert plan_vocoder_batches([1892, 86, 1892], 4096) == [[1, 0], [2]]     # 2 x 1892 fits, 3 x 1892 would not
    assert plan_vocoder_batches([5000, 10], 4096) == [[1], [0]]


class _Stub:
    """wav = the mel's first channel repeated `up` times per frame, scaled: enough to tell rows and their order apart."""
    device_ = torch.device("cpu")
    up = 4

    def __init__(self):
        self.calls = []

    def __call__(self, mel):
        self.calls.append(("forward", mel.shape[-1]))
        if bool((mel > 50).any()):
            raise ValueError("bad mel")
        return mel[:, :1, :].repeat_interleave(self.up, dim=2) * 1e-3


class _ManyStub(_Stub):
    def forward_many(self, mels):
        self.calls.append(("many", [m.shape[-1] for m in mels]))
        if any(bool((m > 50).any()) for m in mels):
            raise ValueError("bad mel in the group")
        return [m[:, :1, :].repeat_interleave(self.up, dim=2) * 1e-3 for m in mels]


def _mels(lengths, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(1, 80, f, generator=g) for f in lengths]


def test_vocode_many_one_call_per_group_in_input_order(monkeypatch):
    monkeypatch.delenv("IXTTS_BV_BATCH", raising=False)
    monkeypatch.setenv("IXTTS_BV_BATCH_FRAMES", "40")
    lengths = [12, 30, 5, 7, 19]
    mels = _mels(lengths)
    stub = _ManyStub()
    outs = vocode_many(stub, mels)
    # sorted 5 7 12 | 19 30?  (3 x 12 = 36 <= 40, 4 x 19 > 40; 2 x 30 > 40): groups [5, 7, 12], [19], [30]
    assert stub.calls == [("many", [5, 7, 12]), ("many", [19]), ("many", [30])]
    ref = _Stub()
    for mel, out in zip(mels, outs):
        assert torch.equal(out, vocode(ref, mel))


def test_vocode_many_without_forward_many_or_switched_off(monkeypatch):
    monkeypatch.delenv("IXTTS_BV_BATCH", raising=False)
    mels = _mels([3, 9, 4])
    plain = _Stub()
    outs = vocode_many(plain, mels)
    assert plain.calls == [("forward", 3), ("forward", 9), ("forward", 4)]
    assert all(torch.equal(o, vocode(_Stub(), m)) for o, m in zip(outs, mels))
    monkeypatch.setenv("IXTTS_BV_BATCH", "0")
    many = _ManyStub()
    outs0 = vocode_many(many, mels)
    assert many.calls == [("forward", 3), ("forward", 9), ("forward", 4)]
    assert all(torch.equal(a, b) for a, b in zip(outs, outs0))
    assert vocode_many(_ManyStub(), []) == []


def test_vocode_many_failure_lands_on_the_offending_mel_only(monkeypatch):
    monkeypatch.delenv("IXTTS_BV_BATCH", raising=False)
    monkeypatch.setenv("IXTTS_BV_BATCH_FRAMES", "40")
    mels = _mels([12, 30, 5, 7, 19])
    mels[3] = mels[3] + 100.0  # the 7-frame mel is bad: its group [5, 7, 12] raises and is redone mel by mel
    stub = _ManyStub()
    outs = vocode_many(stub, mels)
    assert stub.calls == [("many", [5, 7, 12]), ("forward", 5), ("forward", 7), ("forward", 12), ("many", [19]), ("many", [30])]
    assert isinstance(outs[3], ValueError) and str(outs[3]) == "bad mel"
    for i in (0, 1, 2, 4):
        assert torch.equal(outs[i], vocode(_Stub(), mels[i]))


def test_hotpath_has_vocode_many():
    from voice_tts_amd.pipeline import HotPath

    assert callable(HotPath.vocode_many)
