"""Two spellings of the same work in the output stage give the same bytes: the assemble kernel with a gain table nobody indexes
against the one without (one kernel body, `GAIN` on and off), and a `LevelPlan` built without `limits=` against the one built with
("sample", False) for every programme (one table layout)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("enc", ["pcm_s16le", "mulaw", "alaw"])
def test_rows_without_a_gain_give_the_bytes_of_pcm_assemble(enc):
    """Rows of n = 0, 1, 3, 4, 5 (and 4 again: the 16-byte load where src is a multiple of 4, the one-by-one path where it is not),
    src = 0 .. 3 (mod 4), gaps of 1 and 7, totals = 1, 2, 3 (mod 4): the last thread's partial store."""
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    x = ((torch.rand(64, generator=torch.Generator().manual_seed(3)) * 2 - 1) * 40000).float().to(dev)  # (beyond int16: the clamp as well)
    gains = torch.tensor([0.5, 2.0], dtype=torch.float32, device=dev)  # a gain that reached a sample would change its code
    lens, srcs = [0, 1, 3, 4, 5, 4, 4, 4, 5], [0, 1, 2, 7, 12, 16, 21, 26, 31]
    assert {s % 4 for s in srcs} == {0, 1, 2, 3} and all(s + n <= x.numel() for s, n in zip(srcs, lens))
    rows, d = [], 0
    for k, (s, n) in enumerate(zip(srcs, lens)):
        rows.append((s, n, d))
        d += n + (1 if k % 2 else 7)
    totals = (d, d + 1, d + 2)  # (d: behind the last row's gap)
    assert [t % 4 for t in totals] == [1, 2, 3]
    for total in totals:
        plain = O.pcm_assemble(x, rows, total, enc).cpu().numpy()
        assert (plain != O.ZERO_CODES[enc]).any()
        for gi in (-1, 2, 5):  # no index, the first index past the table, one further out
            got = O.pcm_assemble_gain(x, [r + (gi,) for r in rows], total, enc, gains).cpu().numpy()
            assert got.dtype == plain.dtype and got.tobytes() == plain.tobytes(), (total, gi)


def test_a_plan_without_limits_is_the_plan_of_sample_mode_without_limiter():
    """8000, 11 025 and 48 000 Hz: a programme shorter than a hop, one of a hop and a sample, one of five hops."""
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    lens = [O.hop_len(8000) - 300, O.hop_len(11025) + 1, 5 * O.hop_len(48000)]
    x = ((torch.rand(sum(lens), generator=torch.Generator().manual_seed(4)) * 2 - 1) * 20000).float().to(dev)
    progs, s = [], 0
    for n, rate, loud, peak in zip(lens, (8000, 11025, 48000), (-23.0, None, -20.0), (-1.0, -3.0, None)):
        progs.append(([(s, n, 0)], n, rate, loud, peak))
        s += n
    a = O.LevelPlan(progs, dev)
    b = O.LevelPlan(progs, dev, limits=[("sample", False)] * len(progs))
    for p in (a, b):
        assert p.n == 3 and p.n2 == 0 and p.limited == [] and p.lim_total == 0 and p.partial_slots == 0 and [h[1] for h in p.hops] == [1, 2, 5]
        assert p.lreqs.numel() == p.ceilings.numel() == p.tables.numel() == 0 and p.modes.tolist() == [0, 0, 0]
    outs = [[t.cpu().numpy().tobytes() for t in O.measure_levels(x, p)] for p in (a, b)]
    for name, u, v in zip(("energy", "hop_peak", "records", "gains"), *outs):
        assert len(u) > 0 and u == v, name
    with pytest.raises(ValueError, match="interpolator"):
        O.true_peaks(x, a)
