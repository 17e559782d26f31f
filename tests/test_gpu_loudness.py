"""The measurement and the gating / gain kernels of the output stage's level control (csrc/output.hip, `output.measure_levels`) against
the fp64 twin of tests/loudness_ref.py, on the smallest programmes at which they can go wrong.

Tolerances.  Hop energies: |e - e_twin| <= 1e-9 max_k e_twin -- fp64 roundoff 1.1e-16 times the recursion's noise gain, at most
1 / (1 - r)^2 = 4e4, plus the tail the run-in leaves, at most 1e-10: about 5e-12, two orders under the bound (with a run-in of ONE
hop the 45 Hz tone below misses it at 1.2e-9: every chunk of a tone errs the same way; the kernel runs in over a hop and a half).  Peak: equal.
L within 1e-6 dB, the gain within 2 ulp (fp32) of the twin's fp64 gain rounded to fp32, flags equal."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RATES = [8000, 11025, 22050, 48000]
E_TOL, L_TOL = 1e-9, 1e-6


def _measure(x, progs, rates, targets, ceilings):
    """-> per programme (energy fp64 [hops], hop peaks fp32 [hops], record): one `measure_levels` call for all of them."""
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    plan = O.LevelPlan([(rows, extent, fs, t, c) for (rows, extent), fs, t, c in zip(progs, rates, targets, ceilings)], dev)
    energy, hop_peak, records, gains = O.measure_levels(torch.from_numpy(x).to(dev), plan)
    energy, hop_peak, gains = energy.cpu().numpy(), hop_peak.cpu().numpy(), gains.cpu().numpy()
    recs = O.read_records(records, plan.n)
    assert np.array_equal(recs["gain"], gains)  # the gain the conversion reads is the record's
    return [(energy[s:s + h].copy(), hop_peak[s:s + h].copy(), recs[q]) for q, (s, h, _) in enumerate(plan.hops)]


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _check(got, segments, gap, fs, target, ceiling, worst):
    """One programme's device numbers against the twin; -> the twin's (e, L, flags)."""
    import loudness_ref as LR
    from voice_tts_amd import output as O

    energy, hop_peak, rec = got
    H = O.hop_len(fs)
    prog = LR.lay_out(segments, gap)
    e = LR.hop_energies(prog, fs)
    assert energy.size == -(-prog.size // H) and e.size == prog.size // H
    if e.size:
        err = np.abs(energy[:e.size] - e).max()
        assert err <= E_TOL * e.max(), (fs, err, e.max())  # (silence: exact zeros)
        if e.max() > 0:
            worst.append(err / e.max())
    p = float(np.abs(prog).max()) if prog.size else 0.0
    assert float(rec["peak"]) == p and (hop_peak.max() if hop_peak.size else 0.0) == p
    L = LR.integrated(e, H)
    g, flags = LR.gain(L, p, target, ceiling)
    assert int(rec["flags"]) == flags and int(rec["blocks"]) == max(e.size - 3, 0)
    if L is None:
        assert math.isnan(rec["lufs"])
    else:
        assert abs(float(rec["lufs"]) - L) <= L_TOL, (fs, float(rec["lufs"]), L)
    assert _ulps(rec["gain"], np.float32(g)) <= 2, (fs, float(rec["gain"]), g)
    return e, L, flags


@pytest.mark.parametrize("fs", RATES)
def test_edge_shapes_against_the_twin(fs):
    import loudness_ref as LR
    from voice_tts_amd import output as O

    H = O.hop_len(fs)
    C = -(-H // 64) | 1  # samples of one lane's chunk
    gap = O.gap_len(fs, 200)
    tone = (20000.0 * np.sin(2 * np.pi * 45.0 * np.arange(5 * H) / fs + 1.0)).astype(np.float32)
    assert abs(tone[-1]) > 2000  # the tone ends at a hop's end, away from a zero crossing
    shapes = {
        "shorter than one hop": ([LR.noise(H - 1, fs, 1)], 0, -23.0, -1.0),
        "exactly 4 hops": ([LR.noise(4 * H, fs, 2)], 0, -23.0, -1.0),
        "4 hops + 1 sample": ([LR.noise(4 * H + 1, fs, 3)], 0, -16.0, None),
        "no multiple of the chunk": ([LR.noise(6 * H + C + 1, fs, 4)], 0, -30.0, -1.0),
        "three rows, gaps, an empty row": ([LR.noise(H + 13, fs, 5), LR.noise(0, fs, 6), LR.noise(2 * H + 5, fs, 7), LR.noise(3 * H // 2, fs, 8)], gap, -23.0, -3.0),
        "rows that start and end inside a chunk": ([LR.noise(2 * H + C // 2, fs, 9), LR.noise(3 * H + 2 * C - 1, fs, 10)], C + C // 2 + 2, None, -12.0),
        "45 Hz tone cut off before a gap": ([tone, LR.noise(3 * H, fs, 11)], 3 * H + 5, -23.0, -1.0),
        "loud: the ceiling binds": ([LR.noise(5 * H, fs, 12, rms=6000.0)], 0, -8.0, -6.0),
        "silence": ([np.zeros(5 * H, np.float32)], 0, -23.0, -1.0),
    }
    x, progs = LR.pack([(segs, g) for segs, g, _, _ in shapes.values()])
    got = _measure(x, progs, [fs] * len(shapes), [s[2] for s in shapes.values()], [s[3] for s in shapes.values()])
    worst, seen = [], {}
    for name, out, (segs, g, target, ceiling) in zip(shapes, got, shapes.values()):
        seen[name] = _check(out, segs, g, fs, target, ceiling, worst) + (out,)
    print(f"loudness {fs} Hz: largest |e - e_twin| / max e = {max(worst):.3e}")
    # what each shape is there for
    assert seen["shorter than one hop"][1] is None and float(seen["shorter than one hop"][3][2]["gain"]) == 1.0
    assert seen["shorter than one hop"][2] == LR.NO_BLOCK
    assert seen["exactly 4 hops"][0].size == 4 and int(seen["exactly 4 hops"][3][2]["blocks"]) == 1 and seen["exactly 4 hops"][1] is not None
    assert seen["4 hops + 1 sample"][0].size == 4 and seen["4 hops + 1 sample"][3][0].size == 5 and int(seen["4 hops + 1 sample"][3][2]["blocks"]) == 1
    assert seen["loud: the ceiling binds"][2] == LR.CEILING_BOUND
    assert seen["silence"][2] == LR.NO_BLOCK and float(seen["silence"][3][2]["gain"]) == 1.0 and float(seen["silence"][3][2]["peak"]) == 0.0
    segs, g = shapes["rows that start and end inside a chunk"][:2]
    assert len(segs[0]) % H % C and (len(segs[0]) + g) % H % C  # the first row ends, the second starts, inside a lane's chunk of its hop
    # the tone rings on into the gap: the hops that lie wholly inside it carry energy, as the twin's do -- a filter run per row, or
    # restarted at a row's end, would leave exact zeros there.  (The ringing dies with e^(-2 pi 38 t): the first hop of the gap has
    # nearly all of it, the second 1e-20 of that.)
    e, _, _, (energy, _, _) = seen["45 Hz tone cut off before a gap"]
    assert e[5] > 1e-4 * e.max() and energy[5] > 1e-4 * e.max() and e[6] > 0 and energy[6] > 0
    assert np.abs(energy[5:8] - e[5:8]).max() <= E_TOL * e.max()


def test_five_requests_of_one_launch_equal_their_own_launches_bit_for_bit():
    import loudness_ref as LR
    from voice_tts_amd import output as O

    rates = [8000, 48000, 22050, 11025, 8000]
    targets = [-23.0, -16.0, None, -30.0, -9.0]
    ceilings = [-1.0, -1.0, -9.0, None, -2.0]
    progs = []
    for k, fs in enumerate(rates):
        H = O.hop_len(fs)
        progs.append(([LR.noise(2 * H + 31 * k + 7, fs, 20 + k), LR.noise(3 * H + 11, fs, 30 + k, rms=2000.0 * (k + 1))], O.gap_len(fs, 150)))
    x, tables = LR.pack(progs)
    together = _measure(x, tables, rates, targets, ceilings)
    worst = []
    for k, (fs, t, c) in enumerate(zip(rates, targets, ceilings)):
        _check(together[k], progs[k][0], progs[k][1], fs, t, c, worst)
        xa, ta = LR.pack([progs[k]], lead=k)  # alone, at another offset of its buffer
        (energy, hop_peak, rec), = _measure(xa, ta, [fs], [t], [c])
        assert energy.tobytes() == together[k][0].tobytes() and hop_peak.tobytes() == together[k][1].tobytes()
        assert rec.tobytes() == together[k][2].tobytes()
    assert len({int(r[2]["flags"]) for r in together}) > 1  # some bound by their ceiling, some not


def test_bad_tables_are_refused_or_skipped():
    import ctypes as C

    from voice_tts_amd import _lib
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    with pytest.raises(ValueError):
        O.LevelPlan([([(0, 10, 0), (10, 10, 5)], 30, 8000, -23.0, -1.0)], dev)  # overlapping rows
    with pytest.raises(ValueError):
        O.LevelPlan([([(0, 10, 25)], 30, 8000, -23.0, -1.0)], dev)  # a row that leaves its programme
    L = _lib.lib()
    x = torch.zeros(8, device=dev)
    rc = L.ixtts_loudness_measure(C.c_void_p(x.data_ptr()), 8, None, 0, None, None, 1, 1, None, None, 1, None)
    assert rc == -1 and b"null" in L.ixtts_last_error()
    # a source range outside the input reads as silence, a hop slot outside the arrays is not written
    plan = O.LevelPlan([([(4, 100, 0)], 4000, 8000, -23.0, -1.0)], dev)
    energy, hop_peak, records, gains = O.measure_levels(x, plan)
    assert not energy.any() and not hop_peak.any() and float(gains[0]) == 1.0
    assert int(O.read_records(records, 1)[0]["flags"]) == _lib.LOUDNESS_NO_BLOCK
