"""The true-peak and the limiter kernels of the output stage (csrc/limiter.hip; `output.true_peaks`, `output.limit`, and the flow of
`output.finish_pcm_many` around them) against the fp64 twin of tests/limiter_ref.py, on the smallest programmes at which they can go
wrong.

Tolerances.  The kernel's gain a differs from the twin's by the order of its fp64 sums alone, about 1e-14 relative; that can flip the
fp32 rounding of a by one ulp, the step toward zero by one more, and the product rounds once: the limited programme is within 3 ulp
(fp32) of the twin's everywhere.  A true hop peak is an fp64 sum of twelve products rounded to fp32 once: within 1 ulp.  The smallest
gain gets the same 1 ulp; the count of limited samples is the twin's.  Bytes are the host conversion of the device's own fp32, exactly."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RATES = [8000, 22050, 48000]
DEV = "cuda:0"


def _spike(n, fs, seed, at, value=32000.0):
    """Quiet noise (far under any ceiling of the tests) with samples `at` set to `value`."""
    import loudness_ref as LR

    x = LR.noise(n, fs, seed, rms=600.0)
    for k, i in enumerate(at):
        x[i] = value if k % 2 == 0 else -value
    return x


def _limit(x, progs, rates, peaks, modes, gains=None):
    """One plan, one `true_peaks` and one `limit` launch for all programmes -> per programme (limited fp32, (smallest, count), hop
    peaks fp32 of its hops)."""
    from voice_tts_amd import output as O

    dev = torch.device(DEV)
    plan = O.LevelPlan([(rows, extent, fs, None, pk) for (rows, extent), fs, pk in zip(progs, rates, peaks)], dev, limits=[(m, True) for m in modes])
    xd = torch.from_numpy(x).to(dev)
    g = None if gains is None else torch.tensor(gains, dtype=torch.float32, device=dev)
    out, stats = O.limit(xd, plan, g)
    peaks_dev = O.true_peaks(xd, plan).cpu().numpy()
    out = out.cpu().numpy()
    assert plan.limited == list(range(len(progs)))
    return [(out[plan.lim_off[q]:plan.lim_off[q] + progs[q][1]].copy(), stats[q], peaks_dev[s:s + h].copy()) for q, (s, h, _) in enumerate(plan.hops)]


def _against_the_twin(got, segments, gap, tail, fs, peak, mode, g, name):
    import limiter_ref as LM

    out, (smallest, count), hop_peaks = got
    x = np.concatenate([LM.lay_out(segments, gap), np.zeros(tail, np.float32)])
    ref = LM.limit(LM.levelled(x, g), fs, peak, mode)
    assert out.size == x.size
    d = LM.ulps(out, ref["out"])
    assert (d.max() if d.size else 0) <= 3, (name, fs, mode, int(d.max()), int(d.argmax()))
    assert count == ref["count"], (name, fs, mode, count, ref["count"])
    assert LM.ulps(smallest, ref["smallest"]) <= 1, (name, fs, mode, float(smallest), float(ref["smallest"]))
    if mode == "true":  # (the hop peaks are those of the programme as it is measured: before the gain)
        tp = LM.hop_true_peaks(x, fs)
        assert hop_peaks.size == tp.size and (LM.ulps(hop_peaks, tp).max() if tp.size else 0) <= 1, (name, fs)
        assert (hop_peaks >= LM.hop_sample_peaks(x, fs)).all()
    else:
        assert not hop_peaks.any()  # a programme in sample mode keeps the slots the measurement filled
    return ref, out


@pytest.mark.parametrize("fs", RATES)
def test_edge_shapes_against_the_twin(fs):
    import loudness_ref as LR
    from voice_tts_amd import _lib
    from voice_tts_amd import output as O

    T, W = _lib.limiter_tile(), O.lookaround(fs)
    assert T == _lib.LIMITER_TILE and T > 4 * W
    N = T + W + 50
    gap = O.gap_len(fs, 20)
    loud = lambda n, seed: LR.noise(n, fs, seed, rms=12000.0)  # noqa: E731
    a, b, c3 = _spike(W + 9, fs, 31, [W + 8]), _spike(0, fs, 32, []), _spike(2 * W + 3, fs, 33, [0, 2 * W + 2])
    shapes = {  # name: (segments, gap, tail, ceiling, gain)
        "shorter than W": ([loud(W - 3, 1)], 0, 0, -1.0, 1.0),
        "exactly T": ([loud(T, 2)], 0, 0, -1.0, 1.25),
        "T + 1": ([loud(T + 1, 3)], 0, 0, -2.0, 1.0),
        "the only peak at 0": ([_spike(N, fs, 4, [0])], 0, 0, -1.0, 1.0),
        "the only peak at N - 1": ([_spike(N, fs, 5, [N - 1])], 0, 0, -2.0, 1.0),
        "the only peak at T - 1": ([_spike(N, fs, 6, [T - 1])], 0, 0, -1.0, 1.0),
        "the only peak at T": ([_spike(N, fs, 7, [T])], 0, 0, -1.0, 0.97),
        "two peaks 2W apart": ([_spike(N, fs, 8, [T - W - 5, T + W - 5])], 0, 0, -1.0, 1.0),
        "two peaks 2W + 1 apart": ([_spike(N, fs, 9, [T - W - 5, T + W - 4])], 0, 0, -1.0, 1.0),
        "three segments, gaps, peaks beside a gap, an empty row": ([a, b, c3, loud(W, 34)], gap, 0, -2.0, 1.1),
        "silence": ([np.zeros(T + 5, np.float32)], 0, 0, -1.0, 1.3),
        "under the ceiling": ([LR.noise(T + 77, fs, 10, rms=600.0)], 0, 0, -1.0, 1.0),
        "a totals tail": ([_spike(T - 30, fs, 11, [T - 31])], 0, 2 * W + 40, -1.0, 1.0),
    }
    x, progs = LR.pack([(segs, g) for segs, g, _, _, _ in shapes.values()])
    progs = [(rows, extent + s[2]) for (rows, extent), s in zip(progs, shapes.values())]
    seen = {}
    for mode in O.PEAK_MODES:
        got = _limit(x, progs, [fs] * len(shapes), [s[3] for s in shapes.values()], [mode] * len(shapes), [s[4] for s in shapes.values()])
        for name, out, (segs, g, tail, peak, gn) in zip(shapes, got, shapes.values()):
            seen[name, mode] = _against_the_twin(out, segs, g, tail, fs, peak, mode, gn, name) + (out[1],)
    for mode in O.PEAK_MODES:
        # what each shape is there for
        for name in ("the only peak at 0", "the only peak at N - 1", "the only peak at T - 1", "the only peak at T"):
            ref, out, (smallest, count) = seen[name, mode]
            at = {"0": 0, "N - 1": N - 1, "T - 1": T - 1, "T": T}[name.split("at ")[1]]
            touched = np.nonzero(ref["a"] < 1.0)[0]
            assert touched.min() <= max(at - 2 * W, 0) and touched.max() >= min(at + 2 * W, N - 1)
            if at in (T - 1, T):  # the halo has to carry r across the tile's edge, in both directions
                assert (ref["a32"][:T] < 1.0).any() and (ref["a32"][T:] < 1.0).any()
            assert count > 0 and smallest < 1.0 and abs(float(out[at])) <= O.ceiling(-2.0 if name.endswith("N - 1") else -1.0) * (1.0 + 2.0 ** -23)
        ref, out, (smallest, count) = seen["silence", mode]
        assert count == 0 and smallest == 1.0 and not out.any() and (ref["a32"] == 1.0).all()
        ref, out, (smallest, count) = seen["under the ceiling", mode]
        assert count == 0 and smallest == 1.0 and out.tobytes() == LR.lay_out(shapes["under the ceiling"][0], 0).tobytes()  # y, bit for bit
        ref, out, _ = seen["a totals tail", mode]
        assert not out[T - 30:].any() and (ref["a"][T - 30:T - 31 + 2 * W] < 1.0).all()  # the gain is reduced over the tail, silence stays silence
        ref, out, _ = seen["three segments, gaps, peaks beside a gap, an empty row", mode]
        assert not out[W + 9:W + 9 + gap].any() and ref["count"] > 0
    # 2W apart: one sample, halfway, has both peaks in its window; 2W + 1 apart: none has, and every sample between them has one
    for name, both in (("two peaks 2W apart", 1), ("two peaks 2W + 1 apart", 0)):
        r, m = seen[name, "sample"][0]["r"], seen[name, "sample"][0]["m"][W:W + N]
        p1, p2 = np.nonzero(r < 1.0)[0]
        assert p2 - p1 == 2 * W + 1 - both and (m[p1:p2 + 1] < 1.0).all()


@pytest.mark.parametrize("peak", [-1.0, -2.0])
def test_bytes_and_the_ceiling(peak):
    """Through `finish_pcm_many`: all three encodings are the host conversion of the device's own limited fp32, gaps and tail carry the
    zero code, no delivered sample passes floor(c), and with the limiter the gating kernel does not give way."""
    import limiter_ref as LM
    import loudness_ref as LR
    from voice_tts_amd import _lib
    from voice_tts_amd import output as O

    dev = torch.device(DEV)
    fs, target = 22050, -10.0
    segs = [LR.noise(6 * 2205 + 17, fs, 40, rms=5000.0), LR.noise(5 * 2205 + 3, fs, 41, rms=2500.0)]
    gap, tail = O.gap_len(fs, 200), 300
    x, ((rows, extent),) = LR.pack([(segs, gap)])
    extent += tail
    c = O.ceiling(peak)
    for mode in O.PEAK_MODES:
        # the low-level path: the gain the gating kernel leaves, then the limiter
        plan = O.LevelPlan([(rows, extent, fs, target, peak)], dev, limits=[(mode, True)])
        xd = torch.from_numpy(x).to(dev)
        _, hop_peak, records, gains = O.measure_levels(xd, plan)
        limited, (stats,) = O.limit(xd, plan, gains)
        limited, rec = limited.cpu().numpy(), O.read_records(records, 1)[0]
        prog = np.concatenate([LR.lay_out(segs, gap), np.zeros(tail, np.float32)])
        L = LR.loudness(prog, fs)
        p = LM.true_peak(prog) if mode == "true" else float(np.abs(prog).max())
        assert LM.ulps(rec["peak"], np.float32(p)) <= 1
        full = 10.0 ** ((target - L) / 20.0)
        assert LR.gain(L, p, target, peak)[1] == LR.CEILING_BOUND  # today the gain gives way here ...
        assert not int(rec["flags"]) & _lib.LOUDNESS_CEILING_BOUND and LM.ulps(rec["gain"], np.float32(full)) <= 2  # ... with the limiter it does not
        ref = LM.limit(LM.levelled(prog, rec["gain"]), fs, peak, mode)
        assert LM.ulps(limited, ref["out"]).max() <= 3 and stats[1] == ref["count"] > 0
        for enc in O.ENCODINGS:
            reports = []
            (sr, pcm), = O.finish_pcm_many([[torch.from_numpy(s).to(dev)[None] for s in segs]], [None], [enc], 200, [target], [peak], reports,
                                           totals=[extent], peak_mode=[mode], limiter=[True])
            pcm = pcm[:, 0]
            assert sr == fs and pcm.size == extent and pcm.tobytes() == LR.encode(limited, enc).tobytes()
            zero = O.ZERO_CODES[enc]
            assert (pcm[len(segs[0]):len(segs[0]) + gap] == zero).all() and (pcm[extent - tail:] == zero).all()
            rep = reports[0]
            assert rep["peak_mode"] == mode and rep["limited"] is True and rep["max_reduction_db"] < 0 and 0 < rep["limited_fraction"] < 1
            assert abs(rep["max_reduction_db"] - 20.0 * math.log10(float(ref["smallest"]))) < 1e-4
            assert rep["limited_fraction"] == ref["count"] / extent
            delivered = LR.loudness(limited, fs)
            assert abs(rep["delivered_lufs"] - delivered) < 1e-6 and rep["target_met"] == (abs(delivered - target) <= O.LOUDNESS_TOLERANCE_LU)
            dp = LM.true_peak(limited) if mode == "true" else float(np.abs(limited).max())
            assert abs(rep["delivered_peak_dbfs"] - 20.0 * math.log10(dp / 32768.0)) < 1e-5 and dp <= c * (1.0 + 1e-4)
            if enc == "pcm_s16le":
                assert int(np.abs(pcm.astype(np.int32)).max()) <= math.floor(c)
        assert int(np.abs(LR.pcm_s16(limited).astype(np.int32)).max()) <= math.floor(c)


def test_requests_of_one_call_equal_their_own_calls_bit_for_bit():
    import loudness_ref as LR
    from voice_tts_amd import output as O

    dev = torch.device(DEV)
    rates = [8000, 48000, None, 16000, 8000, 44100]
    encs = ["mulaw", None, "pcm_s16le", "alaw", "mulaw", "pcm_s16le"]
    loud = [-16.0, -14.0, None, -18.0, -12.0, -20.0]
    peak = [None, -2.0, -3.0, -1.0, -1.0, -1.0]
    mode = ["true", "sample", "true", "true", None, None]
    lim = [True, True, True, None, True, None]  # request 3: true mode without the limiter; request 5: none of the new controls
    wavs = [[torch.from_numpy(LR.noise(5000 + 700 * k + 13 * j, 22050, 50 + 3 * k + j, rms=3000.0 * (1 + k % 3))).to(dev)[None] for j in range(1 + k % 2)]
            for k in range(6)]
    reports = []
    together = O.finish_pcm_many(wavs, rates, encs, 150, loud, peak, reports, peak_mode=mode, limiter=lim)
    assert sorted(reports[5]) == sorted(["measured_lufs", "gain_db", "peak_dbfs_in", "target_met"]) and "limited" in reports[3] and any(r["limited"] for r in reports[:5])
    for k in range(6):
        own = []
        (sr, pcm), = O.finish_pcm_many([wavs[k]], [rates[k]], [encs[k]], 150, [loud[k]], [peak[k]], own, peak_mode=[mode[k]], limiter=[lim[k]])
        assert sr == together[k][0] and pcm.dtype == together[k][1].dtype and pcm.tobytes() == together[k][1].tobytes(), k
        assert own[0] == reports[k], k
    # the request without a new control: the bytes and the report of a call without the new arguments
    old = []
    (sr, pcm), = O.finish_pcm_many([wavs[5]], [rates[5]], [encs[5]], 150, [loud[5]], [peak[5]], old)
    assert pcm.tobytes() == together[5][1].tobytes() and old[0] == reports[5]
    # the low-level launches: five programmes of different rates and modes in one plan, and each in its own, at another offset
    progs = [([LR.noise(1500 + 211 * k, fs, 70 + k, rms=9000.0), LR.noise(900 + 5 * k, fs, 80 + k, rms=4000.0)], O.gap_len(fs, 30))
             for k, fs in enumerate([8000, 48000, 22050, 16000, 8000])]
    fss, modes, peaks = [8000, 48000, 22050, 16000, 8000], ["true", "sample", "true", "sample", "true"], [-1.0, -2.0, -6.0, -1.0, -3.0]

    def run(x, tables, sel):
        plan = O.LevelPlan([(rows, extent, fss[k], -14.0, peaks[k]) for (rows, extent), k in zip(tables, sel)], dev, limits=[(modes[k], True) for k in sel])
        xd = torch.from_numpy(x).to(dev)
        _, hop_peak, records, gains = O.measure_levels(xd, plan)
        out, stats = O.limit(xd, plan, gains)
        out, hop_peak, recs = out.cpu().numpy(), hop_peak.cpu().numpy(), O.read_records(records, plan.n)
        return [(out[plan.lim_off[q]:plan.lim_off[q] + tables[q][1]].tobytes(), stats[q], hop_peak[s:s + h].tobytes(), recs[q].tobytes())
                for q, (s, h, _) in enumerate(plan.hops)]

    x, tables = LR.pack(progs)
    all5 = run(x, tables, range(5))
    for k in range(5):
        xa, ta = LR.pack([progs[k]], lead=k)
        assert run(xa, ta, [k])[0] == all5[k], k
    assert any(s[1][1] > 0 for s in all5)


def test_bad_tables_are_refused_on_the_host():
    from voice_tts_amd import output as O

    dev = torch.device(DEV)
    lim = [("true", True)]
    with pytest.raises(ValueError):
        O.LevelPlan([([(0, 10, 0), (10, 10, 5)], 30, 8000, None, -1.0)], dev, limits=lim)  # overlapping rows
    with pytest.raises(ValueError):
        O.LevelPlan([([(0, 10, 25)], 30, 8000, None, -1.0)], dev, limits=lim)  # a row that leaves its programme
    with pytest.raises(ValueError):
        O.LevelPlan([([(0, 10, 0)], 30, 96000, None, -1.0)], dev, limits=lim)  # a hop over LOUDNESS_MAX_HOP
    with pytest.raises(ValueError):
        O.LevelPlan([([(0, 10, 0)], 30, 8000, None, -1.0)], dev, limits=[("rms", True)])
    with pytest.raises(ValueError):
        O.finish_pcm_many([[torch.zeros(1, 100, device=dev)]], [None], [None], 200, [None], [None], peak_mode=["true"])  # nothing to qualify
