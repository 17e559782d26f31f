"""`ixtts_pcm_assemble_gain` (csrc/output.hip, `output.pcm_assemble_gain`): the conversion kernel with a gain per row read from the
device, and `finish_pcm_many` with a loudness target / peak ceiling as the composition of resampler, measurement and that kernel."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ENCODINGS = ["pcm_s16le", "mulaw", "alaw"]


@pytest.mark.parametrize("enc", ENCODINGS)
def test_bytes_are_the_host_conversion_of_the_fp32_product(enc):
    import loudness_ref as LR
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    ints = torch.arange(-32768, 32768, dtype=torch.float32)
    lens, gap, lead = [65536, 1, 441, 1000, 0, 333], 160, 3  # (rows at odd offsets of the input: the one-by-one path; row 0: the quads)
    x = torch.cat([torch.zeros(lead), ints] + [((torch.rand(n, generator=g) * 2 - 1) * 32767).float() for n in lens[1:]] + [torch.zeros(5)])
    gains = torch.tensor([0.37, 1.9, 1.0, 3.1622777], dtype=torch.float32)
    index = [0, 1, -1, 3, 2, 9]  # -1 and 9: no gain of the table, the sample as it is
    rows, s, d = [], lead, 0
    for n, gi in zip(lens, index):
        rows.append((s, n, d, gi))
        s, d = s + n, d + n + gap
    total = d - gap
    dtype = torch.int16 if enc == "pcm_s16le" else torch.uint8
    buf = torch.full((total + 64,), 0x5A, dtype=dtype, device=dev)
    O.pcm_assemble_gain(x.to(dev), rows[::-1], total, enc, gains.to(dev), out=buf)
    got = buf.cpu().numpy()
    want = np.full(total, O.ZERO_CODES[enc], got.dtype)
    xn, gn = x.numpy(), gains.numpy()
    for s, n, d, gi in rows:
        v = xn[s:s + n] * gn[gi] if 0 <= gi < len(gn) else xn[s:s + n]  # fp32 x fp32 in numpy: one rounding
        assert v.dtype == np.float32
        want[d:d + n] = LR.encode(v, enc)
    assert np.array_equal(got[:total], want)
    assert (got[total:] == 0x5A).all()  # nothing written past the end
    # aligned input, so that every thread takes the 16-byte path
    xa = x[lead:lead + 65536].contiguous().to(dev)
    for gi in (1, -1):
        got = O.pcm_assemble_gain(xa, [(0, 65536, 0, gi)], 65536, enc, gains.to(dev)).cpu().numpy()
        assert np.array_equal(got, LR.encode(xn[lead:lead + 65536] * (gn[gi] if gi >= 0 else np.float32(1)), enc))


@pytest.mark.parametrize("enc", ENCODINGS)
def test_unit_gains_give_the_bytes_of_pcm_assemble(enc):
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(8)
    lens, gap = [1, 441, 0, 2049], 37
    x = ((torch.rand(2 + sum(lens), generator=g) * 2 - 1) * 40000).float().to(dev)  # (beyond the int16 range: the clamp as well)
    rows, s, d = [], 2, 0
    for n in lens:
        rows.append((s, n, d))
        s, d = s + n, d + n + gap
    total = d  # (a trailing gap)
    plain = O.pcm_assemble(x, rows, total, enc).cpu().numpy()
    ones = torch.ones(2, dtype=torch.float32, device=dev)
    for index in ([0, 1, 0, 1], [-1, -1, -1, -1]):
        got = O.pcm_assemble_gain(x, [r + (gi,) for r, gi in zip(rows, index)], total, enc, ones).cpu().numpy()
        assert got.dtype == plain.dtype and np.array_equal(got, plain)
    assert (O.pcm_assemble_gain(x, [], 9, enc, ones).cpu().numpy() == O.ZERO_CODES[enc]).all()
    with pytest.raises(ValueError):
        O.pcm_assemble_gain(x, [(0, 10, 0, 0), (10, 10, 5, 0)], 30, enc, ones)


def test_unknown_encoding_is_ixtts_err_arg():
    import ctypes as C

    from voice_tts_amd import _lib

    dev = torch.device("cuda:0")
    x, out = torch.zeros(8, device=dev), torch.zeros(8, dtype=torch.int16, device=dev)
    t = torch.tensor([[0, 8, 0, 0]], dtype=torch.int64, device=dev)
    L, P = _lib.lib(), C.c_void_p
    rc = L.ixtts_pcm_assemble_gain(P(x.data_ptr()), 8, P(out.data_ptr()), 8, P(t.data_ptr()), 1, P(x.data_ptr()), 1, 7, None)
    assert rc == -1 and b"encoding" in L.ixtts_last_error()
    rc = L.ixtts_pcm_assemble_gain(P(x.data_ptr()), 8, P(out.data_ptr()), 8, P(t.data_ptr()), 1, None, 1, 0, None)
    assert rc == -1 and b"null" in L.ixtts_last_error()


def _segments(dev):
    import loudness_ref as LR

    return [[torch.from_numpy(LR.noise(n, 22050, 40 + k + 10 * q, rms=1500.0 * (q + 1))).reshape(1, -1).to(dev) for k, n in enumerate(ns)]
            for q, ns in enumerate(([9000, 4000], [12000], [5000, 1, 7000], [11000, 3000], [2000]))]


def test_finish_pcm_many_measures_what_it_delivers_and_converts_the_product():
    """Five requests in one call, different rates, encodings, targets and ceilings (one without a control, one too short for a
    block): each equals its own call bit for bit, its report is the twin's reading of the delivered programme, and its bytes are the
    host conversion of fp32(gain) * x over the rows the resampler gives (22 050 Hz: the vocoder's own)."""
    import loudness_ref as LR
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    segs = _segments(dev)
    rates, encs = [22050, 8000, 48000, 11025, None], [None, "mulaw", "pcm_s16le", "alaw", None]
    loud, peak = [-23.0, -16.0, None, None, -23.0], [None, -3.0, -9.0, None, None]
    interval = 120
    reports = []
    many = O.finish_pcm_many(segs, rates, encs, interval, loudness=loud, peak=peak, reports=reports)
    assert len(reports) == 5 and reports[3] is None
    plain = O.finish_pcm_many(segs, rates, encs, interval)
    assert np.array_equal(many[3][1], plain[3][1])  # no control: the bytes of the call without the new arguments
    for q, (ws, sr, enc) in enumerate(zip(segs, rates, encs)):
        rep1 = []
        alone_sr, alone = O.finish_pcm(ws, sr, enc, interval, loudness=loud[q], peak=peak[q], reports=rep1)
        assert many[q][0] == alone_sr == (sr or 22050) and many[q][1].dtype == alone.dtype and np.array_equal(many[q][1], alone)
        if loud[q] is None and peak[q] is None:
            continue
        assert rep1[0] == reports[q]
        fs, enc = sr or 22050, enc or "pcm_s16le"
        rows = ws if fs == 22050 else O.Resampler(fs, dev).forward_many(ws)
        rows = [r.cpu().numpy()[0] for r in rows]
        gap = O.gap_len(fs, interval)
        prog = LR.lay_out(rows, gap)
        L = LR.loudness(prog, fs)
        ceiling = peak[q] if peak[q] is not None else -1.0
        g, flags = LR.gain(L, float(np.abs(prog).max()), loud[q], ceiling)
        rep = reports[q]
        assert (rep["measured_lufs"] is None) == (L is None) and (L is None or abs(rep["measured_lufs"] - L) <= 1e-6)
        assert abs(rep["gain_db"] - 20 * np.log10(float(np.float32(g)))) <= 1e-5
        assert rep["target_met"] == (loud[q] is None or flags == 0)
        # the bytes: the kernel-level composition on the same rows gives the record, and the record's gain gives the bytes
        x, (table,) = LR.pack([(rows, gap)])
        plan = O.LevelPlan([(table[0], table[1], fs, loud[q], ceiling)], dev)
        rec = O.read_records(O.measure_levels(torch.from_numpy(x).to(dev), plan)[2], 1)[0]
        assert O.level_report(rec, loud[q]) == rep
        want = LR.encode(np.float32(rec["gain"]) * prog, enc)
        assert np.array_equal(many[q][1][:, 0], want)
    assert reports[4]["measured_lufs"] is None and reports[4]["target_met"] is False and reports[4]["gain_db"] == 0.0  # 2000 samples: under 4 hops
    assert reports[0]["target_met"] and reports[0]["measured_lufs"] is not None
