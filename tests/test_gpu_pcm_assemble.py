"""The conversion kernel of the output stage (csrc/output.hip, `output.pcm_assemble`): fp32 rows at the +-32767 scale -> int16
(truncation toward zero, `.type(torch.int16)`) or ITU-T G.711 bytes, laid out with the interval silence in one buffer."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ENCODINGS = ["pcm_s16le", "mulaw", "alaw"]
ZERO = {"pcm_s16le": 0, "mulaw": 0xFF, "alaw": 0xD5}


def _host(pcm16, enc):
    from voice_tts_amd import output as O

    return pcm16.astype(np.int16) if enc == "pcm_s16le" else O.g711_encode(pcm16, enc)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_every_int16_value(enc):
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    ints = np.arange(-32768, 32768)
    x = torch.from_numpy(ints.astype(np.float32)).to(dev)
    got = O.pcm_assemble(x, [(0, x.numel(), 0)], x.numel(), enc).cpu().numpy()
    assert got.dtype == (np.int16 if enc == "pcm_s16le" else np.uint8)
    assert np.array_equal(got, _host(ints, enc))  # s16: the identity; G.711: the CPU reference, byte for byte


@pytest.mark.parametrize("enc", ENCODINGS)
def test_fractions_truncate_toward_zero_and_large_values_clamp(enc):
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    vals = [0.5, -0.5, 0.999, -0.999, 32766.9, -32766.9, 1.5, -1.5, 40000.0, -40000.0, 1e9, -1e9, 32767.0, -32767.0, 32767.5]
    want = [0, 0, 0, 0, 32766, -32766, 1, -1, 32767, -32768, 32767, -32768, 32767, -32767, 32767]
    x = torch.tensor(vals, dtype=torch.float32, device=dev)
    got = O.pcm_assemble(x, [(0, len(vals), 0)], len(vals), enc).cpu().numpy()
    assert np.array_equal(got, _host(np.array(want), enc))
    if enc == "pcm_s16le":
        assert got[8] == 32767 and got[9] == -32768  # +-40000: clamped to the int16 range, not wrapped (40000 wraps to -25536)


@pytest.mark.parametrize("enc", ENCODINGS)
def test_rows_land_at_their_offsets_with_the_zero_code_in_the_gaps(enc):
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    lens, gap = [1, 441, 1000], 1600
    lead = 3  # the rows sit at odd offsets of the input
    x = ((torch.rand(lead + sum(lens) + 5, generator=g) * 2 - 1) * 32767).float()
    rows, s, d = [], lead, 0
    for n in lens:
        rows.append((s, n, d))
        s, d = s + n, d + n + gap
    total = d - gap
    assert total == sum(lens) + 2 * gap
    dtype = torch.int16 if enc == "pcm_s16le" else torch.uint8
    sentinel = 0x5A
    for order in (rows, rows[::-1]):  # (the table is sorted by destination on the way in)
        buf = torch.full((total + 64,), sentinel, dtype=dtype, device=dev)
        O.pcm_assemble(x.to(dev), order, total, enc, out=buf)
        got = buf.cpu().numpy()
        want = np.full(total, ZERO[enc], dtype=got.dtype)
        for s, n, d in rows:
            want[d:d + n] = _host(x[s:s + n].numpy().astype(np.int16), enc)  # (numpy's cast truncates toward zero as well)
        assert np.array_equal(got[:total], want)
        assert (got[total:] == sentinel).all()  # nothing written past the end
    # an empty call, a row of n = 0 and no row at all: silence only
    out = O.pcm_assemble(x.to(dev), [(0, 0, 2)], 9, enc).cpu().numpy()
    assert (out == ZERO[enc]).all() and out.size == 9
    assert (O.pcm_assemble(x.to(dev), [], 5, enc).cpu().numpy() == ZERO[enc]).all()
    with pytest.raises(ValueError):
        O.pcm_assemble(x.to(dev), [(0, 10, 0), (10, 10, 5)], 30, enc)  # overlapping rows


def test_unknown_encoding_is_ixtts_err_arg():
    import ctypes as C

    from voice_tts_amd import _lib
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    x = torch.zeros(8, device=dev)
    out = torch.zeros(8, dtype=torch.int16, device=dev)
    t = torch.tensor([[0, 8, 0]], dtype=torch.int64, device=dev)
    L = _lib.lib()
    rc = L.ixtts_pcm_assemble(C.c_void_p(x.data_ptr()), 8, C.c_void_p(out.data_ptr()), 8, C.c_void_p(t.data_ptr()), 1, 7, None)
    assert rc == -1 and b"encoding" in L.ixtts_last_error()
    rc = L.ixtts_pcm_assemble(C.c_void_p(x.data_ptr()), 8, C.c_void_p(out.data_ptr()), -1, C.c_void_p(t.data_ptr()), 1, 0, None)
    assert rc == -1 and b"total" in L.ixtts_last_error()
    with pytest.raises(ValueError):
        O.pcm_assemble(x, [(0, 8, 0)], 8, "mp3")


def test_finish_pcm_many_lays_out_requests_of_mixed_formats():
    """Three requests in one call -- plain rate as s16, 16 kHz s16, 8 kHz mu-law: each result equals `finish_pcm` of its own segments,
    and the 22 050 Hz s16 one is the host path's cat and `.type(torch.int16)`."""
    from voice_tts_amd import output as O

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(6)
    segs = [[((torch.rand(1, n, generator=g) * 2 - 1) * 30000).float().to(dev) for n in ns] for ns in ([700, 1300], [441], [1000, 1, 333])]
    rates, encs = [22050, 16000, 8000], [None, "pcm_s16le", "mulaw"]
    many = O.finish_pcm_many(segs + [[]], rates + [None], encs + [None], 30)
    assert many[3] is None
    for ws, sr, enc, (got_sr, got) in zip(segs, rates, encs, many[:3]):
        alone_sr, alone = O.finish_pcm(ws, sr, enc, 30)
        assert got_sr == alone_sr == sr and got.dtype == alone.dtype and np.array_equal(got, alone)
        gap = int(sr * 30 / 1000.0)
        assert got.shape == (sum(O.resampled_len(w.shape[1], 22050, sr) for w in ws) + gap * (len(ws) - 1), 1)
    sil = torch.zeros(1, int(22050 * 30 / 1000.0))
    host = torch.cat([segs[0][0].cpu(), sil, segs[0][1].cpu()], dim=1).type(torch.int16).numpy().T
    assert np.array_equal(many[0][1], host)
