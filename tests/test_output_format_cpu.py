"""The output stage, host side (voice-tts_amd/output.py): the tap table `prompt.sinc_resample` and the device resampler share, the
lengths of a laid-out result, the G.711 reference, the RIFF containers and the refusals.  No GPU."""
import hashlib
import io
import math
import struct
import wave

import numpy as np
import pytest
import torch

from voice_tts_amd import output as O
from voice_tts_amd.prompt import sinc_resample

RATES = [sr for sr in O.SAMPLE_RATES if sr != 22050]
# (orig, new, width, widest band of non-zero taps) against 22050 Hz
FACTS = {8000: (441, 160, 17, 34), 11025: (2, 1, 13, 25), 16000: (441, 320, 9, 17), 24000: (147, 160, 7, 13),
         32000: (441, 640, 7, 13), 44100: (1, 2, 7, 13), 48000: (147, 320, 7, 13)}


def _table_as_sinc_resample_built_it(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """The formula as `sinc_resample` carried it before the builder was factored out, kept here word for word."""
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base)
    idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
    t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / orig)
    return kern.to(torch.float32), width


@pytest.mark.parametrize("sr", RATES)
def test_resample_taps_is_the_table_sinc_resample_builds(sr):
    h, width = O.resample_taps(22050, sr, "cpu")
    ref, ref_width = _table_as_sinc_resample_built_it(22050, sr)
    orig, new, w, band = FACTS[sr]
    assert width == ref_width == w and h.dtype == torch.float32 and tuple(h.shape) == (new, 1, 2 * w + orig)
    assert h.numpy().tobytes() == ref.numpy().tobytes()  # bit for bit
    assert O.resample_taps(22050, sr, "cpu")[0] is h  # cached
    # what the kernel reads: per phase a contiguous run of non-zero taps, the widest of them `band` long, nothing outside the bands
    bands, starts, L = O.tap_bands(22050, sr)
    assert L == band and bands.numel() % 4 == 0 and bands.numel() >= new * (L | 1)
    full = torch.zeros(new, 2 * w + orig)
    rows = bands[:new * (L | 1)].view(new, L | 1)
    assert bool((rows[:, L:] == 0).all()) and int(starts.min()) >= 0 and int(starts.max()) + L <= 2 * w + orig
    for p in range(new):
        full[p, int(starts[p]):int(starts[p]) + L] = rows[p, :L]
        nz = torch.nonzero(h[p, 0])[:, 0]
        assert int(nz[-1] - nz[0]) + 1 == nz.numel()
    assert torch.equal(full, h[:, 0])  # (as values: what underflowed outside a band is +0 or -0 in the table)


# sha256 of `sinc_resample`'s output on the seeded input below, taken BEFORE the table builder moved to output.resample_taps.  The
# conversion is a GEMM on the CPU; these four ratios have more than one output phase, where its bits did not depend on the thread
# count (with one phase it is a GEMV, whose bits moved with the thread count before and after the change alike).
SINC_HASHES = {
    (24000, 22050): "f3e6cb8744780b2dddfa24977af08b1d9bb70b1a25f68a78715bdbedc113299f",
    (22050, 44100): "8bf71024facc49dc55aed3304ba13d79a12901b0e8ceefc3599c402d384846f0",
    (22050, 24000): "3af2c9ed2ea1bb17e38e749b5bbd709c97f6ab66ce7c9bdf35e837650bde6f02",
    (22050, 48000): "61184e1068d951e552d31c7fde97ceb6636b051533dde89eee85b30c8399adf2",
}


def test_sinc_resample_is_unchanged_by_the_refactor():
    g = torch.Generator().manual_seed(20260)
    x = torch.rand(2, 3001, generator=g) * 2 - 1
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        for (a, b), want in SINC_HASHES.items():
            y = sinc_resample(x, a, b)
            assert y.shape[-1] == math.ceil(3001 * b / a)
            assert hashlib.sha256(y.contiguous().numpy().tobytes()).hexdigest() == want, (a, b)
    finally:
        torch.set_num_threads(n)
    assert sinc_resample(x, 22050, 22050) is x


@pytest.mark.parametrize("sr", RATES)
def test_lengths_of_rows_and_gaps(sr):
    orig, new = FACTS[sr][:2]
    assert O.resample_ratio(22050, sr) == (orig, new)
    for n in (0, 1, 2, orig - 1, orig, orig + 1, 2 * orig + 3, 22050, 100001):
        assert O.resampled_len(n, 22050, sr) == math.ceil(n * new / orig) == -(-n * new // orig)
        if n:
            assert sinc_resample(torch.zeros(1, n), 22050, sr).shape[-1] == O.resampled_len(n, 22050, sr)
    assert O.gap_len(sr, 200) == int(sr * 200 / 1000.0) == sr // 5
    assert O.gap_len(sr, 0) == 0 and O.gap_len(11025, 30) == 330 and O.gap_len(22050, 200) == 4410


def _g711_from_the_standard(s, law):
    """ITU-T G.711 written out sample by sample: sign, magnitude (mu-law: 14 bits, clipped at 8159, biased by 33; A-law: 13 bits),
    segment = the first segment end that holds it, four mantissa bits, the law's bit inversion."""
    out = np.empty(len(s), np.uint8)
    for i, v in enumerate(int(x) for x in s):
        if law == "mulaw":
            v >>= 2
            mask = 0x7F if v < 0 else 0xFF
            v = min(abs(v), 8159) + 33
            seg = next((k for k in range(8) if v <= (0x40 << k) - 1), 8)
            code = 0x7F if seg == 8 else (seg << 4) | ((v >> (seg + 1)) & 0xF)
        else:
            v >>= 3
            mask = 0xD5 if v >= 0 else 0x55
            v = v if v >= 0 else -v - 1
            seg = next((k for k in range(8) if v <= (0x20 << k) - 1), 8)
            code = 0x7F if seg == 8 else (seg << 4) | ((v >> (1 if seg < 2 else seg)) & 0xF)
        out[i] = code ^ mask
    return out


@pytest.mark.parametrize("law", ["mulaw", "alaw"])
def test_g711_reference_equals_audioop_for_every_int16(law):
    s = np.arange(-32768, 32768).astype(np.int16)
    got = O.g711_encode(s, law)
    assert got.dtype == np.uint8 and np.array_equal(got, _g711_from_the_standard(s, law))
    try:
        import audioop
    except ImportError:  # (gone from the standard library in 3.13: the written-out standard above is the yardstick then)
        audioop = None
    if audioop is not None:
        ref = (audioop.lin2ulaw if law == "mulaw" else audioop.lin2alaw)(s.tobytes(), 2)
        assert got.tobytes() == ref
    assert int(O.g711_encode(np.zeros(1, np.int16), law)[0]) == O.ZERO_CODES[law] == {"mulaw": 0xFF, "alaw": 0xD5}[law]


def test_wav_bytes_s16_is_what_wave_writes():
    pcm = (np.arange(4411) * 37 % 65536 - 32768).astype(np.int16).reshape(-1, 1)
    for sr in (22050, 16000, 48000):
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes(pcm.astype("<i2").tobytes())
        assert O.wav_bytes(sr, pcm, "pcm_s16le") == O.wav_bytes(sr, pcm) == buf.getvalue()


@pytest.mark.parametrize("law,tag", [("mulaw", 7), ("alaw", 6)])
@pytest.mark.parametrize("n", [4410, 4411, 1])
def test_wav_bytes_g711_header_parses_back(law, tag, n):
    pcm = (np.arange(n) % 256).astype(np.uint8).reshape(-1, 1)
    raw = O.wav_bytes(8000, pcm, law)
    pad = n & 1
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8
    assert struct.unpack("<I", raw[16:20])[0] == 18
    assert struct.unpack("<HHIIHHH", raw[20:38]) == (tag, 1, 8000, 8000, 1, 8, 0)  # tag, channels, rate, bytes/s, block, bits, cbSize
    assert raw[38:42] == b"fact" and struct.unpack("<II", raw[42:50]) == (4, n)
    assert raw[50:54] == b"data" and struct.unpack("<I", raw[54:58])[0] == n
    assert raw[58:58 + n] == pcm.tobytes() and len(raw) == 58 + n + pad and len(raw) % 2 == 0 and raw[58 + n:] == b"\0" * pad
    info = O.riff_info(raw)
    assert (info["tag"], info["rate"], info["bits"], info["cb_size"], info["fact"], info["frames"], info["padded"]) == (tag, 8000, 8, 0, n, n, True)


def test_tts_request_refuses_values_outside_the_sets():
    from pydantic import ValidationError

    from voice_tts_amd.server import TTSRequest

    hexs = "00ff" * 60
    ok = TTSRequest(text="hi", spk_audio=hexs, sample_rate=8000, encoding="mulaw")
    assert (ok.sample_rate, ok.encoding) == (8000, "mulaw")
    plain = TTSRequest(text="hi", spk_audio=hexs)
    assert plain.sample_rate is None and plain.encoding is None
    with pytest.raises(ValidationError, match="8000"):
        TTSRequest(text="hi", spk_audio=hexs, sample_rate=12345)
    with pytest.raises(ValidationError, match="mulaw"):
        TTSRequest(text="hi", spk_audio=hexs, encoding="mp3")


def test_finish_pcm_refuses_values_outside_the_sets():
    wavs = [torch.zeros(1, 100)]
    with pytest.raises(ValueError, match="12345.*8000"):
        O.finish_pcm(wavs, sample_rate=12345)
    with pytest.raises(ValueError, match="mp3.*pcm_s16le"):
        O.finish_pcm(wavs, encoding="mp3")
    with pytest.raises(ValueError):
        O.finish_pcm_many([wavs, wavs], [None, 44000], [None, None])
    with pytest.raises(ValueError):
        O.Resampler(12345, "cpu")
    assert O.check_format() == (22050, "pcm_s16le") and O.check_format(48000, "alaw") == (48000, "alaw")


def test_an_encoding_on_a_stream_is_refused_before_any_device_work():
    """`infer(stream_return=True, output_encoding=...)`: ValueError from the call itself; the object here has no model, no engine and
    no device behind it, so anything but the refusal would fail differently."""
    from indextts.infer_v2 import IndexTTS2

    m = IndexTTS2.__new__(IndexTTS2)
    with pytest.raises(ValueError, match="stream_return"):
        m.infer(b"", "Hello.", None, stream_return=True, output_encoding="mulaw")
    with pytest.raises(ValueError, match="stream_return"):
        next(m.infer_generator(b"", "Hello.", None, stream_return=True, output_sample_rate=8000, output_encoding="pcm_s16le"))
    with pytest.raises(ValueError, match="12345"):
        m.infer(b"", "Hello.", None, output_sample_rate=12345)
    with pytest.raises(ValueError, match="mp3"):
        next(m.infer_generator(b"", "Hello.", None, output_encoding="mp3"))
