"""The output stage: what leaves the vocoder (fp32 rows at 22 050 Hz, scaled to +-32767) becomes the sample rate and sample encoding
the caller asked for, ON THE DEVICE (csrc/output.hip), and reaches the host in one copy.

  resample_taps     the Hann-windowed sinc table of `torchaudio.transforms.Resample` -- the ONE builder; `prompt.sinc_resample` (the
                    CPU restatement used on the prompt side) and the device resampler both take their table from it
  Resampler         packed rows of unequal length -> the requested rate, one launch for all of them
  pcm_assemble      rows -> one buffer of int16 / G.711 bytes, the gaps (interval silence) holding the encoding's code for zero
  OutputSpec        what ONE request asks of the stage, resolved: rate, encoding, loudness, peak, peak mode, limiter, total
  finish            the tail of `infer` / `infer_many`, the one entry: the segments and the spec of every request of a call ->
                    resample, measure, limit, convert, lay out, copy to the host once; `finish_pcm(_many)` spell the specs as lists
  k_weighting       the two biquads of ITU-R BS.1770 at a sample rate -- the ONE builder, for the measurement kernel and the tests
  measure_levels    K-weighted hop energies and sample peak of every programme of a call, then gating and gain: two launches
  pcm_assemble_gain `pcm_assemble` with a gain per row, read from the device
  true_peak_taps    the 4x interpolator of the true peak (BS.1770 Annex 2), limiter_window: the limiter's smoothing window -- the ONE
                    builder each, for the kernels of csrc/limiter.hip and the tests
  true_peaks, limit the true peak of every hop in place of the sample peak; a look-ahead limiter under the ceiling: one launch each
  wav_bytes         the RIFF container of a result

With nothing requested none of this runs: `infer` keeps its host-side cat and `.type(torch.int16)`.
"""
import ctypes as C
import io
import math
import struct
import wave
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib

MODEL_RATE = 22050
SAMPLE_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
ENCODINGS = ("pcm_s16le", "mulaw", "alaw")
WAVE_FORMAT_TAGS = {"pcm_s16le": 1, "alaw": 6, "mulaw": 7}
ZERO_CODES = {"pcm_s16le": 0, "mulaw": 0xFF, "alaw": 0xD5}

_TAPS = {}
_BANDS = {}


def check_format(sample_rate=None, encoding=None):
    """-> (rate, encoding) with the defaults filled in; ValueError for anything outside the two sets.  (An arbitrary rate can reduce
    against 22050 to a tap table of hundreds of millions of entries: the rates are a closed set.)"""
    if sample_rate is not None and (isinstance(sample_rate, bool) or sample_rate not in SAMPLE_RATES):
        raise ValueError(f"output sample rate {sample_rate!r} is not one of {SAMPLE_RATES}")
    if encoding is not None and encoding not in ENCODINGS:
        raise ValueError(f"output encoding {encoding!r} is not one of {ENCODINGS}")
    return (MODEL_RATE if sample_rate is None else int(sample_rate)), ("pcm_s16le" if encoding is None else encoding)


def resample_ratio(sr_in, sr_out):
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_in) // g, int(sr_out) // g


def resample_taps(sr_in, sr_out, device="cpu", lowpass_filter_width=6, rolloff=0.99):
    """-> (h fp32 [new, 1, 2 * width + orig] on `device`, width): the kernel bank of `torchaudio.transforms.Resample(sr_in, sr_out)`
    (sinc_interp_hann), computed in fp64 and rounded to fp32.  Cached per (ratio, settings, device)."""
    orig, new = resample_ratio(sr_in, sr_out)
    device = torch.device(device)
    key = (orig, new, lowpass_filter_width, rolloff, device)
    if key not in _TAPS:
        base = min(orig, new) * rolloff
        width = math.ceil(lowpass_filter_width * orig / base)
        idx = torch.arange(-width, width + orig, dtype=torch.float64)[None, None] / orig
        t = torch.arange(0, -new, -1, dtype=torch.float64)[:, None, None] / new + idx
        t = (t * base).clamp_(-lowpass_filter_width, lowpass_filter_width)
        window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
        t = t * math.pi
        kern = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / orig)
        _TAPS[key] = (kern.to(torch.float32).to(device), width)
    return _TAPS[key]


def resampled_len(n, sr_in, sr_out):
    orig, new = resample_ratio(sr_in, sr_out)
    return -(-int(n) * new // orig)


def tap_bands(sr_in, sr_out):
    """The table as the kernel reads it: -> (bands fp32 [new, L | 1] flattened and padded to whole float4s, starts int32 [new], L).
    In the fp32 table the clamped window underflows to exactly 0 outside a short run per phase; L is the widest such run, and
    bands[p][k] = h[p][starts[p] + k] (a shorter run is followed by the table's own zeros)."""
    h = resample_taps(sr_in, sr_out, "cpu")[0][:, 0]
    new, K = h.shape
    nz = h != 0
    first = torch.where(nz.any(1), nz.int().argmax(1), torch.zeros(new, dtype=torch.long))
    last = torch.where(nz.any(1), K - 1 - nz.flip(1).int().argmax(1), torch.zeros(new, dtype=torch.long))
    L = int((last - first + 1).max())
    starts = torch.minimum(first, torch.full_like(first, K - L))
    Ls = L | 1
    bands = torch.zeros((new * Ls + 3) // 4 * 4, dtype=torch.float32)
    rows = bands[:new * Ls].view(new, Ls)
    rows[:, :L] = h.gather(1, starts[:, None] + torch.arange(L)[None])
    return bands, starts.to(torch.int32), L


def _row_table(rows, device, cols=3):
    """[(src, n, dst)] -> int64 [R, 3] on the device, copied from pinned memory so that the host does not wait for the stream."""
    t = torch.tensor(rows, dtype=torch.int64).reshape(-1, cols)
    if device.type == "cuda":
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


class Resampler:
    """22 050 Hz -> `sr_out` on the device, with the semantics of `prompt.sinc_resample(x, 22050, sr_out)` and the result clamped to
    +-32767 (a band-limited filter overshoots on full-scale input)."""

    def __init__(self, sr_out, device, sr_in=MODEL_RATE):
        self.sr_in, self.sr_out = int(sr_in), check_format(sr_out)[0]
        if self.sr_in == self.sr_out:
            raise ValueError(f"Resampler: {self.sr_out} Hz is the rate the rows already have")
        self.device = torch.device(device)
        self.orig, self.new = resample_ratio(self.sr_in, self.sr_out)
        self.width = resample_taps(self.sr_in, self.sr_out, "cpu")[1]
        key = (self.orig, self.new, self.device)
        if key not in _BANDS:
            bands, starts, L = tap_bands(self.sr_in, self.sr_out)
            _BANDS[key] = (bands.to(self.device), starts.to(self.device), L)
        self.bands, self.starts, self.band = _BANDS[key]

    def out_len(self, n):
        return -(-int(n) * self.new // self.orig)

    def resample_into(self, x, y, rows):
        """ONE launch: for every (src, n, dst) of `rows`, x[src : src + n] resampled into y[dst : dst + out_len(n)].  x, y: flat
        contiguous fp32 device tensors; nothing outside those ranges is written."""
        assert x.dtype == y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and x.device == y.device == self.bands.device
        rows = [(int(s), int(n), int(d)) for s, n, d in rows]
        for s, n, d in rows:
            if s < 0 or n < 0 or d < 0 or s + n > x.numel() or d + self.out_len(n) > y.numel():
                raise ValueError(f"resample row (src={s}, n={n}, dst={d}) leaves its buffers ({x.numel()} in, {y.numel()} out)")
        if not rows or max(n for _, n, _ in rows) == 0:
            return y
        table = _row_table(rows, x.device)
        _lib.check(_lib.lib().ixtts_resample_varlen_f32(
            C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(y.data_ptr()), y.numel(), C.c_void_p(table.data_ptr()), len(rows),
            max(n for _, n, _ in rows), C.c_void_p(self.bands.data_ptr()), self.bands.numel(), C.c_void_p(self.starts.data_ptr()),
            self.orig, self.new, self.width, self.band, _lib.current_stream_ptr()), "ixtts_resample_varlen_f32")
        return y

    def forward_many(self, rows):
        """fp32 [1, n_i] device tensors -> fp32 [1, ceil(n_i * new / orig)], one launch for all of them."""
        rows = [r.to(self.device, torch.float32).reshape(-1) for r in rows]
        if not rows:
            return []
        x = torch.cat(rows) if len(rows) > 1 else rows[0].contiguous()
        lens = [r.numel() for r in rows]
        outs = [self.out_len(n) for n in lens]
        y = torch.empty(sum(outs), dtype=torch.float32, device=self.device)
        table, s, d = [], 0, 0
        for n, m in zip(lens, outs):
            table.append((s, n, d))
            s, d = s + n, d + m
        self.resample_into(x, y, table)
        return [t.reshape(1, -1) for t in y.split(outs)]


def _assemble(x, rows, total, encoding, gains, out):
    """`pcm_assemble` (`gains` None: rows of three columns) and `pcm_assemble_gain` (four): validation, table, ONE launch."""
    if encoding not in ENCODINGS:
        raise ValueError(f"output encoding {encoding!r} is not one of {ENCODINGS}")
    cols = 3 if gains is None else 4
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert gains is None or (gains.dtype == torch.float32 and gains.is_contiguous() and gains.device == x.device)
    rows = sorted((tuple(int(v) for v in r) for r in rows), key=lambda r: (r[2], r[1]))
    end = 0
    for r in rows:
        s, n, d = r[:3]
        if len(r) != cols or s < 0 or n < 0 or d < end or s + n > x.numel() or d + n > total:
            raise ValueError(f"assemble row (src={s}, n={n}, dst={d}) overlaps its neighbour or leaves its buffers ({x.numel()} in, {total} out)")
        end = d + n
    dtype = torch.int16 if encoding == "pcm_s16le" else torch.uint8
    if out is None:
        out = torch.empty(int(total), dtype=dtype, device=x.device)
    assert out.dtype == dtype and out.is_contiguous() and out.numel() >= total and out.device == x.device
    table = _row_table(rows if rows else [(0, 0, 0, -1)[:cols]], x.device, cols)
    P = C.c_void_p
    head = (P(x.data_ptr()), x.numel(), P(out.data_ptr()), int(total), P(table.data_ptr()), len(rows))
    tail = (_lib.PCM_ENCODINGS[encoding], _lib.current_stream_ptr())
    if gains is None:
        _lib.check(_lib.lib().ixtts_pcm_assemble(*head, *tail), "ixtts_pcm_assemble")
    else:
        _lib.check(_lib.lib().ixtts_pcm_assemble_gain(*head, P(gains.data_ptr()), gains.numel(), *tail), "ixtts_pcm_assemble_gain")
    return out


def pcm_assemble(x, rows, total, encoding, out=None):
    """ONE launch: `total` samples of `encoding` -- x[src : src + n] converted at [dst, dst + n) for every (src, n, dst) of `rows`
    (ascending in dst, disjoint), the encoding's code for silence everywhere else.  -> int16 / uint8 [total] on x's device (`out`:
    write into this tensor's first `total` elements instead)."""
    return _assemble(x, rows, total, encoding, None, out)


def gap_len(sample_rate, interval_silence=200):
    return int(sample_rate * interval_silence / 1000.0)


# --------------------------------------------------------------------------- a target duration: the frame counts that fit it
HOP = 256  # samples of one mel frame at MODEL_RATE


class DurationError(ValueError):
    """A `duration` the speaking-rate range cannot reach.  `natural_s`: what the request delivers at its natural pace; `min_s`,
    `max_s`: the durations its fastest and slowest allowed pace deliver (both can be asked for), all at the delivered rate."""

    def __init__(self, duration, natural_s, min_s, max_s):
        self.duration, self.natural_s, self.min_s, self.max_s = float(duration), float(natural_s), float(min_s), float(max_s)
        super().__init__(f"duration {duration!r} s cannot be met: the natural duration is {natural_s:.3f} s, a duration in "
                         f"[{min_s:.3f}, {max_s:.3f}] s can be")


def check_duration(duration):
    """-> None, or `duration` as a float; ValueError for a bool, a NaN, an infinity, anything that is not a number or not positive."""
    if duration is None:
        return None
    if isinstance(duration, bool) or not isinstance(duration, (int, float, np.integer, np.floating)) or not 0.0 < float(duration) < math.inf:
        raise ValueError(f"duration {duration!r} is not a positive number of seconds")
    return float(duration)


def delivered_len(frames, sample_rate=MODEL_RATE, interval_silence=200):
    """Samples a programme of segments of `frames` mel frames delivers at `sample_rate`: every segment under the resampler's
    ceil(n * new / orig) rule, `gap_len` samples between two segments."""
    return sum(resampled_len(f * HOP, MODEL_RATE, sample_rate) for f in frames) + max(0, len(frames) - 1) * gap_len(sample_rate, interval_silence)


def share_frames(natural, total):
    """`total` frames among the segments in proportion to their `natural` frame counts, by the largest remainder: every count within
    1 of its exact share, and at least 1 (total >= len(natural))."""
    assert total >= len(natural) and all(f >= 1 for f in natural)
    S = sum(natural)
    out = [f * total // S for f in natural]  # exact integer floors of the shares
    order = sorted(range(len(natural)), key=lambda i: (-(natural[i] * total % S), i))
    for i in order[:total - sum(out)]:
        out[i] += 1
    for i in range(len(out)):  # a share below 1 that rounded down: one frame from the segment furthest above its share
        if out[i] == 0:
            j = max((k for k in range(len(out)) if out[k] >= 2), key=lambda k: out[k] * S - natural[k] * total)
            out[j] -= 1
            out[i] = 1
    return out


def fit_frames(natural, duration, sample_rate=MODEL_RATE, interval_silence=200, speed_range=None):
    """The frame counts with which segments of `natural` frames (>= 1 each) fill `duration` seconds at `sample_rate` -> (frames,
    N, pad): N = int(duration * sample_rate + 0.5) samples are delivered, `frames` (`share_frames`) has the largest total whose
    `delivered_len` does not exceed N, and pad = N - delivered_len(frames) trailing samples of silence fill the rest -- less than
    one frame's worth of delivered samples plus one sample per segment (each segment's ceil adds less than one).  Speech is never
    cut.  `DurationError` when the implied speed sum(natural) / sum(frames) leaves `speed_range` (`s2mel.SPEED_RANGE`)."""
    if speed_range is None:
        from .s2mel import SPEED_RANGE as speed_range
    natural = [int(f) for f in natural]
    duration = check_duration(duration)
    S, n = sum(natural), len(natural)
    N = int(duration * sample_rate + 0.5)
    orig, new = resample_ratio(MODEL_RATE, sample_rate)
    gaps = max(0, n - 1) * gap_len(sample_rate, interval_silence)
    length = lambda total: delivered_len(share_frames(natural, total), sample_rate, interval_silence)  # noqa: E731
    lo_speed, hi_speed = speed_range
    least = max(n, math.ceil(S / hi_speed))  # the totals whose implied speed lies in the range
    most = max(least, math.floor(S / lo_speed))
    total = (N - gaps) * orig // (HOP * new) if N > gaps else 0  # no larger total fits: a segment delivers at least its exact length
    while total >= max(n, 1) and length(total) > N:
        total -= 1
    if not least <= total <= most:
        raise DurationError(duration, length(S) / sample_rate, length(least) / sample_rate, length(most) / sample_rate)
    frames = share_frames(natural, total)
    return frames, N, N - delivered_len(frames, sample_rate, interval_silence)


# --------------------------------------------------------------------------- loudness target and peak ceiling (ITU-R BS.1770-4)
LOUDNESS_RANGE = (-50.0, -5.0)  # LUFS
PEAK_RANGE = (-20.0, 0.0)  # dBFS, sample peak
DEFAULT_PEAK = -1.0  # the ceiling of a request that gives a loudness target alone
_RECORD = np.dtype([("lufs", "<f8"), ("gain", "<f4"), ("peak", "<f4"), ("flags", "<u4"), ("blocks", "<u4")])
assert _RECORD.itemsize == _lib.LOUDNESS_RECORD_BYTES


def check_level(loudness=None, peak=None):
    """-> None when neither is given, else (loudness | None, peak | None) as floats, the ceiling defaulting to -1 dBFS beside a
    loudness target; ValueError for a bool, a NaN, anything that is not a number and a value outside [-50, -5] LUFS / [-20, 0] dBFS."""
    if loudness is None and peak is None:
        return None
    for name, v, (lo, hi), unit in (("loudness", loudness, LOUDNESS_RANGE, "LUFS"), ("peak", peak, PEAK_RANGE, "dBFS")):
        if v is None:
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not lo <= float(v) <= hi:  # (NaN fails the comparison)
            raise ValueError(f"output {name} {v!r} is not a number in [{lo:g}, {hi:g}] {unit}")
    return (None if loudness is None else float(loudness)), (DEFAULT_PEAK if peak is None else float(peak))


PEAK_MODES = ("sample", "true")  # what the ceiling is held against: the sample peak, or the 4x-oversampled true peak (dBTP)
LOUDNESS_TOLERANCE_LU = 0.5  # what EBU R128 grants a programme around its target
_PARTIAL = np.dtype([("min_gain", "<f4"), ("count", "<u4")])  # what one tile of the limiter leaves


def check_limit(peak_mode=None, limiter=None, level=None):
    """`level`: what `check_level` returned.  -> (level, peak_mode, limiter) with the defaults filled in ("sample", False); the
    limiter is a level control of its own, so with it a missing level becomes (None, -1 dBFS).  ValueError for a mode outside
    `PEAK_MODES`, a limiter that is not a bool, and "true" without a loudness target, a ceiling or the limiter: there is no ceiling
    for it to qualify."""
    if peak_mode is not None and not (isinstance(peak_mode, str) and peak_mode in PEAK_MODES):
        raise ValueError(f"output peak mode {peak_mode!r} is not one of {PEAK_MODES}")
    if limiter is not None and not isinstance(limiter, (bool, np.bool_)):
        raise ValueError(f"output limiter {limiter!r} is not a bool")
    mode, limiter = "sample" if peak_mode is None else peak_mode, bool(limiter)
    if limiter:
        level = (None, DEFAULT_PEAK) if level is None else (level[0], DEFAULT_PEAK if level[1] is None else level[1])
    if mode == "true" and level is None:
        raise ValueError("output peak mode 'true' needs a ceiling to qualify: give a loudness target, a peak ceiling or the limiter")
    return level, mode, limiter


# request key <-> keyword of `infer*`, in the order of `OutputSpec.of`
OUTPUT_KEYS = (("sample_rate", "output_sample_rate"), ("encoding", "output_encoding"), ("loudness", "output_loudness"), ("peak", "output_peak"),
               ("peak_mode", "output_peak_mode"), ("limiter", "output_limiter"))


class OutputSpec(NamedTuple):
    """What one request asks of the stage, resolved: what `check_format`, `check_level` and `check_limit` return, in that order, and
    `total`: the samples the request delivers when a duration was fitted (`_replace(total=...)`), else None."""
    rate: int
    encoding: str
    loudness: Optional[float]
    peak: Optional[float]
    peak_mode: str
    limiter: bool
    total: Optional[int] = None

    @classmethod
    def of(cls, sample_rate=None, encoding=None, loudness=None, peak=None, peak_mode=None, limiter=None, duration=False, stream=False):
        """-> the spec, or None when nothing is asked of the stage: no rate, no encoding, no `duration` (a request with one leaves
        through the stage whatever else it asks) and no level once `check_limit` has spoken -- a mode of "sample" or a limiter of
        False alone asks nothing.  ValueError for what the three checks refuse and, on a `stream` (which yields fp32 segments and has
        no whole programme), for an encoding, a level or a limit; format, level, limit in that order."""
        if stream and encoding is not None:
            raise ValueError("output_encoding cannot be combined with stream_return=True: the stream yields fp32 segments "
                             "(output_sample_rate alone resamples them)")
        rate, enc = check_format(sample_rate, encoding)
        if stream and (loudness is not None or peak is not None):
            raise ValueError("output_loudness / output_peak cannot be combined with stream_return=True: the level is measured over "
                             "the whole programme, which a stream does not have")
        level = check_level(loudness, peak)
        if stream and (peak_mode is not None or limiter is not None):
            raise ValueError("output_peak_mode / output_limiter cannot be combined with stream_return=True: the ceiling is held over "
                             "the whole programme, which a stream does not have")
        level, mode, limiter = check_limit(peak_mode, limiter, level)
        if sample_rate is None and encoding is None and not duration and level is None:
            return None
        return cls(rate, enc, *(level or (None, None)), mode, limiter)

    @property
    def leveled(self):
        return self.loudness is not None or self.peak is not None

    @property
    def limits(self):
        return self.peak_mode, self.limiter


def ceiling(peak):
    """A ceiling in dBFS / dBTP -> sample units."""
    return 32768.0 * 10.0 ** (float(peak) / 20.0)


def true_peak_taps():
    """-> fp64 [49]: h[m] = sinc(m / 4) 0.5 (1 + cos(pi m / 24)), m = -24 .. 24 at index m + 24 -- the 4x interpolator of the true
    peak (ITU-R BS.1770 Annex 2), a Hann-windowed sinc, the same at every rate.  The point n + k / 4 of a programme y is
    z[4 n + k] = sum_j h[k - 4 j] y[n + j]; k = 0 is the sample itself."""
    m = np.arange(-24, 25, dtype=np.float64)
    return np.sinc(m / 4.0) * 0.5 * (1.0 + np.cos(np.pi * m / 24.0))


def lookaround(fs):
    """W: samples the limiter looks to either side (5 ms): 40 at 8 kHz, 110 at 22 050 Hz, 240 at 48 kHz."""
    return (int(fs) + 100) // 200


def limiter_window(fs):
    """-> fp64 [2 W + 1]: the Hann window w[k] = 0.5 (1 - cos(2 pi (k + 1) / (2 W + 2))) over its sum -- what smooths the limiter's
    gain reduction.  No entry is zero."""
    W = lookaround(fs)
    w = 0.5 * (1.0 - np.cos(2.0 * np.pi * (np.arange(2 * W + 1, dtype=np.float64) + 1.0) / (2 * W + 2)))
    return w / w.sum()


def hop_len(fs):
    """Samples of one hop (100 ms) of the gating blocks at `fs`: 1103 at 11 025 Hz."""
    return (int(fs) + 5) // 10


def k_weighting(fs):
    """-> (b_shelf, a_shelf, b_highpass, a_highpass), fp64 [3] each: the K-weighting of ITU-R BS.1770 at `fs`, the analogue prototypes
    behind the standard's 48 kHz table carried to `fs` by the bilinear transform (at 48 000 Hz: the table, within 1e-12)."""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b_s = np.array([Vh + Vb * K / Q + K * K, 2.0 * (K * K - Vh), Vh - Vb * K / Q + K * K], np.float64) / a0
    a_s = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b_h = np.array([1.0, -2.0, 1.0], np.float64)
    a_h = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0], np.float64)
    return b_s, a_s, b_h, a_h


def chunk_transition(fs):
    """-> (Cw, M fp64 [4, 4]): the samples of one lane's chunk in the measurement kernel -- ceil((R + H) / 64) | 1 with H the hop and
    R = H + H // 2 the run-in -- and the zero-input transition of the K-weighting's state over such a chunk, A^Cw, where A updates
    (s1, s2, u1, u2) of the two transposed-direct-form-II sections by one sample."""
    H = hop_len(fs)
    Cw = -(-(H + H // 2 + H) // 64) | 1
    _, a_s, _, a_h = k_weighting(fs)
    A = np.array([[-a_s[1], 1.0, 0.0, 0.0], [-a_s[2], 0.0, 0.0, 0.0], [-a_h[1] - 2.0, 0.0, -a_h[1], 1.0], [1.0 - a_h[2], 0.0, -a_h[2], 0.0]], np.float64)
    return Cw, np.linalg.matrix_power(A, Cw)


def level_report(record, loudness):
    """One record of the gating kernel -> dict(measured_lufs | None, gain_db, peak_dbfs_in, target_met): target_met is False when a
    loudness target was asked for and missed -- the ceiling bound the gain, or the programme has no block to measure."""
    none = bool(record["flags"] & _lib.LOUDNESS_NO_BLOCK)
    bound = bool(record["flags"] & _lib.LOUDNESS_CEILING_BOUND)
    p = float(record["peak"])
    return dict(measured_lufs=None if none else float(record["lufs"]), gain_db=20.0 * math.log10(float(record["gain"])),
                peak_dbfs_in=20.0 * math.log10(p / 32768.0) if p > 0 else float("-inf"),
                target_met=loudness is None or not (none or bound))


def level_report_limit(record, loudness, peak_mode, limiter, extent=0, stats=None, delivered=None):
    """`level_report` of a request that uses `peak_mode` / `limiter`, with the keys they add: peak_mode, limited, max_reduction_db,
    limited_fraction, delivered_lufs | None, delivered_peak_dbfs (in the request's peak mode; so is peak_dbfs_in).  With the
    limiter, `stats` = (smallest gain, samples with a gain below 1) of the programme's `extent` samples, `delivered` = the gating
    kernel's record of the limited programme, and target_met says: an L existed and the delivered loudness is within
    `LOUDNESS_TOLERANCE_LU` of the target.  Without it one gain was applied and nothing was measured twice: delivered = measured
    plus the gain."""
    rep = level_report(record, loudness)
    dbfs = lambda p: 20.0 * math.log10(p / 32768.0) if p > 0 else float("-inf")  # noqa: E731
    rep["peak_mode"] = peak_mode
    if not limiter:
        rep.update(limited=False, max_reduction_db=0.0, limited_fraction=0.0,
                   delivered_lufs=None if rep["measured_lufs"] is None else rep["measured_lufs"] + rep["gain_db"],
                   delivered_peak_dbfs=rep["peak_dbfs_in"] + rep["gain_db"])
        return rep
    smallest, count = float(stats[0]), int(stats[1])
    lufs = None if delivered["flags"] & _lib.LOUDNESS_NO_BLOCK else float(delivered["lufs"])
    rep.update(limited=count > 0, max_reduction_db=20.0 * math.log10(smallest) if 0.0 < smallest < 1.0 else 0.0,
               limited_fraction=count / float(extent) if extent else 0.0, delivered_lufs=lufs, delivered_peak_dbfs=dbfs(float(delivered["peak"])))
    rep["target_met"] = loudness is None or (rep["measured_lufs"] is not None and lufs is not None and abs(lufs - loudness) <= LOUDNESS_TOLERANCE_LU)
    return rep


class LevelPlan:
    """The tables of `measure_levels` for the programmes of a call: programme q = (rows [(src, n, dst)] with dst counted from the
    programme's start, ascending and disjoint; extent; sample rate; loudness target | None; ceiling | None).  Everything goes up in
    ONE pinned copy; `rows`, `reqs`, `lreqs`, `modes`, `coefs`, `targets`, `ceilings`, `tables` are views of it, in that order.

    `limits` (one (peak_mode, limiter) per programme, see `check_limit`; None: ("sample", False) for every one, which leaves `lreqs`,
    `ceilings` and `tables` empty): a programme in true mode has the sample peaks of its hops replaced by true peaks (`modes`).  A
    limited programme gets no ceiling in `targets` -- the gating kernel does not give way -- and a row of the limiter's table
    `lreqs` (`_lib.LIMITER_REQ_COLS`); its ceiling defaults to `DEFAULT_PEAK`; the limited programmes are written one after another,
    programme q at `lim_off[q]` of `lim_total` samples.  The interpolator and one window per distinct rate ride in `tables`.
    `limited_at` (where that region starts in the buffer the rows point into): every limited programme is followed by a second one
    -- programmes n .. n + n2 of the tables: one row over its limited samples, no target, no ceiling -- through which the same
    kernels measure what is delivered."""

    def __init__(self, programmes, device, limits=None, limited_at=None):
        programmes = [tuple(p) for p in programmes]
        limits = [("sample", False)] * len(programmes) if limits is None else [(check_limit(m, bool(lim), (None, None))[1], bool(lim)) for m, lim in limits]
        assert len(limits) == len(programmes)
        self.limited = [q for q, (_, lim) in enumerate(limits) if lim]
        self.lim_off, self.lim_total, second = {}, 0, []
        for q in self.limited:
            extent = int(programmes[q][1])
            self.lim_off[q] = self.lim_total
            if limited_at is not None:
                second.append(([(int(limited_at) + self.lim_total, extent, 0)], extent, programmes[q][2], None, None))
            self.lim_total += max(extent, 0)
        modes = [int(m == "true") for m, _ in limits] + [int(limits[q][0] == "true") for q in self.limited][:len(second)]
        rows, reqs, coefs, targets, at, slot = [], [], [], [], 0, 0
        self.hops = []
        for k, (prog_rows, extent, rate, loudness, peak) in enumerate(programmes + second):
            H, extent = hop_len(rate), int(extent)
            if H > _lib.LOUDNESS_MAX_HOP:
                raise ValueError(f"loudness: a hop of {H} samples ({rate} Hz) is more than the kernel's {_lib.LOUDNESS_MAX_HOP}")
            end = 0
            for s, n, d in prog_rows:
                if s < 0 or n < 0 or d < end or d + n > extent:
                    raise ValueError(f"loudness row (src={s}, n={n}, dst={d}) overlaps its neighbour or leaves its programme of {extent} samples")
                end = d + n
            hops = -(-extent // H)
            reqs.append((len(rows), len(prog_rows), at, extent, H, slot))
            rows += [(int(s), int(n), at + int(d)) for s, n, d in prog_rows]
            b_s, a_s, _, a_h = k_weighting(rate)
            coefs.append([b_s[0], b_s[1], b_s[2], a_s[1], a_s[2], a_h[1], a_h[2], 0.0] + [float(v) for v in chunk_transition(rate)[1].reshape(-1)])
            held = peak is not None and not (k < len(programmes) and limits[k][1])  # (the limiter holds a limited programme's ceiling)
            targets.append([math.nan if loudness is None else loudness, peak if held else math.nan])
            self.hops.append((slot, hops, extent // H))
            at, slot = at + extent, slot + hops
        self.n, self.n2, self.slots, self.n_rows = len(programmes), len(second), slot, len(rows)
        self.max_hops = max([h for _, h, _ in self.hops[:self.n]], default=0)
        self.max_hops2 = max([h for _, h, _ in self.hops[self.n:]], default=0)
        self.any_true, self.any_true2 = any(modes[:self.n]), any(modes[self.n:])
        # the limiter's table, its ceilings, and the interpolator and the windows it and the true peak read
        lreqs, ceilings, tables, w_at, self.tiles, pslot = [], [], [], {}, [], 0
        if self.limited or self.any_true:
            tables.append(true_peak_taps())
        for q in self.limited:
            rate, peak = programmes[q][2], programmes[q][4]
            W = lookaround(rate)
            if not 1 <= W <= _lib.LIMITER_MAX_W:
                raise ValueError(f"limiter: a look-around of {W} samples ({rate} Hz) is outside the kernel's 1 .. {_lib.LIMITER_MAX_W}")
            if rate not in w_at:
                w_at[rate] = sum(t.size for t in tables)
                tables.append(limiter_window(rate))
            tiles = -(-reqs[q][3] // _lib.LIMITER_TILE)
            lreqs.append(reqs[q][:4] + (self.lim_off[q], q, W, w_at[rate], modes[q], pslot))
            ceilings.append(ceiling(DEFAULT_PEAK if peak is None else peak))
            self.tiles.append((pslot, tiles))
            pslot += tiles
        self.partial_slots, self.max_tiles = pslot, max([t for _, t in self.tiles], default=0)
        ints = np.array([v for r in rows + reqs + lreqs for v in r] + modes, np.int64)
        flts = np.concatenate([np.array([v for r in coefs + targets for v in r] + ceilings, np.float64)] + tables)
        blob = torch.from_numpy(np.concatenate([ints, flts.view(np.int64)]))
        if torch.device(device).type == "cuda":
            blob = blob.pin_memory()
        blob = blob.to(device, non_blocking=True)
        cuts = np.cumsum([0, 3 * len(rows), _lib.LOUDNESS_REQ_COLS * len(reqs), _lib.LIMITER_REQ_COLS * len(lreqs), len(modes),
                          _lib.LOUDNESS_COEF_COLS * len(reqs), 2 * len(reqs), len(ceilings), sum(t.size for t in tables)])
        part = [blob[a:b] for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist())]
        self.rows, self.reqs, self.lreqs, self.modes = part[:4]
        self.coefs, self.targets, self.ceilings, self.tables = (p.view(torch.float64) for p in part[4:])


def _level_buffers(plan, dev, records=None):
    """-> (energy fp64 [slots | 1], hop_peak fp32 [..], records uint8, gains fp32 [n + n2 | 1]) for every programme of `plan`."""
    n, k = max(plan.slots, 1), plan.n + plan.n2
    work = torch.zeros(n + (n + 1) // 2, dtype=torch.float64, device=dev)  # (one fill: a hop the kernel skips reads as silence)
    gains = torch.empty(max(k, 1), dtype=torch.float32, device=dev)
    if records is None:
        records = torch.empty(k * _RECORD.itemsize, dtype=torch.uint8, device=dev)
    assert records.dtype == torch.uint8 and records.is_contiguous() and records.numel() >= k * _RECORD.itemsize and records.device == dev
    return work[:n], work[n:].view(torch.float32), records, gains


def _true_peak_launch(x, plan, lo, hi, max_hops, hop_peak):
    P = C.c_void_p
    _lib.check(_lib.lib().ixtts_true_peak(P(x.data_ptr()), x.numel(), P(plan.rows.data_ptr()), plan.n_rows, P(plan.reqs.data_ptr() + 8 * _lib.LOUDNESS_REQ_COLS * lo),
                                          P(plan.modes.data_ptr() + 8 * lo), hi - lo, max_hops, P(plan.tables.data_ptr()), P(hop_peak.data_ptr()), plan.slots,
                                          _lib.current_stream_ptr()), "ixtts_true_peak")


def _level_pass(x, plan, lo, hi, max_hops, true, energy, hop_peak, records, gains):
    """Programmes lo .. hi of `plan`: measurement, true peaks over the sample peaks where asked, gating and gain."""
    if hi <= lo:
        return
    L, P, s = _lib.lib(), C.c_void_p, _lib.current_stream_ptr()
    reqs = plan.reqs.data_ptr() + 8 * _lib.LOUDNESS_REQ_COLS * lo
    _lib.check(L.ixtts_loudness_measure(P(x.data_ptr()), x.numel(), P(plan.rows.data_ptr()), plan.n_rows, P(reqs),
                                        P(plan.coefs.data_ptr() + 8 * _lib.LOUDNESS_COEF_COLS * lo), hi - lo, max_hops, P(energy.data_ptr()),
                                        P(hop_peak.data_ptr()), plan.slots, s), "ixtts_loudness_measure")
    if true:
        _true_peak_launch(x, plan, lo, hi, max_hops, hop_peak)
    _lib.check(L.ixtts_loudness_gain(P(energy.data_ptr()), P(hop_peak.data_ptr()), plan.slots, P(reqs), P(plan.targets.data_ptr() + 16 * lo), hi - lo,
                                     P(records.data_ptr() + _RECORD.itemsize * lo), P(gains.data_ptr() + 4 * lo), s), "ixtts_loudness_gain")


def measure_levels(x, plan, records=None):
    """TWO launches for every programme of `plan`: the K-weighted energy and the sample peak of every hop (fp64 recursion over the fp32
    samples of `x`, through the gaps), then gating, integrated loudness and gain per programme.  -> (energy fp64 [plan.slots],
    hop_peak fp32 [plan.slots], records uint8 [24 n] (`_RECORD`; `records`: write there), gains fp32 [n]), all on the device: the
    gain reaches `pcm_assemble_gain` without visiting the host.  A plan with programmes in true mode: a third launch between the
    two puts their true hop peaks in place of the sample peaks."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    energy, hop_peak, records, gains = _level_buffers(plan, x.device, records)
    if plan.n == 0:
        return energy[:0], hop_peak[:0], records, gains[:0]
    _level_pass(x, plan, 0, plan.n, plan.max_hops, plan.any_true, energy, hop_peak, records, gains)
    return energy[:plan.slots], hop_peak[:plan.slots], records, gains[:plan.n + plan.n2]


def true_peaks(x, plan):
    """ONE launch: -> fp32 [plan.slots] on the device, the 4x-oversampled true peak of every hop (`true_peak_taps`) of the plan's
    programmes in true mode (`limits=` of `LevelPlan`), and 0 in every other slot."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    hop_peak = torch.zeros(max(plan.slots, 1), dtype=torch.float32, device=x.device)
    if plan.n and plan.max_hops:
        if plan.tables.numel() == 0:
            raise ValueError("true_peaks: the plan carries no interpolator (build it with limits=)")
        _true_peak_launch(x, plan, 0, plan.n, plan.max_hops, hop_peak)
    return hop_peak[:plan.slots]


def _limiter_launch(x, plan, gains, out, partials):
    P = C.c_void_p
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= plan.lim_total and out.device == x.device
    assert partials.dtype == torch.uint8 and partials.is_contiguous() and partials.numel() >= plan.partial_slots * _PARTIAL.itemsize
    assert partials.data_ptr() % 4 == 0 and partials.device == x.device
    if not plan.limited or plan.max_tiles == 0:
        return
    _lib.check(_lib.lib().ixtts_limiter(P(x.data_ptr()), x.numel(), P(plan.rows.data_ptr()), plan.n_rows, P(plan.lreqs.data_ptr()), P(plan.ceilings.data_ptr()),
                                        len(plan.limited), plan.max_tiles, P(plan.tables.data_ptr()), plan.tables.numel(),
                                        None if gains is None else P(gains.data_ptr()), 0 if gains is None else gains.numel(), P(out.data_ptr()),
                                        out.numel(), P(partials.data_ptr()), plan.partial_slots, _lib.current_stream_ptr()), "ixtts_limiter")


def limiter_stats(partials, plan):
    """What the limiter's tiles left (uint8 tensor or array of `_PARTIAL`) -> one (smallest gain fp32, samples with a gain below 1)
    per limited programme of `plan`, reduced in tile order; (1.0, 0) for a programme without samples."""
    raw = partials.cpu().numpy() if isinstance(partials, torch.Tensor) else np.asarray(partials)
    tiles = np.frombuffer(raw[:plan.partial_slots * _PARTIAL.itemsize].tobytes(), dtype=_PARTIAL)
    return [(np.float32(tiles["min_gain"][s:s + t].min()) if t else np.float32(1.0), int(tiles["count"][s:s + t].sum(dtype=np.int64))) for s, t in plan.tiles]


def limit(x, plan, gains=None):
    """ONE launch: every limited programme of `plan`, levelled by its entry of `gains` (fp32 on the device, indexed by programme;
    None: 1) and held under its ceiling by the look-ahead limiter -> (fp32 [plan.lim_total] on the device,
    programme q at `plan.lim_off[q]`, gaps and tail included; `limiter_stats` of the launch)."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert gains is None or (gains.dtype == torch.float32 and gains.is_contiguous() and gains.device == x.device)
    out = torch.empty(max(plan.lim_total, 1), dtype=torch.float32, device=x.device)
    partials = torch.empty(max(plan.partial_slots, 1) * _PARTIAL.itemsize, dtype=torch.uint8, device=x.device)
    _limiter_launch(x, plan, gains, out, partials)
    return out[:plan.lim_total], limiter_stats(partials, plan)


def read_records(records, n):
    """The records of `measure_levels` (a uint8 tensor or array) -> numpy structured array [n] of `_RECORD`."""
    raw = records.cpu().numpy() if isinstance(records, torch.Tensor) else np.asarray(records)
    return np.frombuffer(raw[:n * _RECORD.itemsize].tobytes(), dtype=_RECORD)


def pcm_assemble_gain(x, rows, total, encoding, gains, out=None):
    """`pcm_assemble` over rows (src, n, dst, index): a sample of a row with 0 <= index < len(gains) is the conversion of the fp32
    product gains[index] * x (one rounding; `gains`: fp32 on the device), any other index converts x as `pcm_assemble` does."""
    return _assemble(x, rows, total, encoding, gains, out)


def _programme(src, lens, gap, total, request):
    """What one request delivers -> (rows [(src, n, dst)], extent): segment k, `lens[k]` samples at `src[k]` of the arena, goes to dst,
    counted from the programme's start, with `gap` samples of silence between two segments; `extent` is what is delivered: `total`
    where one is given (silence fills the tail; ValueError when the segments and gaps are longer)."""
    rows, end = [], 0
    for k, (s, n) in enumerate(zip(src, lens)):
        end += gap if k else 0
        rows.append((s, n, end))
        end += n
    if total is not None:
        if int(total) < end:
            raise ValueError(f"request {request}: {end} samples of segments and gaps do not fit a total of {int(total)}")
        end = int(total)
    return rows, end


def finish(wav_lists, specs, interval_silence=200):
    """The segments of several requests (each a list of fp32 [1, n_i] device tensors at 22 050 Hz, +-32767) and one `OutputSpec` per
    request -> (results, reports): one `(sr, ndarray [N, 1])` per request, int16 or uint8 (None for a request without segments):
    segment, `int(sr * interval_silence / 1000)` samples of silence, segment ..., and one level report per request (None where no
    level was asked).  One resample launch per distinct target rate, one assemble launch per distinct encoding, then ONE copy to the
    host; the host waits for nothing before that copy.  A request's bytes and report depend on its own segments and spec alone.

    A spec with a level (`loudness` / `peak`, see `check_level`): the request's programme -- what it delivers, at its rate, gaps
    included -- is measured after the resample launches (`measure_levels`), and its samples are converted from the fp32 product
    gain * x; the records ride behind the PCM in the same buffer, so there is still one copy and no wait before it.  Its report is
    `level_report`.

    `total`: the request delivers exactly this many samples -- what follows its last segment holds the encoding's code for zero,
    and a measured programme extends over it.  ValueError, before any device work, when the segments are longer.

    `peak_mode` / `limiter` (see `check_limit`).  "true": the ceiling is held against the 4x-oversampled true peak (`true_peaks`,
    one launch between the measurement and the gating).  A limited programme gets the gain of its loudness target without give-way
    and is then held under its ceiling sample by sample (`limit`, one launch, into a third region of the arena, the programme
    contiguous with its gaps); the same kernels then measure the limited programme, for what the report says is delivered; it is
    converted as ONE row of that region without a gain.  Its second record and the limiter's per-tile numbers ride behind the first
    records: still one copy.  A spec whose `limits` are not ("sample", False) gets the report of `level_report_limit`."""
    results, reports = [None] * len(wav_lists), [None] * len(wav_lists)
    live = [i for i, w in enumerate(wav_lists) if w]
    if not live:
        return results, reports
    device = wav_lists[live[0]][0].device
    segs = {i: [w.to(device, torch.float32).reshape(-1) for w in wav_lists[i]] for i in live}
    n_in = sum(s.numel() for i in live for s in segs[i])
    # one fp32 arena: every segment as it left the vocoder, then every resampled segment, then every limited programme; a request's
    # programme reads its segments where they get converted from
    progs, by_rate, pos, n_rs = {}, {}, 0, 0
    for i in live:
        rate, src, lens = specs[i].rate, [], []
        for s in segs[i]:
            n = m = s.numel()
            if rate == MODEL_RATE:
                src.append(pos)
            else:
                m = resampled_len(n, MODEL_RATE, rate)
                by_rate.setdefault(rate, []).append((pos, n, n_rs))
                src.append(n_in + n_rs)
                n_rs += m
            lens.append(m)
            pos += n
        progs[i] = _programme(src, lens, gap_len(rate, interval_silence), specs[i].total, i)
    n_lim = sum(progs[i][1] for i in live if specs[i].limiter)
    arena = torch.empty(n_in + n_rs + n_lim, dtype=torch.float32, device=device)
    torch.cat([s for i in live for s in segs[i]], out=arena[:n_in])
    for rate, rows in by_rate.items():
        Resampler(rate, device).resample_into(arena[:n_in], arena[n_in:n_in + n_rs], rows)
    # one byte buffer for the call: per encoding one region (16-byte aligned), a request after a request, no gap between requests
    regions, where, nbytes = {}, {}, 0  # encoding -> (samples, byte offset); request -> its first sample in the region
    for enc in ENCODINGS:
        mine = [i for i in live if specs[i].encoding == enc]
        if not mine:
            continue
        total = 0
        for i in mine:
            where[i], total = total, total + progs[i][1]
        regions[enc] = (total, nbytes)
        nbytes = (nbytes + total * (2 if enc == "pcm_s16le" else 1) + 15) // 16 * 16
    # the requests with a level: programme q of the plan; their records, then the limiter's partials, go behind the PCM
    asked = [i for i in live if specs[i].leveled]
    plan = gains = None
    if asked:
        plan = LevelPlan([progs[i] + (specs[i].rate, specs[i].loudness, specs[i].peak) for i in asked], device, [specs[i].limits for i in asked],
                         n_in + n_rs)
        assert plan.lim_total == n_lim
        rec_off, nbytes = nbytes, nbytes + (plan.n + plan.n2) * _RECORD.itemsize
        part_off, nbytes = nbytes, nbytes + plan.partial_slots * _PARTIAL.itemsize
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if asked:
        energy, hop_peak, records, gains = _level_buffers(plan, device, buf[rec_off:part_off])
        _level_pass(arena, plan, 0, plan.n, plan.max_hops, plan.any_true, energy, hop_peak, records, gains)
        if plan.limited:
            _limiter_launch(arena, plan, gains, arena[n_in + n_rs:], buf[part_off:])
            _level_pass(arena, plan, plan.n, plan.n + plan.n2, plan.max_hops2, plan.any_true2, energy, hop_peak, records, gains)
    index = {i: q for q, i in enumerate(asked)}
    for enc, (total, off) in regions.items():
        region = buf[off:off + total * (2 if enc == "pcm_s16le" else 1)]
        region = region.view(torch.int16) if enc == "pcm_s16le" else region
        rows = []
        for i in live:
            if specs[i].encoding != enc:
                continue
            q = index.get(i, -1)
            if plan is not None and q in plan.lim_off:  # ONE row: the limited programme as the limiter wrote it
                rows.append((n_in + n_rs + plan.lim_off[q], progs[i][1], where[i], -1))
            else:
                rows += [(s, n, where[i] + d, q) for s, n, d in progs[i][0]]
        if any(specs[i].encoding == enc for i in asked):
            pcm_assemble_gain(arena, rows, total, enc, gains, out=region)
        else:  # (nobody in this encoding has a gain: the three-column kernel)
            pcm_assemble(arena, [r[:3] for r in rows], total, enc, out=region)
    host = buf.cpu().numpy()  # the one copy (it waits for the stream)
    if asked:
        recs = read_records(host[rec_off:], plan.n + plan.n2)
        stats = dict(zip(plan.limited, limiter_stats(host[part_off:], plan)))
        for q, i in enumerate(asked):
            sp = specs[i]
            if sp.limits == ("sample", False):
                reports[i] = level_report(recs[q], sp.loudness)
            elif q in stats:
                reports[i] = level_report_limit(recs[q], sp.loudness, sp.peak_mode, True, progs[i][1], stats[q], recs[plan.n + plan.limited.index(q)])
            else:
                reports[i] = level_report_limit(recs[q], sp.loudness, sp.peak_mode, False)
    for i in live:
        total, off = regions[specs[i].encoding]
        if specs[i].encoding == "pcm_s16le":
            pcm = host[off:off + total * 2].view(np.int16)[where[i]:where[i] + progs[i][1]]
        else:
            pcm = host[off + where[i]:off + where[i] + progs[i][1]]
        results[i] = (specs[i].rate, pcm.copy().reshape(-1, 1))
    return results, reports


def finish_pcm_many(wav_lists, sample_rates, encodings, interval_silence=200, loudness=None, peak=None, reports=None, totals=None, peak_mode=None,
                    limiter=None):
    """`finish` with the specs spelt as parallel lists (one entry per request, None: not asked; a list left out: nobody asked):
    what `OutputSpec.of` takes, and `totals`.  Every request goes through the stage, 22 050 Hz `pcm_s16le` where it asks for nothing.
    -> the results; `reports`: a list that receives the reports."""
    absent = [None] * len(sample_rates)
    specs = [OutputSpec.of(*asks, duration=True)._replace(total=total) for *asks, total in
             zip(sample_rates, encodings, loudness or absent, peak or absent, peak_mode or absent, limiter or absent, totals or absent)]
    results, levels = finish(wav_lists, specs, interval_silence)
    if reports is not None:
        reports[:] = levels
    return results


def finish_pcm(wavs, sample_rate=None, encoding=None, interval_silence=200, loudness=None, peak=None, reports=None, total=None, peak_mode=None,
               limiter=None):
    """One request's segments -> `(sr, ndarray [N, 1])`, int16 (`pcm_s16le`) or uint8 (`mulaw`, `alaw`); sr = the requested rate, or
    22050.  See `finish_pcm_many`."""
    return finish_pcm_many([list(wavs)], [sample_rate], [encoding], interval_silence, [loudness], [peak], reports, [total], [peak_mode], [limiter])[0]


def wav_bytes(sr, pcm, encoding=None):
    """The RIFF/WAVE file of a result.  pcm_s16le: what `wave` writes.  G.711: format tag 7 (mu-law) / 6 (A-law), 8 bits, the 18-byte
    `fmt ` chunk (cbSize 0) and the `fact` chunk non-PCM formats carry, a pad byte behind an odd `data` chunk."""
    sr, encoding = int(sr), check_format(None, encoding)[1]
    pcm = np.asarray(pcm)
    channels = pcm.shape[1] if pcm.ndim == 2 else 1
    if encoding == "pcm_s16le":
        buf = io.BytesIO()
        with wave.open(buf, "wb") as w:
            w.setnchannels(channels)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes(pcm.astype("<i2").tobytes())
        return buf.getvalue()
    data = pcm.astype(np.uint8).tobytes()
    pad = len(data) & 1
    fmt = struct.pack("<HHIIHHH", WAVE_FORMAT_TAGS[encoding], channels, sr, sr * channels, channels, 8, 0)
    fact = struct.pack("<I", len(data) // channels)
    body = (b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<I", len(fact)) + fact
            + b"data" + struct.pack("<I", len(data)) + data + b"\0" * pad)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def riff_info(buf):
    """The header of a RIFF/WAVE byte string, chunk by chunk -> dict(tag, channels, rate, bits, cb_size, fact, data_bytes, frames,
    padded) (`fact`: the sample count of that chunk or None; `padded`: every chunk ends on an even offset and the RIFF size is the
    file's)."""
    if buf[:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise ValueError("not a RIFF/WAVE byte string")
    info = dict(fact=None, cb_size=None, padded=struct.unpack("<I", buf[4:8])[0] + 8 == len(buf) and len(buf) % 2 == 0)
    pos = 12
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], struct.unpack("<I", buf[pos + 4:pos + 8])[0]
        body = buf[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            info["tag"], info["channels"], info["rate"], _, info["block_align"], info["bits"] = struct.unpack("<HHIIHH", body[:16])
            if size >= 18:
                info["cb_size"] = struct.unpack("<H", body[16:18])[0]
        elif cid == b"fact":
            info["fact"] = struct.unpack("<I", body[:4])[0]
        elif cid == b"data":
            info["data_bytes"] = size
            info["frames"] = size // info["block_align"]
        pos += 8 + size + (size & 1)
    return info


# ------------------------------------------------------------------------------------------------- G.711 on the host (reference)
def g711_encode(pcm16, encoding):
    """ITU-T G.711 of int16 samples in numpy, from the standard's segment tables: the CPU reference the device conversion is held to
    (equal to `audioop.lin2ulaw(b, 2)` / `lin2alaw(b, 2)` for all 65 536 inputs)."""
    s = np.asarray(pcm16).astype(np.int32)
    if encoding == "mulaw":
        v = s >> 2  # 14-bit
        mask = np.where(v < 0, 0x7F, 0xFF)
        v = np.minimum(np.abs(v), 8159) + 0x21  # clip, bias
        seg = np.searchsorted(np.array([0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF]), v, side="left")
        code = np.where(seg >= 8, 0x7F, (np.minimum(seg, 7) << 4) | ((v >> (np.minimum(seg, 7) + 1)) & 0xF))
    elif encoding == "alaw":
        v = s >> 3  # 13-bit
        mask = np.where(v >= 0, 0xD5, 0x55)
        v = np.where(v < 0, -v - 1, v)
        seg = np.searchsorted(np.array([0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF]), v, side="left")
        sg = np.minimum(seg, 7)
        code = np.where(seg >= 8, 0x7F, (sg << 4) | ((v >> np.where(sg < 2, 1, sg)) & 0xF))
    else:
        raise ValueError(f"g711_encode: {encoding!r} is not 'mulaw' or 'alaw'")
    return (code ^ mask).astype(np.uint8)
