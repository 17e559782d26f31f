"""The output stage: what leaves the vocoder (fp32 rows at 22 050 Hz, scaled to +-32767) becomes the sample rate and sample encoding
the caller asked for, ON THE DEVICE (csrc/output.hip), and reaches the host in one copy.

  resample_taps     the Hann-windowed sinc table of `torchaudio.transforms.Resample` -- the ONE builder; `prompt.sinc_resample` (the
                    CPU restatement used on the prompt side) and the device resampler both take their table from it
  Resampler         packed rows of unequal length -> the requested rate, one launch for all of them
  pcm_assemble      rows -> one buffer of int16 / G.711 bytes, the gaps (interval silence) holding the encoding's code for zero
  finish_pcm(_many) the tail of `infer` / `infer_many`: resample, convert, lay out, copy to the host once
  k_weighting       the two biquads of ITU-R BS.1770 at a sample rate -- the ONE builder, for the measurement kernel and the tests
  measure_levels    K-weighted hop energies and sample peak of every programme of a call, then gating and gain: two launches
  pcm_assemble_gain `pcm_assemble` with a gain per row, read from the device
  wav_bytes         the RIFF container of a result

With nothing requested none of this runs: `infer` keeps its host-side cat and `.type(torch.int16)`.
"""
import ctypes as C
import io
import math
import struct
import wave

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


def pcm_assemble(x, rows, total, encoding, out=None):
    """ONE launch: `total` samples of `encoding` -- x[src : src + n] converted at [dst, dst + n) for every (src, n, dst) of `rows`
    (ascending in dst, disjoint), the encoding's code for silence everywhere else.  -> int16 / uint8 [total] on x's device (`out`:
    write into this tensor's first `total` elements instead)."""
    if encoding not in ENCODINGS:
        raise ValueError(f"output encoding {encoding!r} is not one of {ENCODINGS}")
    assert x.dtype == torch.float32 and x.is_contiguous()
    rows = sorted(((int(s), int(n), int(d)) for s, n, d in rows), key=lambda r: (r[2], r[1]))
    end = 0
    for s, n, d in rows:
        if s < 0 or n < 0 or d < end or s + n > x.numel() or d + n > total:
            raise ValueError(f"assemble row (src={s}, n={n}, dst={d}) overlaps its neighbour or leaves its buffers ({x.numel()} in, {total} out)")
        end = d + n
    dtype = torch.int16 if encoding == "pcm_s16le" else torch.uint8
    if out is None:
        out = torch.empty(int(total), dtype=dtype, device=x.device)
    assert out.dtype == dtype and out.is_contiguous() and out.numel() >= total and out.device == x.device
    table = _row_table(rows if rows else [(0, 0, 0)], x.device)
    _lib.check(_lib.lib().ixtts_pcm_assemble(C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(out.data_ptr()), int(total),
                                             C.c_void_p(table.data_ptr()), len(rows), _lib.PCM_ENCODINGS[encoding], _lib.current_stream_ptr()),
               "ixtts_pcm_assemble")
    return out


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


class LevelPlan:
    """The tables of `measure_levels` for the programmes of a call: programme q = (rows [(src, n, dst)] with dst counted from the
    programme's start, ascending and disjoint; extent; sample rate; loudness target | None; ceiling | None).  Everything goes up in
    ONE pinned copy; `rows`, `reqs`, `coefs`, `targets` are views of it."""

    def __init__(self, programmes, device):
        rows, reqs, coefs, targets, at, slot = [], [], [], [], 0, 0
        self.hops = []
        for prog_rows, extent, rate, loudness, peak in programmes:
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
            targets.append([math.nan if loudness is None else loudness, math.nan if peak is None else peak])
            self.hops.append((slot, hops, extent // H))
            at, slot = at + extent, slot + hops
        self.n, self.slots, self.max_hops, self.n_rows = len(reqs), slot, max([h for _, h, _ in self.hops], default=0), len(rows)
        ints = np.array([v for r in rows for v in r] + [v for r in reqs for v in r], np.int64)
        blob = torch.from_numpy(np.concatenate([ints, np.array([v for r in coefs + targets for v in r], np.float64).view(np.int64)]))
        if torch.device(device).type == "cuda":
            blob = blob.pin_memory()
        blob = blob.to(device, non_blocking=True)
        a, b = 3 * len(rows), 3 * len(rows) + _lib.LOUDNESS_REQ_COLS * self.n
        c = b + _lib.LOUDNESS_COEF_COLS * self.n
        self.rows, self.reqs = blob[:a], blob[a:b]
        self.coefs, self.targets = blob[b:c].view(torch.float64), blob[c:].view(torch.float64)


def measure_levels(x, plan, records=None):
    """TWO launches for every programme of `plan`: the K-weighted energy and the sample peak of every hop (fp64 recursion over the fp32
    samples of `x`, through the gaps), then gating, integrated loudness and gain per programme.  -> (energy fp64 [plan.slots],
    hop_peak fp32 [plan.slots], records uint8 [24 n] (`_RECORD`; `records`: write there), gains fp32 [n]), all on the device: the
    gain reaches `pcm_assemble_gain` without visiting the host."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    dev = x.device
    n = max(plan.slots, 1)
    work = torch.zeros(n + (n + 1) // 2, dtype=torch.float64, device=dev)  # (one fill: a hop the kernel skips reads as silence)
    energy, hop_peak = work[:n], work[n:].view(torch.float32)
    gains = torch.empty(max(plan.n, 1), dtype=torch.float32, device=dev)
    if records is None:
        records = torch.empty(plan.n * _RECORD.itemsize, dtype=torch.uint8, device=dev)
    assert records.dtype == torch.uint8 and records.is_contiguous() and records.numel() >= plan.n * _RECORD.itemsize and records.device == dev
    if plan.n == 0:
        return energy[:0], hop_peak[:0], records, gains[:0]
    L, P, s = _lib.lib(), C.c_void_p, _lib.current_stream_ptr()
    _lib.check(L.ixtts_loudness_measure(P(x.data_ptr()), x.numel(), P(plan.rows.data_ptr()), plan.n_rows, P(plan.reqs.data_ptr()), P(plan.coefs.data_ptr()),
                                        plan.n, plan.max_hops, P(energy.data_ptr()), P(hop_peak.data_ptr()), plan.slots, s), "ixtts_loudness_measure")
    _lib.check(L.ixtts_loudness_gain(P(energy.data_ptr()), P(hop_peak.data_ptr()), plan.slots, P(plan.reqs.data_ptr()), P(plan.targets.data_ptr()), plan.n,
                                     P(records.data_ptr()), P(gains.data_ptr()), s), "ixtts_loudness_gain")
    return energy[:plan.slots], hop_peak[:plan.slots], records, gains


def read_records(records, n):
    """The records of `measure_levels` (a uint8 tensor or array) -> numpy structured array [n] of `_RECORD`."""
    raw = records.cpu().numpy() if isinstance(records, torch.Tensor) else np.asarray(records)
    return np.frombuffer(raw[:n * _RECORD.itemsize].tobytes(), dtype=_RECORD)


def pcm_assemble_gain(x, rows, total, encoding, gains, out=None):
    """`pcm_assemble` over rows (src, n, dst, index): a sample of a row with 0 <= index < len(gains) is the conversion of the fp32
    product gains[index] * x (one rounding; `gains`: fp32 on the device), any other index converts x as `pcm_assemble` does."""
    if encoding not in ENCODINGS:
        raise ValueError(f"output encoding {encoding!r} is not one of {ENCODINGS}")
    assert x.dtype == torch.float32 and x.is_contiguous() and gains.dtype == torch.float32 and gains.is_contiguous() and gains.device == x.device
    rows = sorted(((int(s), int(n), int(d), int(g)) for s, n, d, g in rows), key=lambda r: (r[2], r[1]))
    end = 0
    for s, n, d, _ in rows:
        if s < 0 or n < 0 or d < end or s + n > x.numel() or d + n > total:
            raise ValueError(f"assemble row (src={s}, n={n}, dst={d}) overlaps its neighbour or leaves its buffers ({x.numel()} in, {total} out)")
        end = d + n
    dtype = torch.int16 if encoding == "pcm_s16le" else torch.uint8
    if out is None:
        out = torch.empty(int(total), dtype=dtype, device=x.device)
    assert out.dtype == dtype and out.is_contiguous() and out.numel() >= total and out.device == x.device
    table = _row_table(rows if rows else [(0, 0, 0, -1)], x.device, 4)
    _lib.check(_lib.lib().ixtts_pcm_assemble_gain(C.c_void_p(x.data_ptr()), x.numel(), C.c_void_p(out.data_ptr()), int(total), C.c_void_p(table.data_ptr()),
                                                  len(rows), C.c_void_p(gains.data_ptr()), gains.numel(), _lib.PCM_ENCODINGS[encoding],
                                                  _lib.current_stream_ptr()), "ixtts_pcm_assemble_gain")
    return out


def finish_pcm_many(wav_lists, sample_rates, encodings, interval_silence=200, loudness=None, peak=None, reports=None, totals=None):
    """The segments of several requests (each a list of fp32 [1, n_i] device tensors at 22 050 Hz, +-32767) -> one
    `(sr, ndarray [N, 1])` per request, int16 or uint8 (None for a request without segments): segment, `int(sr * interval_silence /
    1000)` samples of silence, segment ...  One resample launch per distinct target rate, one assemble launch per distinct
    encoding, then ONE copy to the host; the host waits for nothing before that copy.  A request's bytes depend on its own
    segments, rate and encoding alone.

    `loudness` / `peak` (one entry per request, None: not asked; see `check_level`): the request's programme -- what it delivers, at
    its rate, gaps included -- is measured after the resample launches (`measure_levels`), and its samples are converted from the
    fp32 product gain * x; the records ride behind the PCM in the same buffer, so there is still one copy and no wait before it.
    `reports`: a list that receives one `level_report` per request (None where no control was asked).  A request without a control
    produces the bytes it produces without these arguments.

    `totals` (one entry per request, None: not asked): the request delivers exactly this many samples -- what follows its last
    segment holds the encoding's code for zero, and a measured programme extends over it.  ValueError when the segments are longer."""
    fmts = [check_format(sr, enc) for sr, enc in zip(sample_rates, encodings)]
    levels = [check_level(lo, pk) for lo, pk in zip(loudness or [None] * len(fmts), peak or [None] * len(fmts))]
    if reports is not None:
        reports[:] = [None] * len(wav_lists)
    live = [i for i, w in enumerate(wav_lists) if w]
    if not live:
        return [None] * len(wav_lists)
    device = wav_lists[live[0]][0].device
    segs = [[w.to(device, torch.float32).reshape(-1) for w in wav_lists[i]] for i in live]
    n_in = sum(s.numel() for ws in segs for s in ws)
    n_rs = sum(resampled_len(s.numel(), MODEL_RATE, fmts[i][0]) for i, ws in zip(live, segs) for s in ws if fmts[i][0] != MODEL_RATE)
    # one fp32 arena: every segment as it left the vocoder, then every resampled segment
    arena = torch.empty(n_in + n_rs, dtype=torch.float32, device=device)
    torch.cat([s for ws in segs for s in ws], out=arena[:n_in])
    src, pos, at = {}, 0, 0  # (request, segment) -> (offset in the arena, samples) of what gets converted
    by_rate = {}
    for i, ws in zip(live, segs):
        for k, s in enumerate(ws):
            n = s.numel()
            if fmts[i][0] == MODEL_RATE:
                src[i, k] = (pos, n)
            else:
                m = resampled_len(n, MODEL_RATE, fmts[i][0])
                by_rate.setdefault(fmts[i][0], []).append((pos, n, at))
                src[i, k] = (n_in + at, m)
                at += m
            pos += n
    for rate, rows in by_rate.items():
        Resampler(rate, device).resample_into(arena[:n_in], arena[n_in:], rows)
    # one byte buffer for the call: per encoding one region (16-byte aligned), a request after a request, no gap between requests
    by_enc, where, nbytes = {}, {}, 0
    for enc in ENCODINGS:
        mine = [i for i in live if fmts[i][1] == enc]
        if not mine:
            continue
        rows, total = [], 0
        for i in mine:
            start, gap = total, gap_len(fmts[i][0], interval_silence)
            for k in range(len(wav_lists[i])):
                total += gap if k else 0
                rows.append((src[i, k][0], src[i, k][1], total))
                total += src[i, k][1]
            if totals is not None and totals[i] is not None:
                if int(totals[i]) < total - start:
                    raise ValueError(f"request {i}: {total - start} samples of segments and gaps do not fit a total of {int(totals[i])}")
                total = start + int(totals[i])
            where[i] = (enc, start, total - start)
        width = 2 if enc == "pcm_s16le" else 1
        by_enc[enc] = (rows, total, nbytes)
        nbytes = (nbytes + total * width + 15) // 16 * 16
    # the requests with a level control: programme q of the plan; their records go behind the PCM
    asked = [i for i in live if levels[i] is not None]
    plan = gains = None
    if asked:
        progs = []
        for i in asked:
            at, gap, mine = 0, gap_len(fmts[i][0], interval_silence), []
            for k in range(len(wav_lists[i])):
                at += gap if k else 0
                mine.append((src[i, k][0], src[i, k][1], at))
                at += src[i, k][1]
            if totals is not None and totals[i] is not None:
                at = max(at, int(totals[i]))  # the trailing silence is part of what is delivered
            progs.append((mine, at, fmts[i][0], levels[i][0], levels[i][1]))
        plan = LevelPlan(progs, device)
        rec_off, nbytes = nbytes, nbytes + plan.n * _RECORD.itemsize
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    if asked:
        gains = measure_levels(arena, plan, records=buf[rec_off:])[3]
    for enc, (rows, total, off) in by_enc.items():
        width = 2 if enc == "pcm_s16le" else 1
        region = buf[off:off + total * width]
        region = region.view(torch.int16) if width == 2 else region
        if any(fmts[i][1] == enc for i in asked):
            index = [asked.index(i) if i in asked else -1 for i in live if fmts[i][1] == enc for _ in wav_lists[i]]
            pcm_assemble_gain(arena, [r + (g,) for r, g in zip(rows, index)], total, enc, gains, out=region)
        else:
            pcm_assemble(arena, rows, total, enc, out=region)
    host = buf.cpu().numpy()  # the one copy (it waits for the stream)
    if asked and reports is not None:
        for i, rec in zip(asked, read_records(host[rec_off:], plan.n)):
            reports[i] = level_report(rec, levels[i][0])
    out = [None] * len(wav_lists)
    for i in live:
        enc, start, n = where[i]
        off = by_enc[enc][2]
        if enc == "pcm_s16le":
            pcm = host[off:off + by_enc[enc][1] * 2].view(np.int16)[start:start + n]
        else:
            pcm = host[off + start:off + start + n]
        out[i] = (fmts[i][0], pcm.copy().reshape(-1, 1))
    return out


def finish_pcm(wavs, sample_rate=None, encoding=None, interval_silence=200, loudness=None, peak=None, reports=None, total=None):
    """One request's segments -> `(sr, ndarray [N, 1])`, int16 (`pcm_s16le`) or uint8 (`mulaw`, `alaw`); sr = the requested rate, or
    22050.  See `finish_pcm_many`."""
    if total is not None:
        return finish_pcm_many([list(wavs)], [sample_rate], [encoding], interval_silence, [loudness], [peak], reports, totals=[total])[0]
    if loudness is None and peak is None:
        return finish_pcm_many([list(wavs)], [sample_rate], [encoding], interval_silence)[0]
    return finish_pcm_many([list(wavs)], [sample_rate], [encoding], interval_silence, [loudness], [peak], reports)[0]


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
