"""The output stage: what leaves the vocoder (fp32 rows at 22 050 Hz, scaled to +-32767) becomes the sample rate and sample encoding
the caller asked for, ON THE DEVICE (csrc/output.hip), and reaches the host in one copy.

  resample_taps     the Hann-windowed sinc table of `torchaudio.transforms.Resample` -- the ONE builder; `prompt.sinc_resample` (the
                    CPU restatement used on the prompt side) and the device resampler both take their table from it
  Resampler         packed rows of unequal length -> the requested rate, one launch for all of them
  pcm_assemble      rows -> one buffer of int16 / G.711 bytes, the gaps (interval silence) holding the encoding's code for zero
  finish_pcm(_many) the tail of `infer` / `infer_many`: resample, convert, lay out, copy to the host once
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


def _row_table(rows, device):
    """[(src, n, dst)] -> int64 [R, 3] on the device, copied from pinned memory so that the host does not wait for the stream."""
    t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 3)
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


def finish_pcm_many(wav_lists, sample_rates, encodings, interval_silence=200):
    """The segments of several requests (each a list of fp32 [1, n_i] device tensors at 22 050 Hz, +-32767) -> one
    `(sr, ndarray [N, 1])` per request, int16 or uint8 (None for a request without segments): segment, `int(sr * interval_silence /
    1000)` samples of silence, segment ...  One resample launch per distinct target rate, one assemble launch per distinct
    encoding, then ONE copy to the host; the host waits for nothing before that copy.  A request's bytes depend on its own
    segments, rate and encoding alone."""
    fmts = [check_format(sr, enc) for sr, enc in zip(sample_rates, encodings)]
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
            where[i] = (enc, start, total - start)
        width = 2 if enc == "pcm_s16le" else 1
        by_enc[enc] = (rows, total, nbytes)
        nbytes = (nbytes + total * width + 15) // 16 * 16
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    for enc, (rows, total, off) in by_enc.items():
        width = 2 if enc == "pcm_s16le" else 1
        region = buf[off:off + total * width]
        pcm_assemble(arena, rows, total, enc, out=region.view(torch.int16) if width == 2 else region)
    host = buf.cpu().numpy()  # the one copy (it waits for the stream)
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


def finish_pcm(wavs, sample_rate=None, encoding=None, interval_silence=200):
    """One request's segments -> `(sr, ndarray [N, 1])`, int16 (`pcm_s16le`) or uint8 (`mulaw`, `alaw`); sr = the requested rate, or
    22050.  See `finish_pcm_many`."""
    return finish_pcm_many([list(wavs)], [sample_rate], [encoding], interval_silence)[0]


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
