"""Yardstick of the output stage's level control, shared by its tests: the meter of ITU-R BS.1770-4 in fp64, run sequentially over the
laid-out programme (`scipy.signal.lfilter` from zero state, through the gaps), on the product's own coefficients
(`output.k_weighting`), and the gain rule for a loudness target under a sample-peak ceiling."""
import numpy as np
from scipy.signal import lfilter

from voice_tts_amd import output as O

CEILING_BOUND, NO_BLOCK = 1, 2


def lay_out(segments, gap):
    """Segments (fp32, the +-32767 scale) -> the programme in sample units, fp32: segment, `gap` zeros, segment ..."""
    parts = []
    for k, s in enumerate(segments):
        if k:
            parts.append(np.zeros(gap, np.float32))
        parts.append(np.asarray(s, np.float32).reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def k_weighted(programme, fs):
    """The programme (sample units) -> its K-weighted signal in full-scale units, fp64."""
    b_s, a_s, b_h, a_h = O.k_weighting(fs)
    x = np.asarray(programme, np.float64) / 32768.0
    return lfilter(b_h, a_h, lfilter(b_s, a_s, x)) if x.size else x


def hop_energies(programme, fs):
    """-> fp64 [len // H]: the sum of squares of the K-weighted signal over every full hop (a trailing partial hop belongs to no block)."""
    H = O.hop_len(fs)
    y = k_weighted(programme, fs)
    n = y.size // H
    return (y[:n * H].reshape(n, H) ** 2).sum(1)


def block_powers(e, H):
    e = np.asarray(e, np.float64)
    if e.size < 4:
        return np.zeros(0)
    return (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * H)


def integrated(e, H):
    """Hop energies -> the gated integrated loudness in LUFS, or None (fewer than 4 hops, or no block above -70 LUFS)."""
    z = block_powers(e, H)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
    keep = l > -70.0
    if not keep.any():
        return None
    gamma = -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    keep &= l > gamma
    return float(-0.691 + 10.0 * np.log10(z[keep].mean()))


def loudness(programme, fs):
    return integrated(hop_energies(programme, fs), O.hop_len(fs))


def gain(L, p, target=None, ceiling=None):
    """-> (g fp64, flags): g = 10^((target - L) / 20) with a target and an L, else 1; with a ceiling (dBFS) and g p above
    32768 10^(ceiling / 20), that over p (p: the sample peak in sample units)."""
    g = 10.0 ** ((target - L) / 20.0) if target is not None and L is not None else 1.0
    flags = NO_BLOCK if L is None else 0
    if ceiling is not None:
        c = 32768.0 * 10.0 ** (ceiling / 20.0)
        if g * p > c:
            g, flags = c / p, flags | CEILING_BOUND
    return g, flags


def pcm_s16(v):
    """The existing conversion of fp32 values: clamp to the int16 range, truncate toward zero."""
    return np.clip(np.asarray(v, np.float32), -32768.0, 32767.0).astype(np.int16)


def encode(v, enc):
    s = pcm_s16(v)
    return s if enc == "pcm_s16le" else O.g711_encode(s, enc)


# ------------------------------------------------------------------------------------------ test programmes, shared by the GPU tests
def noise(n, fs, seed, rms=3000.0):
    """Seeded Gaussian noise under a slow amplitude envelope (0.2 .. 1), fp32 on the +-32767 scale."""
    t = np.arange(n) / float(fs)
    x = np.random.default_rng(seed).standard_normal(n) * rms * (0.2 + 0.8 * np.abs(np.sin(2 * np.pi * 1.3 * t + seed)))
    return np.clip(x, -32767.0, 32767.0).astype(np.float32)


def pack(programmes, lead=3):
    """[(segments, gap)] -> (x fp32: every segment behind `lead` samples of filler, [(rows [(src, n, dst)], extent)]): the arena and
    the row tables `output.LevelPlan` takes, dst counted from each programme's start."""
    parts, out, at = [np.full(lead, 12345.0, np.float32)], [], lead
    for segments, gap in programmes:
        rows, d = [], 0
        for k, s in enumerate(segments):
            d += gap if k else 0
            rows.append((at, len(s), d))
            parts.append(np.asarray(s, np.float32))
            at, d = at + len(s), d + len(s)
        out.append((rows, d))
    return np.concatenate(parts), out
