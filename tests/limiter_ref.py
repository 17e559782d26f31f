"""Yardstick of the output stage's true peak and limiter, shared by their tests: the definitions of DESIGN 4.3d in numpy fp64, written
sequentially over the whole laid-out programme, on the product's own tables (`output.true_peak_taps`, `output.limiter_window`).  The
meter, the gain rule and the conversion are those of tests/loudness_ref.py."""
import numpy as np

from loudness_ref import encode, gain, lay_out, loudness, pcm_s16  # noqa: F401  (the tests take them from here)
from voice_tts_amd import output as O


def levelled(programme, g=1.0):
    """y = fp32(g32 * x): the programme under its gain, one rounding."""
    return (np.float32(g) * np.asarray(programme, np.float32)).astype(np.float32)


def interpolate(y):
    """-> z fp64 [N, 4]: z[n, k] = the point n + k / 4 = sum_j h[k - 4 j] y[n + j] over the taps that exist, ascending j, zeros
    outside [0, N); k = 0 is the sample itself."""
    h = O.true_peak_taps()
    y = np.asarray(y, np.float32)
    N, R = y.size, 7
    pad = np.concatenate([np.zeros(R), y.astype(np.float64), np.zeros(R)])
    z = np.zeros((N, 4))
    z[:, 0] = y
    for k in (1, 2, 3):
        acc = np.zeros(N)
        for j in range(-R, R + 1):
            if abs(k - 4 * j) <= 24:
                acc = acc + h[k - 4 * j + 24] * pad[R + j:R + j + N]
        z[:, k] = acc
    return z


def true_peak(y):
    y = np.asarray(y, np.float32)
    return float(np.abs(interpolate(y)).max()) if y.size else 0.0


def hop_true_peaks(y, fs):
    """-> fp32 [ceil(N / H)]: the largest |z| over the points whose n lies in the hop (a trailing partial hop over what it has)."""
    H = O.hop_len(fs)
    z = np.abs(interpolate(y)).max(1)
    return np.array([z[a:a + H].max() for a in range(0, z.size, H)], np.float64).astype(np.float32)


def hop_sample_peaks(y, fs):
    H = O.hop_len(fs)
    y = np.abs(np.asarray(y, np.float32))
    return np.array([y[a:a + H].max() for a in range(0, y.size, H)], np.float32)


def detector(y, mode):
    """p[n]: |y[n]|; in true mode the largest |z| over the points n - 3/4 .. n + 3/4 (a point between two samples is charged to both)."""
    y = np.asarray(y, np.float32)
    p = np.abs(y.astype(np.float64))
    if mode == "true" and y.size:
        q = np.abs(interpolate(y)[:, 1:]).max(1)
        p = np.maximum(p, q)
        p[1:] = np.maximum(p[1:], q[:-1])
    return p


def limit(y, fs, peak, mode="sample"):
    """The limiter over the levelled programme y (fp32) -> dict(r, m (over [-W, N + W)), a, a32, out fp32, smallest, count)."""
    y = np.asarray(y, np.float32)
    N, W, c, w = y.size, O.lookaround(fs), O.ceiling(peak), O.limiter_window(fs)
    p = detector(y, mode)
    r = np.ones(N)
    r[p > 0] = np.minimum(1.0, c / p[p > 0])
    ext = np.concatenate([np.ones(2 * W), r, np.ones(2 * W)])  # r over [-2W, N + 2W)
    m = np.array([ext[i:i + 2 * W + 1].min() for i in range(N + 2 * W)]) if N + 2 * W <= 4096 else \
        np.lib.stride_tricks.sliding_window_view(ext, 2 * W + 1).min(1)
    d = 1.0 - m
    s = np.zeros(N)
    for k in range(2 * W + 1):
        s = s + w[k] * d[k:k + N]
    a = 1.0 - s
    a32 = a.astype(np.float32)
    over = a32.astype(np.float64) > r
    a32[over] = np.nextafter(a32[over], np.float32(0.0))
    return dict(r=r, m=m, a=a, a32=a32, out=(a32 * y).astype(np.float32), smallest=np.float32(a32.min()) if N else np.float32(1.0),
                count=int((a32 < 1.0).sum()))


def ulps(a, b):
    """fp32 arrays -> the distance of every pair in units in the last place (through the ordered integers, so across zero too)."""
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
