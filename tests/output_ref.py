"""Yardstick of the output stage's resampler, shared by its GPU tests: fp64 arithmetic on the SAME fp32 tap table, and the a-priori
error bound of an fp32 dot product over the table's widest band."""
import numpy as np

from voice_tts_amd import output as O

U = 2.0 ** -24


def gamma(n):
    """gamma_n = n u / (1 - n u): the bound of an fp32 dot product of n terms in any order, with or without FMA."""
    return n * U / (1 - n * U)


def resample_fp64(x, sr):
    """x: fp32 [n] at 22 050 Hz -> (clamp(y64) [ceil(n new / orig)], bound [same]): y64[j] = sum_k h[p][k] xpad[q orig + k] in fp64,
    bound[j] = gamma_band * sum_k |h[p][k]| |xpad[q orig + k]|."""
    h, width = O.resample_taps(22050, sr, "cpu")
    h = h[:, 0].double().numpy()
    orig, new = O.resample_ratio(22050, sr)
    K = h.shape[1]
    band = O.tap_bands(22050, sr)[2]
    x = np.asarray(x, np.float64).reshape(-1)
    m = O.resampled_len(x.size, 22050, sr)
    j = np.arange(m)
    q, p = j // new, j % new
    xp = np.concatenate([np.zeros(width), x, np.zeros(int(q.max(initial=0)) * orig + K)])
    win = np.lib.stride_tricks.sliding_window_view(xp, K)[q * orig]
    y = (h[p] * win).sum(1)
    bound = gamma(band) * (np.abs(h[p]) * np.abs(win)).sum(1)
    return np.clip(y, -32767.0, 32767.0), bound
