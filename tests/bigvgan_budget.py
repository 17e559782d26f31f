"""The cases of the BigVGAN error budget, shared by tests/test_bigvgan_twin.py (fp32 CPU oracle against its fp64 twin),
tests/test_gpu_bigvgan_fp64.py (the device against the twin, every conv tile forced) and tools/bigvgan_error_budget.py (which records the
numbers in profiles/bigvgan_error_budget.json).

The twin is `oracle.vocoder.bigvgan_forward(..., dtype=torch.float64)`: the fp32 weights, mel and filter taps widened, every operation in
fp64.  The fp32 CPU leg is the same function at its default.  Weights and mel are drawn once in fp32, so all legs see the same numbers;
outputs come back as fp64 CPU tensors.  Errors are (max |d| / max |twin|, rms(d) / rms(twin)).

Every case is one production-width AMPBlock1 stage behind conv_pre and one up-sampling conv, on a 1-stage handle (as
test_gpu_bigvgan.py::test_production_width_resblock_slices builds them), sized so that its convs meet the tile edges named below.

What the budget can and cannot see (measured on these five cases, CPU only).  Dropping the low bf16 plane of EVERY conv weight -- a 2^-17
relative error per product, the defect conv1d_x3.hip exists to avoid -- moves the waveform by 7 to 11 times the fp32 CPU leg's own max
error: outside the limits (3 x max, 2 x rms), which is what tests/test_bigvgan_twin.py asserts.  The same defect confined to ONE resblock
conv moves it by only 0.4 to 1.5 times the CPU leg's error, and zeroing the other resblock convs so that one stands alone does not help:
the residual path and the Snake passes set the floor.  So the budget catches a defect of the conv arithmetic as a whole and any structural
error (a missed tap, a wrong column or row at a tile seam); it does not catch a 2^-17 error in a single conv, and does not claim to."""
import contextlib
import os

import numpy as np
import torch

import voice_tts_amd.weights as WR
from oracle import vocoder as OV
from test_split_products_numerics import split3

# case -> resblock width C (upsample_initial_channel = 2C), first resblock's kernel k and dilation d, mel rows B and frames F.
# The resblock convs run at T = 2F.
#   A  Cout 192 = half a 128-row tile / three 64-row tiles; x tile of 178 columns > 64 KiB of LDS; T = 130 = 128 + 2 = 96 + 34;
#      conv_pre at odd T with 80 input channels (5 groups of 16: an odd last chunk)
#   B  Cout 96 in a 128-row tile (32 dead rows); T = 128 = one 128 tile = 96 + 32; f32: the 96x128 tile
#   C  every Cout a multiple of 128 (the only case whose f32 resblock convs go by score); T = 98 = 96 + 2
#   D  Cin_pad 48 (3 groups), f32 CKG = 3, fixed 64x128 tile; conv_pre's Cout 96 goes by score in x3
#   E  Cin_pad 32: a single chunk and one x buffer, fixed 32x128 tile; f32 CKG = 3
CASES = {
    "A": dict(C=192, k=11, d=5, B=2, F=65),
    "B": dict(C=96, k=7, d=3, B=2, F=64),
    "C": dict(C=128, k=3, d=1, B=3, F=49),
    "D": dict(C=48, k=11, d=5, B=2, F=65),
    "E": dict(C=24, k=7, d=3, B=1, F=129),
}

# device arithmetic modes: environment of each (read when the handle is created)
MODES = {"default": {}, "conv_f32": {"IXTTS_BV_CONV": "f32"}}
# the tiles each mode's launcher chooses among by score: the values of IXTTS_BV_TILE
TILES = {"default": ("128x128", "128x96", "64x128"), "conv_f32": ("128x128", "64x128", "64x64")}
# forced-tile runs: the cases with a conv that goes by score (x3: Cout_pad >= 128; f32: Cout a multiple of 128 -- A's conv_pre only)
FORCED = {"default": ("A", "B", "C", "D"), "conv_f32": ("A", "C")}
# rows of unequal length on every forced tile: (mode, case); frames per row as a function of the case's F
VARLEN = (("default", "A"), ("default", "C"), ("conv_f32", "C"))

MAX_FACTOR, RMS_FACTOR, RMS_FLOOR = 3.0, 2.0, 2e-7  # the margins of tests/test_gpu_s2mel_fp64.py


def varlen_frames(case):
    return [CASES[case]["F"], 33, 1, 0]


def config(case):
    c = CASES[case]
    cfg = dict(WR.BIGVGAN_CFG)
    cfg.update(upsample_initial_channel=2 * c["C"], upsample_rates=(2,), upsample_kernel_sizes=(4,),
               resblock_kernel_sizes=(c["k"], 3, 3), resblock_dilation_sizes=((c["d"], 1, 1), (1, 1, 1), (1, 1, 1)))
    return cfg


def weights(case):
    return WR.make_bigvgan_weights(config(case), seed=CASES[case]["C"] + CASES[case]["k"])


def mel(case, rows=None):
    """fp32 [B, 80, F] of the case (`rows`: that many rows instead of the case's B, from the same seed)."""
    c = CASES[case]
    return (torch.randn(rows or c["B"], 80, c["F"], generator=torch.Generator().manual_seed(c["C"])) * 2 - 4).clamp(-11.5, 2)


def drop_low_plane(W):
    """W with every 3-D conv weight replaced by h + m of its bf16 split (the low plane dropped): 2^-17 relative per weight."""
    out = {}
    for name, w in W.items():
        if w.dim() == 3:
            h, m, _ = split3(w.numpy())
            out[name] = torch.from_numpy((h + m).astype(np.float32))  # (h + m has at most 16 significant bits: exact in fp32)
        else:
            out[name] = w
    return out


@contextlib.contextmanager
def mode(name, tile=None):
    """The environment of one arithmetic mode, with IXTTS_BV_TILE = `tile` (or unset), for the creation of a handle."""
    keys = {k for m in MODES.values() for k in m} | {"IXTTS_BV_TILE"}
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(MODES[name])
        if tile is not None:
            os.environ["IXTTS_BV_TILE"] = tile
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def device_model(case, mode_name, tile, device, W=None):
    """One handle for one run: the case's generator in one arithmetic mode, `tile` forced (None: the launcher's own choice)."""
    from voice_tts_amd.bigvgan import BigVGAN

    with mode(mode_name, tile):
        m = BigVGAN(config(case), max_frames=CASES[case]["F"], device=device)
    return m.load_state_dict(weights(case) if W is None else W)


@torch.no_grad()
def run(leg, case, W=None, x=None):
    """Waveform of one case (fp64 CPU tensor) on `leg`: "twin", "cpu" (the fp32 oracle) or a device model of `device_model`."""
    W = weights(case) if W is None else W
    x = mel(case) if x is None else x
    if leg == "twin":
        return OV.bigvgan_forward(x, W, config(case), dtype=torch.float64)
    if leg == "cpu":
        return OV.bigvgan_forward(x, W, config(case)).double()
    return leg(x.to(leg.device_)).detach().to("cpu", torch.float64)


def rel_err(got, ref):
    """(max |got - ref| / max |ref|, rms(got - ref) / rms(ref)) against the twin's fp64 `ref`."""
    d = got.double() - ref
    return d.abs().max().item() / ref.abs().max().item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def limits(base):
    """(max, rms) a device path may reach, from the fp32 CPU leg's (max, rms) on the same inputs."""
    return MAX_FACTOR * base[0], max(RMS_FACTOR * base[1], RMS_FLOOR)


class Legs:
    """Per case the weights and mel, the twin's waveform (`ref`) and the fp32 CPU leg's error against it (`base`: case -> (max, rms)),
    computed once."""

    def __init__(self, cases=tuple(CASES)):
        self.W, self.mel, self.ref, self.base = {}, {}, {}, {}
        for c in cases:
            self.W[c], self.mel[c] = weights(c), mel(c)
            self.ref[c] = run("twin", c, self.W[c], self.mel[c])
            self.base[c] = rel_err(run("cpu", c, self.W[c], self.mel[c]), self.ref[c])

    def device(self, case, mode_name, tile=None, device="cuda:0"):
        """((max, rms) of the device path against the twin, its tile_launches(), its waveform) for one handle made for this run."""
        m = device_model(case, mode_name, tile, device, self.W[case])
        got = run(m, case, self.W[case], self.mel[case])
        return rel_err(got, self.ref[case]), m.tile_launches(), got
