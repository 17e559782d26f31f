"""CPU: the fp64 twin of the vocoder oracle (`oracle.vocoder.bigvgan_forward(..., dtype=torch.float64)`) and the yardstick the GPU
budget of tests/test_gpu_bigvgan_fp64.py is measured with -- the fp32 CPU oracle's own distance from the twin on the five cases of
tests/bigvgan_budget.py.  No GPU.

The limit of what this bar sees (measured on these cases, see bigvgan_budget.py): every conv weight without its low bf16 plane moves the
waveform 7 .. 11 x the fp32 CPU leg's max error and is caught, in every case (asserted below).  The same 2^-17 defect confined to ONE
resblock conv moves it only 0.4 .. 1.5 x the CPU leg's own error -- also when the other resblock convs are zeroed so that one stands
alone: the residual path and the Snake passes set the floor.  So the budget catches a defect of the conv arithmetic as a whole and any
structural error (a missed tap, a wrong column or row at a tile seam); it does not catch a 2^-17 error in a single conv."""
import pytest
import torch

import bigvgan_budget as BB
import voice_tts_amd.weights as WR
from oracle import vocoder as OV


@pytest.fixture(scope="module")
def legs():
    return BB.Legs()


@pytest.mark.parametrize("case", list(BB.CASES))
def test_fp32_oracle_sits_at_the_arithmetic_noise_from_the_twin(legs, case):
    """The yardstick: fp32 rounding of the same generator, 4e-7 .. 1.3e-6 of the waveform's peak -- neither zero (the twin really is a
    different arithmetic) nor a broken CPU leg."""
    c_max, c_rms = legs.base[case]
    print(f"bigvgan twin {case}: fp32 CPU leg max {c_max:.3e} rms {c_rms:.3e}")
    assert 0.0 < c_max < 1e-5 and 0.0 < c_rms < 1e-5, (c_max, c_rms)


@pytest.mark.parametrize("case", list(BB.CASES))
def test_no_sample_of_the_twin_reaches_the_final_clamp(legs, case):
    """clamp(-1, 1) would hide any error of a clamped sample: the cases are chosen so that none is (a condition, not a measurement)."""
    ref = legs.ref[case]
    c = BB.CASES[case]
    assert ref.shape == (c["B"], 1, 2 * c["F"])
    assert int((ref.abs() >= 1.0).sum()) == 0
    assert ref.abs().max().item() > 0.02  # (and the waveform is not degenerate)


@pytest.mark.parametrize("F", [1, 7, 40])
def test_twin_reproduces_the_reference_fixtures(golden, F):
    """The twin against the reference's own waveforms, at the bar test_oracle_golden.py holds the fp32 oracle to."""
    g = golden("bigvgan_tiny.npz")
    cfg = WR.tiny_bigvgan_cfg(int(g["upsample_initial_channel"]))
    W = WR.make_bigvgan_weights(cfg, seed=int(g["seed"]))
    wav = OV.bigvgan_forward(torch.from_numpy(g[f"mel_f{F}"]), W, cfg, dtype=torch.float64)
    ref = torch.from_numpy(g[f"wav_f{F}"])
    assert wav.dtype == torch.float64 and wav.shape == ref.shape == (1, 1, 256 * F)
    assert (wav - ref.double()).abs().max().item() <= 2e-5


def test_default_dtype_is_the_fp32_oracle_bit_for_bit():
    """`dtype` left alone changes nothing: the same bytes with and without the argument, fp32 out."""
    cfg = WR.tiny_bigvgan_cfg(64)
    W = WR.make_bigvgan_weights(cfg, seed=21)
    x = (torch.randn(2, 80, 5, generator=torch.Generator().manual_seed(3)) * 2 - 4).clamp(-11.5, 2)
    a, b = OV.bigvgan_forward(x, W, cfg), OV.bigvgan_forward(x, W, cfg, dtype=torch.float32)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    s = OV.aa_snake(x, W["activation_post.act.alpha"].new_zeros(80), W["activation_post.act.beta"].new_zeros(80))
    assert s.dtype == torch.float32
    assert OV.aa_snake(x, torch.zeros(80), torch.zeros(80), dtype=torch.float64).dtype == torch.float64


@pytest.mark.parametrize("case", list(BB.CASES))
def test_the_bar_bites_a_conv_arithmetic_without_its_low_plane(legs, case):
    """Every conv weight as h + m of its bf16 split (what a split-product kernel that lost its low-plane products computes, 2^-17
    relative per product), evaluated in fp64: outside both limits of the GPU budget in every case.  The fp32-vs-fp32 bars of the suite
    (5e-5, 1e-4) pass it."""
    W = BB.drop_low_plane(legs.W[case])
    assert any(not torch.equal(W[k], legs.W[case][k]) for k in W)
    e_max, e_rms = BB.rel_err(BB.run("twin", case, W, legs.mel[case]), legs.ref[case])
    lim_max, lim_rms = BB.limits(legs.base[case])
    c_max, c_rms = legs.base[case]
    print(f"bigvgan twin {case}: low plane dropped max {e_max:.3e} rms {e_rms:.3e} | fp32 CPU leg max {c_max:.3e} rms {c_rms:.3e} "
          f"| ratio {e_max / c_max:.1f} {e_rms / c_rms:.1f}")
    assert e_max > lim_max, (e_max, lim_max)
    assert e_rms > lim_rms, (e_rms, lim_rms)
    assert e_max < 1e-4  # (and it is the defect the old bar cannot see)
