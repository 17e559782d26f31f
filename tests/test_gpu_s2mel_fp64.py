"""The device paths of the s2mel DiT against its fp64 twin, as an error budget: every path's error (max and rms, relative to the twin's
max and rms) next to the error the fp32 CPU leg has on the same inputs.  The criterion is relative and measured: a device path may
sit at most 3 x (max) and 2 x (rms, floor 2e-7) above the CPU leg -- "the same quality of result, in another summation order", the
margins of test_gpu_gemm_x6.py and of the attention's arithmetic-mode test.  A path whose error grows to 1e-5 passes every fp32-vs-fp32
check of the suite (bars 1e-5 .. 2e-4) and fails here.

tools/s2mel_error_budget.py records the same numbers in profiles/s2mel_error_budget.json."""
import pytest
import torch

import s2mel_budget as SB

pytestmark = pytest.mark.gpu

MAX_FACTOR, RMS_FACTOR, RMS_FLOOR = 3.0, 2.0, 2e-7


@pytest.fixture(scope="module", params=list(SB.CONFIGS))
def legs(request):
    return SB.Legs(request.param, torch.device("cuda:0"))


@pytest.mark.parametrize("case", SB.CASES)
@pytest.mark.parametrize("mode", list(SB.MODES))
def test_device_path_within_the_fp32_budget(legs, mode, case):
    c_max, c_rms = legs.base[case]
    e_max, e_rms = legs.device(case, mode)
    print(f"s2mel budget {legs.name} {case} [{mode}]: device max {e_max:.3e} rms {e_rms:.3e} | fp32 CPU leg max {c_max:.3e} rms {c_rms:.3e}")
    assert 0.0 < c_max < 1e-5 and 0.0 < c_rms < 1e-5  # (the yardstick itself: the arithmetic's noise, not a broken CPU leg)
    assert e_max <= MAX_FACTOR * c_max, (e_max, c_max)
    assert e_rms <= max(RMS_FACTOR * c_rms, RMS_FLOOR), (e_rms, c_rms)


def test_the_modes_are_different_paths(legs):
    """(the three modes really run different kernels: their outputs differ in the last bits)"""
    outs = {}
    for m in SB.MODES:
        with SB.mode(m):
            outs[m] = SB.run(legs.gpu, "dit_step_window", legs.inp)
    assert not torch.equal(outs["default"], outs["library_gemm"]) and not torch.equal(outs["default"], outs["attn_f32"])
