"""csrc/gemm_x6.hip computes each operand copy's address once and advances it per step (a running offset, a k-group counter that wraps
at the end of a tap) instead of deriving it from the step number; its epilogue is picked at compile time.  Neither changes a result:
every case here -- the smallest shapes at which that recurrence can go wrong, and the two production shapes -- must reproduce, bit for
bit, what the kernel gave before the change (tests/golden/gemm_x6_parent.npz, recorded by tests/golden/make_golden_gemm_x6.py at the
parent commit), and stay within the 2e-6-of-scale bound against fp64 of tests/test_gpu_gemm_x6.py.

Cases (make_golden_gemm_x6.cases): the plain entry at (M, N, K) = (1, 64, 64) -- 4 steps, no more than the copies in flight --
(130, 192, 128) and (257, 128, 192), tiles 2..5, with bias / without / accumulating, rows starting at row0 = 5 of a larger plane
buffer; the SwiGLU pair at (300, 128, 64) and (257, 192, 192); the gate pair with 2, 3 and 5 taps over K_a = 64 (the k-group wraps every
4 steps), B in {2, 3}, T in {90, 203}, gate_off != 0, and over a sequence table of three unequal sequences; the two production
shapes, by the sha256 of their output."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_gemm_x6", os.path.join(HERE, "golden", "make_golden_gemm_x6.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

CASES = MG.cases()


@pytest.fixture(scope="module")
def recorded():
    with np.load(MG.PATH) as z:
        return {k: z[k] for k in z.files}


def test_every_case_is_recorded(recorded):
    assert sorted(k for k in recorded if k.endswith("/sha256")) == sorted(cid + "/sha256" for cid, _, _ in CASES)
    assert os.path.getsize(MG.PATH) <= 512 * 1024


@pytest.mark.parametrize("cid,kind,args", CASES, ids=[c[0] for c in CASES])
def test_bit_identical_to_parent_and_within_fp64_bound(recorded, cid, kind, args):
    out, ref, scale = MG.run_case(cid, kind, args, torch.device("cuda:0"))
    err = float((out.double() - ref).abs().max()) / scale
    print(f"{cid}: {tuple(out.shape)} max err {err:.2e} of scale")
    whole = recorded.get(cid + "/out")
    if whole is not None:
        want = torch.from_numpy(whole)
        assert torch.equal(out.cpu(), want), f"{int((out.cpu() != want).sum())} of {want.numel()} elements differ from the recording"
    assert MG.digest(out) == str(recorded[cid + "/sha256"]), "output bytes differ from the recording"
    assert err <= 2e-6


@pytest.mark.parametrize("base", sorted({c[0].rsplit("-t", 1)[0] for c in CASES if "-t" in c[0]}))
def test_tiles_agree(recorded, base):
    """Every tile shape adds the same products in the same order, so the recordings of one case's tiles are one output."""
    assert len({str(recorded[c[0] + "/sha256"]) for c in CASES if c[0].rsplit("-t", 1)[0] == base}) == 1
