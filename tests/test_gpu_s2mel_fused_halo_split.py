"""`ixtts_gemm_x6_split_halo` / `_varlen` (csrc/gemm_x6.hip): the split pass in front of the WaveNet's tap GEMM reads each halo row of
the reflect-padded row buffer from the interior row it mirrors.  Its planes -- padding rows included -- must equal, byte for byte,
those of the separate passes of the same build: `ixtts_reflect_halo_rows_f32` (/ `_varlen_f32`) followed by `ixtts_gemm_x6_split`;
and it must leave the fp32 buffer, stale halo rows included, as it found it.

k = 5 (left = right = 2), C in {64, 128}; (B, T) = (1, 3) -- the shortest sequence that reflects -- (2, 6), (2, 67) -- a sequence
boundary inside a 64-row block of the split, and more than one block -- and one pack of lengths (3, 70, 5)."""
import numpy as np
import pytest
import torch

import voice_tts_amd.gemm as G
import voice_tts_amd.s2mel as S2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LEFT = RIGHT = 2


def _bytes(planes):
    torch.cuda.synchronize()
    return planes.buf.cpu().numpy().copy()


def _poison():
    for buf in G._POOL.values():
        buf.fill_(0xA5)


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B,T", [(1, 3), (2, 6), (2, 67)])
def test_halo_split_equals_refresh_then_split(B, T, C):
    g = torch.Generator().manual_seed(10 * T + B + C)
    P = torch.randn(B, LEFT + T + RIGHT, C, generator=g).to(DEV)  # the halo rows hold noise: they must not be read
    P2 = P.view(-1, C)
    G.planes_buffer(P2.shape[0], C, DEV)
    _poison()
    before = P.clone()
    got = _bytes(G.split(P2, halo=(T, LEFT, RIGHT)))
    assert torch.equal(P, before)
    _poison()
    S2.reflect_halo_rows(P, T, LEFT, RIGHT)
    want = _bytes(G.split(P2))
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"


@pytest.mark.parametrize("C", [64, 128])
def test_packed_halo_split_equals_refresh_then_split(C):
    pp = S2.RowPack([t + LEFT + RIGHT for t in (3, 70, 5)], DEV)
    g = torch.Generator().manual_seed(31 + C)
    P2 = torch.randn(pp.rows, C, generator=g).to(DEV)
    G.planes_buffer(pp.rows, C, DEV)
    _poison()
    before = P2.clone()
    got = _bytes(G.split(P2, halo=(pp, LEFT, RIGHT)))
    assert torch.equal(P2, before)
    _poison()
    S2.reflect_halo_rows_packed(P2, pp, LEFT, RIGHT)
    want = _bytes(G.split(P2))
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
