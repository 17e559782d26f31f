"""`ixtts_adaln_rmsnorm_planes_f32` / `_varlen_f32` (csrc/dit_ops.hip): the AdaLN-RMSNorm in front of [w1; w3] writes the bf16 planes
of csrc/gemm_x6.hip itself.  The whole plane buffer -- the zero rows up to the padded row count included -- must equal, byte for byte,
what the separate passes of the same build leave: `ixtts_adaln_rmsnorm_f32` (fp32 rows) followed by `ixtts_gemm_x6_split`.

Shapes: H in {128, 512}; (B, T) = (1, 1), (1, 63), (2, 33), (2, 65), (3, 5) -- a lone row, the tail of a workgroup's rows, the 64-row
block of the split pass on both sides, a batch boundary inside a workgroup (the modulation vector changes there) -- one pack of three
unequal sequences, and a row whose |mean| is far above its spread."""
import numpy as np
import pytest
import torch

import voice_tts_amd.gemm as G
import voice_tts_amd.s2mel as S2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _inputs(rows, n, H, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, H, generator=g) * 1.7
    if rows > 2:
        x[rows // 2] = 300.0 + torch.randn(H, generator=g)  # |mean| well above the spread
    wb = torch.randn(n, 2 * H, generator=g)
    gg = 1 + 0.1 * torch.randn(H, generator=g)
    return x.to(DEV), wb.to(DEV), gg.to(DEV)


def _bytes(planes):
    torch.cuda.synchronize()
    return planes.buf.cpu().numpy().copy()


def _poison():
    for buf in G._POOL.values():  # neither path may rely on what the scratch buffer held
        buf.fill_(0xA5)


@pytest.mark.parametrize("H", [128, 512])
@pytest.mark.parametrize("B,T", [(1, 1), (1, 63), (2, 33), (2, 65), (3, 5)])
def test_planes_equal_norm_then_split(B, T, H):
    x, wb, gg = _inputs(B * T, B, H, 100 * B + T + H)
    x = x.view(B, T, H)
    G.planes_buffer(B * T, H, DEV)
    _poison()
    want = _bytes(G.split(S2.adaln_rmsnorm(x, wb, gg).view(B * T, H)))
    _poison()
    p = S2.adaln_rmsnorm_planes(x, wb, gg)
    assert (p.rows, p.K) == (B * T, H)
    got = _bytes(p)
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"


@pytest.mark.parametrize("H", [128, 512])
def test_packed_planes_equal_norm_then_split(H):
    pk = S2.RowPack([3, 70, 5], DEV)
    x, wb, gg = _inputs(pk.rows, pk.n, H, 7 + H)
    G.planes_buffer(pk.rows, H, DEV)
    _poison()
    want = _bytes(G.split(S2.adaln_rmsnorm_packed(x, wb, gg, pk)))
    _poison()
    got = _bytes(S2.adaln_rmsnorm_planes(x, wb, gg, pk=pk))
    assert got.shape == want.shape and np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
