"""`ixtts_attn_full_rope_f32` / `_varlen_f32` (csrc/attn_full_x3.hip): RoPE of q and k inside the attention -- the keys rotated as the
split pass writes their planes, the queries as the kernel loads them.  The output must equal, byte for byte, the separate passes of the
same build: `ixtts_rope_qk_f32` in place on the wqkv rows, then `ixtts_attn_full_f32`; and the wqkv rows must be left unrotated.

head_dim 64, H in {1, 2}, B = 2; T = 1, 63, 64, 65 (one key tile, on both sides of its edge), 129 (the second 128-query block), 200,
and 256 / 257 on the two sides of the point where the entry splits the key range (T > 4 tiles of 64) and merges; one pack of four
unequal sequences.

The standalone rotation (`ixtts_rope_qk_f32`, whose roundings the fused forms copy) against torch's complex multiply in
`S2Mel._rotary`: the build before the fused forms was NOT bit-equal to it -- the kernel rounds the sine product and fuses the cosine
product into the sum, torch rounds differently -- but bit-equal to that formula evaluated in exact steps, and 2.0 ulp of the larger
product away from torch at worst (B = 2, T = 200, 2 heads).  This build is held to the same: bit-equal to the formula, and within
2.5 ulp of the larger product p of torch -- whatever torch fuses, the two results round one exact value up to three times in all,
one product (<= 0.5 ulp(p)) and each final sum (|sum| <= 2p: <= 1 ulp(p) each)."""

import numpy as np
import pytest
import torch

import voice_tts_amd.s2mel as S2
from voice_tts_amd.s2mel import _hip_call

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HD = 64


def _table(T):
    ang = torch.outer(torch.arange(max(T, 64)).float(), 1.0 / (10000.0 ** (torch.arange(0, HD, 2).float() / HD)))
    return torch.polar(torch.ones_like(ang), ang).to(DEV)


def _qkv(rows, nh, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3, nh, HD, generator=g)
    qkv[:, 0] *= 2.0  # sharper softmax
    return qkv.to(DEV)


def _same(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("nh", [1, 2])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 129, 200, 256, 257])
def test_rope_inside_equals_rope_then_attention(T, nh):
    B = 2
    fc = _table(T)[:T]
    qkv = _qkv(B * T, nh, 1000 * nh + T).view(B, T, 3, nh, HD)
    before = qkv.clone()
    got = S2.attn_full(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], rope=fc)
    assert torch.equal(qkv, before), "the wqkv rows were modified"
    with torch.cuda.device(DEV):
        _hip_call("ixtts_rope_qk_f32", qkv.data_ptr(), torch.view_as_real(fc).data_ptr(), B, T, nh * HD, HD)
    assert torch.equal(qkv[:, :, 2], before[:, :, 2]) and (T == 1 or not torch.equal(qkv[:, 1:, :2], before[:, 1:, :2]))  # the reference did rotate
    want = S2.attn_full(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2])
    assert torch.isfinite(want).all()
    assert _same(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


@pytest.mark.parametrize("nh", [1, 2])
def test_packed_rope_inside_equals_rope_then_attention(nh):
    pk = S2.RowPack([3, 130, 64, 1], DEV)
    fc = _table(max(pk.lens))[:max(pk.lens)]
    qkv = _qkv(pk.rows, nh, 77 + nh)
    before = qkv.clone()
    got = S2.attn_full_packed(qkv[:, 0], qkv[:, 1], qkv[:, 2], pk, rope=fc)
    assert torch.equal(qkv, before), "the wqkv rows were modified"
    S2.rope_qk_packed(qkv.view(pk.rows, 3 * nh * HD), fc, pk, HD)
    want = S2.attn_full_packed(qkv[:, 0], qkv[:, 1], qkv[:, 2], pk)
    assert torch.isfinite(want).all()
    assert _same(got, want), f"{int((got != want).sum())} of {want.numel()} elements differ"


def rope_vs_torch(T=200, nh=2, B=2):
    """(bit-equal to torch's complex multiply?, bit-equal to the kernel's formula?, worst |kernel - torch| in ulps of the larger product)."""
    fc = _table(T)[:T]
    qkv = _qkv(B * T, nh, 5).view(B, T, 3, nh, HD)
    ref = torch.stack([S2.S2Mel._rotary(qkv[:, :, j], fc) for j in range(2)], 2).cpu()
    x = qkv[:, :, :2].cpu().double().reshape(B, T, 2, nh, HD // 2, 2)
    c, s = fc.real.cpu().double()[None, :, None, None, :], fc.imag.cpu().double()[None, :, None, None, :]
    x0, x1 = x[..., 0], x[..., 1]
    # the kernel: the sine product rounded to fp32 on its own, the cosine product exact inside the fused multiply-add (the fp64
    # product of two fp32 values is exact, and so is its sum with an fp32 value up to one rounding, taken to fp32 at once)
    re = (x0 * c - (x1 * s).float().double()).float()
    im = (x1 * c + (x0 * s).float().double()).float()
    formula = torch.stack([re, im], -1).reshape(B, T, 2, nh, HD)
    with torch.cuda.device(DEV):
        _hip_call("ixtts_rope_qk_f32", qkv.data_ptr(), torch.view_as_real(fc).data_ptr(), B, T, nh * HD, HD)
    out = qkv[:, :, :2].cpu()
    big = torch.maximum((x0 * c).abs(), (x1 * s).abs()).float()
    ulp = torch.stack([big, torch.maximum((x1 * c).abs(), (x0 * s).abs()).float()], -1).reshape(B, T, 2, nh, HD)
    ulp = 2.0 ** (torch.floor(torch.log2(ulp.clamp_min(1e-30))) - 23)
    return torch.equal(out, ref), torch.equal(out, formula), float(((out - ref).abs() / ulp).max())


def test_standalone_rope_keeps_its_roundings():
    eq_torch, eq_formula, worst = rope_vs_torch()
    print(f"rope_qk vs torch complex multiply: bit-equal {eq_torch}, worst {worst:.2f} ulp of the larger product; vs its own formula: bit-equal {eq_formula}")
    assert eq_formula
    assert not eq_torch  # as recorded for the build before; a change here means the roundings moved
    assert worst <= 2.5
