"""Every entry of csrc/dit_ops.hip against the plain formula in fp64 on the same fp32 inputs (NOT the wrappers' torch branches, which
are fp32 and, for the norms, cannot tell a two-pass variance from a one-pass one on the inputs used so far), at the widths where the
row kernels change path (H/4 = 63, 64, 65: the lane / chunk boundary; 2048: all eight float4 per lane; 4: one lane), at row counts that
are no multiple of the 4 rows per workgroup, over packed sequences of 1..300 rows, on rows with a large common offset, constant rows
and rows of very different scale, and at arguments where expf overflows.

Found with it: `row_norm_mod_kernel<true>` (LayerNorm) centred a row by its fp32 mean alone, which on a row with offset 300 is off by
a few ulp of 300 -- 1.15e-4 (H = 260) and 1.33e-4 (H = 1028) of the normalised row on single-row inputs, against bounds of 4.3e-5 and
1.6e-5.  The kernel now also centres such rows (|mean| > 4 sigma) by the mean of their residuals; other rows keep their bits."""
import math
import types

import pytest
import torch

from voice_tts_amd import _lib
from voice_tts_amd import s2mel as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 2e-6  # the project's bar for the row kernels: 2e-6 x max(1, |ref|max)
WIDTHS = [4, 64, 252, 256, 260, 512, 1028, 2048]
DENSE = [(1, 1), (1, 3), (2, 37), (3, 5)]
PACKS = [[1] * 67 + [5, 300], [7], [1, 70, 5, 300, 64, 2]]
FAMILIES = ["randn3", "offset30", "offset300", "zero_const", "scales"]


def _bar(ref):
    return BAR * max(1.0, ref.abs().max().item())


def _rows(family, rows, H, g):
    x = torch.randn(rows, H, generator=g)
    if family == "randn3":
        return x * 3 + 0.5
    if family == "offset30":
        return 30 + x
    if family == "offset300":
        return 300 + x
    if family == "zero_const":  # rstd = 1 / sqrt(eps): the output is the bias / shift
        x[0] = 0
        if rows > 1:
            x[-1] = 7.25
        if rows > 2:
            x[rows // 2] = -3072.0
        return x
    s = torch.where(torch.arange(rows) % 2 == 0, 1e-2, 1e2)  # neighbours in one workgroup differ by 1e4 in scale
    return x * s[:, None]


def _rms_ref(x, mod, gain, eps):
    """bias + weight * (x / sqrt(mean(x^2) + eps) * g), mod = (weight | bias) per row."""
    H = x.shape[-1]
    x = x.double()
    n = x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * gain.double()
    return mod[:, H:].double() + mod[:, :H].double() * n


def _ln_mod(n, mod):
    H = n.shape[-1]
    return n * (1 + mod[:, H:].to(n.dtype)) + mod[:, :H].to(n.dtype)


def _ln_ref(x, mod, eps):
    """layer_norm(x) * (1 + scale) + shift, mod = (shift | scale) per row."""
    x = x.double()
    c = x - x.mean(-1, keepdim=True)
    return _ln_mod(c / torch.sqrt((c * c).mean(-1, keepdim=True) + eps), mod)


def _ln_two_pass_f32(x, mod, eps):
    H = x.shape[-1]
    m = x.sum(-1, keepdim=True) / H
    c = x - m
    return _ln_mod(c / torch.sqrt((c * c).sum(-1, keepdim=True) / H + eps), mod)


def _ln_one_pass_f32(x, mod, eps):
    H = x.shape[-1]
    m = x.sum(-1, keepdim=True) / H
    return _ln_mod((x - m) / torch.sqrt((x * x).sum(-1, keepdim=True) / H - m * m + eps), mod)


def _err(got, ref):
    e = (got.double() - ref).abs().max().item()
    return math.inf if math.isnan(e) else e


def ln_offset_bound(x, mod, eps):
    """Bound of the centred LayerNorm on rows with a large common offset: 4 x the error of the two-pass fp32 formula in torch against
    fp64 on the same tensor (the factor covers another summation tree), floored at the family-1 bar.  Returns (ref, bound, error of the
    fp32 one-pass formula E[x^2] - mean^2)."""
    ref = _ln_ref(x, mod, eps)
    return ref, max(4.0 * _err(_ln_two_pass_f32(x, mod, eps), ref), _bar(ref)), _err(_ln_one_pass_f32(x, mod, eps), ref)


def _check_norm(op, got, x, mod, gain, family, what):
    """got: device output [rows, H]; mod [rows, 2H]: each row's own modulation vectors."""
    got = got.cpu()
    assert torch.isfinite(got).all(), what
    eps = 1e-5 if op == "rms" else 1e-6
    H = x.shape[-1]
    if op == "ln" and family.startswith("offset"):
        ref, bound, e_one = ln_offset_bound(x, mod, eps)
        # the inputs must tell a centred variance from E[x^2] - mean^2, or this case checks nothing.  The error of the one-pass formula
        # on ONE row is a matter of that row's rounding (0.2 .. 1000 x the bound over the 1..7-row tensors here); the maximum over 15
        # rows or more is not: 11 .. 37 x the bound at offset 30, above 100 x at offset 300, for every width (computed on the CPU)
        if x.shape[0] >= 15:
            assert e_one >= 10.0 * bound, (what, "the one-pass formula is no longer told apart", e_one, bound)
    else:
        ref = _rms_ref(x, mod, gain, eps) if op == "rms" else _ln_ref(x, mod, eps)
        bound = _bar(ref)  # RMSNorm has no centring: an offset does not hurt it, the family-1 bar holds
    e = _err(got, ref)
    assert e <= bound, (what, e, bound)
    if family == "zero_const":
        out0 = mod[0, H:] if op == "rms" else mod[0, :H]
        assert torch.equal(got[0], out0), (what, "an all-zero row gives the bias / shift exactly")


def _modulation(n, H, g):
    return torch.randn(n, 2 * H, generator=g), 1 + 0.1 * torch.randn(H, generator=g)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("op", ["rms", "ln"])
def test_row_norms_dense_vs_fp64(op, H):
    g = torch.Generator().manual_seed(1000 + H)
    for B, T in DENSE:
        for family in FAMILIES:
            x = _rows(family, B * T, H, g)
            mod, gain = _modulation(B, H, g)
            xd, md = x.view(B, T, H).to(DEV), mod.to(DEV)
            got = S.adaln_rmsnorm(xd, md, gain.to(DEV)) if op == "rms" else S.ln_modulate(xd, md)
            rowmap = torch.arange(B * T) // T
            _check_norm(op, got.view(B * T, H), x, mod[rowmap], gain, family, (op, H, B, T, family))


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("op", ["rms", "ln"])
def test_row_norms_packed_vs_fp64(op, H):
    g = torch.Generator().manual_seed(2000 + H)
    for lens in PACKS:
        pk = S.RowPack(lens, DEV)
        rowmap = torch.repeat_interleave(torch.arange(pk.n), torch.tensor(lens))
        for family in FAMILIES:
            x = _rows(family, pk.rows, H, g)
            mod, gain = _modulation(pk.n, H, g)
            got = S.adaln_rmsnorm_packed(x.to(DEV), mod.to(DEV), gain.to(DEV), pk) if op == "rms" else S.ln_modulate_packed(x.to(DEV), mod.to(DEV), pk)
            _check_norm(op, got, x, mod[rowmap], gain, family, (op, H, len(lens), family))


def test_offset_rows_tell_one_pass_from_two_pass():
    """The numbers behind the offset-row bound, on the CPU alone: at H = 512, 64 rows, the two-pass fp32 formula and the one-pass one
    against fp64 (3.7e-6 vs 4.6e-4 at offset 30, 3.3e-5 vs 3.9e-2 at offset 300, in units of the normalised row)."""
    g = torch.Generator().manual_seed(5)
    for family, lo in (("offset30", 30.0), ("offset300", 300.0)):
        x = _rows(family, 64, 512, g)
        mod = torch.zeros(64, 1024)
        ref, bound, e_one = ln_offset_bound(x, mod, 1e-6)
        e_two = _err(_ln_two_pass_f32(x, mod, 1e-6), ref)
        print(f"layer_norm rows {family}: two-pass fp32 {e_two:.2e}, one-pass fp32 {e_one:.2e}, bound {bound:.2e}")
        assert e_one >= 100.0 * e_two and e_one >= 10.0 * bound


SENTINEL = -12345.0


def _refused(name, out, *args):
    with pytest.raises(_lib.IxttsError):
        S._hip_call(name, *args)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, SENTINEL)), (name, "a refused call wrote to its output")


def test_row_norms_refuse_what_the_kernel_cannot_hold():
    """H above 2048, H no multiple of 4, empty shapes: an error code before anything is launched (buffers sized for the claimed shape)."""
    import ctypes as C

    n = 4 * 2052
    x, mod, gain = torch.randn(n, device=DEV), torch.randn(2 * n, device=DEV), torch.ones(n, device=DEV)
    out = torch.full((n,), SENTINEL, device=DEV)
    tab = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()  # noqa: E731
    for B, T, H in ((2, 2, 2052), (2, 2, 6), (2, 2, 0), (0, 2, 64), (2, 0, 64)):
        _refused("ixtts_adaln_rmsnorm_f32", out, p(x), p(mod), p(gain), p(out), B, T, H, C.c_float(1e-5))
        _refused("ixtts_ln_modulate_f32", out, p(x), p(mod), p(out), B, T, H, C.c_float(1e-6))
    for nseq, rows, H in ((2, 4, 2052), (2, 4, 6), (2, 4, 0), (0, 4, 64), (2, 0, 64)):
        _refused("ixtts_adaln_rmsnorm_varlen_f32", out, p(x), p(mod), p(gain), p(out), p(tab), nseq, rows, H, C.c_float(1e-5))
        _refused("ixtts_ln_modulate_varlen_f32", out, p(x), p(mod), p(out), p(tab), nseq, rows, H, C.c_float(1e-6))


# ---------------------------------------------------------------------------------- RoPE
def _rope_table(hd, T):
    """The model's own table: `S2Mel._rope_cache` (fp32 angles, complex64)."""
    return S.S2Mel._rope_cache(types.SimpleNamespace(head_dim=hd, _rope=None, device=DEV, dtype=torch.float32), T)


def _check_rope(got, qkv, pos, fc, H, hd, what):
    """got / qkv [rows, 3H] after / before; pos [rows]: each row's position in its sequence."""
    got = got.cpu()
    rows = qkv.shape[0]
    f = fc.cpu().to(torch.complex128)[pos][:, None, :]
    for j in range(2):
        xc = torch.view_as_complex(qkv[:, j * H:(j + 1) * H].double().reshape(rows, H // hd, hd // 2, 2))
        ref = torch.view_as_real(xc * f).reshape(rows, H)
        e = _err(got[:, j * H:(j + 1) * H], ref)
        assert e <= _bar(ref), (what, "qk"[j], e)
    assert torch.equal(got[:, 2 * H:], qkv[:, 2 * H:]), (what, "the v third is not rotated")


@pytest.mark.parametrize("hd", [4, 32, 64, 128])
@pytest.mark.parametrize("heads", [1, 3])
def test_rope_qk_vs_fp64(hd, heads):
    H = hd * heads
    g = torch.Generator().manual_seed(3000 + H)
    for B, T in ((2, 3), (1, 2400)):
        fc = _rope_table(hd, T)
        assert fc.shape == (T, hd // 2) and fc.dtype == torch.complex64
        qkv = torch.randn(B * T, 3 * H, generator=g) * 2
        d = qkv.to(DEV)
        S._hip_call("ixtts_rope_qk_f32", d.data_ptr(), torch.view_as_real(fc).data_ptr(), B, T, H, hd)
        _check_rope(d, qkv, torch.arange(B * T) % T, fc, H, hd, ("dense", hd, heads, B, T))
    lens = [1, 70, 5, 2400, 64, 2]
    pk = S.RowPack(lens, DEV)
    fc = _rope_table(hd, max(lens))
    qkv = torch.randn(pk.rows, 3 * H, generator=g) * 2
    pos = torch.cat([torch.arange(t) for t in lens])
    _check_rope(S.rope_qk_packed(qkv.to(DEV), fc, pk, hd), qkv, pos, fc, H, hd, ("packed", hd, heads))


# ---------------------------------------------------------------------------------- SwiGLU and the WaveNet gate
PLANTED = [v * s for v in (0.0, 1e-8, 20.0, 88.0, 89.0, 104.0, 1e4) for s in (1.0, -1.0)]  # expf(89) overflows, expf(-104) underflows


def _check_swiglu(got, u, what):
    got = got.cpu()
    Fd = u.shape[-1] // 2
    a, b = u[:, :Fd].double(), u[:, Fd:].double()
    ref = a * torch.sigmoid(a) * b
    assert torch.isfinite(got).all(), (what, "NaN / Inf")
    excess = (got.double() - ref).abs() - BAR * ref.abs().clamp(min=1.0)
    assert excess.max().item() <= 0.0, (what, excess.max().item())


@pytest.mark.parametrize("Fd", [4, 260, 1536])
@pytest.mark.parametrize("rows", [1, 5, 74])
def test_swiglu_vs_fp64(Fd, rows):
    u = torch.randn(rows, 2 * Fd, generator=torch.Generator().manual_seed(Fd + rows)) * 2
    _check_swiglu(S.swiglu(u.to(DEV)), u, (Fd, rows))


def test_swiglu_where_expf_overflows():
    """Every pair of planted values (gate half x linear half): x / (1 + inf) must be +-0, never NaN."""
    n = len(PLANTED)
    Fd = 16
    u = torch.randn(n, 2 * Fd, generator=torch.Generator().manual_seed(9)) * 2
    u[:, :n] = torch.tensor(PLANTED)[:, None]
    u[:, Fd:Fd + n] = torch.tensor(PLANTED)[None, :]
    got = S.swiglu(u.to(DEV))
    _check_swiglu(got, u, "planted")
    neg_big = torch.tensor([v <= -89.0 for v in PLANTED])
    assert (got.cpu()[neg_big][:, :n] == 0).all()


def _gate_ref(xa, xb):
    return torch.tanh(xa.double()) * torch.sigmoid(xb.double())


def _check_gate(got, ref, what):
    got = got.cpu()
    assert torch.isfinite(got).all(), (what, "NaN / Inf")
    e = _err(got, ref)
    assert e <= BAR, (what, e)  # absolute: the gate is bounded by 1


def _plant(a, g):
    flat = a.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:min(len(PLANTED), flat.numel() // 2)]
    flat[idx] = torch.tensor(PLANTED)[:idx.numel()]
    return a


@pytest.mark.parametrize("B,C_,T,stride,off", [(2, 3, 7, 2 * 3 * 3 + 1, 7), (2, 64, 53, 3 * 128, 128)])
def test_wn_gate_channel_major_vs_fp64(B, C_, T, stride, off):
    g = torch.Generator().manual_seed(C_)
    a = _plant(torch.randn(B, 2 * C_, T, generator=g) * 2, g)
    gv = torch.randn(B, stride, generator=g)
    x = a.double() + gv[:, off:off + 2 * C_, None].double()
    _check_gate(S.wn_gate(a.to(DEV), gv.to(DEV), off, C_), _gate_ref(x[:, :C_], x[:, C_:]), (B, C_, T))


@pytest.mark.parametrize("C_", [4, 64, 132])
def test_wn_gate_rows_vs_fp64(C_):
    g = torch.Generator().manual_seed(40 + C_)
    B, rpb = 3, 37
    rows = B * rpb + 3  # the last three rows fall past B * rows_per_batch: they take the last entry's biases
    a = _plant(torch.randn(rows, 2 * C_, generator=g) * 2, g)
    gv = torch.randn(B, 3 * 2 * C_, generator=g)
    off = 2 * C_
    b = (torch.arange(rows) // rpb).clamp(max=B - 1)
    assert b[-1] == B - 1 and rows // rpb == B
    x = a.double() + gv[b, off:off + 2 * C_].double()
    _check_gate(S.wn_gate_rows(a.to(DEV), gv.to(DEV), off, C_, rpb), _gate_ref(x[:, :C_], x[:, C_:]), ("rows", C_))
    # packed: the WaveNet's call (rows = padded rows - (k - 1)), and one with rows past the pack (the last sequence's gate)
    lens = [7, 41, 1 + 4, 9]
    pp = S.RowPack(lens, DEV)
    gv = torch.randn(pp.n, 3 * 2 * C_, generator=g)
    for rows in (pp.rows - 4, pp.rows + 3):
        a = _plant(torch.randn(rows, 2 * C_, generator=g) * 2, g)
        b = torch.cat([torch.repeat_interleave(torch.arange(pp.n), torch.tensor(lens)), torch.full((3,), pp.n - 1)])[:rows]
        x = a.double() + gv[b, off:off + 2 * C_].double()
        _check_gate(S.wn_gate_rows_packed(a.to(DEV), gv.to(DEV), off, C_, pp), _gate_ref(x[:, :C_], x[:, C_:]), ("packed", C_, rows))


# ---------------------------------------------------------------------------------- reflect halo
def _padded(interior, left, right):
    """F.pad(mode='reflect') of [B, T, C] rows along T."""
    return torch.nn.functional.pad(interior.transpose(1, 2), (left, right), mode="reflect").transpose(1, 2)


@pytest.mark.parametrize("C_", [4, 64, 132])
@pytest.mark.parametrize("B", [1, 3])
def test_reflect_halo_rows_bit_exact(B, C_):
    g = torch.Generator().manual_seed(50 + C_ + B)
    for left, right in ((2, 2), (3, 1), (0, 4), (4, 0), (0, 0)):
        for T in (max(left, right) + 1, 37):
            p = torch.randn(B, left + T + right, C_, generator=g)
            want = _padded(p[:, left:left + T], left, right)
            got = S.reflect_halo_rows(p.clone().to(DEV), T, left, right).cpu()
            assert torch.equal(got[:, left:left + T], p[:, left:left + T]), ("interior rows changed", left, right, T)
            assert torch.equal(got, want), (left, right, T)


def test_reflect_halo_rows_packed_and_refusal():
    g = torch.Generator().manual_seed(61)
    left = right = 2
    lens = [3 + 4, 37 + 4, 5 + 4]
    pp = S.RowPack(lens, DEV)
    for C_ in (4, 64, 132):
        p = torch.randn(pp.rows, C_, generator=g)
        got = S.reflect_halo_rows_packed(p.clone().to(DEV), pp, left, right).cpu()
        for s in range(pp.n):
            a, b = pp.span(s)
            assert torch.equal(got[a:b], _padded(p[None, a + left:b - right], left, right)[0]), (C_, s)
    # T <= left: refused by the dense entry, nothing written
    out = torch.full((3, 16, 8), SENTINEL, device=DEV)  # room for every claimed shape
    for T, l_, r_ in ((2, 2, 2), (1, 2, 0), (3, 0, 4), (0, 0, 0)):
        _refused("ixtts_reflect_halo_rows_f32", out, out.data_ptr(), 3, T, 8, l_, r_)
    _refused("ixtts_reflect_halo_rows_f32", out, out.data_ptr(), 3, 3, 6, 1, 1)  # C no multiple of 4
