"""Row N1: the linear layers of the s2mel DiT / WaveNet on the HIP split-product GEMM (csrc/gemm_x6.hip) instead of the library's
fp32 GEMM.  `PackedLinear` holds a weight matrix split once into the bf16 planes the kernel streams; `split(x)` turns activation
rows into the same planes (one small pass; several GEMMs over the same input -- or over row-shifted windows of it, the taps of a
Conv1d -- share it); `linear(x, pl, ...)` = `F.linear` / `addmm_`.  Device tensors only (the CPU leg of the glue keeps torch's GEMM)."""
import ctypes as C
import os

import torch

from . import _lib


class PackedLinear:
    """W [N, K] fp32 (K a multiple of 64) -> packed planes on W's device; `bias` [N] or None rides along."""

    __slots__ = ("N", "K", "packed", "bias")

    def __init__(self, weight, bias=None):
        assert weight.is_cuda and weight.dim() == 2 and weight.shape[1] % 64 == 0, tuple(weight.shape)
        w = weight.detach().to(torch.float32).contiguous()
        self.N, self.K = int(w.shape[0]), int(w.shape[1])
        nbytes = _lib.lib().ixtts_gemm_x6_packed_bytes(self.N, self.K)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
        with torch.cuda.device(w.device):
            _lib.check(_lib.lib().ixtts_gemm_x6_pack(w.data_ptr(), self.packed.data_ptr(), self.N, self.K, _lib.current_stream_ptr()), "ixtts_gemm_x6_pack")
            torch.cuda.current_stream().synchronize()  # `w` may be a temporary
        self.bias = None if bias is None else bias.detach().to(w.device, torch.float32).contiguous()


class Planes:
    """Activation rows [rows, K] as split planes (device buffer) -- what `linear` consumes."""

    __slots__ = ("buf", "rows", "K")

    def __init__(self, buf, rows, K):
        self.buf, self.rows, self.K = buf, rows, K


_POOL = {}  # (device, bytes) -> scratch buffers reused across calls: the planes of an input live until the next split of that size


def usable(x, K):
    """Whether `split` can take x [..., K] as it is: device fp32, 16-byte aligned rows, last dim contiguous, K % 64 == 0."""
    return x.is_cuda and x.dtype == torch.float32 and K % 64 == 0 and x.shape[-1] == K and x.stride(-1) == 1 and x.data_ptr() % 16 == 0 and \
        (x.dim() == 1 or (x.stride(-2) % 4 == 0 and x.stride(-2) >= K))


def fused():
    """Whether the s2mel glue passes ride in their neighbours: the AdaLN norm in front of [w1; w3] writes the planes itself, the
    WaveNet split reads its halo rows from their mirror rows, the attention rotates q and k as it splits them.
    `IXTTS_S2MEL_FUSED=0` takes the separate passes (A/B runs, tests) -- the same bytes either way."""
    return os.environ.get("IXTTS_S2MEL_FUSED", "1") != "0"


def planes_buffer(rows, K, device, slot=0):
    """The scratch buffer `split` would put the planes of [rows, K] into."""
    nbytes = (K // 16) * 6 * int(_lib.lib().ixtts_gemm_x6_rows_padded(rows)) * 16
    key = (device, nbytes, slot)
    buf = _POOL.get(key)
    if buf is None:
        buf = _POOL[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return buf


def split(x, slot=0, halo=None):
    """x [..., K] fp32 (contiguous, or a 2-D view with one row stride) -> Planes.  `slot` names the scratch buffer: planes made with
    the same (size, slot) overwrite each other.  halo: x is a reflect-padded row buffer whose halo rows are taken from the interior
    rows they mirror, whatever they hold (the planes of `reflect_halo_rows` + split) -- (T, left, right) for sequences of
    left + T + right rows back to back, (pack, left, right) for a pack of padded sequences (`.tab` int32 device offsets, `.n`)."""
    K = int(x.shape[-1])
    if x.dim() != 2:
        x = x.reshape(-1, K) if x.is_contiguous() else x.contiguous().reshape(-1, K)
    rows, lda = int(x.shape[0]), int(x.stride(0))
    L = _lib.lib()
    buf = planes_buffer(rows, K, x.device, slot)
    with torch.cuda.device(x.device):
        if halo is None:
            _lib.check(L.ixtts_gemm_x6_split(x.data_ptr(), lda, buf.data_ptr(), rows, K, _lib.current_stream_ptr()), "ixtts_gemm_x6_split")
        elif isinstance(halo[0], int):
            T, left, right = halo
            _lib.check(L.ixtts_gemm_x6_split_halo(x.data_ptr(), lda, buf.data_ptr(), rows, K, T, left, right, _lib.current_stream_ptr()),
                       "ixtts_gemm_x6_split_halo")
        else:
            pk, left, right = halo
            assert rows == pk.rows and min(pk.lens) - left - right > max(left, right)
            _lib.check(L.ixtts_gemm_x6_split_halo_varlen(x.data_ptr(), lda, buf.data_ptr(), rows, K, pk.tab.data_ptr(), pk.n, left, right,
                                                         _lib.current_stream_ptr()), "ixtts_gemm_x6_split_halo_varlen")
    return Planes(buf, rows, K)


def linear(x, pl, out=None, accumulate=False, bias=True, tile=0, row0=0, rows=None, lead=None):
    """out[..., N] (+)= x[..., K] @ W^T (+ bias).  x: an fp32 device tensor (split here) or `Planes` (then rows [row0, row0 + rows) of
    it are the GEMM's A: a row-shifted window = one Conv1d tap).  out: fp32 tensor with contiguous rows, or None (allocated, shaped
    `lead + (N,)`).  accumulate=True adds to what `out` holds (torch's addmm_)."""
    K, N = pl.K, pl.N
    if not isinstance(x, Planes):
        lead = tuple(x.shape[:-1]) if lead is None else lead
        x = split(x)
    assert x.K == K, (x.K, K)
    M = (x.rows - row0) if rows is None else int(rows)
    if out is None:
        assert not accumulate
        out = torch.empty(*(lead if lead is not None else (M,)), N, dtype=torch.float32, device=pl.packed.device)
    assert out.shape[-1] == N and out.stride(-1) == 1 and out.numel() >= M * N
    ldc = int(out.stride(-2)) if out.dim() >= 2 else N
    b = pl.bias if (bias and pl.bias is not None) else None
    with torch.cuda.device(pl.packed.device):
        rc = _lib.lib().ixtts_gemm_x6_f32(x.buf.data_ptr(), x.rows, int(row0), pl.packed.data_ptr(), b.data_ptr() if b is not None else None, out.data_ptr(), ldc,
                                          M, N, K, 1 if accumulate else 0, int(tile), _lib.current_stream_ptr())
    _lib.check(rc, "ixtts_gemm_x6_f32")
    return out


SWIGLU, GATE = 1, 2  # pair epilogues of `pair_linear` (csrc/gemm_x6.hip EPI_*)


def interleave_halves(a, b):
    """Rows of a and b [F, ...] -> [2F, ...] interleaved in 32-row blocks (a[32q:32q+32], b[32q:32q+32], ...): the packing the pair
    epilogues read, so one 64-column block of the GEMM holds matching columns of both halves.  F a multiple of 32."""
    F = a.shape[0]
    assert b.shape == a.shape and F % 32 == 0, (tuple(a.shape), tuple(b.shape))
    return torch.stack([a.reshape(F // 32, 32, *a.shape[1:]), b.reshape(F // 32, 32, *b.shape[1:])], 1).reshape(2 * F, *a.shape[1:]).contiguous()


def pair_linear(x, pl, epilogue, taps=1, out=None, gate=None, gate_off=0, rows_per_batch=1, row0=0, rows=None, tile=0, seq_off=None):
    """out[M, N/2] = f(a, b) over a GEMM whose packed weights hold two halves interleaved (`interleave_halves`): SWIGLU silu(a) * b,
    GATE tanh(a + g_a) * sigmoid(b + g_b) with (g_a | g_b) = gate[batch of the row, gate_off : gate_off + N] and rows_per_batch rows per
    batch entry -- or, with `seq_off` (GATE only: an object with `.tab`, an int32 device tensor starting with the n + 1 row offsets of
    packed sequences, and `.n`), the gate row of the row's own sequence.  taps > 1: the weights are [N, taps * K_a] over planes of K_a
    columns, tap j reading the planes' rows shifted down by j (one GEMM for a k-tap Conv1d over a padded row buffer); M defaults to the
    rows the last tap still covers."""
    if not isinstance(x, Planes):
        x = split(x)
    assert pl.K == taps * x.K and pl.N % 64 == 0, (pl.K, taps, x.K, pl.N)
    M = (x.rows - row0 - (taps - 1)) if rows is None else int(rows)
    if out is None:
        out = torch.empty(M, pl.N // 2, dtype=torch.float32, device=pl.packed.device)
    assert out.shape[-1] == pl.N // 2 and out.stride(-1) == 1 and out.numel() >= M * (pl.N // 2)
    ldc = int(out.stride(-2)) if out.dim() >= 2 else pl.N // 2
    gp, gld, nb = None, 0, 1
    if epilogue == GATE:
        assert gate.is_contiguous() and gate.dim() == 2 and gate_off + pl.N <= gate.shape[1]
        gp, gld, nb = gate.data_ptr() + 4 * int(gate_off), int(gate.shape[1]), int(gate.shape[0])
    b = pl.bias
    if seq_off is not None:
        assert epilogue == GATE and seq_off.tab.is_cuda and gate.shape[0] >= seq_off.n
        with torch.cuda.device(pl.packed.device):
            rc = _lib.lib().ixtts_gemm_x6_pair_gate_varlen_f32(x.buf.data_ptr(), x.rows, int(row0), int(taps), pl.packed.data_ptr(),
                                                               b.data_ptr() if b is not None else None, gp, gld, seq_off.tab.data_ptr(), int(seq_off.n),
                                                               out.data_ptr(), ldc, M, pl.N, pl.K, int(tile), _lib.current_stream_ptr())
        _lib.check(rc, "ixtts_gemm_x6_pair_gate_varlen_f32")
        return out
    with torch.cuda.device(pl.packed.device):
        rc = _lib.lib().ixtts_gemm_x6_pair_f32(x.buf.data_ptr(), x.rows, int(row0), int(taps), pl.packed.data_ptr(), b.data_ptr() if b is not None else None,
                                               gp, gld, int(rows_per_batch), nb, out.data_ptr(), ldc, M, pl.N, pl.K, int(epilogue), int(tile),
                                               _lib.current_stream_ptr())
    _lib.check(rc, "ixtts_gemm_x6_pair_f32")
    return out
