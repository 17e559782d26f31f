"""The dense DiT attention (`ixtts_attn_full_f32`: csrc/attn_full.hip, attn_full_x3.hip) against fp64 softmax(scale q k^T) v at the
lengths where its launch logic changes: the last unsplit lengths, the first split ones, and the lengths at which
ceil(tiles / KSPLIT) tiles per split leave one or two splits WITHOUT keys (their partials are m = -inf, l = 0, and the merge kernel
must give them weight 0).  Both builds: the default (three bf16 pieces per operand) and IXTTS_ATTN_FULL=f32 (fp32 MFMA).

The boundary cases bring a workspace of their own, pre-filled with 0xFF bytes (NaN as floats): a split without keys that left its
partials unwritten poisons the merge (tried: 29 cases of this file fail, no older test does).  The merge kernel's `m > -inf` guard
itself is not what they rest on: without it the weight is exp2(-inf - M) = 0 all the same, and every case passes."""
import contextlib
import ctypes as C
import functools
import math
import os
import re

import pytest
import torch

from voice_tts_amd import _lib
from voice_tts_amd import s2mel as S

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BAR = 2e-5  # the project's bar for this kernel: 2e-5 x max(1, |ref|max)
MODES = ["x3", "f32"]
KT, KSPLIT = 64, {"x3": 5, "f32": 4}  # keys per tile, key-range splits (csrc/attn_full.h; held to the header below)

# (B, H, T): T at the launch boundaries with (1, 2); one split case with all three factors of the workspace row index
# (split * B * H + bh) * T + t above 1; the unsplit kernel over 17 tiles, the last with one key
BOUNDARY = [(1, 2, t) for t in (127, 128, 129, 255, 256, 257, 320, 321, 384, 385, 576, 704, 1024)] + [(2, 3, 321), (4, 16, 1025)]
# what the launcher is expected to do there: (splits?, tiles per split of the x3 build, of the fp32 build)
EXPECTED = {
    127: (False, None, None), 128: (False, None, None), 129: (False, None, None), 255: (False, None, None), 256: (False, None, None),
    257: (True, [1, 1, 1, 1, 1], [2, 2, 1, 0]), 320: (True, [1, 1, 1, 1, 1], [2, 2, 1, 0]),
    321: (True, [2, 2, 2, 0, 0], [2, 2, 2, 0]), 384: (True, [2, 2, 2, 0, 0], [2, 2, 2, 0]),
    385: (True, [2, 2, 2, 1, 0], [2, 2, 2, 1]), 576: (True, [2, 2, 2, 2, 1], [3, 3, 3, 0]),
    704: (True, [3, 3, 3, 2, 0], [3, 3, 3, 2]), 1024: (True, [4, 4, 4, 4, 0], [4, 4, 4, 4]), 1025: (False, None, None),
}


def should_split(B, H, T):
    """The launcher's condition (attn_full.hip): more than four tiles, and an unsplit grid that cannot give every SIMD two waves."""
    return T > 256 and math.ceil(T / 128) * B * H < 512


def shares(T, ksplit):
    tiles = math.ceil(T / KT)
    per = math.ceil(tiles / ksplit)
    return [max(0, min(per, tiles - s * per)) for s in range(ksplit)]


@contextlib.contextmanager
def _mode(mode):
    old = os.environ.get("IXTTS_ATTN_FULL")
    try:
        os.environ.pop("IXTTS_ATTN_FULL", None)
        if mode == "f32":
            os.environ["IXTTS_ATTN_FULL"] = "f32"
        yield
    finally:
        os.environ.pop("IXTTS_ATTN_FULL", None)
        if old is not None:
            os.environ["IXTTS_ATTN_FULL"] = old


def _ref(q, k, v, scale=None):
    """softmax(scale q k^T) v in fp64 (plain formula, on the device's fp64 units); q, k, v [B, T, H, 64]."""
    sc = 1.0 / math.sqrt(q.shape[-1]) if scale is None else scale
    q, k, v = (t.double().transpose(1, 2) for t in (q, k, v))
    return (torch.softmax(q @ k.transpose(-1, -2) * sc, dim=-1) @ v).transpose(1, 2)


def _err(out, ref):
    assert torch.isfinite(out).all()
    return (out.double() - ref).abs().max().item()


def _direct(q, k, v, scale=None, workspace=True, head_dim=64):
    """The C entry as `s2mel.attn_full` calls it, with a workspace of this test's own, pre-filled with 0xFF bytes (NaN as floats):
    returns (rc, out, whether the key-split partials were written)."""
    B, T, H, d = q.shape
    L = _lib.lib()
    out = torch.full((B, T, H, 64), -12345.0, device=DEV)
    nws = L.ixtts_attn_full_workspace_bytes(B, H, T) if workspace else 0
    ws = torch.full((max(nws, 16),), 0xFF, dtype=torch.uint8, device=DEV)
    sc = float(scale if scale is not None else 1.0 / math.sqrt(64))
    with torch.cuda.device(DEV):
        rc = L.ixtts_attn_full_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, T, head_dim, q.stride(0), q.stride(1), q.stride(2),
                                   out.stride(0), out.stride(1), out.stride(2), C.c_float(sc), ws.data_ptr() if workspace else None, nws,
                                   _lib.current_stream_ptr())
    torch.cuda.synchronize()
    partial_bytes = max(KSPLIT.values()) * B * H * T * (64 + 2) * 4
    return rc, out, bool(workspace and (ws[:partial_bytes] != 0xFF).any().item())


def _qkv(B, H, T, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, T, H, 64, generator=g).to(DEV) for _ in range(3))
    return q * 2.0, k, v  # a sharper softmax


@functools.lru_cache(maxsize=None)
def _boundary(B, H, T, mode):
    """(error against fp64, |ref|max, whether the keys were split) of one boundary shape in one build; computed once."""
    q, k, v = _qkv(B, H, T, 7 * T + B)
    with _mode(mode):
        rc, out, split = _direct(q, k, v)
    assert rc == 0
    ref = _ref(q, k, v)
    return _err(out, ref), ref.abs().max().item(), split


def test_launch_table_is_the_headers():
    """The shapes above are edges of THIS launch logic: 64-key tiles, 4 / 5 splits, split when T > 256 and ceil(T/128) B H < 512.  A
    change of those constants moves the edges: this test then fails, and the shapes above are due for review."""
    here = os.path.dirname(os.path.abspath(S.__file__))
    hdr = open(os.path.join(here, "csrc", "attn_full.h")).read()
    const = {n: int(v) for n, v in re.findall(r"constexpr int (\w+) = (\d+);", hdr)}
    assert (const["AF_KT"], const["AF_KSPLIT"], const["AX_KSPLIT"], const["AF_QW"] * const["AF_WAVES"]) == (KT, KSPLIT["f32"], KSPLIT["x3"], 128)
    src = open(os.path.join(here, "csrc", "attn_full.hip")).read()
    assert "T > 4 * AF_KT && (long)qblocks * B * H * AF_WAVES < 2 * 1024" in src
    for B, H, T in BOUNDARY:
        want, x3, f32 = EXPECTED[T]
        assert should_split(B, H, T) == want, (B, H, T)
        if want:
            assert shares(T, KSPLIT["x3"]) == x3 and shares(T, KSPLIT["f32"]) == f32, (T, shares(T, 5), shares(T, 4))
    assert any(0 in EXPECTED[t][1] for t in EXPECTED if EXPECTED[t][0]) and any(0 in EXPECTED[t][2] for t in EXPECTED if EXPECTED[t][0])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,H,T", BOUNDARY)
def test_attn_full_at_the_launch_boundaries(B, H, T, mode):
    e, scale, split = _boundary(B, H, T, mode)
    print(f"attn_full {mode} (B, H, T) = ({B}, {H}, {T}): max|err| {e:.3e}, |ref|max {scale:.2f}, split {split}")
    assert split == should_split(B, H, T) == EXPECTED[T][0], "the launcher split (or did not) against the table"
    assert e <= BAR * max(1.0, scale), e


@pytest.mark.parametrize("B,H,T", BOUNDARY)
def test_both_builds_give_the_same_quality(B, H, T):
    (e_x3, _, _), (e_f32, _, _) = _boundary(B, H, T, "x3"), _boundary(B, H, T, "f32")
    assert e_x3 <= 3.0 * e_f32 + 1e-7, (e_x3, e_f32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("scale", [0.25, 1.0])
def test_attn_full_scale(scale, mode):
    q, k, v = _qkv(1, 2, 321, 11)
    with _mode(mode):
        out = S.attn_full(q, k, v, scale=scale)
    ref = _ref(q, k, v, scale)
    assert _err(out, ref) <= BAR * max(1.0, ref.abs().max().item())
    assert not torch.allclose(ref, _ref(q, k, v), atol=1e-3)  # (the scale matters on these inputs)


@pytest.mark.parametrize("T", [385, 1024])
def test_attn_full_dominant_key_moves_between_splits(T):
    """One planted key per query, 12 above its typical score (exp(-12) = 6e-6 for the others): in the first tile for even queries, in
    the last split that has keys for odd ones.  The running maximum is then set by another split for every second query, and the merge
    weighs the other splits by 2^(m_s - M) far below 1."""
    B, H = 1, 2
    g = torch.Generator().manual_seed(T)
    q, k, v = (torch.randn(B, T, H, 64, generator=g) for _ in range(3))
    last_tile = KT * (math.ceil(T / KT) - 1)
    for mode in MODES:  # the planted keys of odd queries sit in the last split with keys, in both builds
        sh = shares(T, KSPLIT[mode])
        lo = KT * sum(sh[:max(s for s in range(len(sh)) if sh[s])])
        assert lo <= last_tile < T
    i = torch.arange(T)
    j = torch.where(i % 2 == 0, i % KT, last_tile + i % (T - last_tile))
    kj = k[:, j]  # [B, T, H, 64]: each query's planted key
    q = q + 12.0 * 8.0 * kj / (kj * kj).sum(-1, keepdim=True)  # q . k_j grows by 96: 12 after the 1/8 scale
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    ref = _ref(q, k, v)
    w = torch.softmax(torch.einsum("bthd,bshd->bhts", q.double(), k.double()) / 8.0, -1)
    assert (w.argmax(-1).cpu() == j).all() and w.max(-1).values.min().item() > 0.5  # (the planted key dominates every row)
    errs = {}
    for mode in MODES:
        with _mode(mode):
            errs[mode] = _err(S.attn_full(q, k, v), ref)
        assert errs[mode] <= BAR * max(1.0, ref.abs().max().item()), (mode, errs[mode])
    assert errs["x3"] <= 3.0 * errs["f32"] + 1e-7, errs


@pytest.mark.parametrize("mode", MODES)
def test_attn_full_strided_views_of_the_fused_buffer(mode):
    """q, k, v as the DiT hands them over: views of one [B, T, 3, H, 64] buffer."""
    B, H, T = 2, 3, 321
    qkv = (torch.randn(B, T, 3, H, 64, generator=torch.Generator().manual_seed(4)) * 1.5).to(DEV)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    assert not q.is_contiguous() and should_split(B, H, T)
    with _mode(mode):
        out = S.attn_full(q, k, v)
    ref = _ref(q, k, v)
    assert _err(out, ref) <= BAR * max(1.0, ref.abs().max().item())


def test_attn_full_without_a_workspace_and_refusals():
    """No workspace: the unsplit fp32 kernel whatever the build asked for (bit-identical to IXTTS_ATTN_FULL=f32 where that does not
    split either), at the same bar.  Empty shapes need no workspace; head_dim 32 is refused and nothing is written."""
    q, k, v = _qkv(1, 2, 300, 5)
    rc, out, split = _direct(q, k, v, workspace=False)
    ref = _ref(q, k, v)
    assert rc == 0 and not split and _err(out, ref) <= BAR * max(1.0, ref.abs().max().item())
    q, k, v = _qkv(1, 2, 256, 6)
    rc, bare, _ = _direct(q, k, v, workspace=False)
    with _mode("f32"):
        rc2, f32, _ = _direct(q, k, v)
    rc3, x3, _ = _direct(q, k, v)
    assert rc == rc2 == rc3 == 0 and torch.equal(bare, f32) and not torch.equal(bare, x3)
    L = _lib.lib()
    for shape in ((0, 2, 300), (1, 0, 300), (1, 2, 0), (-1, 2, 300)):
        assert L.ixtts_attn_full_workspace_bytes(*shape) == 0
    assert L.ixtts_attn_full_workspace_bytes(1, 2, 300) > 0
    q32 = torch.randn(1, 64, 2, 32, device=DEV)
    rc, out, _ = _direct(q32, q32, q32, head_dim=32)
    assert rc != 0 and torch.equal(out, torch.full_like(out, -12345.0))
    with pytest.raises(_lib.IxttsError):
        _lib.check(rc, "ixtts_attn_full_f32")
