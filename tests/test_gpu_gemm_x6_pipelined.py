"""Tile 6 of csrc/gemm_x6.hip: the 128 x 128 tile on a pipelined main loop -- the fragment reads of step s + 1 go into a second
register set and the copies of step s + 3 are issued among the MFMAs of step s.  For every accumulator the products and their order
are tile 3's, so every case runs tile 6 and tile 3 on the same inputs and requires the same bytes, and -- where
tests/golden/gemm_x6_parent.npz holds the case (recorded for tile 3 by tests/golden/make_golden_gemm_x6.py, whose case builder is
loaded unchanged) -- the recorded sha256 too.

Shapes: the smallest at which the pipeline can go wrong.  Plain entry at (M, N, K) = (1, 64, 64): 4 steps, the ring's depth, so the
loop body never runs and only the written-out last four steps do; (130, 192, 128): 8 steps, partial row and column tiles;
(257, 128, 192): 12 steps; each with bias, without, and accumulating, rows starting at row0 = 5 of a larger plane buffer.  Gate pair:
2, 3 and 5 taps over K_a = 64 (the k-group wraps every 4 steps: inside the ring's depth), B in {2, 3}, T in {90, 203}, gate_off != 0,
and over a sequence table of three unequal sequences.  Poison: NaN in the planes' padding rows and around the output's valid rows
and columns.  Selection: tile 0 on the WaveNet tap shape gives the same bytes with IXTTS_GEMM_X6_PIPE on and off."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_gemm_x6", os.path.join(HERE, "golden", "make_golden_gemm_x6.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

PIPE, BASE = 6, 3  # the pipelined tile and the tile whose bytes it has to give

PLAIN = [(M, N, K, var) for M, N, K in MG.PLAIN_SHAPES for var in MG.PLAIN_VARIANTS]
GATE = [(taps, B, T) for taps in (2, 3, 5) for B in (2, 3) for T in (90, 203)]
PROD = "prod-gate-k5-B2-T1909-512"  # the bench's WaveNet in_layer (tile 0): 3822 x (5 x 512) -> 1024


@pytest.fixture(scope="module")
def recorded():
    with np.load(MG.PATH) as z:
        return {k: z[k] for k in z.files}


def _both_tiles(recorded, base, kind, args):
    """Run the case `base` (id without its tile) on tile 6 and on tile 3; same bytes, and the bytes recorded for tile 3."""
    dev = torch.device("cuda:0")
    cid = f"{base}-t{BASE}"
    out6, ref, scale = MG.run_case(cid, kind, args + (PIPE,), dev)  # (the tiles of one case share a seed: the id's tile is not part of it)
    out6 = out6.clone()
    out3, _, _ = MG.run_case(cid, kind, args + (BASE,), dev)
    err = float((out6.double() - ref).abs().max()) / scale
    print(f"{base}: {tuple(out6.shape)} tile {PIPE} max err {err:.2e} of scale; differs from tile {BASE} in {int((out6 != out3).sum())} elements")
    assert torch.equal(out6, out3)
    assert cid + "/sha256" in recorded, cid
    assert MG.digest(out6) == str(recorded[cid + "/sha256"]), "output bytes differ from the recording"
    assert err <= 2e-6


@pytest.mark.parametrize("M,N,K,var", PLAIN, ids=[f"{M}x{N}x{K}-{var}" for M, N, K, var in PLAIN])
def test_plain_same_bytes_as_tile3(recorded, M, N, K, var):
    _both_tiles(recorded, f"plain-{M}x{N}x{K}-{var}", "plain", (M, N, K, var))


@pytest.mark.parametrize("taps,B,T", GATE, ids=[f"k{taps}-B{B}-T{T}" for taps, B, T in GATE])
def test_gate_taps_same_bytes_as_tile3(recorded, taps, B, T):
    _both_tiles(recorded, f"gate-k{taps}-B{B}-T{T}", "gate", (taps, B, T))


def test_gate_over_sequence_table_same_bytes_as_tile3(recorded):
    _both_tiles(recorded, "gate-varlen-k5", "varlen", (5,))


def _poison_plane_padding(G, planes):
    """NaN (bf16 0x7fc0) in every plane row past the split's own rows: what the tiles' last, partial row tile reads beside its rows."""
    Mpad = int(G._lib.lib().ixtts_gemm_x6_rows_padded(planes.rows))
    units = planes.buf.view(torch.int16).view(planes.K // 16, 6, Mpad, 8)
    assert Mpad > planes.rows
    units[:, :, planes.rows:, :] = 0x7FC0
    return Mpad - planes.rows


@pytest.mark.parametrize("kind", ["plain", "gate", "varlen"])
def test_poisoned_padding_changes_nothing_and_nothing_else_is_written(kind):
    from types import SimpleNamespace

    from voice_tts_amd import gemm as G

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(11)
    if kind == "plain":
        M, N, K, row0, rows_total = 130, 192, 128, 5, 141
        x = torch.randn(rows_total, K, generator=g).to(dev)
        pl = G.PackedLinear((torch.randn(N, K, generator=g) / K ** 0.5).to(dev), torch.randn(N, generator=g).to(dev))
        ncol = N

        def run(planes, out):
            G.linear(planes, pl, out=out, row0=row0, rows=M, tile=PIPE)
    else:
        taps, C, N, nl = 3, 64, 192, 3
        lens = (37, 101, 64) if kind == "varlen" else (92, 92)  # B = 2 sequences of T + taps - 1 = 92 rows
        rows_total = sum(lens)
        M, ncol = rows_total - (taps - 1), N // 2
        x = torch.randn(rows_total, C, generator=g).to(dev)
        w = torch.randn(N, C * taps, generator=g) / (C * taps) ** 0.5
        b = 0.1 * torch.randn(N, generator=g)
        pl = G.PackedLinear(G.interleave_halves(w[:ncol], w[ncol:]).to(dev), G.interleave_halves(b[:ncol], b[ncol:]).to(dev))
        gate = torch.randn(len(lens), N * nl, generator=g).to(dev)
        offs = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=dev)
        so = SimpleNamespace(tab=offs, n=len(lens)) if kind == "varlen" else None

        def run(planes, out):
            G.pair_linear(planes, pl, G.GATE, taps=taps, out=out, gate=gate, gate_off=N, rows_per_batch=lens[0], seq_off=so, tile=PIPE)

    clean = torch.empty(M, ncol, device=dev)
    run(G.split(x), clean)
    assert bool(torch.isfinite(clean).all())
    planes = G.split(x)
    npad = _poison_plane_padding(G, planes)
    big = torch.full((M + 7, ncol + 5), float("nan"), device=dev)  # the valid block sits at the top left, row stride ncol + 5
    run(planes, big[:M, :ncol])
    torch.cuda.synchronize()
    print(f"{kind}: {M} x {ncol} valid outputs, {npad} poisoned plane rows, {big.numel() - M * ncol} poisoned output elements")
    assert torch.equal(big[:M, :ncol], clean), "NaN from the padding reached a valid output"
    assert bool(torch.isnan(big[M:]).all()) and bool(torch.isnan(big[:, ncol:]).all()), "written outside the valid rows and columns"


_CHILD = """
import importlib.util, os, sys, torch
sys.path.insert(0, sys.argv[1])
spec = importlib.util.spec_from_file_location("make_golden_gemm_x6", os.path.join(sys.argv[1], "tests", "golden", "make_golden_gemm_x6.py"))
MG = importlib.util.module_from_spec(spec); spec.loader.exec_module(MG)
out, _, _ = MG.run_case(sys.argv[2], "prodgate", (), torch.device("cuda:0"))
print("DIGEST", MG.digest(out))
"""


def _tile0_digest_in_child(pipe):
    """The library reads IXTTS_GEMM_X6_PIPE once, so each setting gets a process of its own."""
    env = dict(os.environ)
    env.pop("IXTTS_GEMM_X6_PIPE", None)
    if not pipe:
        env["IXTTS_GEMM_X6_PIPE"] = "0"
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.dirname(HERE), PROD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0]


def test_tile0_on_the_tap_shape_same_bytes_with_the_pipelined_loop_on_and_off(recorded):
    if os.environ.get("IXTTS_GEMM_X6_PIPE") is None:
        out, ref, scale = MG.run_case(PROD, "prodgate", (), torch.device("cuda:0"))
        assert float((out.double() - ref).abs().max()) / scale <= 2e-6
        on = MG.digest(out)
    else:
        on = _tile0_digest_in_child(True)
    off = _tile0_digest_in_child(False)
    print(f"tile 0, {PROD}: pipelined loop on {on[:16]} off {off[:16]} recorded {str(recorded[PROD + '/sha256'])[:16]}")
    assert on == off == str(recorded[PROD + "/sha256"])
