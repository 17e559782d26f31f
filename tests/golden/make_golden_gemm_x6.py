"""Recorded outputs of csrc/gemm_x6.hip for tests/test_gpu_gemm_x6_addressing.py: run ONCE, on a GPU, at the commit whose results the
kernel has to keep (the parent of the change that moved the operand addressing out of the main loop), never regenerated from the code
under test:

    python tests/golden/make_golden_gemm_x6.py      # -> tests/golden/gemm_x6_parent.npz

Every case's inputs come from a seeded CPU generator (`run_case`), so the test rebuilds them; the file holds, per case, the sha256 of the
output's bytes and -- for the first tile of a case, where the output is at most WHOLE_BYTES -- the output itself (all of them would
not fit a 0.5 MB file).  The cases are the smallest shapes at which a step-to-step address recurrence can go wrong: fewer steps than
copies in flight, row tiles that start inside a larger plane buffer (row0 = 5), ragged M and N, every tile shape, taps whose k-group
wraps every 4 steps."""
import hashlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "gemm_x6_parent.npz")
WHOLE_BYTES = 80 * 1024

PLAIN_SHAPES = [(1, 64, 64), (130, 192, 128), (257, 128, 192)]  # (M, N, K)
PLAIN_VARIANTS = ["bias", "nobias", "acc"]
SWIGLU_SHAPES = [(300, 128, 64), (257, 192, 192)]  # (M, N = 2 Fd, K)
GATE_N, GATE_KA, GATE_LAYERS = 192, 64, 3  # N / 2 = 96 output columns: the second 128-wide column tile is half empty
VARLEN_LENS = (37, 101, 64)  # three packed sequences of unequal length (rows, halo included)


def cases():
    """[(id, kind, args)] in a fixed order."""
    out = []
    for M, N, K in PLAIN_SHAPES:
        for var in PLAIN_VARIANTS:
            for tile in (2, 3, 4, 5):
                out.append((f"plain-{M}x{N}x{K}-{var}-t{tile}", "plain", (M, N, K, var, tile)))
    for M, N, K in SWIGLU_SHAPES:
        for tile in (2, 3):
            out.append((f"swiglu-{M}x{N}x{K}-t{tile}", "swiglu", (M, N, K, tile)))
    for taps in (2, 3, 5):
        for B in (2, 3):
            for T in (90, 203):
                for tile in (2, 3):
                    out.append((f"gate-k{taps}-B{B}-T{T}-t{tile}", "gate", (taps, B, T, tile)))
    for tile in (2, 3):
        out.append((f"gate-varlen-k5-t{tile}", "varlen", (5, tile)))
    out.append(("prod-swiglu-4644x3072x512", "swiglu", (4644, 3072, 512, 0)))
    out.append(("prod-gate-k5-B2-T1909-512", "prodgate", ()))
    return out


def _seed(cid):
    return int.from_bytes(hashlib.sha256(cid.rsplit("-t", 1)[0].encode()).digest()[:4], "little")  # the tiles of one case share inputs


def _gate_case(G, dev, g, taps, B, T, tile, C, N, nl, lens=None):
    """k taps over ONE split of a padded row buffer + bias + gate biases by batch entry (or by packed sequence, `lens`)."""
    rows = sum(lens) if lens is not None else B * (T + taps - 1)
    P = torch.randn(rows, C, generator=g)
    w = torch.randn(N, C, taps, generator=g) / (C * taps) ** 0.5
    bias = 0.1 * torch.randn(N, generator=g)
    nb = len(lens) if lens is not None else B
    gate = torch.randn(nb, N * nl, generator=g)
    off, h = N, N // 2  # gate_off != 0: layer 1's gate biases
    M = rows - (taps - 1)
    wcat = torch.cat([w[:, :, j] for j in range(taps)], 1)
    pl = G.PackedLinear(G.interleave_halves(wcat[:h], wcat[h:]).to(dev), G.interleave_halves(bias[:h], bias[h:]).to(dev))
    if lens is not None:
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        so = SimpleNamespace(tab=torch.from_numpy(offs).to(dev), n=len(lens))
        out = G.pair_linear(G.split(P.to(dev)), pl, G.GATE, taps=taps, gate=gate.to(dev), gate_off=off, seq_off=so, tile=tile)
        bidx = torch.from_numpy(np.searchsorted(offs[1:-1], np.arange(M), side="right"))
    else:
        out = G.pair_linear(G.split(P.to(dev)), pl, G.GATE, taps=taps, gate=gate.to(dev), gate_off=off, rows_per_batch=T + taps - 1, tile=tile)
        bidx = (torch.arange(M) // (T + taps - 1)).clamp(max=B - 1)
    Pd, wd = P.to(dev).double(), w.to(dev).double()
    acc = bias.to(dev).double() + sum(Pd[j:j + M] @ wd[:, :, j].t() for j in range(taps))
    xg = acc + gate.to(dev).double()[bidx.to(dev), off:off + N]
    ref = torch.tanh(xg[:, :h]) * torch.sigmoid(xg[:, h:])
    return out, ref, float(xg.abs().max())  # error on the GEMM's own scale (tests/test_gpu_s2mel_gemm.py)


def run_case(cid, kind, args, dev):
    """-> (out fp32 device tensor, fp64 reference, scale of the 2e-6 error bound)."""
    from voice_tts_amd import gemm as G

    g = torch.Generator().manual_seed(_seed(cid))
    if kind == "plain":
        M, N, K, var, tile = args
        row0, rows_total = 5, M + 11  # the GEMM's rows start inside a larger plane buffer
        xa = torch.randn(rows_total, K, generator=g) * torch.exp(torch.randn(rows_total, 1, generator=g))
        w = torch.randn(N, K, generator=g) / K ** 0.5
        b = torch.randn(N, generator=g)
        c0 = torch.randn(M, N, generator=g)
        pl = G.PackedLinear(w.to(dev), b.to(dev))
        out = c0.to(dev)  # without `accumulate` the kernel overwrites it
        G.linear(G.split(xa.to(dev)), pl, out=out, accumulate=var == "acc", bias=var != "nobias", tile=tile, row0=row0, rows=M)
        ref = xa[row0:row0 + M].to(dev).double() @ w.to(dev).double().t()
        if var != "nobias":
            ref = ref + b.to(dev).double()
        if var == "acc":
            ref = ref + c0.to(dev).double()
        return out, ref, float(ref.abs().max())
    if kind == "swiglu":
        M, N, K, tile = args
        Fd = N // 2
        x = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
        w1, w3 = torch.randn(Fd, K, generator=g) / K ** 0.5, torch.randn(Fd, K, generator=g) / K ** 0.5
        pl = G.PackedLinear(G.interleave_halves(w1, w3).to(dev))
        out = G.pair_linear(x.to(dev), pl, G.SWIGLU, tile=tile)
        xd = x.to(dev).double()
        a, b = xd @ w1.to(dev).double().t(), xd @ w3.to(dev).double().t()
        ref = a * torch.sigmoid(a) * b
        return out, ref, float(ref.abs().max())
    if kind == "gate":
        taps, B, T, tile = args
        return _gate_case(G, dev, g, taps, B, T, tile, GATE_KA, GATE_N, GATE_LAYERS)
    if kind == "varlen":
        taps, tile = args
        return _gate_case(G, dev, g, taps, None, None, tile, GATE_KA, GATE_N, GATE_LAYERS, lens=VARLEN_LENS)
    assert kind == "prodgate", kind
    return _gate_case(G, dev, g, 5, 2, 1909, 0, 512, 1024, 8)  # the bench's WaveNet in_layer: 3822 x (5 x 512) -> 1024


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    dev = torch.device("cuda:0")
    rec = {}
    for cid, kind, args in cases():
        out, ref, scale = run_case(cid, kind, args, dev)
        err = float((out.double() - ref).abs().max()) / scale
        assert err <= 2e-6, (cid, err)
        rec[cid + "/sha256"] = np.array(digest(out))
        if args and args[-1] in (2, 0) and out.numel() * 4 <= WHOLE_BYTES:
            rec[cid + "/out"] = out.cpu().numpy()
        print(f"{cid}: {tuple(out.shape)} max err {err:.2e} of scale {rec[cid + '/sha256']}", flush=True)
    np.savez(PATH, **rec)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
