"""The whole s2mel stage with producers writing the planes of csrc/gemm_x6.hip themselves (the FFN AdaLN norm) and the WaveNet split
reading its halo rows from their mirror rows, against the separate passes of the same build (`IXTTS_S2MEL_FUSED=0`): the mel must be
the same bytes.  The tiny s2mel of tests/synthetic_model_dir.py (hidden 128, 2 heads of 64, depth 3, WaveNet 128), 3 Euler steps, one
segment through `__call__` and three unequal ones through `solve_many` (packed rows)."""
import numpy as np
import pytest
import torch

import voice_tts_amd.gemm as G
import voice_tts_amd.s2mel as S2
from synthetic_model_dir import twin_cfgs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny():
    cfg = twin_cfgs()[2]
    m = S2.S2Mel(S2.make_s2mel_weights(cfg, seed=77), cfg, device=DEV)
    g = torch.Generator().manual_seed(78)
    items, noises = [], []
    for n, Tp in [(20, 30), (41, 17), (9, 40)]:
        items.append((torch.randn(1, n, cfg["gpt_dim"], generator=g).to(DEV), torch.randint(0, cfg["codebook_size"], (1, n), generator=g).to(DEV),
                      torch.randn(1, Tp, cfg["content_dim"], generator=g).to(DEV), (torch.randn(1, 80, Tp, generator=g) * 2 - 5).to(DEV),
                      torch.randn(1, cfg["style_dim"], generator=g).to(DEV)))
        noises.append(torch.randn(1, 80, Tp + int(n * 1.72), generator=g).to(DEV))
    return m, items, noises


def _poison():
    for buf in G._POOL.values():
        buf.fill_(0xA5)


def _both(monkeypatch, run):
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("IXTTS_S2MEL_FUSED", flag)
        _poison()
        outs.append([np.ascontiguousarray(o.cpu().numpy()) for o in run()])
    return outs


def test_uniform_mel_bytes_equal(tiny, monkeypatch):
    m, items, noises = tiny
    assert m._x6(m.x6_w13) and m._x6(m.x6_wn)
    it, z = items[0], noises[0]
    fused, separate = _both(monkeypatch, lambda: [m(it[0], it[1], torch.tensor([it[1].shape[1]], device=DEV), it[2], it[3], it[4], n_timesteps=3, noise=z)])
    assert np.isfinite(fused[0]).all()
    assert np.array_equal(fused[0].view(np.uint8), separate[0].view(np.uint8))


def test_cached_t_tables_leave_the_mel_bytes(tiny, monkeypatch):
    """What a DiT evaluation derives from t alone is kept per (n_timesteps, step, batch): the solve that fills the tables, a solve that
    reads them (another segment, another length) and a solve with `IXTTS_S2MEL_TCACHE=0` give the same bytes; another n_timesteps
    and the stack without CFG get tables of their own."""
    m, items, noises = tiny
    run = lambda i, **kw: np.ascontiguousarray(m(items[i][0], items[i][1], torch.tensor([items[i][1].shape[1]], device=DEV), items[i][2], items[i][3],  # noqa: E731
                                                 items[i][4], noise=noises[i], **kw).cpu().numpy()).view(np.uint8)
    cases = [(0, dict(n_timesteps=3)), (1, dict(n_timesteps=3)), (1, dict(n_timesteps=2)), (0, dict(n_timesteps=3, inference_cfg_rate=0.0))]
    monkeypatch.setenv("IXTTS_S2MEL_TCACHE", "0")
    m._t_consts.clear()
    plain = [run(i, **kw) for i, kw in cases]
    assert not m._t_consts
    monkeypatch.delenv("IXTTS_S2MEL_TCACHE")
    for rnd in range(2):  # the first round fills the tables, the second only reads them
        for (i, kw), want in zip(cases, plain):
            assert np.array_equal(run(i, **kw), want), (rnd, i, kw)
    assert {k[0] for k in m._t_consts} == {(3, s, 2) for s in (1, 2, 3)} | {(2, s, 2) for s in (1, 2)} | {(3, s, 1) for s in (1, 2, 3)}


def test_solve_many_mel_bytes_equal(tiny, monkeypatch):
    m, items, noises = tiny
    assert all(m.packable(it[2].shape[1] + int(it[1].shape[1] * 1.72), it[3].shape[-1]) for it in items)
    fused, separate = _both(monkeypatch, lambda: m.solve_many(items, n_timesteps=3, noises=noises))
    for a, b in zip(fused, separate):
        assert np.isfinite(a).all()
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
