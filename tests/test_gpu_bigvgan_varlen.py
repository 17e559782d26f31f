"""GPU: one BigVGAN pass over rows of unequal length (`ixtts_bigvgan_forward_varlen`, `BigVGAN.forward_varlen` / `forward_many`).

Bounds are those of test_gpu_bigvgan.py: 5e-5 max-abs on the tiny 64-channel, 6-stage generator (fixtures and CPU oracle), 1e-4 x
max(1, |ref|max) on the production-width one-stage slices.  On top of them every row must be BIT-identical to `forward` on that row
alone, and to itself whatever lies in the padding, in the other rows and in the workspace: padding is masked by selection (it is never
read), and an output element is one lane's accumulator over the same sequence of products in whatever tile it falls.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EDGE_FRAMES = [4, 5, 3, 8, 40, 1, 0, 33]  # 4 = one 1024-sample Snake tile at the last stage, 5 = that + 256; 1, 3 < the filter halo; 0 empty; 40 = Fmax


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _mel(B, F, seed):
    return (torch.randn(B, 80, F, generator=torch.Generator().manual_seed(seed)) * 2 - 4).clamp(-11.5, 2)


@pytest.fixture(scope="module")
def tiny(dev):
    import voice_tts_amd.weights as WR
    from voice_tts_amd.bigvgan import BigVGAN

    cfg = WR.tiny_bigvgan_cfg(64)
    W = WR.make_bigvgan_weights(cfg, seed=21)
    m = BigVGAN(cfg, max_frames=64, device=dev).load_state_dict(W)
    return m, cfg, W


@pytest.fixture(scope="module")
def edge(tiny):
    """The edge rows in a [8, 80, 40] mel (row b valid up to EDGE_FRAMES[b]) and the CPU oracle's waveform of each row alone."""
    from oracle import vocoder as OV

    m, cfg, W = tiny
    mel = _mel(len(EDGE_FRAMES), 40, 31)
    refs = [OV.bigvgan_forward(mel[b:b + 1, :, :f], W, cfg) if f else torch.zeros(1, 1, 0) for b, f in enumerate(EDGE_FRAMES)]
    return mel, refs


def _check_rows(wav, refs, frames, up, bound):
    for b, f in enumerate(frames):
        got = wav[b:b + 1, :, :f * up]
        assert got.shape == refs[b].shape
        if f:
            err = (got - refs[b]).abs().max().item()
            print(f"row {b} frames {f}: max|err| {err:.3g}")
            assert err <= bound, (b, f, err)


def test_reference_fixture_rows_in_one_call(golden, tiny, dev):
    m, cfg, W = tiny
    g = golden("bigvgan_tiny.npz")
    frames = [1, 7, 40]
    mel = torch.zeros(3, 80, 40)
    for b, f in enumerate(frames):
        mel[b, :, :f] = torch.from_numpy(g[f"mel_f{f}"])[0]
    wav = m.forward_varlen(mel.to(dev), frames).cpu()
    _check_rows(wav, [torch.from_numpy(g[f"wav_f{f}"]) for f in frames], frames, m.total_up, 5e-5)


def test_edge_lengths_vs_oracle(tiny, edge, dev):
    m, cfg, W = tiny
    mel, refs = edge
    wav = m.forward_varlen(mel.to(dev), EDGE_FRAMES).cpu()
    _check_rows(wav, refs, EDGE_FRAMES, m.total_up, 5e-5)
    for b, f in enumerate(EDGE_FRAMES):  # nothing is written past a row's length
        assert not wav[b, :, f * m.total_up:].any()


def test_edge_lengths_f32_convs(tiny, edge, dev, monkeypatch):
    """The same call on the fp32-MFMA conv kernels (conv1d.hip), on a handle created under IXTTS_BV_CONV=f32."""
    from voice_tts_amd.bigvgan import BigVGAN

    _, cfg, W = tiny
    mel, refs = edge
    monkeypatch.setenv("IXTTS_BV_CONV", "f32")
    m = BigVGAN(cfg, max_frames=64, device=dev).load_state_dict(W)
    monkeypatch.delenv("IXTTS_BV_CONV")
    wav = m.forward_varlen(mel.to(dev), EDGE_FRAMES).cpu()
    _check_rows(wav, refs, EDGE_FRAMES, m.total_up, 5e-5)
    for b, f in enumerate(EDGE_FRAMES):
        if f:
            assert torch.equal(wav[b:b + 1, :, :f * m.total_up], m(mel[b:b + 1, :, :f].contiguous().to(dev)).cpu()), (b, f)


def test_whole_tiles_of_padding(tiny, edge, dev):
    """Fmax = 129 with every row <= 7 frames: most tiles of every kernel lie wholly in the padding."""
    m, cfg, W = tiny
    mel, refs = edge
    rows = [b for b, f in enumerate(EDGE_FRAMES) if f <= 7]
    frames = [EDGE_FRAMES[b] for b in rows]
    pad = torch.full((len(rows), 80, 129), float("nan"))
    for i, b in enumerate(rows):
        pad[i, :, :frames[i]] = mel[b, :, :frames[i]]
    wav = m.forward_varlen(pad.to(dev), frames).cpu()
    _check_rows(wav, [refs[b] for b in rows], frames, m.total_up, 5e-5)
    for i, f in enumerate(frames):
        assert not wav[i, :, f * m.total_up:].any()


def test_padding_independence_bitwise(tiny, edge, dev):
    """Same (B, Fmax, frames) twice: mel padding 0 / NaN, the other rows different, the second call on a handle whose workspace a
    longer call has just filled.  Row 4 (40 frames) and row 1 (5 frames) are the same in both; both must come out bit-identical,
    every element inside a row's length written, everything past it untouched."""
    from voice_tts_amd.bigvgan import BigVGAN

    m, cfg, W = tiny
    mel, _ = edge
    up = m.total_up
    keep = (1, 4)

    def call(model, pad_value, seed):
        x = _mel(len(EDGE_FRAMES), 40, seed)
        for b in keep:
            x[b] = mel[b]
        for b, f in enumerate(EDGE_FRAMES):
            x[b, :, f:] = pad_value
        out = torch.full((len(EDGE_FRAMES), 1, 40 * up), float("nan"), device=dev)
        model.forward_varlen(x.to(dev), EDGE_FRAMES, out=out)
        return out.cpu()

    a = call(m, 0.0, 101)
    m2 = BigVGAN(cfg, max_frames=64, device=dev).load_state_dict(W)
    m2(_mel(6, 64, 7).to(dev) * float("inf"))  # a longer call (6 x 64 >= 8 x 40 frames: the same buffers) leaves NaN all over the workspace
    b_ = call(m2, float("nan"), 202)
    for r, f in enumerate(EDGE_FRAMES):
        for w in (a, b_):
            assert not torch.isnan(w[r, :, :f * up]).any(), r
            assert torch.isnan(w[r, :, f * up:]).all(), r
    for r in keep:
        f = EDGE_FRAMES[r]
        assert torch.equal(a[r, :, :f * up], b_[r, :, :f * up]), r
    assert not torch.equal(a[3, :, :8 * up], b_[3, :, :8 * up])  # (the other rows really differed)


def test_rows_bit_identical_to_forward_alone(tiny, edge, dev):
    m, cfg, W = tiny
    mel, _ = edge
    wav = m.forward_varlen(mel.to(dev), EDGE_FRAMES).cpu()
    for b, f in enumerate(EDGE_FRAMES):
        alone = m(mel[b:b + 1, :, :f].contiguous().to(dev)).cpu()
        diff = (wav[b:b + 1, :, :f * m.total_up] - alone).abs().max().item() if f else 0.0
        print(f"row {b} frames {f}: max|varlen - alone| {diff:.3g}")
        assert torch.equal(wav[b:b + 1, :, :f * m.total_up], alone), (b, f, diff)


def test_forward_many_order_groups_and_empty(tiny, edge, dev, monkeypatch):
    m, cfg, W = tiny
    mel, _ = edge
    assert m.forward_many([]) == []
    monkeypatch.setenv("IXTTS_BV_BATCH_FRAMES", "64")  # several groups, and the 40-frame row on its own
    frames = [f for f in EDGE_FRAMES if f]
    mels = [mel[b:b + 1, :, :f].contiguous().to(dev) for b, f in enumerate(EDGE_FRAMES) if f]
    outs = m.forward_many(mels)
    assert len(outs) == len(mels)
    for x, f, w in zip(mels, frames, outs):
        assert w.shape == (1, 1, f * m.total_up)
        assert torch.equal(w, m(x))


@pytest.mark.parametrize("C_,k,d", [(768, 11, 5), (384, 7, 3), (192, 3, 1), (96, 11, 5), (48, 7, 1), (24, 11, 3)])
def test_production_width_slices_varlen(dev, C_, k, d):
    """The one-stage production-width handles of test_production_width_resblock_slices with B = 3, lengths [F, 33, 1]: all three
    tile shapes of conv1d_x3.hip (Cout 768 .. 24) with rows that end inside a tile, and tiles wholly past a row's end."""
    from oracle import vocoder as OV
    import voice_tts_amd.weights as WR
    from voice_tts_amd.bigvgan import BigVGAN

    cfg = dict(WR.BIGVGAN_CFG)
    cfg.update(upsample_initial_channel=2 * C_, upsample_rates=(2,), upsample_kernel_sizes=(4,),
               resblock_kernel_sizes=(k, 3, 3), resblock_dilation_sizes=((d, 1, 1), (1, 1, 1), (1, 1, 1)))
    W = WR.make_bigvgan_weights(cfg, seed=C_ + k)
    F = 70 if C_ >= 384 else 150
    frames = [F, 33, 1]
    mel = _mel(3, F, C_)
    m = BigVGAN(cfg, max_frames=F, device=dev).load_state_dict(W)
    pad = mel.clone()
    for b, f in enumerate(frames):
        pad[b, :, f:] = float("nan")
    wav = m.forward_varlen(pad.to(dev), frames).cpu()
    for b, f in enumerate(frames):
        ref = OV.bigvgan_forward(mel[b:b + 1, :, :f], W, cfg)
        got = wav[b:b + 1, :, :f * m.total_up]
        err = (got - ref).abs().max().item()
        print(f"C {C_} row {b} frames {f}: max|err| {err:.3g} (|ref|max {ref.abs().max().item():.3g})")
        assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (b, f, err)
        assert torch.equal(got, m(mel[b:b + 1, :, :f].contiguous().to(dev)).cpu()), (b, f)
    assert OV.bigvgan_forward(mel[:1], W, cfg).abs().max() > 0.02


def test_arguments(tiny, dev):
    from voice_tts_amd import _lib

    m, cfg, W = tiny
    L = _lib.lib()
    mel = _mel(2, 8, 3).to(dev)
    wav = torch.zeros(2, 1, 8 * m.total_up, device=dev)
    fd = torch.tensor([8, 9], dtype=torch.int32, device=dev)

    def call(frames_host, B, Fmax):
        host = (C.c_int * 2)(*frames_host)
        return L.ixtts_bigvgan_forward_varlen(m._h, mel.data_ptr(), fd.data_ptr(), host, B, Fmax, wav.data_ptr(), _lib.current_stream_ptr())

    assert call([8, 9], 2, 8) == -1  # IXTTS_ERR_ARG: frames_host[1] > Fmax
    assert call([8, -1], 2, 8) == -1
    assert call([8, 8], 0, 8) == 0 and call([8, 8], 2, 0) == 0
    torch.cuda.synchronize(dev)
    assert not wav.any()  # none of those calls wrote anything
    with pytest.raises(_lib.IxttsError):
        m.forward_varlen(mel, [8, 9])
    # the device table alone out of range: the kernels clamp it to Fmax themselves
    assert call([8, 8], 2, 8) == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(wav[1:2], m(mel[1:2].contiguous()))
