"""The HIP BigVGAN against the fp64 twin of its oracle, as an error budget, on every conv tile the launchers can choose.

Each run is one 1-stage production-width handle of tests/bigvgan_budget.py through `ixtts_bigvgan_forward`; its error (max and rms,
relative to the twin's max and rms) stands next to the error the fp32 CPU oracle has on the same inputs.  The criterion is the one of
test_gpu_s2mel_fp64.py: a device path may sit at most 3 x (max) and 2 x (rms, floor 2e-7) above the CPU leg -- the same quality of
result in another summation order.  The fp32-vs-fp32 bars of test_gpu_bigvgan.py (5e-5, 1e-4) are some 250 times the arithmetic's noise;
a conv arithmetic that loses its low bf16 plane passes them and fails here (tests/test_bigvgan_twin.py shows that on the CPU).

At the shapes a test can afford the launchers' scores never choose the larger tiles, so the developer switch IXTTS_BV_TILE forces each
scored tile in turn, and `BigVGAN.tile_launches()` tells the test that the tile it names is the one that ran.  The rows of unequal
length then go through `forward_varlen` on every forced tile and must be bit-identical to `forward` on each row alone.

tools/bigvgan_error_budget.py records the same numbers in profiles/bigvgan_error_budget.json."""
import pytest
import torch

import bigvgan_budget as BB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def legs():
    return BB.Legs()


@pytest.fixture(scope="module")
def by_score(legs, dev):
    """Waveform of (mode, case) with the launcher's own tile choice, computed once."""
    cache = {}

    def get(mode, case):
        if (mode, case) not in cache:
            cache[mode, case] = legs.device(case, mode, None, dev)[2]
        return cache[mode, case]

    return get


def _within_budget(legs, case, mode, tile, dev):
    c_max, c_rms = legs.base[case]
    (e_max, e_rms), launches, wav = legs.device(case, mode, tile, dev)
    print(f"bigvgan budget {case} [{mode}{' tile ' + tile if tile else ''}]: device max {e_max:.3e} rms {e_rms:.3e} | fp32 CPU leg max {c_max:.3e} "
          f"rms {c_rms:.3e} | launches {launches}")
    assert 0.0 < c_max < 1e-5 and 0.0 < c_rms < 1e-5  # (the yardstick itself: the arithmetic's noise, not a broken CPU leg)
    lim_max, lim_rms = BB.limits(legs.base[case])
    assert e_max <= lim_max, (e_max, c_max)
    assert e_rms <= lim_rms, (e_rms, c_rms)
    return launches, wav


def _only_the_forced_tile_ran(launches, mode, tile):
    """Of the tiles the launcher chooses among by score, the forced one has launches and the others none."""
    for t in BB.TILES[mode]:
        assert (launches[t] > 0) == (t == tile), (tile, launches)


@pytest.mark.parametrize("case", list(BB.CASES))
@pytest.mark.parametrize("mode", list(BB.MODES))
def test_default_tile_choice_within_the_fp32_budget(legs, dev, mode, case):
    launches, _ = _within_budget(legs, case, mode, None, dev)
    assert sum(launches.values()) == 20  # conv_pre, the up-sampling conv and six convs in each of the three resblocks: every launch counted


FORCED_RUNS = [(m, c, t) for m in BB.MODES for c in BB.FORCED[m] for t in BB.TILES[m]]


@pytest.mark.parametrize("mode,case,tile", FORCED_RUNS, ids=[f"{m}-{c}-{t}" for m, c, t in FORCED_RUNS])
def test_forced_tile_within_the_fp32_budget(legs, dev, by_score, mode, case, tile):
    launches, wav = _within_budget(legs, case, mode, tile, dev)
    _only_the_forced_tile_ran(launches, mode, tile)
    # an output element is one lane's accumulator over the same (channel chunk, tap, partial product) order in whatever tile it
    # falls: the tile shape moves no bit (the property forward_varlen's bit-identity rests on, here across tile shapes)
    ref = by_score(mode, case)
    assert torch.equal(wav, ref), (wav - ref).abs().max().item()


VARLEN_RUNS = [(m, c, t) for m, c in BB.VARLEN for t in BB.TILES[m]]


@pytest.mark.parametrize("mode,case,tile", VARLEN_RUNS, ids=[f"{m}-{c}-{t}" for m, c, t in VARLEN_RUNS])
def test_forced_tile_rows_of_unequal_length_bit_identical_to_forward_alone(legs, dev, mode, case, tile):
    """Rows [F, 33, 1, 0] in a NaN-padded mel through `forward_varlen` (the kernels' VL instantiations of the forced tile): every row
    bit-identical to `forward` of the same handle on that row alone, nothing written past a row's length."""
    frames = BB.varlen_frames(case)
    F = BB.CASES[case]["F"]
    mel = BB.mel(case, rows=len(frames))
    pad = mel.clone()
    for b, f in enumerate(frames):
        pad[b, :, f:] = float("nan")
    m = BB.device_model(case, mode, tile, dev, legs.W[case])
    up = m.total_up
    out = torch.full((len(frames), 1, F * up), float("nan"), device=dev)
    m.forward_varlen(pad.to(dev), frames, out=out)
    _only_the_forced_tile_ran(m.tile_launches(), mode, tile)
    wav = out.cpu()
    for b, f in enumerate(frames):
        assert torch.isnan(wav[b, :, f * up:]).all(), (b, f)  # untouched
        if f:
            alone = m(mel[b:b + 1, :, :f].contiguous().to(dev)).cpu()
            assert not torch.isnan(alone).any()
            assert torch.equal(wav[b:b + 1, :, :f * up], alone), (b, f, (wav[b:b + 1, :, :f * up] - alone).abs().max().item())
    _only_the_forced_tile_ran(m.tile_launches(), mode, tile)


def test_the_switch_is_read_per_handle_and_refuses_unknown_tiles(dev, monkeypatch):
    from voice_tts_amd._lib import IxttsError
    from voice_tts_amd.bigvgan import BigVGAN

    cfg = BB.config("E")
    for conv, tile in (("x3", "64x64"), ("f32", "128x96"), ("x3", "128"), ("f32", "64X64")):  # each mode refuses the other's tile names
        monkeypatch.setenv("IXTTS_BV_CONV", conv)
        monkeypatch.setenv("IXTTS_BV_TILE", tile)
        with pytest.raises(IxttsError, match="IXTTS_BV_TILE"):
            BigVGAN(cfg, max_frames=4, device=dev)
    monkeypatch.delenv("IXTTS_BV_CONV")
    monkeypatch.setenv("IXTTS_BV_TILE", "128x128")
    m = BigVGAN(cfg, max_frames=4, device=dev).load_state_dict(BB.weights("E"))
    monkeypatch.delenv("IXTTS_BV_TILE")
    assert m.tile_launches() == {"128x128": 0, "128x96": 0, "64x128": 0, "fixed 32x128": 0, "fixed 64x128": 0}
    m(BB.mel("E")[:, :, :4].contiguous().to(dev))
    # E has no conv that goes by score: the switch changes nothing, every conv is counted on its fixed tile
    assert m.tile_launches() == {"128x128": 0, "128x96": 0, "64x128": 0, "fixed 32x128": 19, "fixed 64x128": 1}
