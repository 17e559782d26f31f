"""CPU-side: the decode-slot limits by weight type (`ixtts_gpt_max_batch_for`: 32 / 32 / 16; `ixtts_gpt_max_batch` stays 16) and
the clamp arithmetic of the engines `IndexTTS2` builds beside its own -- `_many_engine_for` and `_beam_group_engine` -- with a
stub in place of `GptEngine` (no GPU: the library only has to load, as in test_cabi_load.py)."""
import os

import pytest

from voice_tts_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def library():
    if not os.path.exists(_lib.LIB_PATH):
        from voice_tts_amd import build
        build.build(verbose=False)
    return _lib.lib()


def test_max_batch_by_weight_type():
    assert _lib.max_batch() == 16  # what every weight type holds: existing callers size themselves by it
    assert _lib.max_batch_for("bf16") == 32 and _lib.max_batch_for("f16") == 32 and _lib.max_batch_for("f32") == 16
    assert [_lib.max_batch_for(code) for code in (0, 1, 2)] == [16, 32, 32]  # IXTTS_DTYPE_F32 / _BF16 / _F16
    assert _lib.max_batch_for(7) == 0
    with pytest.raises(ValueError):
        _lib.max_batch_for("f8")


class StubEngine:
    made = []

    def __init__(self, cfg=None, dtype="f32", max_seq=2048, max_batch=1, device=None):
        assert 1 <= max_batch <= _lib.max_batch_for(dtype), (dtype, max_batch)  # what ixtts_gpt_create would refuse
        self.dtype, self.max_seq, self.max_batch = dtype, max_seq, max_batch
        StubEngine.made.append((dtype, max_batch))

    def share_arena(self, owner):
        self.owner = owner
        return self


@pytest.fixture
def model_of(monkeypatch):
    from voice_tts_amd import infer_v2 as IV

    monkeypatch.setattr(IV, "GptEngine", StubEngine)
    StubEngine.made = []

    def make(dtype):
        m = object.__new__(IV.IndexTTS2)
        m.gpt_dtype, m.gpt_cfg, m.device, m._engines = dtype, {}, "cpu", {}
        m.gpt = StubEngine(dtype=dtype, max_batch=3)
        return m

    return make


@pytest.mark.parametrize("dtype,limit", [("bf16", 32), ("f16", 32), ("f32", 16)])
def test_many_engine_for_clamps_by_the_weight_type(model_of, dtype, limit):
    m = model_of(dtype)
    for slots in (5, 8, 16, 17, 24, 32, 40):
        assert m._many_engine_for(1, slots).max_batch == min(slots, limit)
    assert m._many_engine_for(1, 0).max_batch == 1
    for nb in (2, 3, 4):
        for slots in (8, 16, 31, 32, 64):
            eng = m._many_engine_for(nb, slots)
            groups = max(1, min(slots, limit) // nb)
            assert eng.max_batch == (groups * nb if groups * nb > 4 else 3), (nb, slots)  # up to 4 slots: the register engine
    assert m._many_engine_for(3, 32).max_batch == (30 if limit == 32 else 15)   # 10 groups of 3 | 5
    assert m._many_engine_for(4, 32).max_batch == limit                          # 8 groups of 4 | 4
    assert m._many_engine_for(2, 32).max_batch == limit                          # 16 groups of 2 | 8
    assert m._many_engine_for(1, 8) is m._many_engine_for(1, 8)                  # one engine per shape


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("env,groups16,groups32", [(None, 5, 5), ("10", 5, 10), ("12", 5, 10), ("1", 0, 0), ("3", 3, 3)])
def test_beam_group_engine_at_three_beams(model_of, monkeypatch, dtype, env, groups16, groups32):
    """IXTTS_BEAM_GROUPS caps the groups; the engine's limit caps them too: 10 groups of 3 on a 16-bit model, 5 on an fp32 one.
    Unset, it is 5 as ever (and an fp32 model stays on its register engine)."""
    m = model_of(dtype)
    if env is None:
        monkeypatch.delenv("IXTTS_BEAM_GROUPS", raising=False)
    else:
        monkeypatch.setenv("IXTTS_BEAM_GROUPS", env)
    want = groups16 if dtype == "f32" else groups32
    eng = m._beam_group_engine(3, 13)
    if want < 2 or (dtype == "f32" and env is None):
        assert eng is None
    else:
        assert eng.max_batch == want * 3 and eng.dtype == dtype
        assert m._beam_group_engine(3, 2) is eng  # one engine shape per worker, whatever the request's segment count
    assert m._beam_group_engine(3, 1) is None      # a single segment: the register engine
