"""Which GPT weight type a model gets: `resolve_gpt_dtype(use_fp16, gpt_dtype, env)` -- keyword, then IXTTS_GPT_DTYPE, then the
default, which must stay what it was before the fp16 type existed (bf16 under use_fp16, f32 otherwise).  No GPU involved."""
import itertools

import pytest

from voice_tts_amd.gpt_engine import GPT_DTYPES, resolve_gpt_dtype

NAMES = ("f32", "bf16", "f16")


def test_defaults_did_not_move():
    assert resolve_gpt_dtype(True, None, {}) == "bf16"
    assert resolve_gpt_dtype(False, None, {}) == "f32"
    assert resolve_gpt_dtype(True, None, {"IXTTS_GPT_DTYPE": ""}) == "bf16"  # set but empty counts as unset
    assert set(GPT_DTYPES) == set(NAMES) and GPT_DTYPES["f32"] == 0 and GPT_DTYPES["bf16"] == 1 and GPT_DTYPES["f16"] == 2


@pytest.mark.parametrize("use_fp16,kw,env", list(itertools.product((False, True), (None,) + NAMES + ("f8",), (None,) + NAMES + ("half",))))
def test_every_combination(use_fp16, kw, env):
    environ = {} if env is None else {"IXTTS_GPT_DTYPE": env}
    if kw is not None:  # an explicit keyword wins; the variable is not even looked at
        if kw in NAMES:
            assert resolve_gpt_dtype(use_fp16, kw, environ) == kw
        else:
            with pytest.raises(ValueError) as ei:
                resolve_gpt_dtype(use_fp16, kw, environ)
            assert all(n in str(ei.value) for n in NAMES)
    elif env is not None:
        if env in NAMES:
            assert resolve_gpt_dtype(use_fp16, None, environ) == env
        else:
            with pytest.raises(ValueError) as ei:
                resolve_gpt_dtype(use_fp16, None, environ)
            assert all(n in str(ei.value) for n in NAMES)
    else:
        assert resolve_gpt_dtype(use_fp16, None, environ) == ("bf16" if use_fp16 else "f32")


def test_reads_the_process_environment_when_no_mapping_is_given(monkeypatch):
    monkeypatch.delenv("IXTTS_GPT_DTYPE", raising=False)
    assert resolve_gpt_dtype(True) == "bf16"
    monkeypatch.setenv("IXTTS_GPT_DTYPE", "F16 ")  # case and surrounding blanks are forgiven
    assert resolve_gpt_dtype(True) == "f16" and resolve_gpt_dtype(False) == "f16"
    assert resolve_gpt_dtype(True, "bf16") == "bf16"
    monkeypatch.setenv("IXTTS_GPT_DTYPE", "fp16")
    with pytest.raises(ValueError):
        resolve_gpt_dtype(True)
