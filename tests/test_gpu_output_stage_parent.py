"""The output stage has one request spec (`output.OutputSpec`), one entry (`output.finish`), one table layout in `LevelPlan` and one
assemble kernel body.  Nothing a caller can observe moved with that: every case here must reproduce, byte for byte and report for
report, what the stage gave before, as recorded at the parent commit through its `finish_pcm_many` by
tests/golden/make_golden_output_stage_parent.py into tests/golden/output_stage_parent.npz -- per result the rate, the dtype, the
length, the sha256 of the bytes and the first 512 of them, and the level report with every float exact.  Exact equality, no tolerance,
through the list form `finish_pcm_many` and through `finish` with the equivalent specs.

Cases (make_golden_output_stage_parent.REQUESTS): 8000 / 22 050 / 48 000 Hz and the three encodings against no control, a loudness
target, a ceiling alone, a target in true-peak mode, the limiter alone, target with limiter (sample and true mode), the same with a
`total` longer than the programme, a `total` alone, a request without segments; programmes shorter than one gating block (no
measurement) and longer than one tile of the limiter; all in one call, and each alone.  Two recordings taken at the parent, in two
processes, agreed in every key."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_output_stage_parent", os.path.join(HERE, "golden", "make_golden_output_stage_parent.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)


@pytest.fixture(scope="module")
def recorded():
    with np.load(MG.PATH) as z:
        return {k: z[k] for k in z.files}


def test_the_inputs_are_the_recorded_ones(recorded):
    assert os.path.getsize(MG.PATH) <= 512 * 1024
    assert str(recorded["inputs_sha256"]) == MG.inputs_sha256()
    assert sorted({k.split("/")[0] for k in recorded} - {"inputs_sha256"}) == sorted(c[0] for c in MG.cases())


@pytest.mark.parametrize("run", [MG.run_many, MG.run_finish], ids=["finish_pcm_many", "finish"])
def test_identical_to_parent(recorded, run):
    from voice_tts_amd import _lib
    from voice_tts_amd import output as O

    assert O.resampled_len(13000, O.MODEL_RATE, 48000) > _lib.lib().ixtts_limiter_tile()
    got = MG.record_all(O, run, torch.device("cuda:0"))
    assert sorted(got) == sorted(recorded)
    for k in sorted(recorded):
        if k.endswith("/report"):
            print(k, str(got[k]))
            assert json.loads(str(got[k])) == json.loads(str(recorded[k])), k  # (parsed: float for float, None for None)
        assert got[k].dtype == recorded[k].dtype and got[k].shape == recorded[k].shape and np.array_equal(got[k], recorded[k]), k
