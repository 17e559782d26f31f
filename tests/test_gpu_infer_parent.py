"""`infer`, `infer(stream_return=True)` and `infer_many` share one implementation of every step of a request (generation arguments,
emotion resolution, prompt caches, conditioning, segments, scheduler run, code trimming, latent pass, s2mel, vocoder).  Nothing a
caller can observe moved with that: every case here must reproduce what the two separate bodies gave before, as recorded at the parent
commit by tests/golden/make_golden_infer_parent.py into tests/golden/infer_parent.npz -- each segment's mel codes, the PCM length and
the sha256 of the int16 PCM bytes (for the generator the chunk lengths and the sha256 of the concatenation; for a failed request the
exception's type name).  Exact equality, no tolerance.

Cases (make_golden_infer_parent.cases): F1..F7 on the fake-glue model in fp32 (DecodeScheduler greedy and sampling, gpt.generate
greedy and beams with a scaled emotion vector, the streaming path, infer_many greedy on 4 slots and with beams on the register
engine), F8/F9 on the same model in bf16 (beam groups stepping together; infer_many on 9 slots with one request whose speaker prompt
cannot be encoded), M1..M4 on the model-directory model with the built-in conditioning, s2mel and tokenizer (separate emotion prompt,
the same under IXTTS_S2MEL_BATCH=1, no emotion prompt, infer_many).  Two recordings taken at the parent agreed in every case."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_infer_parent", os.path.join(HERE, "golden", "make_golden_infer_parent.py"))
MG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MG)

CASES = MG.cases()


@pytest.fixture(scope="module")
def recorded():
    with np.load(MG.PATH) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return MG.Models(root=str(tmp_path_factory.mktemp("infer_parent_model_dir")))


def test_every_case_is_recorded(recorded):
    assert sorted({k.split("/")[0] for k in recorded}) == sorted(c[0] for c in CASES)
    assert os.path.getsize(MG.PATH) <= 512 * 1024


@pytest.mark.parametrize("cid,model,kind,call", CASES, ids=[c[0] for c in CASES])
def test_identical_to_parent(recorded, models, cid, model, kind, call):
    got = MG.run_case(cid, kind, call, models(model))
    want = {k: v for k, v in recorded.items() if k.split("/")[0] == cid}
    for k in sorted(got):
        if got[k].ndim == 0:
            print(k, got[k].tolist(), "recorded", want[k].tolist() if k in want else None)
    assert sorted(got) == sorted(want)
    for k in sorted(want, key=lambda k: ("/codes/" not in k and not k.endswith("n_segments"), k)):  # the codes first: they tell most
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        if got[k].dtype.kind in "iu" and got[k].ndim:
            diff = np.abs(got[k].astype(np.int64) - want[k])
            assert not diff.any(), f"{k}: {int((diff != 0).sum())} of {diff.size} differ from the recording, by at most {int(diff.max())}"
        assert np.array_equal(got[k], want[k]), k
