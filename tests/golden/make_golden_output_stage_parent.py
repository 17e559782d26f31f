"""Recorded results of the output stage for tests/test_gpu_output_stage_parent.py: run ONCE, on a GPU, at the commit whose bytes and
reports the stage has to keep (the parent of the change that gave the stage one request spec, `output.OutputSpec`, and one entry,
`output.finish`), through that parent's `finish_pcm_many` alone, never regenerated from the code under test:

    python tests/golden/make_golden_output_stage_parent.py [path]     # -> tests/golden/output_stage_parent.npz

No model is involved.  A request's segments are fp32 rows of integer values, `np.random.default_rng(seed).integers(-20000, 20001)` --
exact on every machine -- with a few samples forced to +-32767, so that ceilings bind and the limiter engages; the file stores the
sha256 of all of them (`inputs_sha256`), which catches a generator that drifts.

Segment lengths: 1, 3, 4, 5, 255; 2205 and 4411, which at 8 kHz deliver less than the four hops of one gating block (the report says
`measured_lufs is None`); 13 000, where a block exists at every rate and the programme delivered at 48 kHz is longer than one tile of
the limiter.  `REQUESTS` crosses the rates 8000 / 22 050 / 48 000 and the three encodings with the controls: none; a loudness target;
a ceiling alone; a target in true-peak mode; the limiter alone; target, limiter and true mode; the same with a `total` longer than
the programme; and one request without segments.  `cases()`: all of them in one call ("mix"), and each one alone ("solo<j>").

Per result the file holds the rate, the dtype and the length, the sha256 of the bytes, the first 512 bytes, and the report as JSON
(its floats are Python floats, whose repr round-trips every bit; None and the infinities are JSON's)."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "output_stage_parent.npz")
HEAD = 512
INTERVAL = 200

# (seed, segment lengths, sample_rate, encoding, loudness, peak, peak_mode, limiter, total)
REQUESTS = [
    (11, [1, 3, 4], 22050, "pcm_s16le", None, None, None, None, None),  # nothing asked of the level
    (12, [5, 255], 8000, "mulaw", -23.0, None, None, None, None),  # a target; no block to measure
    (13, [13000], 48000, "pcm_s16le", -5.0, None, "true", True, None),  # the full chain, more than one tile of the limiter
    (14, [13000, 255], 8000, "mulaw", None, -6.0, None, None, None),  # a ceiling alone
    (15, [13000, 5], 22050, "alaw", -5.0, None, "true", None, None),  # a target the true-peak ceiling binds
    (16, [4411], 22050, "alaw", None, None, None, True, None),  # the limiter alone; no block to measure
    (17, [13000, 3, 1], 48000, "mulaw", -8.0, -3.0, "true", True, 50000),  # the full chain and a tail of silence
    (18, [], 22050, "pcm_s16le", -23.0, None, None, None, None),  # no segments
    (19, [2205], 8000, "pcm_s16le", -23.0, None, None, None, None),  # no block at 8 kHz
    (20, [255, 4], 48000, "alaw", None, None, None, None, None),  # nothing asked, a rate and an encoding
    (21, [13000], 22050, "mulaw", -23.0, None, None, None, None),  # a target at the model's rate
    (22, [4411, 2205], None, None, None, None, "sample", False, 12000),  # nothing but a total
    (23, [13000], 8000, "alaw", -8.0, None, None, True, None),  # a target and the limiter in sample mode, the shortest look-around
]


def segments(seed, lens):
    """fp32 [1, n] numpy rows of integer values; from 4 samples up one sample at +32767 and one at -32767."""
    rng = np.random.default_rng(seed)
    out = []
    for n in lens:
        x = rng.integers(-20000, 20001, size=n).astype(np.float32)
        if n >= 4:
            x[n // 3], x[2 * n // 3] = 32767.0, -32767.0
        out.append(x.reshape(1, -1))
    return out


def inputs_sha256():
    h = hashlib.sha256()
    for seed, lens, *_ in REQUESTS:
        for x in segments(seed, lens):
            h.update(x.astype("<f4").tobytes())
    return h.hexdigest()


def cases():
    """[(id, [index into REQUESTS])]"""
    return [("mix", list(range(len(REQUESTS))))] + [(f"solo{j}", [j]) for j in range(len(REQUESTS))]


def run_many(O, reqs, device):
    """The call of the parent: the list form, every list given."""
    wavs = [[torch.from_numpy(x).to(device) for x in segments(r[0], r[1])] for r in reqs]
    reports = []
    col = lambda k: [r[k] for r in reqs]  # noqa: E731
    results = O.finish_pcm_many(wavs, col(2), col(3), INTERVAL, col(4), col(5), reports, col(8), col(6), col(7))
    return results, reports


def run_finish(O, reqs, device):
    """The same requests as specs through `output.finish` (the change under test has it; the parent does not)."""
    wavs = [[torch.from_numpy(x).to(device) for x in segments(r[0], r[1])] for r in reqs]
    specs = [O.OutputSpec.of(r[2], r[3], r[4], r[5], r[6], r[7], duration=r[8] is not None)._replace(total=r[8]) for r in reqs]
    return O.finish(wavs, specs, INTERVAL)


def record(cid, results, reports):
    """-> {key: array} as the file stores one case."""
    rec = {f"{cid}/n": np.array(len(results), dtype=np.int64)}
    assert len(reports) == len(results)
    for j, (res, rep) in enumerate(zip(results, reports)):
        key = f"{cid}/r{j}"
        rec[key + "/report"] = np.array(json.dumps(rep, sort_keys=True))
        if res is None:
            rec[key + "/result"] = np.array("None")
            continue
        sr, pcm = res
        assert pcm.ndim == 2 and pcm.shape[1] == 1
        raw = np.ascontiguousarray(pcm).tobytes()
        rec[key + "/rate"] = np.array(sr, dtype=np.int64)
        rec[key + "/dtype"] = np.array(pcm.dtype.str)
        rec[key + "/len"] = np.array(pcm.shape[0], dtype=np.int64)
        rec[key + "/sha256"] = np.array(hashlib.sha256(raw).hexdigest())
        rec[key + "/head"] = np.frombuffer(raw[:HEAD], dtype=np.uint8).copy()
    return rec


def record_all(O, run, device):
    rec = {"inputs_sha256": np.array(inputs_sha256())}
    for cid, idx in cases():
        rec.update(record(cid, *run(O, [REQUESTS[j] for j in idx], device)))
    return rec


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from voice_tts_amd import _lib
    from voice_tts_amd import output as O

    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    device = torch.device("cuda:0")
    assert O.resampled_len(13000, O.MODEL_RATE, 48000) > _lib.lib().ixtts_limiter_tile()
    rec = record_all(O, run_many, device)
    np.savez_compressed(path, **rec)
    again = record_all(O, run_many, device)
    assert sorted(rec) == sorted(again) and all(np.array_equal(rec[k], again[k]) for k in rec), "two recordings differ"
    reports = [json.loads(str(rec[f"mix/r{j}/report"])) for j in range(len(REQUESTS))]
    for r, rep in zip(REQUESTS, reports):
        print(r[1:], rep, flush=True)
    assert reports[1]["measured_lufs"] is None and reports[5]["measured_lufs"] is None and reports[8]["measured_lufs"] is None
    assert reports[2]["limited"] and reports[5]["limited"] and reports[6]["limited"] and reports[12]["limited"] and not reports[4]["target_met"]
    assert reports[4]["measured_lufs"] is not None
    assert reports[0] is reports[7] is reports[9] is reports[11] is None
    for j in range(len(REQUESTS)):  # a request's bytes depend on itself alone
        assert all(np.array_equal(rec[k], rec[k.replace(f"mix/r{j}/", f"solo{j}/r0/")]) for k in rec if k.startswith(f"mix/r{j}/"))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
