"""CPU side of the batched latent pass: the pass rule (`ixtts_gpt_latent_plan`, pure host arithmetic) against a restatement in
Python, the hand-written cases of tests/test_gpu_latent_many.py, the error returns and the IXTTS_LATENT_BATCH switch."""
import ctypes as C
import random

import pytest

from voice_tts_amd import _lib
from voice_tts_amd.gpt_engine import GptEngine


def plan(n_prefix, n_codes, row_cap):
    """the pass rule, restated: T rows take ceil64(T) positions; a pass closes when the next entry would not fit; no codes, no room"""
    passes, cur, used = [], 0, 0
    for P, n in zip(n_prefix, n_codes):
        need = -(-(P + n) // 64) * 64 if n > 0 else 0
        if need and used > 0 and used + need > row_cap:
            cur, used = cur + 1, 0
        used += need
        passes.append(cur)
    return passes, (cur + 1 if passes else 0)


def test_plan_against_the_restated_rule_on_seeded_lists():
    rng = random.Random(2024)
    seen_passes = set()
    for _ in range(400):
        n = rng.randrange(0, 24)
        cap = rng.choice([1, 63, 64, 65, 128, 256, 640, 1024, 2048])
        P = [rng.randrange(1, 200) for _ in range(n)]
        c = [rng.choice([0, 0, 1, rng.randrange(1, 64), rng.randrange(1, 400)]) for _ in range(n)]
        got = GptEngine.latent_plan(P, c, cap)
        assert got == plan(P, c, cap), (P, c, cap)
        assert got[0] == sorted(got[0])  # nothing is re-ordered to fill a pass up
        seen_passes.add(got[1])
    assert len(seen_passes) > 5


def test_plan_rounds_every_entry_up_to_64_positions():
    assert GptEngine.latent_plan([1] * 10, [1] * 10, 640) == ([0] * 10, 1)       # T = 2 each, 64 positions each
    assert GptEngine.latent_plan([1] * 11, [1] * 11, 640) == ([0] * 10 + [1], 2)
    assert GptEngine.latent_plan([34, 34], [30, 31], 128) == ([0, 1], 2)           # 64 + 128
    assert GptEngine.latent_plan([34, 34], [30, 30], 128) == ([0, 0], 1)           # 64 + 64
    assert GptEngine.latent_plan([80] * 3, [150] * 3, 640) == ([0, 0, 1], 2)       # T = 230 -> 256 each


def test_plan_gives_an_entry_larger_than_the_cap_a_pass_of_its_own():
    assert GptEngine.latent_plan([9, 137, 9], [9, 1100, 9], 2048) == ([0, 0, 0], 1)   # 64 + 1280 + 64
    assert GptEngine.latent_plan([137, 137], [1100, 1100], 2048) == ([0, 1], 2)       # 2 x 1280 positions do not pack
    assert GptEngine.latent_plan([100], [101], 10) == ([0], 1)
    assert GptEngine.latent_plan([100, 5, 100], [101, 5, 101], 10) == ([0, 1, 2], 3)


def test_plan_entries_without_codes_occupy_nothing():
    assert GptEngine.latent_plan([50, 600, 50], [14, 0, 14], 128) == ([0, 0, 0], 1)
    assert GptEngine.latent_plan([600, 50, 600, 50, 600], [0, 14, 0, 15, 0], 64) == ([0, 0, 0, 1, 1], 2)
    assert GptEngine.latent_plan([3, 3], [0, 0], 64) == ([0, 0], 1)
    assert GptEngine.latent_plan([], [], 64) == ([], 0)


def test_plan_of_the_gpu_tests_edge_cases():
    """tests/test_gpu_latent_many.py, EDGES at max_seq 640 and at rows_max 256"""
    edges = [(1, 1), (20, 11), (40, 23), (34, 30), (1, 64), (100, 28), (128, 1), (51, 150)]
    assert [P + n for P, n in edges] == [2, 31, 63, 64, 65, 128, 129, 201]
    P, c = [p for p, _ in edges], [n for _, n in edges]
    assert GptEngine.latent_plan(P, c, 640) == ([0] * 6 + [1] * 2, 2)      # 64 64 64 64 128 128 = 512; 192 more would make 704
    assert GptEngine.latent_plan(P, c, 256) == ([0, 0, 0, 0, 1, 1, 2, 3], 4)
    order = [5, 0, 1, 2, 3, 4, 6, 7]
    assert GptEngine.latent_plan([P[i] for i in order], [c[i] for i in order], 640) == ([0] * 6 + [1] * 2, 2)


def test_plan_error_returns():
    L = _lib.lib()
    ints = lambda *v: (C.c_int * len(v))(*v)
    out = ints(0, 0)
    assert L.ixtts_gpt_latent_plan(ints(5, 5), ints(5, 5), 2, 0, out) < 0
    assert L.ixtts_gpt_latent_plan(None, ints(5, 5), 2, 64, out) < 0
    assert L.ixtts_gpt_latent_plan(ints(5, 5), None, 2, 64, out) < 0
    assert L.ixtts_gpt_latent_plan(ints(5, 5), ints(5, 5), 2, 64, None) < 0
    assert L.ixtts_gpt_latent_plan(ints(5, 5), ints(5, 5), -1, 64, out) < 0
    assert L.ixtts_gpt_latent_plan(None, None, 0, 64, None) == 0
    with pytest.raises(_lib.IxttsError, match="gpt_latent_plan"):
        GptEngine.latent_plan([5], [5], 0)
    # all of them return the one code of a bad argument
    assert len({L.ixtts_gpt_latent_plan(ints(5, 5), ints(5, 5), 2, 0, out), L.ixtts_gpt_latent_plan(None, ints(5, 5), 2, 64, out),
                L.ixtts_gpt_prefill_plan(None, ints(5, 5), 2, 64, out)}) == 1


def test_switch_resolution(monkeypatch):
    from voice_tts_amd import scheduler as infer_v2

    monkeypatch.delenv("IXTTS_LATENT_BATCH", raising=False)
    assert infer_v2.resolve_latent_batch() is infer_v2.LATENT_BATCH_DEFAULT
    for env, want in (("1", True), ("0", False)):
        monkeypatch.setenv("IXTTS_LATENT_BATCH", env)
        assert infer_v2.resolve_latent_batch() is want
        assert infer_v2.resolve_latent_batch(not want) is (not want)  # the argument wins over the variable
    for bad in ("yes", "2", "on"):
        monkeypatch.setenv("IXTTS_LATENT_BATCH", bad)
        with pytest.raises(ValueError, match="IXTTS_LATENT_BATCH"):
            infer_v2.resolve_latent_batch()
