"""GPU: the slots of the Qwen3 decode engine (csrc/qwen_engine.hip) -- up to 4 sequences per decode step, and the rows
prefill of f16 engines on the f16 matrix cores.

f32 engines: a slot's logits, kept set and ids are bit for bit those of the one-sequence engine given that prompt alone.
f16 engines: the rows prefill against the one-sequence engine (chunk prefill, same weights, fp32 activations) within
1e-4 x max|logit| ("same arithmetic, another accumulation order") and against transformers with fp16-rounded weights on
the CPU within 2e-3 x max|logit|.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import qwen_twin as T  # noqa: E402
from test_gpu_qwen import engine_cfg, hf_greedy, rounded_f16  # noqa: E402

torch.set_grad_enabled(False)

BM = 64  # row tile of qrows_gemm_kernel (RBM)


def make_engine(m, dtype, eos, max_seq, slots):
    from voice_tts_amd.qwen_emotion import QwenEngine

    cfg = engine_cfg(m)
    sd = {k: v for k, v in m.state_dict().items() if k != "lm_head.weight" or not cfg["tie_word_embeddings"]}
    return QwenEngine(cfg, dtype=dtype, max_seq=max_seq, device="cuda:0", eos_token_id=eos, slots=slots).load_state_dict(sd)


def prompts_of(lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 500, (n,), generator=g).tolist() for n in lens]


# ---------------------------------------------------------------------------------------------------- f32: exact slots
SEQ = 64     # KV positions: every slot is finished (EOS or a full cache) after 64 steps
STEPS = 68   # so the last steps find every slot finished


def single_trace(e, prompt, n, **kw):
    """The one-sequence calls, a step at a time: logits [n][V], (ids, finished) after each step."""
    e.prefill(prompt)
    logits, reads = [], []
    for _ in range(n):
        e.step(1, **kw)
        logits.append(e.read_logits())
        reads.append(e.read())
    return np.stack(logits), reads


@pytest.fixture(scope="module")
def f32():
    m = T.make_model(T.twin_config(layers=3), seed=3, std=0.25)
    prompts = prompts_of([1, 5, 37, 42], seed=21)  # 1 id: no prefill; 42 ids: 10 chunks + 1
    free = hf_greedy(m, prompts[1], 48)
    # EOS = a token the 5-id sequence first draws at step >= 30: that slot stops there while others go on
    k = next(i for i in range(30, 48) if free[i] not in free[:i])
    eos = free[k]
    one = make_engine(m, "f32", [eos], SEQ, 1)
    ref = [single_trace(one, p, STEPS) for p in prompts]
    assert ref[1][1][-1][1] == 1 and ref[1][1][-1][0][-1] == eos  # the EOS stop
    assert all(r[1][-1][1] in (1, 2) for r in ref) and any(r[1][-1][1] == 2 for r in ref)
    four = make_engine(m, "f32", [eos], SEQ, 4)
    return dict(m=m, prompts=prompts, eos=eos, one=one, four=four, ref=ref)


def check_trace(e, order, ref, n):
    """prefill_many + n single steps of all slots: every slot, after every step, is the one-sequence engine's."""
    for step in range(n):
        e.step_many(1)
        for s, pi in enumerate(order):
            assert np.array_equal(e.read_logits_slot(s), ref[pi][0][step]), (step, s)
            assert e.read_slot(s) == ref[pi][1][step], (step, s)


def test_slots_are_independent_and_exact(f32):
    e, ref, prompts = f32["four"], f32["ref"], f32["prompts"]
    e.prefill_many(prompts)
    check_trace(e, [0, 1, 2, 3], ref, STEPS)
    assert all(e.read_slot(s)[1] != 0 for s in range(4))
    # every slot is finished: more steps change nothing
    e.step_many(5)
    for s in range(4):
        assert e.read_slot(s) == ref[s][1][-1]
    # the same prompts in another order, through generate_many
    order = [2, 0, 3, 1]
    outs = e.generate_many([prompts[i] for i in order], STEPS)
    for s, pi in enumerate(order):
        # (as `generate`, it steps no further than the room of the shortest prompt: SEQ - 1 steps)
        assert outs[s] == ref[pi][1][-1][0][: SEQ - len(prompts[pi])] and e.read_slot(s) == ref[pi][1][SEQ - 2]
    # only two of them (2 columns wide), and three (a 4-wide step with an idle column)
    for order in ([3, 1], [1, 3, 0]):
        idle = {s: (e.read_logits_slot(s), e.read_slot(s), e.read_kept_slot(s)) for s in range(len(order), 4)}
        e.prefill_many([prompts[i] for i in order])
        check_trace(e, order, ref, 40)
        # the slots the batch did not name are left as they were, logits included
        for s, (lg, rd, kept) in idle.items():
            assert np.array_equal(e.read_logits_slot(s), lg) and e.read_slot(s) == rd
            assert all(np.array_equal(a, b) for a, b in zip(e.read_kept_slot(s), kept))


def test_sampling_per_slot(f32):
    e, one, prompts = f32["four"], f32["one"], f32["prompts"]
    kw = dict(do_sample=True, temperature=0.6, top_k=20, top_p=0.95, seed=123)
    want = [one.generate(p, 24, **kw) for p in prompts]
    assert e.generate_many(prompts, 24, **kw) == want
    assert len({tuple(w) for w in want}) == 4
    assert e.generate_many(prompts, 24, **dict(kw, seed=124)) != want
    # the kept set of the first sampled step
    e.prefill_many(prompts)
    e.step_many(1, **kw)
    for s, p in enumerate(prompts):
        one.prefill(p)
        one.step(1, **kw)
        ids, pr = one.read_kept()
        got_ids, got_pr = e.read_kept_slot(s)
        assert np.array_equal(got_ids, ids) and np.array_equal(got_pr, pr) and 1 <= len(ids) <= 20
        assert e.read_slot(s) == one.read()


def test_the_one_sequence_calls_are_slot_0(f32):
    e, ref, prompts = f32["four"], f32["ref"], f32["prompts"]

    def check():
        for pi in (2, 3):
            logits, reads = single_trace(e, prompts[pi], 12)
            assert np.array_equal(logits, ref[pi][0][:12]) and reads == ref[pi][1][:12]
            assert np.array_equal(e.read_logits_slot(0), logits[-1])
            assert e.generate(prompts[pi], STEPS) == ref[pi][1][-1][0][: SEQ - len(prompts[pi])]

    fresh = make_engine(f32["m"], "f32", [f32["eos"]], SEQ, 4)  # no batched call yet: slots 1.. have no cache
    for pi in (2, 3):
        logits, reads = single_trace(fresh, prompts[pi], 12)
        assert np.array_equal(logits, ref[pi][0][:12]) and reads == ref[pi][1][:12]
    e.generate_many(prompts, 20)
    check()
    # slots 1..3 still hold what the batched call left there
    for s in (1, 2, 3):
        assert e.read_slot(s) == ref[s][1][19]


def test_slot_limits_are_refused(f32):
    from voice_tts_amd import _lib

    e, one, prompts = f32["four"], f32["one"], f32["prompts"]
    with pytest.raises(ValueError, match="slots"):
        one.prefill_many(prompts[:2])
    with pytest.raises(ValueError, match="slots"):
        make_engine(f32["m"], "f32", [0], SEQ, 5)
    with pytest.raises(_lib.IxttsError, match="slot"):
        one.read_slot(1)
    fresh = make_engine(f32["m"], "f32", [0], SEQ, 2)
    with pytest.raises(_lib.IxttsError, match="no prompt"):
        fresh.step_many(1, n=2)


# ---------------------------------------------------------------------------------------------------- f16: rows prefill
PACKS = {  # prompt lengths; rows = sum(len - 1)
    "rows_1": [2, 1],
    "rows_BM-1": [1, 40, 25],
    "rows_BM": [30, 1, 36],
    "rows_BM+1": [1, 50, 12, 6],
    "rows_2BM+3": [70, 1, 42, 22],
}
assert [sum(n - 1 for n in v) for v in PACKS.values()] == [1, BM - 1, BM, BM + 1, 2 * BM + 3]


@pytest.fixture(scope="module")
def f16():
    m = T.make_model(T.twin_config(layers=3), seed=3, std=0.25)
    return dict(m=m, r=rounded_f16(m), one=make_engine(m, "f16", [511], 128, 1), four=make_engine(m, "f16", [511], 128, 4))


def check_rows_pack(f16, e, lens, seed):
    r, one = f16["r"], f16["one"]
    prompts = prompts_of(lens, seed)
    e.prefill_many(prompts)
    e.step_many(1)
    first = [e.read_logits_slot(s) for s in range(len(prompts))]
    steps = 32
    rest = [[] for _ in prompts]
    for _ in range(steps - 1):
        e.step_many(1)
        for s in range(len(prompts)):
            rest[s].append(e.read_logits_slot(s))
    for s, p in enumerate(prompts):
        ref = hf_greedy(r, p, steps, eos=None)
        full = r(torch.tensor([p + ref])).logits[0, len(p) - 1: len(p) - 1 + steps].numpy()
        scale = np.abs(full[0]).max()
        one.prefill(p)
        one.step(1)
        chunk = one.read_logits()
        err_hf, err_one = np.abs(first[s] - full[0]).max(), np.abs(first[s] - chunk).max()
        print(f"lens {lens} slot {s}: vs rounded model {err_hf / scale:.3g}, vs chunk-prefilled engine {err_one / scale:.3g} (x max|logit|)")
        assert err_hf < 2e-3 * scale, (s, err_hf, scale)
        assert err_one < 1e-4 * scale, (s, err_one, scale)
        got = e.read_slot(s)[0]
        lg = [first[s]] + rest[s]
        i = next((i for i, (a, b) in enumerate(zip(got, ref)) if a != b), None)
        if i is None:  # (the engine stops at its EOS id, the oracle run has none)
            assert got == ref[: len(got)] and (len(got) == steps or got[-1] == 511)
        else:
            top2 = np.sort(full[i])[-2:]
            err = np.abs(lg[i] - full[i]).max()
            print(f"slot {s}: ids agree for {i} steps; step {i} margin {top2[1] - top2[0]:.3g}, logit error {err:.3g}")
            assert top2[1] - top2[0] < 2 * err


@pytest.mark.parametrize("name", list(PACKS))
def test_rows_prefill_tile_edges(f16, name):
    check_rows_pack(f16, f16["four"], PACKS[name], seed=31 + len(name))


def test_rows_prefill_in_several_passes(f16, monkeypatch):
    monkeypatch.setenv("IXTTS_QWEN_ROWS_MAX", "48")  # read when the engine is created: 131 rows = 48 + 48 + 35
    e = make_engine(f16["m"], "f16", [511], 128, 4)
    monkeypatch.delenv("IXTTS_QWEN_ROWS_MAX")
    check_rows_pack(f16, e, PACKS["rows_2BM+3"], seed=77)


def test_rows_prefill_production_width():
    """28 layers x 1024, vocabulary 151 936: the real N and K of every GEMM (K = 3072, the 6144-row gate|up)."""
    cfg = T.twin_config(layers=T.PROD["num_hidden_layers"], vocab_size=T.PROD["vocab_size"], hidden_size=T.PROD["hidden_size"],
                        intermediate_size=T.PROD["intermediate_size"], heads=T.PROD["num_attention_heads"], kv_heads=T.PROD["num_key_value_heads"])
    m = T.make_model(cfg, seed=11, std=0.02)
    g = torch.Generator().manual_seed(13)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).tolist() for n in (128, 131, 9)]
    e = make_engine(m, "f16", [0], 256, 3)
    e.prefill_many(prompts)
    e.step_many(1)
    r = rounded_f16(m)
    del m
    for s, p in enumerate(prompts):
        want = r(torch.tensor([p]), logits_to_keep=1).logits[0, -1].numpy()
        err, scale = np.abs(e.read_logits_slot(s) - want).max(), np.abs(want).max()
        print(f"production width, slot {s} ({len(p)} ids): {err / scale:.3g} x max|logit|")
        assert err < 2e-3 * scale, (s, err, scale)
