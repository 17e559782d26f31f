"""`GptEngine.prefill_many`: N sequences into N arbitrary slots in one packed causal pass per layer (csrc/gpt_rows.hip, packed forms
of the QKV epilogue and of the two row-attention kernels).  The contract is bit for bit, so every comparison is `==` on ids and
`array_equal` on logits against the SERIAL TWIN: the same engine, the same slots, filled by `prefill` one by one and given the
same decode call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY = dict(repetition_penalty=10.0, suppress_stop=True)
N_STEPS = 24
MAX_SEQ = 640
ENGINES = [("f32", 16), ("bf16", 32), ("f16", 32)]

# (n_rows, n_left_pad): T = n_rows + 1 - n_left_pad packed rows
EDGES = [(1, 0),      # T 2: the smallest sequence; everything after it starts off-tile
         (63, 0),     # T 64: one row short of a 65-row sequence
         (64, 0),     # T 65: crosses a 64-row GEMM tile
         (127, 0),    # T 128: exactly one attention tile
         (128, 0),    # T 129: the second attention tile holds one row
         (200, 0),    # T 201: two attention tiles
         (40, 3),     # T 38: pad inside the first key tile
         (100, 70),   # T 31: key tiles start at 64
         (130, 64),   # T 67: valid_from exactly on a key tile
         (9, 8)]      # T 2: the smallest sequence with padding
EDGE_SLOTS = [7, 2, 11, 0, 5, 9, 1, 14, 3, 12]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tiny(seed=7):
    import voice_tts_amd.weights as WR

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    return cfg, WR.make_gpt_weights(cfg, seed=seed, head_scale=50.0)


def _prompt(rows, pad, D, g, dev):
    e = torch.randn(rows, D, generator=g) * 0.5
    e[:pad] = 0
    return e.to(dev)


def _edge_entries(dev, order=None, D=128):
    g = torch.Generator().manual_seed(123)
    ent = [(slot, _prompt(rows, pad, D, g, dev), pad) for slot, (rows, pad) in zip(EDGE_SLOTS, EDGES)]
    return [ent[i] for i in order] if order is not None else ent


@pytest.fixture(scope="module", params=ENGINES, ids=[e[0] for e in ENGINES])
def eng(request, dev):
    from voice_tts_amd.gpt_engine import GptEngine

    dt, mb = request.param
    cfg, W = _tiny()
    return dt, mb, GptEngine(cfg, dtype=dt, max_seq=MAX_SEQ, max_batch=mb, device=dev).load_state_dict(W)


def _fill(e, entries, batched, **kw):
    if batched:
        e.prefill_many(entries, **kw)
    else:
        for slot, emb, pad in entries:
            e.prefill(slot, emb, pad)


def _run(e, entries, batched, n_active, **kw):
    """fill, read the first-step logits of the filled slots, N_STEPS greedy steps of slots 0..n_active-1, ids and final logits"""
    _fill(e, entries, batched, **kw)
    slots = [s for s, _, _ in entries]
    firsts = {s: e.read_logits(s).copy() for s in slots}
    e.decode(n_active, N_STEPS, **GREEDY)
    return firsts, {s: e.read(s)[0][:N_STEPS].tolist() for s in slots}, {s: e.read_logits(s).copy() for s in slots}


def _same(got, want):
    for part_g, part_w in zip(got, want):
        assert part_g.keys() == part_w.keys()
        for s in part_w:
            if isinstance(part_w[s], list):
                assert part_g[s] == part_w[s], s
            else:
                assert np.array_equal(part_g[s], part_w[s]), s


def _prime(e, n, dev, D=128):
    """every slot below n holds a sequence (the engine needs a prompt in every active slot); both twins start from this"""
    g = torch.Generator().manual_seed(5)
    for b in range(n):
        e.prefill(b, _prompt(6 + b, 0, D, g, dev), 0)


# ------------------------------------------------------------------------------------------------------- 1. edges of every tile
@pytest.fixture(scope="module")
def edge_twin(eng, dev):
    """the serial twin of the edges case: computed once per engine, never changed"""
    dt, mb, e = eng
    _prime(e, 15, dev)
    return _run(e, _edge_entries(dev), False, 15)


@pytest.mark.parametrize("case", ["as_given", "t128_first", "rows_max_256"])
def test_edges_of_every_tile(eng, edge_twin, dev, case):
    dt, mb, e = eng
    order = [3, 0, 1, 2, 4, 5, 6, 7, 8, 9] if case == "t128_first" else None  # T = 128 first: the next sequence begins at packed row 128
    kw = dict(rows_max=256) if case == "rows_max_256" else {}
    _prime(e, 15, dev)
    got = _run(e, _edge_entries(dev, order), True, 15, **kw)
    _same(got, edge_twin)
    assert len({tuple(v) for v in got[1].values()}) > 5  # (the sequences do differ)


# ------------------------------------------------------------------------------------------- 1b. the other engine classes
@pytest.mark.parametrize("dt,mb", [("f32", 3), ("bf16", 3), ("f16", 4), ("bf16", 8), ("f32", 8)])
def test_register_and_small_wide_engines(dev, dt, mb):
    """max_batch <= 4: the register GEMVs run the head and the decode steps; 5..16: the one-block wide kernels.  The rows pass is the
    same code on all of them; the per-slot head launch after it is not."""
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny()
    e = GptEngine(cfg, dtype=dt, max_seq=MAX_SEQ, max_batch=mb, device=dev).load_state_dict(W)
    g = torch.Generator().manual_seed(77)
    shapes = [(130, 64), (64, 0), (9, 8)]  # T 67 (two GEMM tiles, valid_from on a key tile), 65, 2
    entries = [(slot, _prompt(rows, pad, 128, g, dev), pad) for slot, (rows, pad) in zip([2, 0, 1], shapes)]
    want = _run(e, entries, False, 3)
    _same(_run(e, entries, True, 3), want)
    _same(_run(e, list(reversed(entries)), True, 3, rows_max=70), want)  # three passes
    assert len({tuple(v) for v in want[1].values()}) == 3


# ----------------------------------------------------------------------------------------------------------- 2. fp32 tile switch
def test_fp32_packed_pass_on_the_128_row_tile(dev):
    """8 x 70 = 560 packed rows: the fp32 launcher takes 128-row tiles where each solo pass (70 rows) took 64-row ones"""
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny()
    e = GptEngine(cfg, dtype="f32", max_seq=MAX_SEQ, max_batch=16, device=dev).load_state_dict(W)
    g = torch.Generator().manual_seed(9)
    entries = [(b, _prompt(69, 0, 128, g, dev), 0) for b in range(8)]
    want = _run(e, entries, False, 8)
    got = _run(e, entries, True, 8)
    _same(got, want)


# ------------------------------------------------------------------------------------------------------------------ 3. live slots
def test_live_slots_are_not_touched(eng, dev):
    dt, mb, e = eng
    g = torch.Generator().manual_seed(17)
    first = [(b, _prompt(10 + 5 * b, b % 3, 128, g, dev), b % 3) for b in range(8)]
    refill = [(5, _prompt(33, 2, 128, g, dev), 2), (2, _prompt(70, 0, 128, g, dev), 0)]

    def run(batched):
        _fill(e, first, False)
        e.decode(8, 10, **GREEDY)
        before = [e.read_logits(b).copy() for b in (3, 6)]
        _fill(e, refill, batched)
        after = [e.read_logits(b).copy() for b in (3, 6)]
        e.decode(8, 10, **GREEDY)
        return before, after, [e.read(b)[0][:20].tolist() for b in range(8)], [e.read_logits(b).copy() for b in range(8)]

    before, after, ids_w, logits_w = run(False)
    before_b, after_b, ids, logits = run(True)
    for x, y in zip(before_b, after_b):
        assert np.array_equal(x, y)
    assert ids == ids_w
    for b in range(8):
        assert np.array_equal(logits[b], logits_w[b]), b


# ----------------------------------------------------------------------------------------------------------------- 4. state reset
def test_prefill_many_resets_the_slot_state(eng, dev):
    from voice_tts_amd.gpt_engine import GptEngine

    dt, mb, e = eng
    cfg, W = _tiny()
    g = torch.Generator().manual_seed(23)
    entries = [(1, _prompt(20, 1, 128, g, dev), 1), (0, _prompt(12, 0, 128, g, dev), 0)]
    fresh = GptEngine(cfg, dtype=dt, max_seq=MAX_SEQ, max_batch=mb, device=dev).load_state_dict(W)
    _fill(fresh, entries, False)
    fresh.decode(2, N_STEPS, **GREEDY)
    want = [fresh.read(b)[0][:N_STEPS].tolist() for b in (0, 1)]
    _fill(e, entries, False)
    t0 = want[1][0]
    e.set_bans(1, [t0], [want[1][1]])
    e.set_sequence_bias(1, [((want[1][2], want[1][3]), -3e4)])
    e.set_forced_eos(1, [5])
    e.decode(2, N_STEPS, forced_eos_step=3, **GREEDY)
    assert e.read(1)[0][:N_STEPS].tolist() != want[1]  # the state did bite
    _fill(e, entries, True)
    e.decode(2, N_STEPS, **GREEDY)
    assert [e.read(b)[0][:N_STEPS].tolist() for b in (0, 1)] == want


# ----------------------------------------------------------------------------------------------------------------- 5. beam groups
def test_beam_groups_after_prefill_many(dev):
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny(seed=5)
    e = GptEngine(cfg, dtype="bf16", max_seq=MAX_SEQ, max_batch=32, device=dev).load_state_dict(W)
    g = torch.Generator().manual_seed(41)
    entries = [(3 * i, _prompt(rows, pad, 128, g, dev), pad) for i, (rows, pad) in enumerate([(11, 0), (70, 2), (29, 5), (130, 0)])]

    def run(batched):
        _fill(e, entries, batched)
        for i in range(4):
            e.beam_begin(3, group=i, rng_stream=i)
        e.beam_decode(20, groups=4, repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, seed=7)
        out = []
        for i in range(4):
            ids, done, score = e.beam_read(20, group=i)[:3]
            out.append((np.asarray(ids).tolist(), bool(done), float(score)))
        return out

    want = run(False)
    assert run(True) == want
    assert len({tuple(w[0]) for w in want}) == 4


# ---------------------------------------------------------------------------------------------------------------------- 6. errors
def test_errors_name_the_entry_and_leave_every_slot_alone(eng, dev):
    from voice_tts_amd._lib import IxttsError

    dt, mb, e = eng
    g = torch.Generator().manual_seed(51)
    ok = _prompt(12, 0, 128, g, dev)
    keep = (1, _prompt(15, 1, 128, g, dev), 1)
    e.prefill(0, ok, 0)
    e.prefill(*keep)
    first = e.read_logits(1).copy()
    e.decode(2, N_STEPS, **GREEDY)
    want = e.read(1)[0][:N_STEPS].tolist()
    e.prefill(0, ok, 0)
    e.prefill(*keep)
    long_rows = torch.zeros(MAX_SEQ - 2, 128, device=dev)
    bad = [([(0, ok, 0), (2, ok, 0), (0, ok, 0)], r"entry 2: slot 0 given twice"),
           ([(0, ok, 0), (-1, ok, 0)], r"entry 1: slot -1"),
           ([(mb, ok, 0)], rf"entry 0: slot {mb}"),
           ([(0, ok, 0), (2, long_rows, 0)], r"entry 1 \(slot 2\)"),
           ([(0, ok, 0), (2, ok, 12)], r"entry 1 \(slot 2\)"),
           ([(b % mb, ok, 0) for b in range(mb + 1)], rf"{mb + 1} entries")]
    for entries, msg in bad:
        with pytest.raises(IxttsError, match=msg):
            e.prefill_many(entries)
        assert np.array_equal(e.read_logits(1), first), msg
    e.prefill_many([])  # n = 0: returns without effect
    assert np.array_equal(e.read_logits(1), first)
    e.decode(2, N_STEPS, **GREEDY)
    assert e.read(1)[0][:N_STEPS].tolist() == want


# ------------------------------------------------------------------------------------------------------- 7. IXTTS_ROWS_ATTN=legacy
_LEGACY_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import numpy as np, torch
import test_gpu_prefill_many as T
from voice_tts_amd.gpt_engine import GptEngine
dev = torch.device("cuda:0")
cfg, W = T._tiny()
for dt, mb in T.ENGINES:
    e = GptEngine(cfg, dtype=dt, max_seq=T.MAX_SEQ, max_batch=mb, device=dev).load_state_dict(W)
    T._prime(e, 15, dev)
    want = T._run(e, T._edge_entries(dev), False, 15)
    T._prime(e, 15, dev)
    T._same(T._run(e, T._edge_entries(dev), True, 15), want)
    print("legacy ok", dt, flush=True)
"""


def test_legacy_row_attention_in_a_child_process():
    """IXTTS_ROWS_ATTN is a function-static read: a fresh process, the variable in ITS environment"""
    env = dict(os.environ, IXTTS_ROWS_ATTN="legacy")
    r = subprocess.run([sys.executable, "-c", _LEGACY_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("legacy ok") == len(ENGINES), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------------ 8. production width
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_production_width_16_prompts_in_one_call(dev, dt):
    """D = 1280, 24 layers: the instantiations the tiny model does not reach"""
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    cfg = WR.tiny_gpt_cfg(model_dim=1280, layers=24, heads=20)
    W = WR.make_gpt_weights(cfg, seed=1234)
    e = GptEngine(cfg, dtype=dt, max_seq=3072, max_batch=16, device=dev).load_state_dict(W)
    del W
    g = torch.Generator().manual_seed(100)
    pads = {2: 1, 7: 5, 13: 17}
    entries = [(b, _prompt(120 + (7 * b) % 18, pads.get(b, 0), 1280, g, dev), pads.get(b, 0)) for b in range(16)]
    assert all(120 <= t.shape[0] <= 137 for _, t, _ in entries)
    _fill(e, entries, False)
    want = [e.read_logits(b).copy() for b in range(16)]
    _fill(e, list(reversed(entries)), True)
    for b in range(16):
        assert np.array_equal(e.read_logits(b), want[b]), b
    assert len({w.tobytes() for w in want}) == 16
