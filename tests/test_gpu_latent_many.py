"""`GptEngine.latent_many`: the latent forward of several sequences in packed causal passes (csrc/gpt_rows.hip: the packed QKV
epilogue and row attentions of prefill_many, a pack kernel and a final-norm scatter of its own).  All sequences of a pass share the
scratch sequence's cache at disjoint positions that start on multiples of 64.  The contract is bit for bit, so every comparison is
`torch.equal` against the SERIAL TWIN: `latent` called alone on the same engine."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SEQ = 640
ENGINES = [("f32", 16), ("bf16", 32), ("f16", 32)]
GREEDY = dict(repetition_penalty=10.0, suppress_stop=True)

# (n_prefix, n_codes): T = n_prefix + n_codes rows at ceil64(T) cache positions
EDGES = [(1, 1),       # T 2: the smallest sequence, n_prefix = 1 and n_codes = 1 at once
         (20, 11),     # T 31: the next sequence sits at packed row 31 + .. but at a cache position on a multiple of 64
         (40, 23),     # T 63: one row short of a key tile
         (34, 30),     # T 64: exactly one key tile, the next position needs no rounding
         (1, 64),      # T 65: n_prefix = 1; crosses a 64-row GEMM tile and a key tile
         (100, 28),    # T 128: exactly one attention tile
         (128, 1),     # T 129: n_codes = 1, alone in the second attention tile
         (51, 150)]    # T 201: two attention tiles
ORDERS = {"as_given": None, "t128_first": [5, 0, 1, 2, 3, 4, 6, 7], "t31_first": [1, 0, 2, 3, 4, 5, 6, 7], "rows_max_256": None}
# ceil64: 64 64 64 64 128 128 192 256; as given at 640: 512 | 448.  T = 128 first: 128 + 4 x 64 + 128 = 512 | 448.
# T = 31 first: as given.  rows_max 256: 4 x 64 | 128 128 | 192 | 256
PASSES = {"as_given": 2, "t128_first": 2, "t31_first": 2, "rows_max_256": 4}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _tiny(seed=7):
    import voice_tts_amd.weights as WR

    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2, max_mel_tokens=300)
    return cfg, WR.make_gpt_weights(cfg, seed=seed, head_scale=50.0)


def _entry(P, n, g, dev, D=128):
    return (torch.randn(P, D, generator=g) * 0.5).to(dev), torch.randint(0, 8192, (n,), generator=g, dtype=torch.int32).to(dev)


def _entries(shapes, dev, seed=123, order=None):
    g = torch.Generator().manual_seed(seed)
    ent = [_entry(P, n, g, dev) for P, n in shapes]
    return [ent[i] for i in order] if order is not None else ent


def _engine(dt, mb, dev, max_seq=MAX_SEQ):
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W = _tiny()
    return GptEngine(cfg, dtype=dt, max_seq=max_seq, max_batch=mb, device=dev).load_state_dict(W)


@pytest.fixture(scope="module", params=ENGINES, ids=[e[0] for e in ENGINES])
def eng(request, dev):
    dt, mb = request.param
    return dt, mb, _engine(dt, mb, dev)


def _serial(e, entries):
    return [e.latent(p, c).clone() for p, c in entries]


def _same(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and torch.equal(a, b), i


# ------------------------------------------------------------------------------------------------------- 1. edges of every tile
@pytest.fixture(scope="module")
def edge_twin(eng, dev):
    """the serial twin of the edges case: computed once per engine, never changed"""
    return _serial(eng[2], _entries(EDGES, dev))


@pytest.mark.parametrize("case", list(ORDERS))
def test_edges_of_every_tile(eng, edge_twin, dev, case):
    from voice_tts_amd.gpt_engine import GptEngine

    dt, mb, e = eng
    order = ORDERS[case]
    idx = order if order is not None else list(range(len(EDGES)))
    kw = dict(rows_max=256) if case == "rows_max_256" else {}
    shapes = [EDGES[i] for i in idx]
    assert GptEngine.latent_plan([P for P, _ in shapes], [n for _, n in shapes], kw.get("rows_max", MAX_SEQ))[1] == PASSES[case]
    got = e.latent_many(_entries(EDGES, dev, order=order), **kw)
    _same(got, [edge_twin[i] for i in idx])
    assert all(bool(torch.isfinite(t).all()) for t in got)
    assert not torch.equal(got[idx.index(3)][:11], got[idx.index(1)])  # (the sequences do differ)


# ----------------------------------------------------------------------------------------------------------- 2. fp32 tile switch
def test_fp32_packed_pass_on_the_128_row_tile(dev):
    """9 x 60 + 64 = 604 packed rows at 10 x 64 cache positions, one pass at max_seq 1024: the fp32 launcher takes 128-row GEMM tiles
    where each solo pass (60 rows) took 64-row ones"""
    from voice_tts_amd.gpt_engine import GptEngine

    e = _engine("f32", 2, dev, max_seq=1024)
    shapes = [(35, 25)] * 9 + [(30, 34)]  # T = 60 x 9, 64: 604 rows, 640 positions
    assert GptEngine.latent_plan([P for P, _ in shapes], [n for _, n in shapes], 1024) == ([0] * 10, 1)
    assert sum(P + n for P, n in shapes) >= 600
    entries = _entries(shapes, dev, seed=9)
    _same(e.latent_many(entries), _serial(e, entries))


# ------------------------------------------------------------------------------------------------------------------ 3. live slots
def test_decode_slots_are_not_touched(eng, dev):
    dt, mb, e = eng
    g = torch.Generator().manual_seed(17)
    prompts = [(torch.randn(10 + 5 * b, 128, generator=g) * 0.5).to(dev) for b in range(4)]
    entries = _entries([(20, 11), (34, 30), (100, 28)], dev, seed=31)

    def run(batched):
        for b, p in enumerate(prompts):
            e.prefill(b, p, 0)
        e.decode(4, 10, **GREEDY)
        lat = e.latent_many(entries) if batched else _serial(e, entries)
        lat = [t.clone() for t in lat]
        e.decode(4, 10, **GREEDY)
        return lat, [e.read(b)[0][:20].tolist() for b in range(4)], [e.read_logits(b).copy() for b in range(4)]

    lat_w, ids_w, logits_w = run(False)
    lat, ids, logits = run(True)
    _same(lat, lat_w)
    assert ids == ids_w and len({tuple(i) for i in ids}) > 1
    for b in range(4):
        assert np.array_equal(logits[b], logits_w[b]), b


# -------------------------------------------------------------------------------------------------- 4. more sequences than slots
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_twelve_entries_on_a_one_slot_engine(dev, dt):
    e = _engine(dt, 1, dev)
    shapes = [(10 + 7 * i, 5 + 9 * (i % 5)) for i in range(12)]
    entries = _entries(shapes, dev, seed=77)
    want = _serial(e, entries)
    _same(e.latent_many(entries), want)
    _same(e.latent_many(list(reversed(entries)), rows_max=130), list(reversed(want)))


# ------------------------------------------------------------------------------------------------------------------ 5. degenerate
def test_no_entries_and_entries_without_codes(eng, dev):
    dt, mb, e = eng
    assert e.latent_many([]) == []
    shapes = [(12, 0), (20, 11), (7, 0), (7, 0), (34, 30), (9, 0)]
    entries = _entries(shapes, dev, seed=5)
    got = e.latent_many(entries)
    assert [tuple(t.shape) for t in got] == [(n, 128) for _, n in shapes]
    _same([got[1], got[4]], _serial(e, [entries[1], entries[4]]))
    assert [t.shape[0] for t in e.latent_many([entries[0]])] == [0]


# ---------------------------------------------------------------------------------------------------------------------- 6. errors
def _raw(e, entries, outs, null=None):
    """ixtts_gpt_latent_many on outputs of the caller's; `null` = (entry, "prefix" | "codes" | "latent") passes a null pointer there"""
    from voice_tts_amd import _lib

    n = len(entries)
    ptr = lambda t, i, what: None if null == (i, what) else t.data_ptr()
    pp = (C.c_void_p * n)(*[ptr(p, i, "prefix") for i, (p, _) in enumerate(entries)])
    cp = (C.c_void_p * n)(*[ptr(c, i, "codes") for i, (_, c) in enumerate(entries)])
    op = (C.c_void_p * n)(*[ptr(o, i, "latent") for i, o in enumerate(outs)])
    n_p = (C.c_int * n)(*[p.shape[0] for p, _ in entries])
    n_c = (C.c_int * n)(*[c.numel() for _, c in entries])
    with torch.cuda.device(e.device):
        rc = _lib.lib().ixtts_gpt_latent_many(e._h, n, pp, n_p, cp, n_c, op, 0, e._stream())
    _lib.check(rc, "ixtts_gpt_latent_many")


def test_errors_name_the_entry_and_leave_every_output_alone(eng, dev):
    """host checks, all of them: nothing of a refused call reaches the GPU"""
    from voice_tts_amd._lib import IxttsError

    dt, mb, e = eng
    g = torch.Generator().manual_seed(51)
    ok = _entry(20, 11, g, dev)
    ok2 = _entry(34, 30, g, dev)
    want = _serial(e, [ok, ok2])
    too_long = _entry(MAX_SEQ - 12, 10, g, dev)    # 628 + 10 + 2 = max_seq
    too_many = _entry(5, 302, g, dev)              # 302 + 2 > max_mel_tokens + 3
    cases = [([ok, too_long, ok2], None, r"entry 1: sequence of 640 rows exceeds max_seq 640"),
             ([ok, ok2, too_many], None, r"entry 2: 302 codes exceed the mel position table"),
             ([ok, ok2], (1, "prefix"), r"entry 1: bad argument"),
             ([ok, ok2], (0, "codes"), r"entry 0: bad argument"),
             ([ok, ok2], (1, "latent"), r"entry 1: bad argument")]
    for entries, null, msg in cases:
        outs = [torch.full((c.numel(), 128), -7.5, device=dev) for _, c in entries]
        with pytest.raises(IxttsError, match=msg):
            _raw(e, entries, outs, null)
        torch.cuda.synchronize(dev)
        assert all(bool((o == -7.5).all()) for o in outs), msg
    with pytest.raises(IxttsError, match=r"entry 1: sequence of 640 rows"):
        e.latent_many([ok, too_long])
    outs = [torch.full((11, 128), -7.5, device=dev), torch.full((30, 128), -7.5, device=dev)]
    _raw(e, [ok, ok2], outs)  # the handle still works
    _same(outs, want)


# ---------------------------------------------------------------------------------------------------------- 7. reference fixture
def test_reference_fixture_packed_between_two_sequences(golden, dev):
    import voice_tts_amd.weights as WR
    from voice_tts_amd.gpt_engine import GptEngine

    g = golden("gpt_tiny.npz")
    cfg = WR.tiny_gpt_cfg(model_dim=int(g["model_dim"]), layers=int(g["layers"]), heads=int(g["heads"]))
    W = WR.make_gpt_weights(cfg, seed=int(g["seed"]), head_scale=50.0)
    e = GptEngine(cfg, dtype="f32", max_seq=256, max_batch=2, device=dev).load_state_dict(W)
    conds = torch.from_numpy(g["conds_latent"])
    text = torch.from_numpy(g["text_plain"]).long()
    t = torch.cat((torch.tensor([0]), text, torch.tensor([1])))
    temb = W["text_embedding.weight"][t] + W["text_pos_embedding.emb.weight"][: t.numel()]
    prefix = torch.cat((conds, temb), 0).to(dev)
    codes = torch.from_numpy(g["latent_codes"]).to(torch.int32).to(dev)
    D = int(g["model_dim"])
    rg = torch.Generator().manual_seed(3)
    before, after = _entry(23, 17, rg, dev, D), _entry(9, 40, rg, dev, D)
    solo = e.latent(prefix, codes).clone()
    got = e.latent_many([before, (prefix, codes), after])
    assert GptEngine.latent_plan([23, prefix.shape[0], 9], [17, codes.numel(), 40], 256)[1] == 1
    ref = torch.from_numpy(g["latent"])
    assert got[1].shape == ref.shape
    assert (got[1].cpu() - ref).abs().max().item() <= 1e-4 * max(1.0, ref.abs().max().item())
    assert torch.equal(got[1], solo)
    _same([got[0], got[2]], _serial(e, [before, after]))


# ------------------------------------------------------------------------------------------------------- 8. IXTTS_ROWS_ATTN=legacy
_LEGACY_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch
import test_gpu_latent_many as T
dev = torch.device("cuda:0")
for dt, mb in T.ENGINES:
    e = T._engine(dt, mb, dev)
    want = T._serial(e, T._entries(T.EDGES, dev))
    T._same(e.latent_many(T._entries(T.EDGES, dev)), want)
    print("legacy ok", dt, flush=True)
"""


def test_legacy_row_attention_in_a_child_process():
    """IXTTS_ROWS_ATTN is a function-static read: a fresh process, the variable in ITS environment"""
    env = dict(os.environ, IXTTS_ROWS_ATTN="legacy")
    r = subprocess.run([sys.executable, "-c", _LEGACY_CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("legacy ok") == len(ENGINES), r.stdout + r.stderr
