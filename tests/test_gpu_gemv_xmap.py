"""Lane map of the register GEMVs at production width (csrc/gpt_kernels.h: `RegMap`).

A lane keeps one k slice over all rows of its units: bf16 / f16 at K = 1280 take two full wave-loads per row and one tail load
shared by two rows; fp32 takes five full loads per row.  This only takes effect at model_dim 1280 -- width 128 keeps the flat
map and is what the rest of the suite runs -- so the engines here are 1280 wide, 20 heads, 2 layers, with a vocabulary of 1003
rows: not a multiple of the head kernel's 32 rows per workgroup and odd, so the clamped tail units run and the last unit's
shared tail load has one valid half.

The partition of k over lanes is an order of fp32 summation: against the oracle the engines may be no worse than twice what the
flat map gave (a dropped or doubled element is orders above that), and a slot's arithmetic must not know its company.  (Splitting
K = 5120 of the MLP-out GEMV over the workgroup's waves was built and measured with this map and not kept,
profiles/r09_notes.md: no kernel, so no coverage case for it here.)
"""
import numpy as np
import pytest
import torch

MATS = ("c_attn.weight", "c_proj.weight", "c_fc.weight", "mel_head.weight")
ROUND = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": None}
V, START, STOP = 1003, 1001, 1002
STEPS = 8

# (rms, max) of the logit error after prefill + 8 greedy steps over all B slots, relative to the oracle's largest |logit|, of
# the flat map, measured with the library of the commit before this file by this same function on one MI355X
# (profiles/r09_notes.md section 3).  The oracle runs on the matrices rounded to the weight type; K/V stay unrounded in it.
FLAT_MAP_ERR = {
    ("bf16", 1): (1.4582e-03, 4.5723e-03), ("bf16", 2): (1.4469e-03, 4.5988e-03), ("bf16", 3): (1.4768e-03, 5.4272e-03), ("bf16", 4): (1.4581e-03, 5.4272e-03),
    ("f16", 1): (1.9417e-04, 6.4886e-04), ("f16", 2): (1.8331e-04, 6.4886e-04), ("f16", 3): (1.8735e-04, 7.4671e-04), ("f16", 4): (1.8425e-04, 7.4671e-04),
    ("f32", 1): (2.7730e-07, 1.0556e-06), ("f32", 2): (2.6023e-07, 1.0556e-06), ("f32", 3): (4.1707e-07, 2.1954e-06), ("f32", 4): (3.8335e-07, 2.1954e-06),
}


def _cfg():
    import voice_tts_amd.weights as WR

    return WR.tiny_gpt_cfg(model_dim=1280, layers=2, heads=20, number_mel_codes=V, start_mel_token=START, stop_mel_token=STOP)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def build_model():
    """Seeded weights and four prompts of unequal length (one left-padded)."""
    import voice_tts_amd.weights as WR

    cfg = _cfg()
    W = WR.make_gpt_weights(cfg, seed=77, head_scale=50.0)
    g = torch.Generator().manual_seed(78)
    prompts = []
    for rows, pad in ((21, 0), (34, 3), (9, 0), (27, 1)):
        e = torch.randn(rows, 1280, generator=g) * 0.5
        e[:pad] = 0
        mask = torch.ones(rows + 1, dtype=torch.long)
        mask[:pad] = 0
        prompts.append((e, pad, mask))
    return cfg, W, prompts


def build_oracles(model):
    """The fp32 oracle on the matrices rounded to each weight type."""
    from oracle import gpt as OG

    cfg, W, _ = model
    out = {}
    for name, to in ROUND.items():
        Wq = W if to is None else {k: (v.to(to).to(torch.float32) if k.endswith(MATS) else v) for k, v in W.items()}
        out[name] = OG.GptOracle(Wq, cfg["layers"], cfg["heads"])
    return out


@pytest.fixture(scope="module")
def model():
    return build_model()  # shared and never modified


@pytest.fixture(scope="module")
def oracles(model):
    return build_oracles(model)


def measure_logit_error(model, oracles, dev, dtype, B):
    """(rms, max) over the B slots of |device logits - oracle logits| / max|oracle logit| after prefill + STEPS greedy steps,
    the oracle teacher-forced on the device's own tokens."""
    from oracle import gpt as OG
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W, prompts = model
    eng = GptEngine(cfg, dtype=dtype, max_seq=64, max_batch=B, device=dev).load_state_dict(W)
    for b in range(B):
        eng.prefill(b, prompts[b][0], prompts[b][1])
    eng.decode(B, STEPS, repetition_penalty=10.0, suppress_stop=True)
    sq, n, worst = 0.0, 0, 0.0
    for b in range(B):
        e, pad, mask = prompts[b]
        ids = eng.read(b)[0][:STEPS].tolist()
        ref = OG.teacher_forced_logits(oracles[dtype], e, mask, ids, start_mel=START)[STEPS].numpy().astype(np.float64)
        d = (eng.read_logits(b).astype(np.float64) - ref) / np.abs(ref).max()
        sq, n, worst = sq + float((d * d).sum()), n + d.size, max(worst, float(np.abs(d).max()))
    return (sq / n) ** 0.5, worst


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_production_width_logits_vs_oracle_no_worse_than_twice_the_flat_map(model, oracles, dev, dtype, B):
    rms, worst = measure_logit_error(model, oracles, dev, dtype, B)
    print(f"xmap {dtype} B={B}: logit error / scale rms {rms:.3e} max {worst:.3e}")
    rms0, worst0 = FLAT_MAP_ERR[(dtype, B)]
    assert rms <= 2 * rms0 and worst <= 2 * worst0, (dtype, B, rms, worst, rms0, worst0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_a_slot_is_bit_identical_alone_and_in_company(model, dev, dtype):
    """Every prompt alone on a 1-slot engine, then in every slot b of engines of 2, 3 and 4 slots (the prompts rotated, so a
    prompt meets different slots and different company): tokens and logits after 16 steps byte for byte the same."""
    from voice_tts_amd.gpt_engine import GptEngine

    cfg, W, prompts = model
    n = 16
    one = GptEngine(cfg, dtype=dtype, max_seq=64, max_batch=1, device=dev).load_state_dict(W)
    alone = []
    for e, pad, _ in prompts:
        one.prefill(0, e, pad)
        one.decode(1, n, repetition_penalty=10.0, suppress_stop=True)
        alone.append((one.read(0)[0][:n].tolist(), one.read_logits(0).copy()))
    assert len({tuple(a[0]) for a in alone}) == 4  # four different sequences
    for B in (2, 3, 4):
        eng = GptEngine(cfg, dtype=dtype, max_seq=64, max_batch=B, device=dev)
        eng.share_arena(one)
        for rot in (0, B - 1):
            order = [(b + rot + B) % 4 for b in range(B)]
            for b, p in enumerate(order):
                eng.prefill(b, prompts[p][0], prompts[p][1])
            eng.decode(B, n, repetition_penalty=10.0, suppress_stop=True)
            for b, p in enumerate(order):
                assert eng.read(b)[0][:n].tolist() == alone[p][0], (B, b, p)
                assert eng.read_logits(b).tobytes() == alone[p][1].tobytes(), (B, b, p)


# ------------------------------------------------------------------------------------------------------------------------------
# The maps themselves, without a GPU: `RegMap` of csrc/gpt_kernels.h restated in numpy.


def reg_map(K, PER, ROWS):
    """RegMap of csrc/gpt_kernels.h, function by function: for every wave-load j and lane the row of the unit (::row), the
    element of the unit where the lane's 16 bytes start (::elem), the activation chunk the load multiplies (::chunk) and the
    first k of that chunk in this lane (::xk); and whether the fixed-k map applies (::XMAP)."""
    VEC = PER // 64
    NL, NF = ROWS * K // PER, K // PER
    tail = K % PER != 0
    xmap = K >= PER and (not tail or (K % PER == PER // 2 and ROWS % 2 == 0))
    NFR = ROWS * NF
    lane = np.arange(64)

    def chunk(j):
        return (j % NF if j < NFR else NF) if xmap else j

    def xk(c):
        if not xmap:
            return (c * PER + lane * VEC) % K
        return c * PER + lane * VEC if c < NF else NF * PER + (lane & 31) * VEC

    def row(j):
        if not xmap:
            return (j * PER + lane * VEC) // K
        return np.full(64, j // NF) if j < NFR else 2 * (j - NFR) + (lane >> 5)

    def elem(j):
        return row(j) * K + xk(chunk(j)) if xmap else j * PER + lane * VEC

    return xmap, [(row(j), elem(j), chunk(j), xk(chunk(j))) for j in range(NL)]


@pytest.mark.parametrize("K,PER,ROWS,xmap,chunks", [(1280, 512, 2, True, 3), (1280, 256, 2, True, 5), (128, 512, 4, False, 1)])
def test_register_gemv_lane_map_covers_every_element_once(K, PER, ROWS, xmap, chunks):
    VEC = PER // 64
    got_xmap, loads = reg_map(K, PER, ROWS)
    assert got_xmap == xmap and len(loads) == ROWS * K // PER
    cover = np.zeros(ROWS * K, dtype=int)
    for row, e, chunk, xk in loads:
        assert np.array_equal(e // K, row) and np.array_equal(e % K, xk)  # the lane's activations sit at its weights' k, its sum goes to its row
        for ln in range(64):
            cover[e[ln]: e[ln] + VEC] += 1
    assert (cover == 1).all()
    assert len({c for _, _, c, _ in loads}) == chunks  # floats per lane and slot = chunks * VEC
    if xmap:
        NF = K // PER
        for j, (row, e, _, k) in enumerate(loads):
            if j < ROWS * NF:  # a full load: one row, known without the lane; 16 B per lane, one contiguous run
                assert (row == j // NF).all() and np.array_equal(np.diff(k), np.full(63, VEC))
            else:  # the shared tail: lanes 0..31 row 2t, lanes 32..63 row 2t+1, each half one contiguous run of 32 * 16 bytes
                t = j - ROWS * NF
                assert (row[:32] == 2 * t).all() and (row[32:] == 2 * t + 1).all()
                assert np.array_equal(k[:32], k[32:]) and np.array_equal(np.diff(k[:32]), np.full(31, VEC))
                assert k[0] == NF * PER and k[31] + VEC == K
