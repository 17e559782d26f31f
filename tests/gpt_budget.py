"""The fp64 twin of the GPT trunk and head, its fp32 CPU leg, and the cases of the GPT error budget: shared by tests/test_gpt_twin.py
(what the budget sees, on the CPU), tests/test_gpu_gpt_fp64.py (the device against the twin) and tools/gpt_error_budget.py (which records
the numbers in profiles/gpt_error_budget.json).

`Twin` is one function of the trunk and the head, written from oracle/gpt.py and from the kernels, parameterised by
  * the compute dtype: fp64 = the twin, fp32 = the yardstick leg (the same function, the same sites, the arithmetic's own noise
    including the 16-bit roundings that flip between an fp32 and an fp64 computation);
  * the weight type of the engine ("f32" | "bf16" | "f16"), which selects the ROUNDING SITES of each device path from the tables below:
    where a value is rounded to the 16-bit type on the device, the twin rounds it too.  In "f32" both tables are empty and the twin is
    the plain fp64 oracle (tests/test_gpt_twin.py holds it to `GptOracle` widened to fp64 within 1e-12).
The LayerNorm gains are folded into the matrices they feed, as the engine folds them; in fp64 that changes nothing (1e-15), in the fp32
leg it is the fold's own fp32 noise, which the device has too.

Errors are (max |d| / max |twin|, rms(d) / rms(twin)).  A device path may reach 3 x the yardstick's max and 2 x its rms -- the margins of
tests/test_gpu_s2mel_fp64.py and tests/test_gpu_bigvgan_fp64.py: "the same result in another summation order".  The rms floor is the
largest yardstick rms among the cases of the same family, type and weight set (`Legs.limits`): a case on which the CPU leg was lucky sets
no tighter bar than its neighbours.  No number here comes from a device run.

The second yardstick leg of the 16-bit types (`FLIP LEG` below).  A rounding to bf16 or fp16 whose operand lies within the fp32
arithmetic's noise of a tie goes one way in one summation order and the other way in another, and ONE flipped LayerNorm element of a
mel row moves that row by about 1e-3 of the result (bf16: 2^-8 of an element of size 1, through all 512 c_fc columns at once, onto a
residual stream of size 0.03).  On a 30-row case the fp32 leg has such a flip or has none, by chance: its error is 2e-7 or 1e-3, and
which of the two says nothing about the device, whose noise falls elsewhere.  So the flips get a leg of their own, deterministic: the
fp64 twin in which every rounding whose operand lies within KAPPA x sigma of a tie goes the OTHER way, sigma being the rms, over the
operand's row, of |fp32 - fp64| at that site in a run of both dtypes WITHOUT the activation roundings (so that no flip pollutes the
measurement; the weights are rounded, bit for bit the device's).  KAPPA is 3, the factor a device path is allowed on the max: a device
whose noise is within its allowance flips operands up to that far from a tie.  The yardstick is the larger of the two legs' errors.

Two weight sets per case: "normal" = the GPT-2 initialisation of `make_gpt_weights`, and "sharp" = the same with the q and k columns of
every c_attn.weight multiplied by 8 (score standard deviation about 3.4 instead of 0.05: a peaked softmax whose running maximum moves from
key tile to key tile, so that the rescale of the flash kernel and the merge of the split-S decode attention carry weight).

What the budget does not claim: the wide engines (5..32 slots) and the beam kernels round at other sites (hi + lo activation splits, bf16
`ff`) and need a table of their own."""
import math

import torch
import torch.nn.functional as F

import voice_tts_amd.weights as WR

KINDS = ("f32", "bf16", "f16")
WSETS = ("normal", "sharp")
MAX_FACTOR, RMS_FACTOR = 3.0, 2.0  # the margins of tests/test_gpu_s2mel_fp64.py and tests/test_gpu_bigvgan_fp64.py

# ------------------------------------------------------------------------------------------------------------ rounding sites
# site -> where the device rounds (files under voice-tts_amd/csrc/).  q, the residual stream, every accumulation, the softmax and the
# LayerNorm statistics are fp32 on every path; the biases (b' = b + W beta) stay fp32 (fold_convert_kernel, gpt_kernels.h:2347,2356).
_WEIGHT = ("gpt_kernels.h:2348-2352 fold_convert_kernel: W' = W diag(g) formed in fp32, then rounded (fp16: f16_sat); c_attn, c_proj, c_fc, "
           "mlp.c_proj and, with final_norm folded in, mel_head (gpt_engine.hip:688-694 fold_all; ln_f stays explicit)")
_ROWS_16 = {
    "weight": _WEIGHT,
    "ln": "gpt_rows.hip:68 ln_rows_kernel<K, OT>: store_kv(yr, (v - mean) * rstd), OT = the weights' type (gpt_rows.hip:701,718)",
    "kv": "gpt_rows.hip:483 (RE_QKV) and :456 (RE_QKV_PACKED) gemm_rows_bf16_kernel epilogue: store_kv(cache, acc + bias); "
          "gpt_kernels.h:178-179 (bf16 RNE; fp16 RNE saturating at +-65504)",
    "att": "attn_rows_flash_body.h:146 and attn_rows_body.h:24: store_kv(out, o), OT = Act = the weights' type (gpt_rows.hip:653,689)",
    "gelu": "gpt_rows.hip:474 gemm_rows_bf16_kernel RE_GELU: store_kv(ff, v / (1 + __expf(-u2)))",
}
_REG_16 = {
    "weight": _WEIGHT,
    "kv": "gpt_kernels.h:218 gemv_epilogue EPI_QKV: store_kv(cache, v); the activations of the register GEMVs stay fp32 "
          "(gpt_kernels.h:238-240), `ff` and the attention output are float buffers (gpt_engine.hip:146,161)",
}
ROWS_SITES = {"f32": {}, "bf16": _ROWS_16, "f16": _ROWS_16}  # gpt_rows.hip: prefill, latent pass and their packed forms
REG_SITES = {"f32": {}, "bf16": _REG_16, "f16": _REG_16}     # register decode path, 1..4 slots (gpt_kernels.h gemv_reg / gemv_lds)

F16_MAX = 65504.0


_FORMAT = {"bf16": (7, -126), "f16": (10, -14)}  # explicit significand bits, exponent of the smallest normal number


def _spacing(x, kind):
    """The spacing of the 16-bit type's numbers in x's binade, in x's dtype (exact: a power of two)."""
    mant, emin = _FORMAT[kind]
    e = (torch.frexp(x)[1] - 1).clamp_min(emin)  # floor(log2 |x|), exactly
    return torch.exp2((e - mant).to(x.dtype))


def round_to(x, kind):
    """x (fp32 or fp64) rounded to the 16-bit type of `kind` the way store_kv does (nearest, ties to even; fp16 saturates at +-65504),
    back in x's dtype.  One rounding from x's own dtype: a cast through fp32 would round an fp64 operand twice."""
    if kind not in _FORMAT:
        return x
    q = _spacing(x, kind)
    r = torch.round(x / q) * q  # (x / q and the product are exact: q is a power of two; torch.round rounds halves to even)
    return r.clamp(-F16_MAX, F16_MAX) if kind == "f16" else r


KAPPA = 3.0  # = MAX_FACTOR: how many sigma of the fp32 noise around a tie count as "may go either way" in the flip leg


def round_flipped(x, kind, sigma):
    """`round_to`, but an element within KAPPA * sigma (sigma [rows, 1]) of the tie between its two neighbours takes the farther one."""
    r = round_to(x, kind)
    other = round_to(r + torch.sign(x - r) * _spacing(x, kind), kind)  # the neighbour on x's side of r (r itself where x is exact)
    amb = ((x - 0.5 * (r + other)).abs() <= KAPPA * sigma) & (other != r)
    return torch.where(amb, other, r)


class Tape:
    """The rounding-site calls of one run, in order.  mode "record": the activation sites do not round and their operands are kept;
    mode "flip": call i rounds with `round_flipped` under sigma[i]."""

    def __init__(self, mode, sigma=None):
        self.mode, self.sigma, self.kept, self.i, self.flipped = mode, sigma, [], 0, 0

    @staticmethod
    def sigmas(a, b):
        """Per call the row rms of |a - b| of two recorded runs (fp64 and fp32)."""
        assert len(a.kept) == len(b.kept)
        return [(x.double() - y.double()).pow(2).mean(dim=-1, keepdim=True).sqrt() for x, y in zip(a.kept, b.kept)]


def _ln(x, w=None, b=None):
    return F.layer_norm(x, (x.shape[-1],), w, b, 1e-5)


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


# ------------------------------------------------------------------------------------------------------------ mutants
# Structural errors the budget must see, applied to the twin (tests/test_gpt_twin.py).  Positions are cache positions (left padding
# included), as the kernels' tiles see them.
MUTANTS = ("hide_key", "seam_127", "causal_plus_one", "last_row_blind", "pad_visible", "kv_dup", "no_rescale")
HIDDEN_KEY_AFTER = 9  # hide_key: the key this many positions behind the first valid one
KV_DUP_AFTER = 100    # kv_dup: layer 0's K/V row this many positions behind the first valid one is also written to the next position
FLASH_KT = 64         # key tile of attn_rows_flash_body.h


class Twin:
    """The GPT trunk and head of one engine type in one compute dtype.  `mutant`: one of MUTANTS (or None)."""

    def __init__(self, W, cfg, kind, dtype=torch.float64, mutant=None, tape=None):
        assert kind in KINDS and (mutant is None or mutant in MUTANTS)
        self.kind, self.dt, self.mutant, self.tape = kind, dtype, mutant, tape
        self.rows_sites, self.reg_sites = ROWS_SITES[kind], REG_SITES[kind]
        self.L, self.H, self.D = cfg["layers"], cfg["heads"], cfg["model_dim"]
        self.dh = self.D // self.H
        self.start_mel = cfg["start_mel_token"]
        self.W32 = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in W.items()}
        self.Wd = {k: v.to(dtype) for k, v in self.W32.items() if v.dim() == 1 or "embedding" in k}
        self.M = {}
        for i in range(self.L):
            p = f"gpt.h.{i}."
            self.M[p + "qkv"] = self._fold(p + "attn.c_attn", p + "ln_1", conv1d=True)
            self.M[p + "o"] = self._fold(p + "attn.c_proj", None, conv1d=True)
            self.M[p + "fc"] = self._fold(p + "mlp.c_fc", p + "ln_2", conv1d=True)
            self.M[p + "pr"] = self._fold(p + "mlp.c_proj", None, conv1d=True)
        self.M["head"] = self._fold("mel_head", "final_norm", conv1d=False)

    def _fold(self, name, norm, conv1d):
        """(W' [K, N], b' [N]) in the compute dtype: the norm's gain folded into the matrix, its bias into the matrix's bias."""
        w = self.W32[name + ".weight"]
        w = w if conv1d else w.t()  # [K, N]
        b = self.W32[name + ".bias"].to(self.dt)
        g = beta = None
        if norm is not None:
            g, beta = self.W32[norm + ".weight"], self.W32[norm + ".bias"]
            b = b + beta.to(self.dt) @ w.to(self.dt)
        if "weight" in self.rows_sites:  # the device's own fp32 product, then the rounding: the stored weights, bit for bit
            wf = round_to(w if g is None else w * g.view(-1, 1), self.kind).to(self.dt)
        else:
            wf = w.to(self.dt) if g is None else w.to(self.dt) * g.to(self.dt).view(-1, 1)
        return wf.contiguous(), b

    def _r(self, sites, site, x):
        if site not in sites:
            return x
        t = self.tape
        if t is None:
            return round_to(x, self.kind)
        if t.mode == "record":
            t.kept.append(x)
            return x
        y = round_flipped(x, self.kind, t.sigma[t.i])
        t.flipped += int((y != round_to(x, self.kind)).sum())
        t.i += 1
        return y

    # ------------------------------------------------------------------ attention
    def _allow(self, qpos, S, valid_from):
        """[T, S] bool: query at cache position qpos[i] sees key j iff valid_from <= j <= qpos[i] -- and what the mutant changes of that."""
        kpos = torch.arange(S).view(1, S)
        q = torch.as_tensor(qpos).view(-1, 1)
        allow = (kpos <= q) & (kpos >= valid_from)
        m = self.mutant
        if m == "hide_key":
            allow &= ~((kpos == valid_from + HIDDEN_KEY_AFTER) & (q > kpos))
        elif m == "seam_127":
            allow &= ~((kpos == 127) & (q >= 128))
        elif m == "causal_plus_one":
            allow |= (kpos == q + 1)
        elif m == "last_row_blind":
            allow &= ~((kpos == q) & (q == S - 1))
        return allow

    def _attend(self, q, k, v, allow):
        """softmax(q k^T / sqrt(dh) + mask) v per head; q [T, D], k / v [S, D], allow [T, S]."""
        T, S, H, dh = q.shape[0], k.shape[0], self.H, self.dh
        qh, kh, vh = (t.view(-1, H, dh).transpose(0, 1) for t in (q, k, v))
        sc = (qh @ kh.transpose(-1, -2)) / math.sqrt(dh)
        sc = sc.masked_fill(~allow.view(1, T, S), float("-inf"))
        if self.mutant == "no_rescale":
            out = flash_tiled(sc, vh, rescale=False)
        else:
            out = torch.softmax(sc, dim=-1) @ vh
        return out.transpose(0, 1).reshape(T, self.D)

    # ------------------------------------------------------------------ layers
    def _layers(self, x, qpos, valid_from, sites, past=None, rows_pass=False):
        """x [T, D] rows at cache positions qpos through the layers; `past`: per layer (k, v) [S0, D] of positions 0 .. S0 - 1 (rows
        before valid_from hold zeros and are masked).  Returns (residual stream [T, D], per layer (k, v) of all positions)."""
        D, M = self.D, self.M
        S = (0 if past is None else past[0][0].shape[0]) + x.shape[0]
        allow = self._allow(qpos, S, valid_from)
        cache = []
        for i in range(self.L):
            p = f"gpt.h.{i}."
            xn = self._r(sites, "ln", _ln(x))
            qkv = xn @ M[p + "qkv"][0] + M[p + "qkv"][1]
            q, k, v = qkv.split(D, dim=-1)
            k, v = self._r(sites, "kv", k), self._r(sites, "kv", v)
            if past is not None:
                k, v = torch.cat((past[i][0], k)), torch.cat((past[i][1], v))
            if self.mutant == "kv_dup" and i == 0 and rows_pass:
                j = valid_from + KV_DUP_AFTER
                k, v = k.clone(), v.clone()
                k[j + 1], v[j + 1] = k[j], v[j]
            cache.append((k, v))
            att = self._r(sites, "att", self._attend(q, k, v, allow))
            x = x + (att @ M[p + "o"][0] + M[p + "o"][1])
            xn = self._r(sites, "ln", _ln(x))
            ff = self._r(sites, "gelu", _gelu_new(xn @ M[p + "fc"][0] + M[p + "fc"][1]))
            x = x + (ff @ M[p + "pr"][0] + M[p + "pr"][1])
        return x, cache

    def head(self, x):
        """ln_f (explicit), final_norm (its affine folded into mel_head), mel_head: fp32 activations on the device (gemv_head)."""
        h = _ln(x, self.Wd["gpt.ln_f.weight"], self.Wd["gpt.ln_f.bias"])
        return _ln(h) @ self.M["head"][0] + self.M["head"][1]

    # ------------------------------------------------------------------ the passes of the engine
    def latent(self, prefix, codes):
        """`GptEngine.latent`: rows = prefix, then [start, codes[:-1]] at mel positions 0..; ln_f and final_norm explicit, both in
        fp32 on the device (final_norm_row).  -> [n, D].  (Causal: the latent of codes[:m] is rows [:m] of this.)"""
        W = self.Wd
        codes = torch.as_tensor(codes, dtype=torch.long)
        n = codes.numel()
        tok = torch.cat((torch.tensor([self.start_mel]), codes[:-1]))
        mel = W["mel_embedding.weight"][tok] + W["mel_pos_embedding.emb.weight"][:n]
        x = torch.cat((torch.as_tensor(prefix, dtype=torch.float32).to(self.dt), mel))
        x, _ = self._layers(x, torch.arange(x.shape[0]), 0, self.rows_sites, rows_pass=True)
        h = _ln(x[prefix.shape[0]:], W["gpt.ln_f.weight"], W["gpt.ln_f.bias"])
        return _ln(h, W["final_norm.weight"], W["final_norm.bias"])

    def prefill(self, embeds, n_left_pad=0):
        """`GptEngine.prefill` then `read_logits`: the un-padded rows and the start row at cache positions n_left_pad .. (the device
        skips the padding rows: they are masked as keys).  -> (logits [V], state for `decode_step`).
        Mutant pad_visible: the last padding row (a row of zeros) takes part as if it were valid: `valid_from` one too small."""
        W = self.Wd
        vf = int(n_left_pad)
        if self.mutant == "pad_visible":
            assert vf >= 1
            vf -= 1
        P = embeds.shape[0] + 1
        start = W["mel_embedding.weight"][self.start_mel] + W["mel_pos_embedding.emb.weight"][0]
        x = torch.cat((torch.as_tensor(embeds, dtype=torch.float32)[vf:].to(self.dt), start.view(1, -1)))
        x, cache = self._layers(x, torch.arange(vf, P), vf, self.rows_sites,
                                past=[(torch.zeros(vf, self.D, dtype=self.dt),) * 2 for _ in range(self.L)] if vf else None, rows_pass=True)
        return self.head(x[-1]), dict(cache=cache, valid_from=vf)

    def decode_step(self, token, k, state):
        """One step of the register decode path: the k-th generated id (k >= 1) at mel position k + 1, over the cache the prefill and
        the earlier steps left.  -> (logits [V], state)."""
        W = self.Wd
        x = (W["mel_embedding.weight"][int(token)] + W["mel_pos_embedding.emb.weight"][k + 1]).view(1, -1)
        S = state["cache"][0][0].shape[0]
        x, cache = self._layers(x, torch.tensor([S]), state["valid_from"], self.reg_sites, past=state["cache"])
        return self.head(x[-1]), dict(cache=cache, valid_from=state["valid_from"])


def flash_tiled(sc, vh, rescale=True):
    """softmax(sc) @ vh as the flash kernel forms it: key tiles of FLASH_KT, running maximum m, row sum l and accumulator O.
    sc [H, T, S] with -inf where masked, vh [H, S, dh].  `rescale=False`: O is NOT multiplied by alpha when the maximum rises (l is)."""
    H, T, S = sc.shape
    m = torch.full((H, T, 1), float("-inf"), dtype=sc.dtype)
    l = torch.zeros(H, T, 1, dtype=sc.dtype)
    O = torch.zeros(H, T, vh.shape[-1], dtype=sc.dtype)
    for t0 in range(0, S, FLASH_KT):
        s = sc[:, :, t0:t0 + FLASH_KT]
        mn = torch.maximum(m, s.max(dim=-1, keepdim=True).values)
        mref = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
        alpha = torch.exp(m - mref)
        pw = torch.exp(s - mref)
        l = l * alpha + pw.sum(dim=-1, keepdim=True)
        O = (O * alpha if rescale else O) + pw @ vh[:, t0:t0 + FLASH_KT]
        m = mn
    return O / l


# ------------------------------------------------------------------------------------------------------------ model and cases
MAX_SEQ = 640


def config():
    """The tiny model (D 128, 2 layers, 2 heads) with a mel position table long enough for the 506-code latent pass."""
    return WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2, max_mel_tokens=520)


def weights(wset):
    cfg = config()
    W = WR.make_gpt_weights(cfg, seed=1234)
    if wset == "sharp":
        D = cfg["model_dim"]
        for i in range(cfg["layers"]):
            w = W[f"gpt.h.{i}.attn.c_attn.weight"].clone()
            w[:, :2 * D] *= 8.0
            W[f"gpt.h.{i}.attn.c_attn.weight"] = w
    else:
        assert wset == "normal"
    return W


def _randn(seed, rows, D=128):
    return torch.randn(rows, D, generator=torch.Generator().manual_seed(seed)) * 0.5


def _codes(seed, n):
    return torch.randint(0, 8192, (n,), generator=torch.Generator().manual_seed(seed))


# 3a. latent pass, prefix of 7 rows (no tile starts at a sequence start), n codes; the device computes T = 7 + n rows (the two trailing
# rows of the reference's 7 + n + 2 are never needed: causal), so every edge is met twice: by 7 + n + 2 and by 7 + n:
#   the wave's 32 query rows 31 32 33 | the 64-key tile 64 65 | the 128-row query and GEMM tile 127 128 129 257
#   | f32 only: 513, where the launcher switches to the 128-row fp32 GEMM tile (gpt_rows.hip:670)
LATENT_PREFIX = 7
_EDGES = (31, 32, 33, 64, 65, 127, 128, 129, 257)


def latent_counts(kind):
    edges = _EDGES + ((513,) if kind == "f32" else ())
    return sorted({t - LATENT_PREFIX - 2 for t in edges} | {t - LATENT_PREFIX for t in edges})


def latent_inputs():
    return _randn(11, LATENT_PREFIX), _codes(12, max(latent_counts("f32")))


# 3b. prefill then head: left padding in front of 140 valid rows (valid_from on both sides of a key-tile edge; 64 and 65 mask a whole
# first tile), and one prompt of a single row
PREFILL_CASES = {"pad0": (0, 140), "pad5": (5, 140), "pad63": (63, 140), "pad64": (64, 140), "pad65": (65, 140), "one_row": (0, 1)}
# the case of the mutants: the 205-row left-padded prompt of test_gpu_gpt.py's flash test
MUTANT_PREFILL = (5, 200)
MUTANT_LATENT = 250


def prefill_inputs(pad, valid, seed=21):
    """[pad + valid, D]: zero rows, then the valid ones."""
    return torch.cat((torch.zeros(pad, 128), _randn(seed + pad + valid, valid)))


# 3c. packed passes: four sequences whose row counts (100, 60, 130, 30) put the sequence boundaries 100, 160 and 290 inside the 128-row
# GEMM tiles [0, 128), [128, 256), [256, 384); the third has a 128-row attention tile of its own and a tail; each its own rows
PACKED_LATENT = ((7, 93), (20, 40), (7, 123), (9, 21))          # (prefix rows, codes)
PACKED_PREFILL = ((0, 99), (5, 59), (65, 129), (0, 29))         # (left padding, valid rows): T = valid + 1


def packed_latent_inputs(i):
    p, n = PACKED_LATENT[i]
    return _randn(31 + i, p), _codes(41 + i, n)


def packed_prefill_inputs(i):
    pad, valid = PACKED_PREFILL[i]
    return prefill_inputs(pad, valid, seed=51 + i), pad


# 3d. legacy row attention (IXTTS_ROWS_ATTN=legacy, a fresh process): the T = 129 latent cases and the 65-row-pad prefill, sharp set
LEGACY_LATENT = (129 - LATENT_PREFIX - 2, 129 - LATENT_PREFIX)
LEGACY_PREFILL = "pad65"

# 3e. register decode, teacher-forced: prompts of 200 (1-slot engine; slot 0 of the 3-slot engine), 150 and 9 rows, 60 forced tokens
# each; with the 200-row prompt the context reaches 256 keys at step 55 (the split-S bucket edge)
DECODE_PROMPTS = (200, 150, 9)
DECODE_STEPS = 60
DECODE_CHECK = (0, 1, 54, 55, 56, 59)


def decode_inputs(i):
    """(embeds [rows, D], forced ids [60]) of sequence i."""
    g = torch.Generator().manual_seed(71 + i)
    forced = torch.randint(0, 8192, (DECODE_STEPS,), generator=g)
    forced[:8] = torch.tensor([7, 8193 - 5, 4000, 17, 17, 256, 8191, 3])
    return _randn(61 + i, DECODE_PROMPTS[i]), forced.tolist()


# ------------------------------------------------------------------------------------------------------------ errors, limits
def rel_err(got, ref):
    """(max |got - ref| / max |ref|, rms(got - ref) / rms(ref)) against the twin's fp64 `ref`."""
    d = torch.as_tensor(got).double().cpu() - ref
    return d.abs().max().item() / ref.abs().max().item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def limits(base, floor=0.0):
    """(max, rms) a device path may reach, from the yardstick's (max, rms) on the same inputs; `floor`: the rms floor (see `Legs`)."""
    return MAX_FACTOR * base[0], max(RMS_FACTOR * base[1], floor)


def run_family(family, kind, t):
    """The cases of one family through the twin `t`: {key: fp64 / fp32 CPU tensor}.  Keys: ("latent", n), ("prefill", case),
    ("packed_latent", i), ("packed_prefill", i), ("decode", i, step)."""
    out = {}
    if family == "latent":
        prefix, codes = latent_inputs()
        a = t.latent(prefix, codes[:max(latent_counts(kind))])
        for n in latent_counts(kind):  # (causal: rows [:n] of the long pass are the pass of n codes)
            out["latent", n] = a[:n]
    elif family == "prefill":
        for name, (pad, valid) in PREFILL_CASES.items():
            out["prefill", name] = t.prefill(prefill_inputs(pad, valid), pad)[0]
    elif family == "packed_latent":
        for i in range(len(PACKED_LATENT)):
            out["packed_latent", i] = t.latent(*packed_latent_inputs(i))
    elif family == "packed_prefill":
        for i in range(len(PACKED_PREFILL)):
            out["packed_prefill", i] = t.prefill(*packed_prefill_inputs(i))[0]
    elif family == "decode":
        for i in range(len(DECODE_PROMPTS)):
            e, forced = decode_inputs(i)
            lg, st = t.prefill(e, 0)
            for step in range(DECODE_STEPS):
                if step in DECODE_CHECK:
                    out["decode", i, step] = lg
                if step + 1 < DECODE_STEPS:
                    lg, st = t.decode_step(forced[step], step + 1, st)
    elif family == "mutants":
        pad, valid = MUTANT_PREFILL
        out["mutants", "prefill"] = t.prefill(prefill_inputs(pad, valid), pad)[0]
        prefix, codes = latent_inputs()
        out["mutants", "latent"] = t.latent(prefix, codes[:MUTANT_LATENT])
    else:
        raise KeyError(family)
    return out


FAMILIES = ("latent", "prefill", "packed_latent", "packed_prefill", "decode", "mutants")


class Legs:
    """Per family the twin's results (`ref`), the two legs' errors against it (`leg32`, `flip`: key -> (max, rms); `flip` is absent in
    f32, which has no rounding site) and the yardstick (`base`, the larger of the two) of one (kind, wset), computed on first use."""

    def __init__(self, kind, wset):
        self.kind, self.wset = kind, wset
        self.cfg, self.W = config(), weights(wset)
        self.ref, self.base, self.leg32, self.flip, self.clean32, self.n_flipped = {}, {}, {}, {}, {}, {}
        self._done = set()

    def twin(self, dtype=torch.float64, mutant=None, tape=None):
        return Twin(self.W, self.cfg, self.kind, dtype, mutant, tape)

    @torch.no_grad()
    def need(self, family):
        if family in self._done:
            return self
        self._done.add(family)
        ref = run_family(family, self.kind, self.twin())
        leg = run_family(family, self.kind, self.twin(torch.float32))
        self.ref.update(ref)
        for k in ref:
            self.leg32[k] = self.base[k] = rel_err(leg[k], ref[k])
        if ROWS_SITES[self.kind]:
            ta, tb = Tape("record"), Tape("record")
            clean64 = run_family(family, self.kind, self.twin(tape=ta))
            clean32 = run_family(family, self.kind, self.twin(torch.float32, tape=tb))
            tf = Tape("flip", Tape.sigmas(ta, tb))
            flip = run_family(family, self.kind, self.twin(tape=tf))
            assert tf.i == len(tf.sigma)
            self.n_flipped[family] = tf.flipped
            for k in ref:
                self.clean32[k] = rel_err(clean32[k], clean64[k])  # the fp32 arithmetic alone, no rounding to flip
                self.flip[k] = rel_err(flip[k], ref[k])
                self.base[k] = tuple(max(x, y) for x, y in zip(self.leg32[k], self.flip[k]))
        else:
            self.clean32.update({k: self.leg32[k] for k in ref})
        return self

    @torch.no_grad()
    def mutant(self, name):
        """The "mutants" cases through the twin with one structural error: {key: result}."""
        return run_family("mutants", self.kind, self.twin(mutant=name))

    def limits(self, key):
        """(max, rms) limit of one case: 3 x its yardstick's max; 2 x its rms, but no less than 2 x the largest yardstick rms among the
        cases of its family."""
        self.need(key[0])
        floor = RMS_FACTOR * max(b[1] for k, b in self.base.items() if k[0] == key[0])
        return limits(self.base[key], floor)


_LEGS = {}


def legs(kind, wset):
    if (kind, wset) not in _LEGS:
        _LEGS[kind, wset] = Legs(kind, wset)
    return _LEGS[kind, wset]


# ------------------------------------------------------------------------------------------------------------ the device
_ENGINES = {}


def engine(kind, wset, max_batch, device="cuda:0"):
    """One engine per (type, weight set, slots), kept for the process."""
    from voice_tts_amd.gpt_engine import GptEngine

    key = (kind, wset, max_batch, str(device))
    if key not in _ENGINES:
        _ENGINES[key] = GptEngine(config(), dtype=kind, max_seq=MAX_SEQ, max_batch=max_batch, device=device).load_state_dict(weights(wset))
    return _ENGINES[key]


def device_latent(eng, n):
    prefix, codes = latent_inputs()
    return eng.latent(prefix, codes[:n]).cpu()


def device_prefill(eng, name, slot=0):
    pad, valid = PREFILL_CASES[name]
    eng.prefill(slot, prefill_inputs(pad, valid), pad)
    return torch.from_numpy(eng.read_logits(slot))


def device_packed_latent(eng):
    return [t.cpu() for t in eng.latent_many([packed_latent_inputs(i) for i in range(len(PACKED_LATENT))])]


def device_packed_prefill(eng):
    """prefill_many into slots 3, 0, 2, 1 (any order is allowed), then each slot's logits, in the order of PACKED_PREFILL."""
    slots = (3, 0, 2, 1)
    eng.prefill_many([(slots[i],) + packed_prefill_inputs(i) for i in range(len(PACKED_PREFILL))])
    return [torch.from_numpy(eng.read_logits(s)) for s in slots]


def device_decode(eng, n_slots):
    """Teacher-forced decode of sequences 0 .. n_slots - 1 on `eng`: {(i, step): logits} at DECODE_CHECK."""
    seqs = [decode_inputs(i) for i in range(n_slots)]
    for b, (e, _) in enumerate(seqs):
        eng.prefill(b, e, 0)
    out = {}
    for step in range(DECODE_STEPS):
        if step in DECODE_CHECK:
            for b in range(n_slots):
                out[b, step] = torch.from_numpy(eng.read_logits(b))
        if step + 1 < DECODE_STEPS:
            for b, (_, forced) in enumerate(seqs):
                eng.force_next(b, forced[step])
            eng.decode(n_slots, 1, repetition_penalty=10.0)
    return out


def report(what, L, key, err, lim):
    leg, flip = L.leg32[key], L.flip.get(key)
    print(f"gpt budget {what} [{L.kind} {L.wset}]: device max {err[0]:.3e} rms {err[1]:.3e} | yardstick: fp32 CPU leg max {leg[0]:.3e} rms {leg[1]:.3e}"
          + (f", flip leg max {flip[0]:.3e} rms {flip[1]:.3e}" if flip else "") + f" | limit max {lim[0]:.3e} rms {lim[1]:.3e}", flush=True)


def within(what, L, key, got):
    """Print the device error of `got` beside its yardstick, then assert the limits.  -> (max, rms)."""
    L.need(key[0])
    err, base, lim = rel_err(got, L.ref[key]), L.base[key], L.limits(key)
    report(what, L, key, err, lim)
    clean = L.clean32[key]  # (the fp32 arithmetic itself, before any 16-bit rounding can flip: noise, not a broken CPU leg)
    assert 0.0 < clean[0] < 1e-5 and 0.0 < clean[1] < 1e-5, clean
    assert err[0] <= lim[0], (what, err, base)
    assert err[1] <= lim[1], (what, err, base)
    return err
