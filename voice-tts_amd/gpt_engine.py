"""Seam 1: the decode engine that stands where DeepSpeed's injected model stands.

Mirrors the surface `UnifiedVoice.inference_speech` uses on `self.inference_model`
(indextts/gpt/model_v2.py:698,724-729): `store_mel_emb(embeds)` then
`generate(inputs, bos_token_id, pad_token_id, eos_token_id, attention_mask, max_length,
logits_processor, num_return_sequences, **hf_generate_kwargs)` returning a LongTensor
`[num_return_sequences, P + n]`; plus the latent forward of `UnifiedVoice.forward`
(model_v2.py:554-596).  All arithmetic runs in libixtts_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .weights import GPT_CFG

# weight (and K/V cache) types of the engine -> ixtts_gpt_cfg.weight_dtype (include/ixtts_hip.h)
GPT_DTYPES = {"f32": 0, "bf16": 1, "f16": 2}


def _dtype_code(dtype):
    if dtype not in GPT_DTYPES:
        raise ValueError(f"GPT weight dtype {dtype!r}: expected one of " + ", ".join(GPT_DTYPES))
    return GPT_DTYPES[dtype]


def resolve_gpt_dtype(use_fp16, gpt_dtype=None, env=None):
    """The GPT's weight type for a model built with `use_fp16`: an explicit `gpt_dtype` wins, then `IXTTS_GPT_DTYPE` (read from
    `env`, default the process environment), then the default -- bf16 under `use_fp16`, f32 otherwise.  `f16` is the
    reference's own precision under `use_fp16=True` (IEEE half).  Anything but f32 / bf16 / f16 raises ValueError."""
    import os

    if gpt_dtype is None:
        gpt_dtype = (os.environ if env is None else env).get("IXTTS_GPT_DTYPE") or None
        if gpt_dtype is not None:
            gpt_dtype = gpt_dtype.strip().lower()
    if gpt_dtype is None:
        return "bf16" if use_fp16 else "f32"
    _dtype_code(gpt_dtype)
    return gpt_dtype


GPT_TENSOR_PREFIXES = ("gpt.h.", "gpt.ln_f.", "final_norm.", "mel_head.", "mel_embedding.", "mel_pos_embedding.")


CONSTRAINT_KEYS = ("min_new_tokens", "min_length", "no_repeat_ngram_size", "suppress_tokens", "begin_suppress_tokens", "min_p")


def generation_constraints(kwargs, prompt_len=None):
    """The constraint keywords of HF `generate()` out of `kwargs` (popped; None counts as not given) -> (cfg, bans): `cfg` holds
    the engine's keyword names `min_new_tokens`, `no_repeat_ngram_size`, `min_p` -- only those that were given and are not off --
    and `bans` is `(suppress_tokens, begin_suppress_tokens)` as tuples of ints, or None when neither list holds an id.
    `min_length=L` means `min_new_tokens = max(0, L - prompt_len)`; `min_new_tokens` wins when both are given
    (generation_utils.py:1445-1453).  With `prompt_len=None` (a caller whose segments differ in prompt length) a surviving
    `min_length` is handed back under its own name for `resolve_min_length`."""
    got = {k: kwargs.pop(k) for k in CONSTRAINT_KEYS if k in kwargs}
    got = {k: v for k, v in got.items() if v is not None}
    cfg = {}
    if "min_new_tokens" in got:
        if int(got["min_new_tokens"]):
            cfg["min_new_tokens"] = int(got["min_new_tokens"])
    elif "min_length" in got:
        if prompt_len is None:
            cfg["min_length"] = int(got["min_length"])
        elif int(got["min_length"]) - int(prompt_len) > 0:
            cfg["min_new_tokens"] = int(got["min_length"]) - int(prompt_len)
    if int(got.get("no_repeat_ngram_size", 0)):
        cfg["no_repeat_ngram_size"] = int(got["no_repeat_ngram_size"])
    if float(got.get("min_p", 0.0)) != 0.0:
        cfg["min_p"] = float(got["min_p"])
    lists = tuple(tuple(int(t) for t in np.asarray(got.get(k, ()), dtype=np.int64).reshape(-1)) for k in ("suppress_tokens", "begin_suppress_tokens"))
    return cfg, (lists if lists[0] or lists[1] else None)


def resolve_min_length(cfg, prompt_len):
    """`cfg` of `generation_constraints(..., prompt_len=None)` for a sequence whose prompt holds `prompt_len` ids: `min_length`
    turned into that sequence's `min_new_tokens` (left out when it asks for nothing)."""
    if "min_length" not in cfg:
        return cfg
    out = {k: v for k, v in cfg.items() if k != "min_length"}
    m = int(cfg["min_length"]) - int(prompt_len)
    if m > 0:
        out["min_new_tokens"] = m
    return out


PROCESSOR_KEYS = ("sequence_bias", "bad_words_ids", "forced_eos_token_id", "exponential_decay_length_penalty", "epsilon_cutoff", "eta_cutoff",
                  "renormalize_logits")


def _is_id(t):
    return isinstance(t, (int, np.integer)) and not isinstance(t, bool) and t >= 0


def sequence_bias_table(sequence_bias=None, bad_words_ids=None, eos_token_id=None, vocab=None):
    """`sequence_bias` ({tuple(ids): float} or HF's list form [[[ids], bias], ...]) and `bad_words_ids` ([[ids], ...]) of HF
    `generate()` -> the sequence's table for `ixtts_gpt_set_sequence_bias`: a list of (ids tuple, bias), the biased sequences
    first, then the bad words with a bias of -inf (entries equal to `[eos_token_id]` dropped, as NoBadWordsLogitsProcessor
    drops them).  None = not given.  Checked as HF checks them (SequenceBiasLogitsProcessor._validate_arguments,
    NoBadWordsLogitsProcessor._validate_arguments), ids against `vocab` too, and against the table's limits: ValueError."""
    table = []
    if sequence_bias is not None:
        sb = sequence_bias
        if not isinstance(sb, (dict, list)) or len(sb) == 0:
            raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
        if isinstance(sb, list):
            for item in sb:
                if not (isinstance(item, (list, tuple)) and len(item) == 2 and isinstance(item[0], (list, tuple))):
                    raise ValueError(f"Each element in `sequence_bias` has to be a list of a non-empty list of ids and a float, but is {item}.")
            sb = {tuple(item[0]): item[1] for item in sb}
        for ids, bias in sb.items():
            if not isinstance(ids, tuple) or len(ids) == 0 or not all(_is_id(t) for t in ids):
                raise ValueError(f"Each sequence in `sequence_bias` has to be a non-empty tuple of non-negative integers, but is {ids}.")
            if not isinstance(bias, (float, np.floating)) or bias != bias:
                raise ValueError(f"`sequence_bias` has to hold floats as biases, but {ids} has {bias!r}.")
            table.append((tuple(int(t) for t in ids), float(bias)))
    if bad_words_ids is not None:
        bw = bad_words_ids
        if not isinstance(bw, list) or len(bw) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
        if any(not isinstance(w, list) for w in bw):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
        if any(len(w) == 0 or not all(_is_id(t) for t in w) for w in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a non-empty list of non-negative integers, but is {bw}.")
        eos = eos_token_id.tolist() if torch.is_tensor(eos_token_id) else eos_token_id
        eos = [] if eos is None else [int(e) for e in np.asarray(eos).reshape(-1)]
        words = {tuple(int(t) for t in w): None for w in bw if all(list(w) != [e] for e in eos)}
        table.extend((w, float("-inf")) for w in words)
    if len(table) > _lib.SEQ_BIAS_MAX:
        raise ValueError(f"`sequence_bias` and `bad_words_ids` hold {len(table)} sequences together: the table of a sequence holds at most "
                         f"IXTTS_SEQ_BIAS_MAX = {_lib.SEQ_BIAS_MAX}")
    for ids, _ in table:
        if len(ids) > _lib.SEQ_BIAS_LEN:
            raise ValueError(f"sequence {ids} holds {len(ids)} ids: at most IXTTS_SEQ_BIAS_LEN = {_lib.SEQ_BIAS_LEN}")
        if vocab is not None and any(t >= vocab for t in ids):
            raise ValueError(f"sequence {ids}: id outside 0..{int(vocab) - 1}")
    return table


def generation_processors(kwargs, eos_token_id, vocab=None):
    """The other processor keywords of HF `generate()` out of `kwargs` (popped; None counts as not given) -- `sequence_bias`,
    `bad_words_ids`, `forced_eos_token_id`, `exponential_decay_length_penalty`, `epsilon_cutoff`, `eta_cutoff`,
    `renormalize_logits` -> (cfg, state).  `cfg` holds the engine's keyword names `exp_decay_start`, `exp_decay_factor`,
    `epsilon_cutoff`, `eta_cutoff`, `renormalize_logits` -- only those that were given and are not off.  `state` is what belongs
    to the sequence's slot, or None: a dict with `table` (`sequence_bias_table`'s list, for `set_sequence_bias`) and `forced_eos`
    (the forced ids, for `set_forced_eos`; the step they are forced at, `forced_eos_step` = the sequence's own max_new, is the
    caller's to add to the cfg).  `vocab`: ids must lie below it.  A bad value raises ValueError, as HF's classes do."""
    got = {k: kwargs.pop(k) for k in PROCESSOR_KEYS if k in kwargs}
    got = {k: v for k, v in got.items() if v is not None}
    cfg = {}
    for k in ("epsilon_cutoff", "eta_cutoff"):
        if k in got:
            v = float(got[k])
            if not 0.0 <= v < 1.0:
                raise ValueError(f"`{k}` has to be a float >= 0 (off) and < 1, but is {got[k]}")
            if v > 0.0:
                cfg[k] = v
    if "exponential_decay_length_penalty" in got:
        pen = got["exponential_decay_length_penalty"]
        if not isinstance(pen, (tuple, list)) or len(pen) != 2:
            raise ValueError(f"`exponential_decay_length_penalty` has to be (start_index, decay_factor), but is {pen}")
        start, factor = pen
        if not _is_id(start):
            raise ValueError(f"`exponential_decay_length_penalty`: start_index has to be an integer >= 0, but is {start!r}")
        if isinstance(factor, bool) or not isinstance(factor, (int, float, np.integer, np.floating)) or not 0.0 < float(factor) < float("inf"):
            raise ValueError(f"`exponential_decay_length_penalty`: decay_factor has to be a finite number > 0, but is {factor!r}")
        cfg["exp_decay_start"], cfg["exp_decay_factor"] = int(start), float(factor)
    if got.get("renormalize_logits") is True:  # (`is True`, as generation_utils.py:1068 tests it)
        cfg["renormalize_logits"] = True
    table = sequence_bias_table(got.get("sequence_bias"), got.get("bad_words_ids"), eos_token_id, vocab)
    forced = ()
    if "forced_eos_token_id" in got:
        f = got["forced_eos_token_id"]
        f = [f] if isinstance(f, (int, np.integer)) and not isinstance(f, bool) else f
        if not isinstance(f, (list, tuple)) or len(f) == 0 or not all(_is_id(t) for t in f):
            raise ValueError(f"`forced_eos_token_id` has to be a non-negative integer or a non-empty list of them, but is {got['forced_eos_token_id']}")
        if vocab is not None and any(t >= vocab for t in f):
            raise ValueError(f"`forced_eos_token_id` {list(f)}: id outside 0..{int(vocab) - 1}")
        forced = tuple(int(t) for t in f)
    state = dict(table=table, forced_eos=forced) if table or forced else None
    return cfg, state


class GptEngine:
    def __init__(self, cfg=None, dtype="f32", max_seq=2048, max_batch=1, device=None):
        code = _dtype_code(dtype)
        cfg = dict(GPT_CFG if cfg is None else cfg)
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda:0")
        self.dtype = dtype
        c = _lib.GptCfg()
        c.model_dim = cfg["model_dim"]
        c.layers = cfg["layers"]
        c.heads = cfg["heads"]
        c.n_mel_codes = cfg["number_mel_codes"]
        c.n_mel_pos = cfg["max_mel_tokens"] + 3
        c.n_text_tokens = cfg["number_text_tokens"] + 1
        c.n_text_pos = cfg["max_text_tokens"] + 2
        c.start_mel_token = cfg["start_mel_token"]
        c.stop_mel_token = cfg["stop_mel_token"]
        c.max_seq = max_seq
        c.max_batch = max_batch
        c.weight_dtype = code
        self._c = c
        self.max_seq = max_seq
        self.max_batch = max_batch
        self.D = cfg["model_dim"]
        self.V = cfg["number_mel_codes"]
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_create(C.byref(self._h), C.byref(c)), "ixtts_gpt_create")
        self._loaded = False
        self.cached_mel_emb = None

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd):
        """Feed the engine from a `UnifiedVoice.state_dict()`-style mapping (fp32 host tensors)."""
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for name, t in sd.items():
                if not name.startswith(GPT_TENSOR_PREFIXES):
                    continue
                t = t.detach().to("cpu", torch.float32).contiguous()
                shape = (C.c_int64 * t.dim())(*t.shape)
                _lib.check(L.ixtts_gpt_set_tensor(self._h, name.encode(), t.data_ptr(), shape, t.dim()), f"ixtts_gpt_set_tensor({name})")
            _lib.check(L.ixtts_gpt_finalize(self._h), "ixtts_gpt_finalize")
        self._loaded = True
        return self

    def arena(self):
        p, n = C.c_void_p(), C.c_size_t()
        _lib.check(_lib.lib().ixtts_gpt_arena(self._h, C.byref(p), C.byref(n)), "ixtts_gpt_arena")
        return p.value, n.value

    def adopt_arena(self):
        _lib.check(_lib.lib().ixtts_gpt_adopt_arena(self._h), "ixtts_gpt_adopt_arena")
        self._loaded = True

    def share_arena(self, owner):
        """Read `owner`'s device weights instead of holding a copy (same model, same dtype): a second engine shape -- e.g. the
        wide beam-group engine beside the register engine -- costs its KV cache only."""
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_share_arena(self._h, owner._h), "ixtts_gpt_share_arena")
        self._owner = owner  # keep it alive
        self._loaded = True
        return self

    # ------------------------------------------------------------------ low level
    def _stream(self):
        return _lib.current_stream_ptr()

    def prefill(self, slot, embeds, n_left_pad=0):
        """embeds [P-1, D] fp32 (cond + text rows, left-padded with zero rows)."""
        e = embeds.to(self.device, torch.float32).contiguous()
        assert e.dim() == 2 and e.shape[1] == self.D
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_prefill(self._h, slot, e.data_ptr(), e.shape[0], int(n_left_pad), self._stream())
        _lib.check(rc, "ixtts_gpt_prefill")
        self._keep = e  # keep alive until the stream has consumed it

    def prefill_many(self, entries, rows_max=0):
        """`prefill` of several sequences into several slots in one packed pass per layer: entries = [(slot, embeds, n_left_pad),
        ...], any slots in any order, none twice.  Every slot ends bit for bit as `prefill(slot, embeds, n_left_pad)` alone
        leaves it; slots not named are untouched.  `rows_max` caps the packed rows of a pass (0: what the workspaces hold,
        max_seq): more passes, the same bits."""
        entries = list(entries)
        n = len(entries)
        keep = []
        for slot, embeds, n_left_pad in entries:
            e = embeds.to(self.device, torch.float32).contiguous()
            assert e.dim() == 2 and e.shape[1] == self.D
            keep.append(e)
        slots = (C.c_int * max(n, 1))(*[int(s) for s, _, _ in entries])
        ptrs = (C.c_void_p * max(n, 1))(*[e.data_ptr() for e in keep])
        rows = (C.c_int * max(n, 1))(*[int(e.shape[0]) for e in keep])
        pads = (C.c_int * max(n, 1))(*[int(p) for _, _, p in entries])
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_prefill_many(self._h, n, slots, ptrs, rows, pads, int(rows_max), self._stream())
        _lib.check(rc, "ixtts_gpt_prefill_many")
        if keep:
            self._keep_many = keep  # keep alive until the stream has consumed them

    @staticmethod
    def prefill_plan(n_rows, n_left_pad, row_cap):
        """The passes `prefill_many` cuts a list of prompts into (host arithmetic, no GPU): -> (pass index of each, pass count)."""
        n = len(n_rows)
        assert len(n_left_pad) == n
        out = (C.c_int * max(n, 1))()
        rc = _lib.lib().ixtts_gpt_prefill_plan((C.c_int * max(n, 1))(*map(int, n_rows)), (C.c_int * max(n, 1))(*map(int, n_left_pad)), n, int(row_cap), out)
        if rc < 0:
            _lib.check(rc, "ixtts_gpt_prefill_plan")
        return list(out[:n]), rc

    @staticmethod
    def _sampler_cfg(v):
        """One SamplerCfg from a dict with every keyword of `decode()` / `beam_decode()` (`length_penalty` may be missing)."""
        return _lib.SamplerCfg(v["repetition_penalty"], v["temperature"], int(v["top_k"]), v["top_p"], int(bool(v["do_sample"])),
                               int(bool(v["suppress_stop"])), int(v["seed"]), float(v["typical_mass"]), float(v.get("length_penalty", 0.0)),
                               int(v["min_new_tokens"]), int(v["no_repeat_ngram_size"]), float(v["min_p"]),
                               int(v["exp_decay_start"]), float(v["exp_decay_factor"]), float(v["epsilon_cutoff"]), float(v["eta_cutoff"]),
                               int(bool(v["renormalize_logits"])), int(v["forced_eos_step"]), 0)

    def decode(self, n_active, n_steps, repetition_penalty=10.0, temperature=1.0, top_k=0, top_p=1.0,
               do_sample=False, suppress_stop=False, seed=0, typical_mass=0.0, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0,
               exp_decay_start=0, exp_decay_factor=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, renormalize_logits=False, forced_eos_step=0):
        """`min_new_tokens`, `no_repeat_ngram_size`, `min_p`: the processors HF `generate()` builds from the keywords of the same
        names (0 = off; `min_p` acts when sampling only); the two id lists of the family belong to the slot: `set_bans`.
        `exp_decay_start`, `exp_decay_factor`: `exponential_decay_length_penalty=(start_index, factor)` (factor 0 = off);
        `epsilon_cutoff`, `eta_cutoff`: the two truncation samplers (sampling only); `renormalize_logits` (no effect without
        beams); `forced_eos_step=N`: the N-th generated token is one of the slot's forced ids (`set_forced_eos`; HF's
        `forced_eos_token_id` with N = max_length - prompt length).  The table of `sequence_bias` / `bad_words_ids` belongs to the
        slot: `set_sequence_bias`."""
        sc = self._sampler_cfg(dict(repetition_penalty=repetition_penalty, temperature=temperature, top_k=top_k, top_p=top_p, do_sample=do_sample,
                                    suppress_stop=suppress_stop, seed=seed, typical_mass=typical_mass, min_new_tokens=min_new_tokens,
                                    no_repeat_ngram_size=no_repeat_ngram_size, min_p=min_p, exp_decay_start=exp_decay_start,
                                    exp_decay_factor=exp_decay_factor, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff,
                                    renormalize_logits=renormalize_logits, forced_eos_step=forced_eos_step))
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_decode(self._h, n_active, n_steps, C.byref(sc), self._stream())
        _lib.check(rc, "ixtts_gpt_decode")

    _DECODE_KEYS = dict(repetition_penalty=10.0, temperature=1.0, top_k=0, top_p=1.0, do_sample=False, suppress_stop=False, seed=0,
                        typical_mass=0.0, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0, exp_decay_start=0, exp_decay_factor=0.0,
                        epsilon_cutoff=0.0, eta_cutoff=0.0, renormalize_logits=False, forced_eos_step=0)
    _BEAM_KEYS = dict(repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, suppress_stop=False, seed=0, typical_mass=0.0,
                      length_penalty=0.0, do_sample=True, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0, exp_decay_start=0,
                      exp_decay_factor=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, renormalize_logits=False, forced_eos_step=0)

    @staticmethod
    def _sampler_array(cfgs, defaults, what):
        """A list of dicts (the keyword names and defaults of `decode()` / `beam_decode()`) -> a ctypes array of SamplerCfg."""
        arr = (_lib.SamplerCfg * len(cfgs))()
        for i, cfg in enumerate(cfgs):
            unknown = set(cfg) - set(defaults)
            if unknown:
                raise TypeError(f"{what}: entry {i} has unexpected keys {sorted(unknown)}")
            v = {**defaults, **cfg}
            arr[i] = GptEngine._sampler_cfg(v)
        return arr

    def decode_slots(self, n_steps, cfgs, streams=None):
        """`decode()` with the settings and the random stream belonging to each sequence: slots 0..len(cfgs)-1 step together,
        slot b under `cfgs[b]` (a dict with `decode()`'s keyword names; what it leaves out takes `decode()`'s default) and drawing
        from stream `streams[b]` (None: the slot index, as `decode()` does)."""
        n = len(cfgs)
        arr = self._sampler_array(cfgs, self._DECODE_KEYS, "decode_slots")
        st = None
        if streams is not None:
            assert len(streams) == n, (len(streams), n)
            st = (C.c_uint32 * n)(*[int(s) for s in streams])
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_decode_slots(self._h, n, n_steps, arr, st, self._stream())
        _lib.check(rc, "ixtts_gpt_decode_slots")

    def read(self, slot):
        ids = np.zeros(self.max_seq, dtype=np.int32)
        n, fin = C.c_int(), C.c_int()
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_read(self._h, slot, ids.ctypes.data, ids.size, C.byref(n), C.byref(fin), self._stream())
        _lib.check(rc, "ixtts_gpt_read")
        return ids[: n.value].copy(), bool(fin.value)

    def read_logits(self, slot):
        out = np.zeros(self.V, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_read_logits(self._h, slot, out.ctypes.data, self._stream()), "ixtts_gpt_read_logits")
        return out

    def read_probs(self, slot):
        out = np.zeros(self.V, dtype=np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_read_probs(self._h, slot, out.ctypes.data, self._stream()), "ixtts_gpt_read_probs")
        return out

    def set_bans(self, slot, suppress_tokens=(), begin_suppress_tokens=()):
        """`suppress_tokens` (ids banned at every step) and `begin_suppress_tokens` (at the first generated token only) of the
        sequence in `slot`, as HF `generate()` takes them.  Call it after the slot's `prefill` (which clears them) and before its
        first decode step; with beams, on the group's first slot.  An id outside the vocabulary raises IxttsError."""
        a = np.ascontiguousarray(np.asarray(list(suppress_tokens), dtype=np.int64).astype(np.int32).reshape(-1))
        f = np.ascontiguousarray(np.asarray(list(begin_suppress_tokens), dtype=np.int64).astype(np.int32).reshape(-1))
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_set_bans(self._h, int(slot), a.ctypes.data if a.size else None, a.size, f.ctypes.data if f.size else None, f.size,
                                               self._stream())
        _lib.check(rc, "ixtts_gpt_set_bans")

    def set_sequence_bias(self, slot, sequence_bias=None, bad_words_ids=None):
        """`sequence_bias` ({tuple(ids): float} or [[[ids], bias], ...]) and `bad_words_ids` ([[ids], ...]) of the sequence in
        `slot`, as HF `generate()` takes them -- or a table `sequence_bias_table` made already (a list of (ids tuple, bias)) as
        `sequence_bias`.  They share one table of at most 64 sequences of at most 8 ids; a bad word equal to [stop token] is
        dropped.  Call it after the slot's `prefill` (which clears the table) and before its first decode step; with beams, on
        the group's first slot.  ValueError for what HF refuses and for the limits."""
        made = isinstance(sequence_bias, list) and bad_words_ids is None and all(isinstance(e, tuple) and len(e) == 2 and isinstance(e[0], tuple) for e in sequence_bias)
        try:
            if made:  # (the same checks; entries on one sequence, a bias and a bad word, stay two entries)
                table = list(sequence_bias)
                sequence_bias_table(dict(table) or None, None, None, self.V)
                if len(table) > _lib.SEQ_BIAS_MAX:
                    raise ValueError(f"{len(table)} sequences: the table of a sequence holds at most IXTTS_SEQ_BIAS_MAX = {_lib.SEQ_BIAS_MAX}")
            else:
                table = sequence_bias_table(sequence_bias, bad_words_ids, self.cfg["stop_mel_token"], self.V)
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        flat = np.ascontiguousarray(np.asarray([t for ids, _ in table for t in ids], dtype=np.int32))
        lens = np.ascontiguousarray(np.asarray([len(ids) for ids, _ in table], dtype=np.int32))
        bias = np.ascontiguousarray(np.asarray([b for _, b in table], dtype=np.float32))
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_set_sequence_bias(self._h, int(slot), flat.ctypes.data if flat.size else None, lens.ctypes.data if lens.size else None,
                                                        bias.ctypes.data if bias.size else None, len(table), self._stream())
        _lib.check(rc, "ixtts_gpt_set_sequence_bias")

    def set_forced_eos(self, slot, forced_eos_token_id=()):
        """`forced_eos_token_id` (an id or a list of ids) of the sequence in `slot`: what the `forced_eos_step`-th generated token
        is forced to.  After the slot's `prefill`, which clears it; with beams, on the group's first slot."""
        f = forced_eos_token_id
        f = [f] if isinstance(f, (int, np.integer)) else list(f)
        if not all(_is_id(t) and t < self.V for t in f):
            raise ValueError(f"slot {slot}: forced_eos_token_id {f}: ids must lie in 0..{self.V - 1}")
        a = np.ascontiguousarray(np.asarray(f, dtype=np.int32).reshape(-1))
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_set_forced_eos(self._h, int(slot), a.ctypes.data if a.size else None, a.size, self._stream())
        _lib.check(rc, "ixtts_gpt_set_forced_eos")

    def set_processors(self, slot, state):
        """What `generation_processors` returned as `state`, onto `slot` (after its prefill)."""
        if state is None:
            return
        if state.get("table"):
            self.set_sequence_bias(slot, list(state["table"]))
        if state.get("forced_eos"):
            self.set_forced_eos(slot, state["forced_eos"])

    def force_next(self, slot, token):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_force_next(self._h, slot, int(token), self._stream()), "ixtts_gpt_force_next")

    # ------------------------------------------------------------------ beam-sample
    # Group g = the beams of one prompt (prefilled into slot g * num_beams); groups step together on a wide engine.
    def beam_begin(self, num_beams, group=0, rng_stream=0):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_beam_begin_group(self._h, int(group), int(num_beams), int(rng_stream), self._stream()), "ixtts_gpt_beam_begin_group")
        self._nb = int(num_beams)

    def beam_park(self, group):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_beam_park_group(self._h, int(group), self._stream()), "ixtts_gpt_beam_park_group")

    def beam_decode(self, n_steps, repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, suppress_stop=False, seed=0, typical_mass=0.0,
                    length_penalty=0.0, groups=1, do_sample=True, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0,
                    exp_decay_start=0, exp_decay_factor=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, renormalize_logits=False, forced_eos_step=0):
        """`do_sample=False`: beam search proper -- the joint top 2 * num_beams instead of the multinomial draw, no warpers (`min_p`,
        `epsilon_cutoff` and `eta_cutoff` are three of them).  `no_repeat_ngram_size` and the table of `set_sequence_bias` look at
        each beam's own history.  `renormalize_logits` shifts each beam's candidate scores by the logsumexp over its surviving
        scores (beam search proper: over its whole processed row)."""
        sc = self._sampler_cfg(dict(repetition_penalty=repetition_penalty, temperature=temperature, top_k=top_k, top_p=top_p, do_sample=do_sample,
                                    suppress_stop=suppress_stop, seed=seed, typical_mass=typical_mass, length_penalty=length_penalty,
                                    min_new_tokens=min_new_tokens, no_repeat_ngram_size=no_repeat_ngram_size, min_p=min_p,
                                    exp_decay_start=exp_decay_start, exp_decay_factor=exp_decay_factor, epsilon_cutoff=epsilon_cutoff,
                                    eta_cutoff=eta_cutoff, renormalize_logits=renormalize_logits, forced_eos_step=forced_eos_step))
        self._lp = [float(length_penalty)] * int(groups)  # per group
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_beam_decode_groups(self._h, int(groups), n_steps, C.byref(sc), self._stream()), "ixtts_gpt_beam_decode_groups")

    def beam_decode_groups(self, n_steps, cfgs):
        """`beam_decode(groups=len(cfgs))` with one cfg per group: group g steps under `cfgs[g]` (a dict with `beam_decode()`'s
        keyword names but `groups`; what it leaves out takes `beam_decode()`'s default), `beam_read(group=g)` finalizes with its own
        length penalty.  The groups' random streams are the ones `beam_begin` gave them."""
        arr = self._sampler_array(cfgs, self._BEAM_KEYS, "beam_decode_groups")
        self._lp = [float(a.length_penalty) for a in arr]  # per group
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_beam_decode_groups_cfg(self._h, len(cfgs), n_steps, arr, self._stream()), "ixtts_gpt_beam_decode_groups_cfg")

    def beam_force(self, picks, group=0):
        a = np.ascontiguousarray(np.asarray(picks, dtype=np.int32))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_beam_force_group(self._h, int(group), a.ctypes.data, a.size, self._stream()), "ixtts_gpt_beam_force_group")

    def beam_read(self, max_new, group=0):
        ids = np.zeros(self.max_seq + 1, dtype=np.int32)
        n, done, score = C.c_int(), C.c_int(), C.c_float()
        bs = np.zeros(self._nb, np.float32)
        lt = np.zeros(self._nb, np.int32)
        src = np.zeros(self._nb, np.int32)
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_beam_read_group(self._h, int(group), int(max_new), ids.ctypes.data, ids.size, C.byref(n), C.byref(done), C.byref(score),
                                                      bs.ctypes.data, lt.ctypes.data, src.ctypes.data, self._stream())
        _lib.check(rc, "ixtts_gpt_beam_read_group")
        return ids[: n.value].copy(), bool(done.value), float(score.value), bs, lt, src

    def latent(self, prefix, codes):
        """prefix [34+L+2, D] fp32 (conds ; text_emb); codes int [n] -> latent [n, D] (model_v2.py:554-596)."""
        p = prefix.to(self.device, torch.float32).contiguous()
        c = codes.to(self.device, torch.int32).contiguous()
        out = torch.empty(c.numel(), self.D, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_latent(self._h, p.data_ptr(), p.shape[0], c.data_ptr(), c.numel(), out.data_ptr(), self._stream())
        _lib.check(rc, "ixtts_gpt_latent")
        self._keep2 = (p, c)
        return out

    def latent_many(self, entries, rows_max=0):
        """`latent` of several sequences in packed passes over the weights: entries = [(prefix [P_i, D], codes [n_i]), ...] -> a
        list of [n_i, D] fp32 tensors (views of one ragged buffer), each bit for bit what `latent(prefix, codes)` alone returns.
        No decode slot is touched and the count is not bounded by max_batch.  `rows_max` caps the cache positions of a pass (0:
        what the workspaces hold, max_seq): more passes, the same bits."""
        entries = list(entries)
        n = len(entries)
        keep = []
        for prefix, codes in entries:
            p = prefix.to(self.device, torch.float32).contiguous()
            c = torch.as_tensor(codes).to(self.device, torch.int32).contiguous().reshape(-1)
            assert p.dim() == 2 and p.shape[1] == self.D
            keep.append((p, c))
        counts = [int(c.numel()) for _, c in keep]
        buf = torch.empty(max(sum(counts), 1), self.D, device=self.device, dtype=torch.float32)
        outs, at = [], 0
        for k in counts:
            outs.append(buf[at:at + k])
            at += k
        m = max(n, 1)
        pp = (C.c_void_p * m)(*[p.data_ptr() for p, _ in keep])
        cp = (C.c_void_p * m)(*[c.data_ptr() if c.numel() else None for _, c in keep])
        op = (C.c_void_p * m)(*[o.data_ptr() if o.shape[0] else None for o in outs])
        np_ = (C.c_int * m)(*[int(p.shape[0]) for p, _ in keep])
        nc = (C.c_int * m)(*counts)
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_latent_many(self._h, n, pp, np_, cp, nc, op, int(rows_max), self._stream())
        _lib.check(rc, "ixtts_gpt_latent_many")
        if keep:
            self._keep_latents = keep  # keep alive until the stream has consumed them
        return outs

    @staticmethod
    def latent_plan(n_prefix, n_codes, row_cap):
        """The passes `latent_many` cuts a list of sequences into (host arithmetic, no GPU): -> (pass index of each, pass count)."""
        n = len(n_prefix)
        assert len(n_codes) == n
        out = (C.c_int * max(n, 1))()
        rc = _lib.lib().ixtts_gpt_latent_plan((C.c_int * max(n, 1))(*map(int, n_prefix)), (C.c_int * max(n, 1))(*map(int, n_codes)), n, int(row_cap), out)
        if rc < 0:
            _lib.check(rc, "ixtts_gpt_latent_plan")
        return list(out[:n]), rc

    def step_bytes(self, B, S):
        return _lib.lib().ixtts_gpt_step_bytes(self._h, B, S)

    def bench_gemv(self, which, layer, batch=1):
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_gpt_bench_gemv(self._h, which, layer, batch, self._stream()), "ixtts_gpt_bench_gemv")

    # ------------------------------------------------------------------ reference-shaped surface
    def store_mel_emb(self, mel_emb):
        """GPT2InferenceModel.store_mel_emb (model_v2.py:87-88)."""
        self.cached_mel_emb = mel_emb

    def generate(self, inputs, bos_token_id=None, pad_token_id=None, eos_token_id=None, attention_mask=None,
                 max_length=None, logits_processor=None, num_return_sequences=1, do_sample=True, top_p=1.0, top_k=0,
                 temperature=1.0, num_beams=1, repetition_penalty=1.0, length_penalty=0.0, sync_every=64,
                 suppress_stop=False, **unused):
        """The slice of HF `generate()` that `inference_speech` exercises (model_v2.py:724-729).

        `inputs` = fake ids [1, P] (only its length matters, model_v2.py:652-661); the
        prompt rows come from `store_mel_emb`.  Greedy == `top_k=1` or `do_sample=False`
        (SURVEY.md F3).  Host syncs once per `sync_every` steps (finished flag), not per token.
        """
        if self.cached_mel_emb is None:
            raise RuntimeError("generate(): call store_mel_emb first (model_v2.py:137)")
        if num_beams != 1 and not (2 <= num_beams <= min(self.max_batch, 4)):
            raise NotImplementedError("beam mode needs 2 <= num_beams <= min(max_batch, 4) (beam-sample, the served configuration, or with do_sample=False beam search)")
        # the one custom processor inference_speech ever builds is TypicalLogitsWarper(mass=typical_mass) (model_v2.py:717-722):
        # it runs on the device; anything else has no kernel
        typical_mass = float(unused.pop("typical_mass", 0.0)) if unused.pop("typical_sampling", False) else 0.0
        # the constraints HF builds from plain keywords (generation_utils.py:902-1049): scalars into the sampler cfg, id lists onto the slot
        cons, bans = generation_constraints(unused, inputs.shape[1])
        # the rest of that family (generation_utils.py:862-1069): scalars into the cfg, the table and the forced ids onto the slot
        procs, pstate = generation_processors(unused, eos_token_id if eos_token_id is not None else self.cfg["stop_mel_token"], self.V)
        cons = {**cons, **procs}
        for proc in (logits_processor or []):
            if type(proc).__name__ == "TypicalLogitsWarper" and hasattr(proc, "mass"):
                typical_mass = float(proc.mass)
            else:
                raise NotImplementedError(f"logits processor {type(proc).__name__} has no device implementation (only typical sampling does)")
        if inputs.shape[0] != 1:
            raise NotImplementedError("one prompt per generate() call (autoregressive_batch_size = 1, infer_v2.py:602)")
        nret = int(num_return_sequences)
        if nret != 1 and (num_beams != 1 or not (1 <= nret <= self.max_batch)):
            raise NotImplementedError("num_return_sequences > 1 is built for sampling without beams, up to max_batch sequences "
                                      "(HF expands the prompt and draws independent continuations, generation_utils.py:2128-2135)")
        greedy = (not do_sample) or top_k == 1
        if num_beams != 1 and do_sample and not (1 <= top_k <= 128):
            raise NotImplementedError("beam-sample keeps at most 128 candidates per beam on the device: 1 <= top_k <= 128 (sampling without beams takes any top_k, 0 = off)")
        top_k = max(0, int(top_k))
        P = inputs.shape[1]
        emb = self.cached_mel_emb
        emb = emb[0] if emb.dim() == 3 else emb
        assert emb.shape[0] == P - 1, (emb.shape, P)
        n_pad = 0
        if attention_mask is not None:
            m = attention_mask.reshape(-1)
            n_pad = int((m == 0).sum().item())
            assert n_pad == 0 or bool((m[:n_pad] == 0).all()), "only left padding is produced by prepare_gpt_inputs (model_v2.py:639-642)"
        max_new = (max_length - P) if max_length is not None else (self.max_seq - P - 2)
        # the mel position table bounds what can be embedded (inference_speech's own default cap: max_mel_tokens - 1, model_v2.py:699-703)
        max_new = max(0, min(max_new, self.max_seq - P - 2, self.cfg["max_mel_tokens"] - 1))
        if pstate is not None and pstate["forced_eos"] and max_new >= 1:
            # ForcedEOSTokenLogitsProcessor(max_length, ids): the token at position max_length - 1 = P + max_new - 1, the last one this
            # call can generate
            cons["forced_eos_step"] = max_new
        self.prefill(0, emb, n_pad)
        if bans is not None:
            self.set_bans(0, *bans)
        self.set_processors(0, pstate)
        if num_beams != 1:
            # served default: 3-beam beam-sample (infer_v2.py:598-605,641-658); do_sample=False: beam search (generation_utils.py:3520-3524)
            self.beam_begin(num_beams)
            done_steps, fin = 0, False
            ids = np.zeros(0, np.int32)
            while done_steps < max_new and not fin:
                n = min(sync_every, max_new - done_steps)
                self.beam_decode(n, repetition_penalty=repetition_penalty, temperature=temperature, top_k=top_k, top_p=top_p,
                                 suppress_stop=suppress_stop, seed=int(unused.get("seed", 0)), typical_mass=typical_mass, length_penalty=length_penalty,
                                 do_sample=do_sample, **cons)
                done_steps += n
                ids, fin = self.beam_read(max_new)[:2]
            out = torch.cat([inputs.reshape(1, -1).to(torch.long).cpu(), torch.from_numpy(ids.astype(np.int64)).reshape(1, -1)], dim=1)
            return out.to(inputs.device)
        if nret > 1:
            # `input_ids.repeat_interleave(num_return_sequences)`: the same prompt in nret slots, each drawing from its own stream
            # (the slot index is part of the counter-based RNG); rows are right-padded with pad_token_id as HF pads finished rows
            for b in range(1, nret):
                self.prefill(b, emb, n_pad)
                if bans is not None:
                    self.set_bans(b, *bans)
                self.set_processors(b, pstate)
            done, fins = 0, [False] * nret
            rows = [np.zeros(0, np.int32)] * nret
            while done < max_new and not all(fins):
                n = min(sync_every, max_new - done)
                self.decode(nret, n, repetition_penalty=repetition_penalty, temperature=temperature, top_k=top_k, top_p=top_p,
                            do_sample=not greedy, suppress_stop=suppress_stop, seed=int(unused.get("seed", 0)), typical_mass=typical_mass, **cons)
                done += n
                for b in range(nret):
                    rows[b], fins[b] = self.read(b)
            rows = [r[:max_new] for r in rows]
            width = max(len(r) for r in rows)
            pad = int(pad_token_id if pad_token_id is not None else self.cfg["stop_mel_token"])
            body = np.full((nret, width), pad, np.int64)
            for b, r in enumerate(rows):
                body[b, : len(r)] = r
            out = torch.cat([inputs.reshape(1, -1).to(torch.long).cpu().repeat(nret, 1), torch.from_numpy(body)], dim=1)
            return out.to(inputs.device)
        done = 0
        ids, fin = np.zeros(0, np.int32), False
        while done < max_new and not fin:
            n = min(sync_every, max_new - done)
            self.decode(1, n, repetition_penalty=repetition_penalty, temperature=temperature, top_k=top_k, top_p=top_p,
                        do_sample=not greedy, suppress_stop=suppress_stop, seed=int(unused.get("seed", 0)), typical_mass=typical_mass, **cons)
            done += n
            ids, fin = self.read(0)
        ids = ids[:max_new]
        out = torch.cat([inputs.reshape(1, -1).to(torch.long).cpu(), torch.from_numpy(ids.astype(np.int64)).reshape(1, -1)], dim=1)
        return out.to(inputs.device)

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.lib().ixtts_gpt_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass
