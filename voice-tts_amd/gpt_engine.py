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

    def decode(self, n_active, n_steps, repetition_penalty=10.0, temperature=1.0, top_k=0, top_p=1.0,
               do_sample=False, suppress_stop=False, seed=0, typical_mass=0.0, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0):
        """`min_new_tokens`, `no_repeat_ngram_size`, `min_p`: the processors HF `generate()` builds from the keywords of the same
        names (0 = off; `min_p` acts when sampling only); the two id lists of the family belong to the slot: `set_bans`."""
        sc = _lib.SamplerCfg(repetition_penalty, temperature, top_k, top_p, int(do_sample), int(suppress_stop), seed, float(typical_mass), 0.0,
                             int(min_new_tokens), int(no_repeat_ngram_size), float(min_p))
        with torch.cuda.device(self.device):
            rc = _lib.lib().ixtts_gpt_decode(self._h, n_active, n_steps, C.byref(sc), self._stream())
        _lib.check(rc, "ixtts_gpt_decode")

    _DECODE_KEYS = dict(repetition_penalty=10.0, temperature=1.0, top_k=0, top_p=1.0, do_sample=False, suppress_stop=False, seed=0,
                        typical_mass=0.0, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0)
    _BEAM_KEYS = dict(repetition_penalty=10.0, temperature=0.8, top_k=30, top_p=0.8, suppress_stop=False, seed=0, typical_mass=0.0,
                      length_penalty=0.0, do_sample=True, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0)

    @staticmethod
    def _sampler_array(cfgs, defaults, what):
        """A list of dicts (the keyword names and defaults of `decode()` / `beam_decode()`) -> a ctypes array of SamplerCfg."""
        arr = (_lib.SamplerCfg * len(cfgs))()
        for i, cfg in enumerate(cfgs):
            unknown = set(cfg) - set(defaults)
            if unknown:
                raise TypeError(f"{what}: entry {i} has unexpected keys {sorted(unknown)}")
            v = {**defaults, **cfg}
            arr[i] = _lib.SamplerCfg(v["repetition_penalty"], v["temperature"], int(v["top_k"]), v["top_p"], int(bool(v["do_sample"])),
                                     int(bool(v["suppress_stop"])), int(v["seed"]), float(v["typical_mass"]), float(v.get("length_penalty", 0.0)),
                                     int(v["min_new_tokens"]), int(v["no_repeat_ngram_size"]), float(v["min_p"]))
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
                    length_penalty=0.0, groups=1, do_sample=True, min_new_tokens=0, no_repeat_ngram_size=0, min_p=0.0):
        """`do_sample=False`: beam search proper -- the joint top 2 * num_beams instead of the multinomial draw, no warpers (`min_p`
        is one of them).  `no_repeat_ngram_size` looks at each beam's own history."""
        sc = _lib.SamplerCfg(repetition_penalty, temperature, top_k, top_p, int(bool(do_sample)), int(suppress_stop), seed, float(typical_mass), float(length_penalty),
                             int(min_new_tokens), int(no_repeat_ngram_size), float(min_p))
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
        self.prefill(0, emb, n_pad)
        if bans is not None:
            self.set_bans(0, *bans)
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
