"""Emotion from text: `QwenEmotion` of the reference (indextts/infer_v2.py:795-906) on the HIP Qwen3 decode engine.

The reference loads a Qwen3 causal LM (`model_dir/<qwen_emo_path>`, fp16), asks it to classify the emotion of a text
through a chat prompt, and turns the JSON it answers into the 8-value `emo_vector`.  Here the tokenizer and the chat
template are the model's own (transformers, local files only); every decode step runs in libixtts_hip.so
(csrc/qwen_engine.hip); the post-processing is the reference's, line for line.
"""
import ctypes as C
import json
import logging
import os
import re
import time
import warnings

import numpy as np
import torch

from . import _lib

logger = logging.getLogger(__name__)

THINK_END_ID = 151668  # </think> in the Qwen3 vocabulary (infer_v2.py:869-873)
# generation defaults as transformers 4.52.1 (the version the reference pins) resolves a key its generation_config.json lacks
GEN_DEFAULTS = dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0)


# ---------------------------------------------------------------------------------------------------- model directory
def read_config(model_dir):
    """config.json -> the engine's dimensions; refuses what the engine does not compute."""
    cfg = json.load(open(os.path.join(model_dir, "config.json")))
    if cfg.get("model_type") != "qwen3":
        raise ValueError(f"{model_dir}: model_type {cfg.get('model_type')!r}, the emotion engine decodes qwen3 only")
    rope = cfg.get("rope_scaling")
    params = cfg.get("rope_parameters") or {}
    for r in (rope, params):
        if r and (r.get("rope_type") or r.get("type") or "default") != "default":
            raise NotImplementedError(f"{model_dir}: rope scaling {r} is not built (only the default rotary embedding)")
    if cfg.get("attention_bias"):
        raise NotImplementedError(f"{model_dir}: attention_bias true is not built")
    if cfg.get("use_sliding_window") or "sliding_attention" in (cfg.get("layer_types") or []):
        raise NotImplementedError(f"{model_dir}: sliding-window attention is not built")
    heads = int(cfg["num_attention_heads"])
    theta = cfg.get("rope_theta", params.get("rope_theta", 10000.0))
    return dict(hidden_size=int(cfg["hidden_size"]), layers=int(cfg["num_hidden_layers"]), heads=heads,
                kv_heads=int(cfg.get("num_key_value_heads", heads)), head_dim=int(cfg.get("head_dim") or cfg["hidden_size"] // heads),
                intermediate_size=int(cfg["intermediate_size"]), vocab_size=int(cfg["vocab_size"]),
                rms_norm_eps=float(cfg.get("rms_norm_eps", 1e-6)), rope_theta=float(theta),
                tie_word_embeddings=bool(cfg.get("tie_word_embeddings", False)), eos_token_id=cfg.get("eos_token_id"))


def read_generation_config(model_dir, cfg=None):
    """generation_config.json over GEN_DEFAULTS; eos ids as a list (int or list in the file, config.json's as fallback)."""
    path = os.path.join(model_dir, "generation_config.json")
    g = json.load(open(path)) if os.path.isfile(path) else {}
    out = {k: g.get(k, v) if g.get(k) is not None else v for k, v in GEN_DEFAULTS.items()}
    eos = g.get("eos_token_id", (cfg or {}).get("eos_token_id"))
    out["eos_token_id"] = [] if eos is None else [int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos])]
    return out


def read_state_dict(model_dir):
    """model.safetensors, or the shards a model.safetensors.index.json names -> {name: fp32 CPU tensor}."""
    from safetensors.torch import load_file

    single = os.path.join(model_dir, "model.safetensors")
    index = os.path.join(model_dir, "model.safetensors.index.json")
    if os.path.isfile(single):
        files = [single]
    elif os.path.isfile(index):
        files = [os.path.join(model_dir, f) for f in sorted(set(json.load(open(index))["weight_map"].values()))]
    else:
        raise FileNotFoundError(f"{model_dir}: neither model.safetensors nor model.safetensors.index.json")
    sd = {}
    for f in files:
        sd.update({k: v.to(torch.float32) for k, v in load_file(f).items()})
    return sd


def load_model_dir(model_dir):
    """-> (engine cfg, generation cfg, state dict).  lm_head is the embedding when tied or absent."""
    cfg = read_config(model_dir)
    gen = read_generation_config(model_dir, cfg)
    sd = read_state_dict(model_dir)
    if cfg["tie_word_embeddings"] or "lm_head.weight" not in sd:
        cfg["tie_word_embeddings"] = True
        sd.pop("lm_head.weight", None)
    if not gen["eos_token_id"]:
        raise ValueError(f"{model_dir}: no eos_token_id in generation_config.json or config.json")
    return cfg, gen, sd


# ---------------------------------------------------------------------------------------------------- engine
class QwenEngine:
    """ctypes wrapper of ixtts_qwen_*: `slots` sequences (1..4), each with a KV cache of max_seq positions.  Slot 0 is the
    sequence of prefill / step / read / generate; the *_many calls decode up to `slots` prompts per step."""

    def __init__(self, cfg, dtype="f16", max_seq=2048, device=None, eos_token_id=None, slots=1):
        self.device = torch.device(device if device is not None else "cuda:0")
        eos = eos_token_id if eos_token_id is not None else cfg.get("eos_token_id")
        eos = [] if eos is None else [int(eos)] if isinstance(eos, int) else [int(e) for e in eos]
        if not 1 <= len(eos) <= _lib.QWEN_MAX_EOS:
            raise ValueError(f"1..{_lib.QWEN_MAX_EOS} eos ids needed, got {eos}")
        c = _lib.QwenCfg()
        for k in ("hidden_size", "layers", "heads", "kv_heads", "head_dim", "intermediate_size", "vocab_size"):
            setattr(c, k, int(cfg[k]))
        c.rms_norm_eps, c.rope_theta = float(cfg["rms_norm_eps"]), float(cfg["rope_theta"])
        c.tie_word_embeddings = int(bool(cfg["tie_word_embeddings"]))
        c.max_seq, c.weight_dtype = int(max_seq), {"f32": 0, "f16": 2}[dtype]
        c.n_eos = len(eos)
        for i, e in enumerate(eos):
            c.eos_ids[i] = int(e)
        self.cfg, self.dtype, self.max_seq, self.V, self.eos = dict(cfg), dtype, int(max_seq), int(cfg["vocab_size"]), eos
        self.slots = int(slots)
        if not 1 <= self.slots <= _lib.QWEN_MAX_SLOTS:
            raise ValueError(f"slots={slots}: an engine holds 1..{_lib.QWEN_MAX_SLOTS} sequences")
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_create_slots(C.byref(self._h), C.byref(c), self.slots), "ixtts_qwen_create_slots")
        self.prompt_len = 0
        self.prompt_lens = []

    def load_state_dict(self, sd):
        L = _lib.lib()
        with torch.cuda.device(self.device):
            for name, t in sd.items():
                if name == "lm_head.weight" and self.cfg["tie_word_embeddings"]:
                    continue
                t = t.detach().to("cpu", torch.float32).contiguous()
                shape = (C.c_int64 * t.dim())(*t.shape)
                _lib.check(L.ixtts_qwen_set_tensor(self._h, name.encode(), t.data_ptr(), shape, t.dim()), f"ixtts_qwen_set_tensor({name})")
            _lib.check(L.ixtts_qwen_finalize(self._h), "ixtts_qwen_finalize")
        return self

    def _stream(self):
        return _lib.current_stream_ptr()

    @staticmethod
    def sampling(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=0):
        if do_sample and not (1 <= int(top_k) <= _lib.QWEN_TOPK_MAX):
            raise NotImplementedError(f"top_k={top_k}: the device token selection keeps 1..{_lib.QWEN_TOPK_MAX} candidates "
                                      "(full-vocabulary sampling, top_k=0, is not built)")
        return _lib.QwenSampling(int(bool(do_sample)), float(temperature), int(top_k), float(top_p), int(seed) & (2**64 - 1))

    def prefill(self, ids):
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        if not 1 <= a.size < self.max_seq:
            raise ValueError(f"prompt of {a.size} ids does not fit a KV cache of {self.max_seq} positions")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_prefill(self._h, a.ctypes.data, a.size, self._stream()), "ixtts_qwen_prefill")
        self.prompt_len = a.size

    def step(self, n_steps=1, **sampling):
        sc = self.sampling(**sampling)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_step(self._h, int(n_steps), C.byref(sc), self._stream()), "ixtts_qwen_step")

    def read(self):
        ids = np.zeros(self.max_seq + 1, np.int32)
        n, fin = C.c_int(), C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_read(self._h, ids.ctypes.data, ids.size, C.byref(n), C.byref(fin), self._stream()), "ixtts_qwen_read")
        return ids[: n.value].tolist(), int(fin.value)

    def generate(self, ids, max_new_tokens, **sampling):
        """Prompt ids -> generated ids (EOS included when drawn), HF `generate` for one sequence.  max_new_tokens beyond the KV
        capacity is capped, with a warning."""
        self.prefill(ids)
        cap = self.max_seq - self.prompt_len
        n_max = int(max_new_tokens)
        if n_max > cap:
            n_max = cap
        sc = self.sampling(**sampling)
        out = np.zeros(n_max + 1, np.int32)
        n, fin = C.c_int(), C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_generate(self._h, n_max, C.byref(sc), out.ctypes.data, out.size, C.byref(n), C.byref(fin),
                                                      self._stream()), "ixtts_qwen_generate")
        if int(max_new_tokens) > cap and not fin.value and n.value >= n_max:
            warnings.warn(f"emotion model: max_new_tokens={max_new_tokens} capped to the {cap} positions the KV cache has left "
                          f"(max_seq={self.max_seq}); the answer was cut there")
        return out[: n.value].tolist()

    def read_logits(self):
        out = np.zeros(self.V, np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_read_logits(self._h, out.ctypes.data, self._stream()), "ixtts_qwen_read_logits")
        return out

    def read_kept(self):
        ids = np.zeros(_lib.QWEN_TOPK_MAX, np.int32)
        pr = np.zeros(_lib.QWEN_TOPK_MAX, np.float32)
        n = C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_read_kept(self._h, ids.ctypes.data, pr.ctypes.data, ids.size, C.byref(n), self._stream()),
                       "ixtts_qwen_read_kept")
        return ids[: n.value].copy(), pr[: n.value].copy()

    def draw(self, seed, n):
        out = np.zeros(int(n), np.int32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_draw(self._h, int(seed) & (2**64 - 1), int(n), out.ctypes.data, self._stream()), "ixtts_qwen_draw")
        return out

    # ---- slots
    def prefill_many(self, prompts):
        """Slots 0..len(prompts)-1 take the prompts: each one's first len-1 positions run through the layers."""
        arrs = [np.asarray(p, dtype=np.int32).reshape(-1) for p in prompts]
        if not 1 <= len(arrs) <= self.slots:
            raise ValueError(f"{len(arrs)} prompts for an engine of {self.slots} slots")
        for a in arrs:
            if not 1 <= a.size < self.max_seq:
                raise ValueError(f"prompt of {a.size} ids does not fit a KV cache of {self.max_seq} positions")
        ids = np.ascontiguousarray(np.concatenate(arrs))
        lens = np.ascontiguousarray(np.array([a.size for a in arrs], dtype=np.int32))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_prefill_slots(self._h, len(arrs), ids.ctypes.data, lens.ctypes.data, self._stream()),
                       "ixtts_qwen_prefill_slots")
        self.prompt_lens = lens.tolist()
        self.prompt_len = self.prompt_lens[0]

    def step_many(self, n_steps=1, n=None, **sampling):
        sc = self.sampling(**sampling)
        n = len(self.prompt_lens) if n is None else int(n)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_step_slots(self._h, n, int(n_steps), C.byref(sc), self._stream()), "ixtts_qwen_step_slots")

    def read_slot(self, slot):
        ids = np.zeros(self.max_seq + 1, np.int32)
        n, fin = C.c_int(), C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_read_slot(self._h, int(slot), ids.ctypes.data, ids.size, C.byref(n), C.byref(fin), self._stream()),
                       "ixtts_qwen_read_slot")
        return ids[: n.value].tolist(), int(fin.value)

    def read_logits_slot(self, slot):
        out = np.zeros(self.V, np.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_read_logits_slot(self._h, int(slot), out.ctypes.data, self._stream()), "ixtts_qwen_read_logits_slot")
        return out

    def read_kept_slot(self, slot):
        ids = np.zeros(_lib.QWEN_TOPK_MAX, np.int32)
        pr = np.zeros(_lib.QWEN_TOPK_MAX, np.float32)
        n = C.c_int()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_read_kept_slot(self._h, int(slot), ids.ctypes.data, pr.ctypes.data, ids.size, C.byref(n),
                                                            self._stream()), "ixtts_qwen_read_kept_slot")
        return ids[: n.value].copy(), pr[: n.value].copy()

    def generate_many(self, prompts, max_new_tokens, **sampling):
        """`generate` for up to `slots` prompts at once -> one id list per prompt, each what `generate` gives for it alone
        (f32 engines: bit for bit; f16 engines prefill the batch on the matrix cores)."""
        self.prefill_many(prompts)
        sc = self.sampling(**sampling)
        n = len(self.prompt_lens)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ixtts_qwen_generate_slots(self._h, n, int(max_new_tokens), C.byref(sc), self._stream()),
                       "ixtts_qwen_generate_slots")
        outs = []
        for s, plen in enumerate(self.prompt_lens):
            ids, fin = self.read_slot(s)
            cap = self.max_seq - plen
            if int(max_new_tokens) > cap and fin != 1 and len(ids) >= cap:
                warnings.warn(f"emotion model: max_new_tokens={max_new_tokens} capped to the {cap} positions the KV cache has left "
                              f"(max_seq={self.max_seq}); the answer was cut there")
            outs.append(ids[: min(int(max_new_tokens), cap)])
        return outs

    def step_bytes(self, S):
        return _lib.lib().ixtts_qwen_step_bytes(self._h, int(S))

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                _lib.lib().ixtts_qwen_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------- the reference class
class QwenEmotion:
    """Mirror of the reference's QwenEmotion (infer_v2.py:795-906).  `dtype="f16"` as the reference loads it
    (torch_dtype="float16"); "f32" is the parity mode of the tests.  `seed` feeds the device sampler when the model's
    generation config samples."""

    def __init__(self, model_dir, dtype="f16", device=None, max_seq=2048, seed=0, tokenizer=None, engine=None, slots=None):
        self.model_dir = model_dir
        if tokenizer is None:
            from transformers import AutoTokenizer

            tokenizer = AutoTokenizer.from_pretrained(model_dir, local_files_only=True)
        self.tokenizer = tokenizer
        self.engine = engine
        self.generation = dict(GEN_DEFAULTS)
        if engine is None and model_dir is not None:
            cfg, self.generation, sd = load_model_dir(model_dir)
            if slots is None:
                slots = int(os.environ.get("IXTTS_QWEN_SLOTS", "4"))  # sequences decoded per step by inference_many; 1 = off
            self.engine = QwenEngine(cfg, dtype=dtype, max_seq=max_seq, device=device, eos_token_id=self.generation["eos_token_id"],
                                     slots=slots).load_state_dict(sd)
        self.seed = int(seed)
        self.prompt = "文本情感分类"
        self.cn_key_to_en = {
            "高兴": "happy",
            "愤怒": "angry",
            "悲伤": "sad",
            "恐惧": "afraid",
            "反感": "disgusted",
            # the model maps "低落" (melancholic) to "悲伤" (sad); see melancholic_words
            "低落": "melancholic",
            "惊讶": "surprised",
            "自然": "calm",
        }
        self.desired_vector_order = ["高兴", "愤怒", "悲伤", "恐惧", "反感", "低落", "惊讶", "自然"]
        self.melancholic_words = {
            # emotion text phrases that turn the model's "悲伤" (sad) into "低落" (melancholic)
            "低落",
            "melancholy",
            "melancholic",
            "depression",
            "depressed",
            "gloomy",
        }
        self.max_score = 1.2
        self.min_score = 0.0
        self.last_time = 0.0

    def clamp_score(self, value):
        return max(self.min_score, min(self.max_score, value))

    def convert(self, content):
        # fixed key order, English keys, clamped values, 0.0 for missing keys; all zero -> calm
        emotion_dict = {
            self.cn_key_to_en[cn_key]: self.clamp_score(content.get(cn_key, 0.0))
            for cn_key in self.desired_vector_order
        }
        if all(val <= 0.0 for val in emotion_dict.values()):
            logger.info("no emotions detected; using default calm/neutral voice")
            emotion_dict["calm"] = 1.0
        return emotion_dict

    def prompt_ids(self, text_input):
        messages = [
            {"role": "system", "content": f"{self.prompt}"},
            {"role": "user", "content": f"{text_input}"},
        ]
        text = self.tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True, enable_thinking=False)
        return self.tokenizer([text], return_tensors="pt").input_ids[0].tolist()

    def parse(self, output_ids, text_input):
        """The reference's post-processing of the generated ids (infer_v2.py:868-906)."""
        try:
            # rindex finding 151668 (</think>)
            index = len(output_ids) - output_ids[::-1].index(THINK_END_ID)
        except ValueError:
            index = 0
        content = self.tokenizer.decode(output_ids[index:], skip_special_tokens=True)
        try:
            content = json.loads(content)
        except json.decoder.JSONDecodeError:
            # invalid JSON; fall back to manual string parsing
            content = {
                m.group(1): float(m.group(2))
                for m in re.finditer(r'([^\s":.,]+?)"?\s*:\s*([\d.]+)', content)
            }
        text_input_lower = text_input.lower()
        if any(word in text_input_lower for word in self.melancholic_words):
            content["悲伤"], content["低落"] = content.get("低落", 0.0), content.get("悲伤", 0.0)
        return self.convert(content)

    def inference(self, text_input, max_new_tokens=32768):
        if self.engine is None:
            raise RuntimeError("QwenEmotion built without a model (parse-only)")
        start = time.perf_counter()
        ids = self.prompt_ids(text_input)
        g = self.generation
        out = self.engine.generate(ids, max_new_tokens, do_sample=g["do_sample"], temperature=g["temperature"], top_k=g["top_k"],
                                   top_p=g["top_p"], seed=self.seed)
        res = self.parse(out, text_input)
        self.last_time = time.perf_counter() - start
        return res

    def inference_many(self, texts, max_new_tokens=32768):
        """`inference` for several texts -> one dict per text, in order.  Equal texts are decoded once; the unique prompts go
        through the engine in groups of at most its `slots`, longest first (prompts of similar length share a group)."""
        if self.engine is None:
            raise RuntimeError("QwenEmotion built without a model (parse-only)")
        texts = list(texts)
        slots = int(getattr(self.engine, "slots", 1))
        if slots <= 1 or not hasattr(self.engine, "generate_many"):
            return [self.inference(t, max_new_tokens) for t in texts]
        start = time.perf_counter()
        unique = list(dict.fromkeys(texts))
        prompts = {t: self.prompt_ids(t) for t in unique}
        order = sorted(unique, key=lambda t: -len(prompts[t]))  # stable: equal lengths keep the order of the texts
        g = self.generation
        outs = {}
        for i in range(0, len(order), slots):
            group = order[i: i + slots]
            ids = self.engine.generate_many([prompts[t] for t in group], max_new_tokens, do_sample=g["do_sample"], temperature=g["temperature"],
                                            top_k=g["top_k"], top_p=g["top_p"], seed=self.seed)
            outs.update(zip(group, ids))
        res = [self.parse(outs[t], t) for t in texts]
        self.last_time = time.perf_counter() - start
        return res
