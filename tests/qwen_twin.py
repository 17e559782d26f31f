"""Seeded Qwen3 twins of the text-emotion model, written as the reference's model directory holds it.

`write_twin(dir)` saves a `Qwen3ForCausalLM` with head_dim 128 and 2:1 GQA (as Qwen3-0.6B) but few layers and a small
vocabulary, a generation_config.json, and a byte-level `tokenizers` tokenizer with the Qwen chat tokens and a chat
template that honours `enable_thinking`.  transformers itself is the oracle the tests compare against.
"""
import json
import os

import torch

SPECIALS = ["<|endoftext|>", "<|im_start|>", "<|im_end|>", "<think>", "</think>"]
CHAT_TEMPLATE = (
    "{%- for m in messages %}{{ '<|im_start|>' + m['role'] + '\\n' + m['content'] + '<|im_end|>\\n' }}{%- endfor %}"
    "{%- if add_generation_prompt %}{{ '<|im_start|>assistant\\n' }}"
    "{%- if enable_thinking is defined and enable_thinking is false %}{{ '<think>\\n\\n</think>\\n\\n' }}{%- endif %}{%- endif %}"
)

# Qwen3-0.6B (config.json of the production qwen0.6bemo4-merge/)
PROD = dict(hidden_size=1024, intermediate_size=3072, num_hidden_layers=28, num_attention_heads=16, num_key_value_heads=8, head_dim=128,
            vocab_size=151936, rms_norm_eps=1e-6, rope_theta=1000000.0, max_position_embeddings=40960, tie_word_embeddings=True)


def _byte_vocab():
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): i for i, c in enumerate(cs)}


def write_tokenizer(path):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast

    vocab = _byte_vocab()
    for s in SPECIALS:
        vocab[s] = len(vocab)
    tok = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)
    tok.decoder = decoders.ByteLevel()
    tok.add_special_tokens(SPECIALS)
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, eos_token="<|im_end|>", pad_token="<|endoftext|>")
    fast.chat_template = CHAT_TEMPLATE
    fast.save_pretrained(path)
    return {s: vocab[s] for s in SPECIALS}


def twin_config(layers=3, vocab_size=512, hidden_size=512, intermediate_size=1024, heads=4, kv_heads=2, tie=True, eos=None):
    from transformers import Qwen3Config

    return Qwen3Config(hidden_size=hidden_size, intermediate_size=intermediate_size, num_hidden_layers=layers, num_attention_heads=heads,
                       num_key_value_heads=kv_heads, head_dim=128, vocab_size=vocab_size, rms_norm_eps=1e-6, rope_theta=1000000.0,
                       max_position_embeddings=4096, tie_word_embeddings=tie, eos_token_id=eos, attention_bias=False)


def make_model(cfg, seed, std=0.02):
    """Qwen3ForCausalLM with seeded N(0, std) matrices and norm gains around 1 (fp32, eager attention)."""
    from transformers import Qwen3ForCausalLM

    torch.manual_seed(seed)
    cfg._attn_implementation = "eager"
    m = Qwen3ForCausalLM(cfg).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(std * torch.randn(p.shape, generator=g))
    return m


def write_twin(path, seed=0, layers=3, std=0.25, generation=None, **cfg_kw):
    """Model + tokenizer + generation config under `path`; returns (model, special ids)."""
    os.makedirs(path, exist_ok=True)
    ids = write_tokenizer(path)
    cfg = twin_config(layers=layers, eos=[ids["<|im_end|>"], ids["<|endoftext|>"]], **cfg_kw)
    m = make_model(cfg, seed, std)
    m.save_pretrained(path, safe_serialization=True)
    gen = dict(bos_token_id=ids["<|endoftext|>"], eos_token_id=[ids["<|im_end|>"], ids["<|endoftext|>"]], pad_token_id=ids["<|endoftext|>"])
    gen.update(generation or {})
    json.dump(gen, open(os.path.join(path, "generation_config.json"), "w"))
    return m, ids
