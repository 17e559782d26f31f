"""CPU: QwenEmotion's post-processing against the reference's own class (tests/golden/qwen_emo_parse.json), and the
model-directory loader of the emotion engine (config refusals, tied lm_head, sharded index, generation defaults)."""
import json
import os

import pytest
import torch

from voice_tts_amd import qwen_emotion as Q

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "qwen_emo_parse.json"), encoding="utf-8"))


class ScriptedTokenizer:
    def __init__(self):
        self.decoded, self.calls = None, []

    def decode(self, ids, skip_special_tokens=False):
        assert skip_special_tokens
        self.calls.append([int(i) for i in ids])
        return self.decoded


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_parse_matches_reference(case):
    tok = ScriptedTokenizer()
    q = Q.QwenEmotion(None, tokenizer=tok)
    tok.decoded = case["decoded"]
    res = q.parse(list(case["output_ids"]), case["text"])
    assert tok.calls == [case["decode_ids"]]
    assert [[k, v] for k, v in res.items()] == case["result"]
    assert [type(v) for _, v in res.items()] == [type(v) for _, v in case["result"]]


def test_golden_covers_the_listed_cases():
    names = {c["name"] for c in GOLDEN["cases"]}
    for need in ("valid_json", "json_after_think", "regex_fallback", "clamp_high_low", "missing_keys", "all_zero"):
        assert need in names
    for w in ("低落", "melancholy", "melancholic", "depression", "depressed", "gloomy"):
        assert f"melancholic_{w}" in names
        if w.isascii():
            assert f"melancholic_{w.upper()}" in names


def test_inference_without_model_raises():
    with pytest.raises(RuntimeError):
        Q.QwenEmotion(None, tokenizer=ScriptedTokenizer()).inference("x")


# ---------------------------------------------------------------------------------------------------- loader
def _config(**over):
    c = dict(model_type="qwen3", hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
             num_key_value_heads=2, head_dim=128, vocab_size=256, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False,
             attention_bias=False, eos_token_id=7)
    c.update(over)
    return c


def _tensors(cfg, lm_head=True):
    D, I, V, qd, kvd = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"], 4 * 128, 2 * 128
    g = torch.Generator().manual_seed(0)
    sd = {"model.embed_tokens.weight": torch.randn(V, D, generator=g), "model.norm.weight": torch.ones(D)}
    for l in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{l}."
        sd.update({p + "self_attn.q_proj.weight": torch.randn(qd, D, generator=g), p + "self_attn.k_proj.weight": torch.randn(kvd, D, generator=g),
                   p + "self_attn.v_proj.weight": torch.randn(kvd, D, generator=g), p + "self_attn.o_proj.weight": torch.randn(D, qd, generator=g),
                   p + "self_attn.q_norm.weight": torch.ones(128), p + "self_attn.k_norm.weight": torch.ones(128),
                   p + "mlp.gate_proj.weight": torch.randn(I, D, generator=g), p + "mlp.up_proj.weight": torch.randn(I, D, generator=g),
                   p + "mlp.down_proj.weight": torch.randn(D, I, generator=g), p + "input_layernorm.weight": torch.ones(D),
                   p + "post_attention_layernorm.weight": torch.ones(D)})
    if lm_head:
        sd["lm_head.weight"] = torch.randn(V, D, generator=g)
    return sd


def _write(d, cfg, sd=None, gen=None, shards=0):
    from safetensors.torch import save_file

    os.makedirs(d, exist_ok=True)
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    if gen is not None:
        json.dump(gen, open(os.path.join(d, "generation_config.json"), "w"))
    if sd is None:
        return d
    sd = {k: v.to(torch.float16) for k, v in sd.items()}
    if not shards:
        save_file(sd, os.path.join(d, "model.safetensors"))
        return d
    names = sorted(sd)
    wm = {}
    for i in range(shards):
        part = names[i::shards]
        fn = f"model-{i + 1:05d}-of-{shards:05d}.safetensors"
        save_file({k: sd[k] for k in part}, os.path.join(d, fn))
        wm.update({k: fn for k in part})
    json.dump({"metadata": {}, "weight_map": wm}, open(os.path.join(d, "model.safetensors.index.json"), "w"))
    return d


@pytest.mark.parametrize("over, err", [
    (dict(model_type="llama"), ValueError),
    (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0}), NotImplementedError),
    (dict(rope_parameters={"rope_type": "linear", "factor": 2.0, "rope_theta": 1e6}), NotImplementedError),
    (dict(attention_bias=True), NotImplementedError),
    (dict(use_sliding_window=True, sliding_window=128), NotImplementedError),
])
def test_config_refusals(tmp_path, over, err):
    with pytest.raises(err):
        Q.read_config(_write(str(tmp_path / "m"), _config(**over)))


def test_config_accepts_default_rope(tmp_path):
    c = Q.read_config(_write(str(tmp_path / "a"), _config(rope_scaling=None)))
    assert c["rope_theta"] == 1e6 and c["head_dim"] == 128 and c["kv_heads"] == 2
    c = Q.read_config(_write(str(tmp_path / "b"), {k: v for k, v in _config(rope_parameters={"rope_type": "default", "rope_theta": 5e5}).items()
                                                   if k != "rope_theta"}))
    assert c["rope_theta"] == 5e5


def test_lm_head_tied_when_absent(tmp_path):
    cfg = _config()
    d = _write(str(tmp_path / "m"), cfg, _tensors(cfg, lm_head=False), gen={"eos_token_id": [7, 8]})
    ec, gen, sd = Q.load_model_dir(d)
    assert ec["tie_word_embeddings"] and "lm_head.weight" not in sd
    d2 = _write(str(tmp_path / "n"), cfg, _tensors(cfg, lm_head=True), gen={"eos_token_id": 7})
    ec2, gen2, sd2 = Q.load_model_dir(d2)
    assert not ec2["tie_word_embeddings"] and "lm_head.weight" in sd2
    assert gen["eos_token_id"] == [7, 8] and gen2["eos_token_id"] == [7]


def test_sharded_index(tmp_path):
    cfg = _config()
    ref = _tensors(cfg)
    d = _write(str(tmp_path / "m"), cfg, ref, shards=3)
    assert not os.path.exists(os.path.join(d, "model.safetensors"))
    _, _, sd = Q.load_model_dir(d)
    assert set(sd) == set(ref)
    for k, v in ref.items():
        assert sd[k].dtype == torch.float32 and torch.equal(sd[k], v.to(torch.float16).float())


def test_generation_defaults_of_transformers_4_52(tmp_path):
    d = _write(str(tmp_path / "m"), _config())
    g = Q.read_generation_config(d, Q.read_config(d))
    assert g == dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, eos_token_id=[7])
    d2 = _write(str(tmp_path / "n"), _config(), gen={"do_sample": True, "temperature": 0.6, "top_k": 20, "top_p": 0.95, "eos_token_id": [151645, 151643]})
    g2 = Q.read_generation_config(d2, Q.read_config(d2))
    assert g2 == dict(do_sample=True, temperature=0.6, top_k=20, top_p=0.95, eos_token_id=[151645, 151643])
    d3 = _write(str(tmp_path / "o"), _config(), gen={"temperature": 0.7})
    assert Q.read_generation_config(d3, Q.read_config(d3))["top_k"] == 50


def test_top_k_limit_is_named():
    with pytest.raises(NotImplementedError, match="64"):
        Q.QwenEngine.sampling(do_sample=True, top_k=0)
    with pytest.raises(NotImplementedError, match="64"):
        Q.QwenEngine.sampling(do_sample=True, top_k=65)
    assert Q.QwenEngine.sampling(do_sample=False, top_k=0).do_sample == 0
