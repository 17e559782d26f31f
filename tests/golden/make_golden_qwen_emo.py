"""Generate tests/golden/qwen_emo_parse.json from the REFERENCE's QwenEmotion (build container only).

    python tests/golden/make_golden_qwen_emo.py --reference <root of the reference repository>

Importing indextts/infer_v2.py needs packages this container lacks (and its maskgct imports break under transformers
5.x), so only the body of `class QwenEmotion` is taken from the reference file at generation time and executed with
AutoTokenizer / AutoModelForCausalLM replaced by fakes: the fake model "generates" scripted ids, the fake tokenizer
decodes scripted strings.  The JSON holds data only: per case the text, the generated ids, the string the decode
returns, the ids decode was asked for and the dict `inference` returned.
"""
import argparse
import ast
import json
import os
import re
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PROMPT_IDS = [1, 2, 3, 4]
THINK_END = 151668

# (name, text_input, generated ids, decoded string)
CASES = [
    ("valid_json", "今天天气真好", [11, 12, 13, 99],
     '{"高兴": 0.85, "愤怒": 0.0, "悲伤": 0.05, "恐惧": 0.0, "反感": 0.0, "低落": 0.0, "惊讶": 0.3, "自然": 0.1}'),
    ("json_after_think", "我很害怕", [21, 22, THINK_END, 23, 24, 99],
     '{"恐惧": 0.9, "惊讶": 0.2}'),
    ("json_after_last_think", "last marker wins", [THINK_END, 31, THINK_END, 32, 99],
     '{"愤怒": 0.4}'),
    ("regex_fallback", "text", [41, 42, 99],
     '高兴: 0.7, "愤怒":0.2 and 悲伤 : 1.0, 自然: 0.05 (not json'),
    ("regex_fallback_quoted", "text", [43, 99],
     '{"高兴": 0.6, "恐惧": 0.1,}'),
    ("clamp_high_low", "text", [51, 99],
     '{"高兴": 1.5, "愤怒": -0.3, "悲伤": 1.2, "惊讶": 3}'),
    ("missing_keys", "text", [61, 99],
     '{"惊讶": 0.7}'),
    ("all_zero", "text", [71, 99],
     '{"高兴": 0.0, "愤怒": 0.0}'),
    ("empty_object", "text", [72, 99],
     '{}'),
    ("garbage", "text", [73, 99],
     'no scores here'),
]
for w in ("低落", "melancholy", "melancholic", "depression", "depressed", "gloomy"):
    for variant in dict.fromkeys((w, w.upper(), w.capitalize())):
        CASES.append((f"melancholic_{variant}", f"I feel {variant} today", [81, 99], '{"悲伤": 0.8, "低落": 0.1, "自然": 0.2}'))
CASES.append(("melancholic_absent_keys", "so GLOOMY", [82, 99], '{"高兴": 0.3}'))


def load_class(reference):
    src = open(os.path.join(reference, "indextts", "infer_v2.py"), encoding="utf-8").read()
    tree = ast.parse(src)
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "QwenEmotion")
    return ast.get_source_segment(src, node)


class _Inputs(dict):
    def __init__(self, ids):
        super().__init__(input_ids=torch.tensor([ids]))
        self.input_ids = self["input_ids"]

    def to(self, device):
        return self


class FakeTokenizer:
    eos_token_id = 99

    def __init__(self):
        self.decoded = None
        self.calls = []

    def apply_chat_template(self, messages, tokenize=False, add_generation_prompt=True, enable_thinking=False):
        return json.dumps(messages, ensure_ascii=False)

    def __call__(self, texts, return_tensors="pt"):
        return _Inputs(PROMPT_IDS)

    def decode(self, ids, skip_special_tokens=False):
        self.calls.append([int(i) for i in ids])
        return self.decoded


class FakeModel:
    device = "cpu"

    def __init__(self):
        self.out = None

    def generate(self, input_ids=None, max_new_tokens=None, pad_token_id=None, **kw):
        return torch.tensor([PROMPT_IDS + self.out])


class _Logger:
    def info(self, *a, **k):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    tok, model = FakeTokenizer(), FakeModel()
    ns = dict(json=json, re=re, time=time, torch=torch, logger=_Logger(),
              AutoTokenizer=type("AT", (), {"from_pretrained": staticmethod(lambda d, **k: tok)}),
              AutoModelForCausalLM=type("AM", (), {"from_pretrained": staticmethod(lambda d, **k: model)}))
    exec(compile(load_class(args.reference), "QwenEmotion", "exec"), ns)
    q = ns["QwenEmotion"]("unused")
    cases = []
    for name, text, out_ids, decoded in CASES:
        tok.decoded, tok.calls, model.out = decoded, [], list(out_ids)
        res = q.inference(text)
        cases.append(dict(name=name, text=text, output_ids=out_ids, decoded=decoded, decode_ids=tok.calls[0],
                          result=[[k, v] for k, v in res.items()]))
    path = os.path.join(HERE, "qwen_emo_parse.json")
    json.dump(dict(prompt_ids=PROMPT_IDS, cases=cases), open(path, "w", encoding="utf-8"), ensure_ascii=False, indent=1)
    print(f"wrote {len(cases)} cases to {path}")


if __name__ == "__main__":
    main()
