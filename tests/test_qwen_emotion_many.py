"""CPU: `QwenEmotion.inference_many` over a scripted engine (dedup, groups of `slots`, order, per-text parse) and the
emotion texts `IndexTTS2.infer_many` hands to the emotion model."""

from voice_tts_amd import qwen_emotion as Q
from voice_tts_amd.infer_v2 import IndexTTS2


class WordTokenizer:
    """A prompt is one id per character of the text; an answer id i decodes to ANSWERS[i]."""

    ANSWERS = ['{"悲伤": 0.8, "高兴": 0.1}', '{"高兴": 0.9}', '{"愤怒": 1.5}', "no json at all"]

    def apply_chat_template(self, messages, **kw):
        return messages[1]["content"]

    def __call__(self, texts, return_tensors=None):
        import torch

        class Out:
            input_ids = torch.tensor([[ord(c) % 251 for c in texts[0]]])

        return Out()

    def decode(self, ids, skip_special_tokens=False):
        return self.ANSWERS[ids[0]]


class ScriptedEngine:
    """generate_many answers by prompt length: a prompt of n ids gets [n % 4]."""

    def __init__(self, slots):
        self.slots, self.groups, self.singles = slots, [], []

    def generate_many(self, prompts, max_new_tokens, **sampling):
        assert 1 <= len(prompts) <= self.slots and sampling["seed"] == 9 and max_new_tokens == 77
        self.groups.append([len(p) for p in prompts])
        return [[len(p) % 4] for p in prompts]

    def generate(self, prompt, max_new_tokens, **sampling):
        self.singles.append(len(prompt))
        return [len(prompt) % 4]


TEXTS = ["aaaa", "a gloomy day", "bb", "aaaa", "ccccccc", "dddddddddd", "e"]  # lengths 4, 12, 2, 4, 7, 10, 1


def _q(slots):
    return Q.QwenEmotion(None, tokenizer=WordTokenizer(), engine=ScriptedEngine(slots), seed=9)


def test_inference_many_dedups_groups_and_keeps_the_order():
    q = _q(4)
    res = q.inference_many(TEXTS, max_new_tokens=77)
    # six different texts, longest prompts first, in groups of at most 4
    assert q.engine.groups == [[12, 10, 7, 4], [2, 1]] and q.engine.singles == []
    assert res == [q.parse([len(t) % 4], t) for t in TEXTS]
    assert res[0] == res[3] and res[0]["sad"] == 0.8 and res[0]["happy"] == 0.1
    # "a gloomy day" answers the same JSON (12 % 4 == 0) but its text swaps sad and melancholic
    assert res[1]["melancholic"] == 0.8 and res[1]["sad"] == 0.0
    assert res[2]["angry"] == 1.2 and res[6]["happy"] == 0.9  # clamped; per-text answers
    assert res[4]["calm"] == 1.0  # 7 % 4 == 3: no JSON, nothing detected
    assert _q(3).inference_many(TEXTS, max_new_tokens=77) == res
    q2 = _q(2)
    q2.inference_many(TEXTS[:3], max_new_tokens=77)
    assert q2.engine.groups == [[12, 4], [2]]


def test_inference_many_with_one_slot_is_the_loop_over_inference():
    q = _q(1)
    res = q.inference_many(TEXTS, max_new_tokens=77)
    assert q.engine.groups == [] and q.engine.singles == [len(t) for t in TEXTS]
    assert res == _q(4).inference_many(TEXTS, max_new_tokens=77)


class RecordingEmotion:
    def __init__(self):
        self.calls = []

    def inference(self, text):
        self.calls.append(text)
        return dict(zip("abcdefgh", [len(text) / 100] * 8))


class ManyEmotion(RecordingEmotion):
    def inference_many(self, texts):
        self.calls.append(list(texts))
        return [dict(zip("abcdefgh", [len(t) / 100] * 8)) for t in texts]


REQS = [dict(text="one", use_emo_text=True, emo_text="so very angry"), dict(text="plain"), dict(text="the text itself", use_emo_text=True),
        dict(text="off", use_emo_text=False, emo_text="ignored")]


def _bare(emo):
    m = IndexTTS2.__new__(IndexTTS2)
    m.qwen_emo, m.qwen_emo_dir = emo, None
    return m


def test_infer_many_hands_the_batch_to_inference_many_or_loops_over_inference():
    failed = {}
    many = ManyEmotion()
    vec = _bare(many)._emo_text_vectors(REQS, failed)
    assert many.calls == [["so very angry", "the text itself"]] and failed == {}
    assert vec == {0: [0.13] * 8, 2: [0.15] * 8}
    rec = RecordingEmotion()
    assert _bare(rec)._emo_text_vectors(REQS, failed) == vec and rec.calls == ["so very angry", "the text itself"]
    assert _bare(rec)._emo_text_vectors([REQS[1], REQS[3]], failed) == {} and len(rec.calls) == 2


def test_infer_many_without_the_model_fails_those_requests_alone():
    failed = {}
    assert _bare(None)._emo_text_vectors(REQS, failed) == {}
    assert sorted(failed) == [0, 2] and all(isinstance(e, NotImplementedError) and "qwen_emo_path" in str(e) for e in failed.values())
