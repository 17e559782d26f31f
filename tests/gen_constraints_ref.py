"""TEST INFRASTRUCTURE: a torch restatement of the logits processors HF `generate()` builds from plain keywords --
NoRepeatNGram, MinNewTokensLength, SuppressTokens, SuppressTokensAtBegin, MinP -- and of the whole chain they sit in
(`_get_logits_processor`, transformers_generation_utils.py:900-1049):

    RepetitionPenalty -> NoRepeatNGram -> MinNewTokens -> SuppressTokens -> SuppressTokensAtBegin -> Temperature -> TopK -> TopP -> MinP

`tests/golden/gen_constraints.npz` holds what the reference's own classes give on seeded inputs; tests/test_gen_constraints.py
pins this file against it, the GPU tests compare the HIP sampler with this file applied to the device's own logits.
Histories are the ones HF sees: the fake prompt ids `[1] * (P - 1) + [start_mel]` followed by the generated tokens.
"""
import torch

from oracle import gpt as OG

NEG_INF = float("-inf")


def history_of(P, generated, start_mel=8192):
    return [1] * (P - 1) + [start_mel] + [int(t) for t in generated]


def ngram_banned(history, n):
    """Ids NoRepeatNGramLogitsProcessor(n) bans after `history`: the token that followed every earlier occurrence of the last
    n - 1 tokens (n = 1: every id of the history)."""
    h = [int(t) for t in history]
    if n <= 0 or len(h) < n:
        return set()
    suffix = h[len(h) - (n - 1):] if n > 1 else []
    return {h[j + n - 1] for j in range(len(h) - n + 1) if h[j:j + n - 1] == suffix}


def min_p_filter(scores, min_p, min_keep=1):
    """MinPLogitsWarper: ids whose softmax probability is below min_p * the largest go; the `min_keep` best never."""
    probs = torch.softmax(scores, dim=-1)
    remove = probs < min_p * probs.max()
    remove[torch.topk(probs, min(min_keep, probs.numel())).indices] = False
    return scores.masked_fill(remove, NEG_INF)


def constrain(scores, history, P, stop, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=(), begin_suppress_tokens=()):
    """The four processors, in the chain's order, on one row of scores."""
    s = scores.clone()
    banned = sorted(ngram_banned(history, no_repeat_ngram_size))
    if banned:
        s[torch.tensor(banned, dtype=torch.long)] = NEG_INF
    if min_new_tokens > 0 and len(history) - P < min_new_tokens:
        s[stop] = NEG_INF
    if len(suppress_tokens):
        s[torch.as_tensor(list(suppress_tokens), dtype=torch.long)] = NEG_INF
    if len(begin_suppress_tokens) and len(history) == P:
        s[torch.as_tensor(list(begin_suppress_tokens), dtype=torch.long)] = NEG_INF
    return s


def process(scores, history, P, stop=8193, theta=10.0, no_repeat_ngram_size=0, min_new_tokens=0, suppress_tokens=(), begin_suppress_tokens=(),
            sampling=False, temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, min_keep=1, suppress_stop=False):
    """The whole chain on one row (`scores`: the logits, or their log_softmax in beam mode); the warpers run when `sampling`."""
    s = scores.to(torch.float32).clone()
    if suppress_stop:
        s[stop] = NEG_INF
    if theta != 1.0:
        s = OG.repetition_penalty(s, history, theta)
    s = constrain(s, history, P, stop, no_repeat_ngram_size, min_new_tokens, suppress_tokens, begin_suppress_tokens)
    if sampling:
        if temperature != 1.0:
            s = s / temperature
        if top_k > 0:
            s = OG.top_k_filter(s, top_k, min_keep)
        if top_p < 1.0:
            s = OG.top_p_filter(s, top_p, min_keep)
        if min_p > 0.0:
            s = min_p_filter(s, min_p, min_keep)
    return s


def min_p_margin(scores, min_p):
    """How close (relative) the nearest probability lies to the MinP threshold min_p * max: membership is decided by rounding when
    this is tiny.  `scores`: the row MinP sees (after TopP)."""
    probs = torch.softmax(scores.to(torch.float64), dim=-1)
    thr = min_p * float(probs.max())
    live = probs[probs > 0]
    return float(((live - thr).abs() / thr).min())
