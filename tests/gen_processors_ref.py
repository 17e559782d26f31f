"""TEST INFRASTRUCTURE: a torch restatement of the other half of the logits processors HF `generate()` builds from plain
keywords -- SequenceBias, NoBadWords, ForcedEOSToken, ExponentialDecayLengthPenalty, EpsilonLogitsWarper, EtaLogitsWarper,
LogitNormalization -- and of the whole chain (`_get_logits_processor`, transformers_generation_utils.py:862-1069):

    SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinNewTokens -> ForcedEOS -> ExponentialDecayLengthPenalty
    -> SuppressTokens -> SuppressTokensAtBegin -> Temperature -> TopK -> TopP -> MinP -> EpsilonCutoff -> EtaCutoff -> LogitNormalization

`tests/golden/gen_processors.npz` holds what the reference's own classes give on seeded inputs; tests/test_gen_processors.py pins
this file against it, the GPU tests compare the HIP sampler with this file applied to the device's own logits.  Histories are
the ones HF sees: the fake prompt ids `[1] * (P - 1) + [start_mel]` followed by the generated tokens.  A table is a list of
(ids tuple, bias), as `voice_tts_amd.gpt_engine.sequence_bias_table` makes it.
"""
import torch

import gen_constraints_ref as GC
from oracle import gpt as OG

NEG_INF = float("-inf")
history_of = GC.history_of


def sequence_bias(scores, history, table):
    """SequenceBiasLogitsProcessor (NoBadWordsLogitsProcessor with biases of -inf): a one-id entry sets the bias of its id, a
    longer one adds its bias to its last id when the history ends with its other ids; longer than the history: ignored."""
    h = [int(t) for t in history]
    bias = torch.zeros_like(scores)
    for ids, b in table:
        if len(ids) == 1:
            bias[ids[0]] = b
    for ids, b in table:
        if len(ids) == 1 or len(ids) > len(h):
            continue
        if h[len(h) - (len(ids) - 1):] == [int(t) for t in ids[:-1]]:
            bias[ids[-1]] += b
    return scores + bias


def bad_words_table(bad_words_ids, eos):
    """What NoBadWordsLogitsProcessor(bad_words_ids, eos) keeps: every word but `[eos]`, at -inf."""
    return [(tuple(int(t) for t in w), NEG_INF) for w in bad_words_ids if list(w) != [eos]]


def forced_eos(scores, cur_len, max_length, ids):
    """ForcedEOSTokenLogitsProcessor(max_length, ids) with `cur_len` ids in the history."""
    if cur_len != max_length - 1:
        return scores
    s = torch.full_like(scores, NEG_INF)
    s[torch.as_tensor(list(ids), dtype=torch.long)] = 0
    return s


def exp_decay(scores, generated, start_index, factor, eos):
    """ExponentialDecayLengthPenalty((start_index, factor), eos, P) with `generated` tokens behind the prompt: the power in Python
    floats, times an fp32 tensor."""
    if generated <= start_index:
        return scores
    pen = torch.zeros_like(scores)
    pen[eos] = torch.abs(scores[eos]) * (pow(factor, generated - start_index) - 1)
    return scores + pen


def _cut(scores, probs, thr, min_keep):
    remove = probs < thr
    kth = torch.topk(scores, min(min_keep, scores.numel())).values[-1]
    return scores.masked_fill(remove & (scores < kth), NEG_INF)


def epsilon_filter(scores, epsilon, min_keep=1):
    """EpsilonLogitsWarper: ids whose softmax probability is below epsilon go; a score that reaches the min_keep-th best never."""
    return _cut(scores, torch.softmax(scores, -1), epsilon, min_keep)


def entropy(scores):
    """torch.distributions.Categorical(logits=scores).entropy(): removed ids (-inf) add 0."""
    logp = torch.log_softmax(scores, -1)
    p = torch.exp(logp)
    return -(torch.clamp(logp, min=torch.finfo(scores.dtype).min) * p).sum()


def eta_threshold(scores, eta):
    eps = torch.tensor(eta, dtype=scores.dtype)
    return torch.min(eps, torch.sqrt(eps) * torch.exp(-entropy(scores)))


def eta_filter(scores, eta, min_keep=1):
    """EtaLogitsWarper: the same with the threshold min(eta, sqrt(eta) * exp(-entropy))."""
    return _cut(scores, torch.softmax(scores, -1), eta_threshold(scores, eta), min_keep)


def process(scores, history, P, stop=8193, theta=10.0, sequence_bias_table=(), bad_words=(), no_repeat_ngram_size=0, min_new_tokens=0,
            forced_eos_ids=(), max_length=None, exp_decay_penalty=None, suppress_tokens=(), begin_suppress_tokens=(), sampling=False,
            temperature=1.0, top_k=0, top_p=1.0, min_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, renormalize_logits=False, min_keep=1,
            suppress_stop=False):
    """The whole chain on one row (`scores`: the logits, or their log_softmax in beam mode); the warpers run when `sampling`.
    `bad_words`: a table too (`bad_words_table`); `forced_eos_ids` act when the history holds `max_length - 1` ids;
    `exp_decay_penalty` = (start_index, factor)."""
    s = scores.to(torch.float32).clone()
    h = [int(t) for t in history]
    if suppress_stop:
        s[stop] = NEG_INF
    if len(sequence_bias_table):
        s = sequence_bias(s, h, sequence_bias_table)
    if theta != 1.0:
        s = OG.repetition_penalty(s, h, theta)
    s = GC.constrain(s, h, P, stop, no_repeat_ngram_size=no_repeat_ngram_size)
    if len(bad_words):
        s = sequence_bias(s, h, bad_words)
    s = GC.constrain(s, h, P, stop, min_new_tokens=min_new_tokens)
    if len(forced_eos_ids) and max_length is not None:
        s = forced_eos(s, len(h), max_length, forced_eos_ids)
    if exp_decay_penalty is not None:
        s = exp_decay(s, len(h) - P, int(exp_decay_penalty[0]), float(exp_decay_penalty[1]), stop)
    s = GC.constrain(s, h, P, stop, suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens)
    if sampling:
        if temperature != 1.0:
            s = s / temperature
        if top_k > 0:
            s = OG.top_k_filter(s, top_k, min_keep)
        if top_p < 1.0:
            s = OG.top_p_filter(s, top_p, min_keep)
        if min_p > 0.0:
            s = GC.min_p_filter(s, min_p, min_keep)
        if epsilon_cutoff > 0.0:
            s = epsilon_filter(s, epsilon_cutoff, min_keep)
        if eta_cutoff > 0.0:
            s = eta_filter(s, eta_cutoff, min_keep)
    if renormalize_logits:
        s = torch.log_softmax(s, -1)
    return s


def cut_margin(scores, thr):
    """How close (relative) the nearest live probability of the row a cutoff sees lies to its threshold: membership is decided by
    rounding when this is tiny."""
    probs = torch.softmax(scores.to(torch.float64), dim=-1)
    live = probs[probs > 0]
    return float(((live - float(thr)).abs() / float(thr)).min())
