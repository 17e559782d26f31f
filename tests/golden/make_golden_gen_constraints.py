"""Generate tests/golden/gen_constraints.npz from the classes the reference's `_get_logits_processor`
(indextts/gpt/transformers_generation_utils.py:900-1049) instantiates for plain `generate()` keywords (build container only):

    python tests/golden/make_golden_gen_constraints.py

NoRepeatNGramLogitsProcessor, MinNewTokensLengthLogitsProcessor, SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor and
MinPLogitsWarper run on seeded logits rows and histories; the file holds inputs, settings, processed scores and kept masks.  Three short
beam-search traces (do_sample=False, 3 beams, at most 12 steps) come from the reference's own scorer and model forward, made as
make_golden.py::_gen_beam_case makes gpt_beam_search.npz, with the constraint processors behind the repetition penalty.  Data only.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (installs the reference import harness)

WR = MG.WR
V, START, STOP = 1024, 1022, 1023  # vocabulary of the processor cases (the classes know no special ids but eos)
MINP_GUARD = 1e-5


def _procs():
    from transformers.generation import logits_process as LP

    return LP


def _rows(g, n=1, scale=6.0):
    return torch.randn(n, V, generator=g) * scale


def processor_cases():
    """[(name, settings dict, history, P, logits)] -> processed scores by the reference classes, in the chain's order."""
    LP = _procs()
    g = torch.Generator().manual_seed(2024)
    cases = []

    def add(name, history, P, n=0, min_new=0, suppress=(), begin=()):
        logits = _rows(g)
        ids = torch.tensor([history], dtype=torch.long)
        s = logits.clone()
        if n:
            s = LP.NoRepeatNGramLogitsProcessor(n)(ids, s)
        if min_new:
            s = LP.MinNewTokensLengthLogitsProcessor(P, min_new, STOP, device="cpu")(ids, s)
        if len(suppress):
            s = LP.SuppressTokensLogitsProcessor(list(suppress), device="cpu")(ids, s)
        if len(begin):
            s = LP.SuppressTokensAtBeginLogitsProcessor(list(begin), P, device="cpu")(ids, s)
        cases.append(dict(name=name, history=np.array(history), P=P, n=n, min_new=min_new, suppress=np.array(list(suppress), dtype=np.int64),
                          begin=np.array(list(begin), dtype=np.int64), logits=logits[0].numpy(), scores=s[0].numpy()))

    P = 9
    pre = [1] * (P - 1) + [START]
    add("ngram3_repeat", pre + [11, 700, 256, 11, 700], P, n=3)           # 256 follows the earlier (11, 700)
    add("ngram2_repeat", pre + [11, 700, 256, 11, 700], P, n=2)
    add("ngram2_overlap", pre + [7, 7, 7], P, n=2)                        # the window (7, 7) overlaps the suffix
    add("ngram3_overlap", pre + [5, 5, 5, 5], P, n=3)
    add("ngram3_ones_prefix", pre + [1, 1], P, n=3)                       # the fake prefix counts: 1 and start banned
    add("ngram4_ones_prefix_start", pre + [40, 1, 1, START], P, n=4)      # (1, 1, start) occurred at the end of the prefix: bans 40
    add("ngram1", pre + [33, 900, 33, 4], P, n=1)                         # every id of the history, 1 and start included
    add("ngram8_short", [1, START], 2, n=8)                               # no complete n-gram yet
    add("ngram8_long", pre + list(range(100, 108)) + [500] + list(range(100, 107)), P, n=8)
    add("ngram_none", pre + [11, 700, 256, 12, 700], P, n=3)
    add("min_new_before", pre + [3, 4], P, min_new=3)
    add("min_new_at", pre + [3, 4, 5], P, min_new=3)
    add("suppress", pre + [3], P, suppress=(0, 17, STOP))
    add("begin_first", pre, P, begin=(17, 18))
    add("begin_later", pre + [17], P, begin=(17, 18))
    add("all", pre + [11, 700, 256, 11, 700], P, n=3, min_new=9, suppress=(5,), begin=(6,))
    add("all_first", pre, P, n=1, min_new=1, suppress=(5,), begin=(6,))
    return cases


def min_p_cases():
    """MinPLogitsWarper after Temperature / TopK / TopP, with min_tokens_to_keep 1 (no beams) and 2 (beams)."""
    LP = _procs()
    out = []
    seed = 77
    for name, T, k, p, mp, keep in (("minp_all", 4.0, 0, 1.0, 0.3, 1), ("minp_topk_topp", 1.5, 30, 0.9, 0.2, 1), ("minp_all_keep2", 4.0, 0, 1.0, 0.9, 2),
                                    ("minp_topk_keep2", 1.0, 30, 1.0, 0.999, 2), ("minp_one", 1.3, 0, 0.95, 1.0, 1)):
        while True:  # a condition on the INPUTS: no surviving probability within MINP_GUARD (relative) of the threshold
            g = torch.Generator().manual_seed(seed)
            seed += 1
            logits = _rows(g, scale=2.0)
            ids = torch.tensor([[1, START]], dtype=torch.long)
            s = logits.clone()
            if T != 1.0:
                s = LP.TemperatureLogitsWarper(T)(ids, s)
            if k:
                s = LP.TopKLogitsWarper(k, min_tokens_to_keep=keep)(ids, s)
            if p < 1.0:
                s = LP.TopPLogitsWarper(p, min_tokens_to_keep=keep)(ids, s)
            probs = torch.softmax(s[0].double(), -1)
            thr = mp * float(probs.max())
            live = probs[probs > 0]
            if float(((live - thr).abs() / thr).min()) > MINP_GUARD or mp == 1.0:
                break
        kept = LP.MinPLogitsWarper(mp, min_tokens_to_keep=keep)(ids, s.clone())
        out.append(dict(name=name, temperature=T, top_k=k, top_p=p, min_p=mp, min_keep=keep, logits=logits[0].numpy(), scores=kept[0].numpy()))
    return out


def beam_case(stop_bias, rng_seed, n=0, min_new=0, suppress=(), nb=3, max_new=12, theta=10.0):
    """Beam search proper through the reference's BeamSearchScorer + model forward (make_golden.py::_gen_beam_case), processors =
    RepetitionPenalty(theta) -> NoRepeatNGram -> MinNewTokens -> SuppressTokens."""
    from indextts.gpt.transformers_beam_search import BeamSearchScorer

    LP = _procs()
    cfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    W = WR.make_gpt_weights(cfg, seed=31, head_scale=50.0)
    W["mel_head.bias"] = W["mel_head.bias"].clone()
    W["mel_head.bias"][8193] += stop_bias
    uv = MG.build_ref_gpt(cfg, W)
    g = torch.Generator().manual_seed(rng_seed)
    D = cfg["model_dim"]
    conds_latent = torch.randn(34, D, generator=g) * 0.5
    text = torch.randint(2, 200, (10,), generator=g).to(torch.int32)
    VV = 8194
    input_ids, embeds, mask = uv.prepare_gpt_inputs(conds_latent.unsqueeze(0), text.unsqueeze(0))
    P = input_ids.shape[1]
    model = uv.inference_model
    model.store_mel_emb(embeds)
    procs = [LP.RepetitionPenaltyLogitsProcessor(theta)] if theta != 1.0 else []
    if n:
        procs.append(LP.NoRepeatNGramLogitsProcessor(n))
    if min_new:
        procs.append(LP.MinNewTokensLengthLogitsProcessor(P, min_new, 8193, device="cpu"))
    if len(suppress):
        procs.append(LP.SuppressTokensLogitsProcessor(list(suppress), device="cpu"))
    scorer = BeamSearchScorer(batch_size=1, num_beams=nb, device="cpu", length_penalty=0.0, do_early_stopping=False, num_beam_hyps_to_keep=1,
                              max_length=P + max_new)
    input_ids = input_ids.repeat_interleave(nb, dim=0)
    mask = mask.repeat_interleave(nb, dim=0)
    beam_scores = torch.zeros(nb)
    beam_scores[1:] = -1e9
    past = None
    all_picks, all_ns, all_nt, all_ni = [], [], [], []
    next_tokens = next_indices = None
    for step in range(max_new):
        inp = model.prepare_inputs_for_generation(input_ids, past_key_values=past, attention_mask=mask, use_cache=True)
        out = model(**inp, return_dict=True)
        past = out.past_key_values
        scores = torch.log_softmax(out.logits[:, -1, :].float(), dim=-1)
        for pr in procs:
            scores = pr(input_ids, scores)
        scores = scores + beam_scores[:, None]
        sc, picks = torch.topk(scores.view(1, nb * VV), 2 * nb, dim=1, largest=True, sorted=True)
        next_indices = torch.div(picks, VV, rounding_mode="floor")
        next_tokens = picks % VV
        bo = scorer.process(input_ids, sc, next_tokens, next_indices, pad_token_id=8193, eos_token_id=8193, decoder_prompt_len=P)
        beam_scores = bo["next_beam_scores"]
        bt, bi = bo["next_beam_tokens"], bo["next_beam_indices"]
        all_picks.append(picks[0].clone())
        all_ns.append(beam_scores.clone())
        all_nt.append(bt.clone())
        all_ni.append(bi.clone())
        input_ids = torch.cat([input_ids[bi, :], bt.unsqueeze(-1)], dim=-1)
        mask = torch.cat([mask, torch.ones(nb, 1, dtype=mask.dtype)], dim=1)
        if hasattr(past, "reorder_cache"):
            past.reorder_cache(bi)
        else:
            past = model._reorder_cache(past, bi)
        if scorer.is_done:
            break
    fin = scorer.finalize(input_ids, beam_scores, next_tokens, next_indices, pad_token_id=8193, eos_token_id=8193, max_length=P + max_new,
                          decoder_prompt_len=P)
    return dict(stop_bias=stop_bias, theta=theta, conds_latent=conds_latent, text=text, max_new=max_new, n=n, min_new=min_new, suppress=np.array(list(suppress), dtype=np.int64),
                picks=torch.stack(all_picks), next_scores=torch.stack(all_ns), next_tokens=torch.stack(all_nt), next_indices=torch.stack(all_ni),
                sequence=fin["sequences"][0, P:], sequence_score=fin["sequence_scores"], done=int(bool(scorer.is_done)))


def main():
    out = dict(V=V, start=START, stop=STOP)
    names = []
    for c in processor_cases():
        names.append(c["name"])
        out.update({f"{c['name']}_{k}": v for k, v in c.items() if k != "name"})
        print(c["name"], "banned", int(np.isinf(c["scores"]).sum()))
    out["cases"] = np.array(names)
    names = []
    for c in min_p_cases():
        names.append(c["name"])
        out.update({f"{c['name']}_{k}": v for k, v in c.items() if k != "name"})
        print(c["name"], "kept", int((~np.isinf(c["scores"])).sum()))
    out["min_p_cases"] = np.array(names)
    # beam traces: the stop token would win step 0 without min_new_tokens; n = 1; the unconstrained trace's first tokens suppressed
    free = beam_case(60.0, 91)
    assert int(free["picks"][0][0]) % 8194 == 8193, "the stop bias must make the stop token the best candidate of step 0"
    r = beam_case(60.0, 91, min_new=4)
    assert 8193 not in r["next_tokens"][:4].flatten().tolist() and not (r["picks"][:4] % 8194 == 8193).any()
    traces = {"min_new": r}
    plain = beam_case(4.0, 94, theta=1.0)  # without the repetition penalty the unconstrained best beam repeats a token at step 7
    traces["ngram1"] = beam_case(4.0, 94, n=1, theta=1.0)
    assert len(set(plain["sequence"].tolist())) < 12 and len(set(traces["ngram1"]["sequence"].tolist())) == 12
    assert traces["ngram1"]["next_tokens"].tolist() != plain["next_tokens"].tolist(), "the ban must change the trace"
    plain3 = beam_case(4.0, 93)
    first = [int(t) for t in plain3["next_tokens"][0]]
    traces["suppress"] = beam_case(4.0, 93, suppress=first)
    assert not set(first) & set(traces["suppress"]["next_tokens"].flatten().tolist())
    for tag, r in traces.items():
        print(tag, "steps", r["picks"].shape[0], "done", r["done"], "seq", r["sequence"].tolist())
        out.update({f"beam_{tag}_{k}": v for k, v in r.items()})
    out["beam_cases"] = np.array(list(traces))
    out["beam_seed"] = 31
    path = os.path.join(HERE, "gen_constraints.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()})
    print(f"wrote gen_constraints.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
