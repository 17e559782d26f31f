"""Generate tests/golden/gen_processors.npz from the classes the reference's `_get_logits_processor`
(indextts/gpt/transformers_generation_utils.py:862-1069) instantiates for the other half of `generate()`'s plain keywords (build
container only):

    python tests/golden/make_golden_gen_processors.py

SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor, ForcedEOSTokenLogitsProcessor, ExponentialDecayLengthPenalty,
EpsilonLogitsWarper, EtaLogitsWarper and LogitNormalization run, at their place in the chain, on seeded logits rows of V = 1024 and
short histories; the file holds inputs, settings (as JSON text), processed scores.  Three short beam-search traces (do_sample=False,
3 beams, at most 12 steps) come from the reference's own scorer and model forward, made as make_golden.py::_gen_beam_case makes
gpt_beam_search.npz, with the new processors at their chain position.  Data only.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (installs the reference import harness)

WR = MG.WR
V, START, STOP = 1024, 1022, 1023  # vocabulary of the processor cases (the classes know no special ids but eos)
GUARD = 1e-5                       # no live probability within this (relative) of a cutoff's threshold


def _lp():
    from transformers.generation import logits_process as LP

    return LP


def chain(cfg, P, eos, keep=1):
    """The processors of `cfg` in `_get_logits_processor` order."""
    LP = _lp()
    procs = []
    if cfg.get("table"):
        procs.append(LP.SequenceBiasLogitsProcessor({tuple(ids): float(b) for ids, b in cfg["table"]}))
    if cfg.get("theta", 1.0) != 1.0:
        procs.append(LP.RepetitionPenaltyLogitsProcessor(cfg["theta"]))
    if cfg.get("n"):
        procs.append(LP.NoRepeatNGramLogitsProcessor(cfg["n"]))
    if cfg.get("bad_words"):
        procs.append(LP.NoBadWordsLogitsProcessor([list(w) for w in cfg["bad_words"]], eos))
    if cfg.get("min_new"):
        procs.append(LP.MinNewTokensLengthLogitsProcessor(P, cfg["min_new"], eos, device="cpu"))
    if cfg.get("forced"):
        procs.append(LP.ForcedEOSTokenLogitsProcessor(cfg["max_length"], list(cfg["forced"]), device="cpu"))
    if cfg.get("decay"):
        procs.append(LP.ExponentialDecayLengthPenalty((int(cfg["decay"][0]), float(cfg["decay"][1])), eos, P))
    if cfg.get("suppress"):
        procs.append(LP.SuppressTokensLogitsProcessor(list(cfg["suppress"]), device="cpu"))
    if cfg.get("sampling"):
        if cfg.get("temperature", 1.0) != 1.0:
            procs.append(LP.TemperatureLogitsWarper(cfg["temperature"]))
        if cfg.get("top_k"):
            procs.append(LP.TopKLogitsWarper(cfg["top_k"], min_tokens_to_keep=keep))
        if cfg.get("top_p", 1.0) < 1.0:
            procs.append(LP.TopPLogitsWarper(cfg["top_p"], min_tokens_to_keep=keep))
        if cfg.get("min_p"):
            procs.append(LP.MinPLogitsWarper(cfg["min_p"], min_tokens_to_keep=keep))
        if cfg.get("epsilon"):
            procs.append(LP.EpsilonLogitsWarper(cfg["epsilon"], min_tokens_to_keep=keep))
        if cfg.get("eta"):
            procs.append(LP.EtaLogitsWarper(cfg["eta"], min_tokens_to_keep=keep, device="cpu"))
    if cfg.get("renorm"):
        procs.append(LP.LogitNormalization())
    return procs


def run(procs, history, logits):
    ids = torch.tensor([history], dtype=torch.long)
    s = logits.clone()
    for pr in procs:
        s = pr(ids, s)
    return s


def processor_cases():
    g = torch.Generator().manual_seed(4711)
    row = torch.randn(1, V, generator=g) * 6.0  # every case's logits: this row with the case's `fix` ({id: value}) written into it
    cases = [dict(name="row", logits=row[0].numpy())]

    def add(name, history, P, fix=None, **cfg):
        logits = row.clone()
        for t, v in (fix or {}).items():
            logits[0, t] = v
        s = run(chain(cfg, P, STOP), history, logits)
        assert not torch.isnan(s).any(), name
        cases.append(dict(name=name, history=np.array(history), P=P, cfg=json.dumps(cfg), fix=json.dumps(fix or {}), scores=s[0].numpy()))
        return logits[0], s[0]

    P = 9
    pre = [1] * (P - 1) + [START]
    add("bias_one_id", pre + [3], P, table=[[[5], -3.0]])
    seq8 = [100, 101, 102, 103, 104, 105, 106]
    lg, s = add("bias_8_ids_match", pre + [9] + seq8, P, table=[[seq8 + [700], 4.0]])
    assert s[700] == lg[700] + 4.0
    lg, s = add("bias_8_ids_no_match", pre + [9] + seq8[:-1] + [99], P, table=[[seq8 + [700], 4.0]])
    assert torch.equal(s, lg)
    lg, s = add("bias_prefix_in_fake_prompt", pre + [40], P, table=[[[1, START, 40, 50], 2.5]])  # [..., 1, start_mel, x]
    assert s[50] == lg[50] + 2.5
    lg, s = add("bias_longer_than_history", [1, START], 2, table=[[[1, START, 7], 2.0], [[START, 8], 1.0]])  # P = 2: the 3-id entry is ignored
    assert s[7] == lg[7] and s[8] == lg[8] + 1.0
    lg, s = add("bias_two_on_one_id", pre + [3], P, table=[[[9], 2.0], [[3, 9], 1.5], [[4, 9], 8.0]])
    assert abs(float(s[9] - lg[9]) - 3.5) < 1e-5
    # a positive bias on a seen id whose raw score is negative, penalty 10: (-2 + 5) / 10 = 0.3 -- the other order gives -15
    lg, s = add("bias_before_penalty", pre + [77], P, fix={77: -2.0}, theta=10.0, table=[[[77], 5.0]])
    assert abs(float(s[77]) - 0.3) < 1e-6
    lg, s = add("bad_word_eos_dropped", pre + [3], P, bad_words=[[STOP], [4], [3, 6], [2, 8]])
    assert torch.isfinite(s[STOP]) and s[4] == -np.inf and s[6] == -np.inf and s[8] == lg[8]
    lg, s = add("bad_word_then_forced_eos", pre + [3, 4], P, bad_words=[[4, STOP]], forced=[STOP], max_length=P + 3)
    assert s[STOP] == 0 and int(torch.isfinite(s).sum()) == 1  # ForcedEOS sits behind NoBadWords
    lg, s = add("bad_word_not_yet_forced", pre + [4], P, bad_words=[[4, STOP]], forced=[STOP], max_length=P + 3)
    assert s[STOP] == -np.inf and int(torch.isfinite(s).sum()) == V - 1  # one step before ForcedEOS's step
    lg, s = add("forced_eos_two_ids", pre + [3, 4], P, forced=[STOP, 17], max_length=P + 3, suppress=[17])
    assert s[STOP] == 0 and s[17] == -np.inf  # SuppressTokens sits behind it
    lg, s = add("forced_eos_over_min_new", pre + [3, 4], P, forced=[STOP], max_length=P + 3, min_new=50)
    assert s[STOP] == 0
    lg, s = add("decay_at_start", pre + [3, 4, 5], P, decay=[3, 1.5])
    assert torch.equal(s, lg)
    lg, s = add("decay_start_plus_1_positive", pre + [3, 4, 5, 6], P, fix={STOP: 2.0}, decay=[3, 1.5])
    assert float(s[STOP]) == 3.0
    lg, s = add("decay_start_plus_1_negative", pre + [3, 4, 5, 6], P, fix={STOP: -2.0}, decay=[3, 1.5])
    assert float(s[STOP]) == -1.0
    add("decay_far_positive", pre + list(range(200, 800)), P, fix={STOP: 1.7}, decay=[5, 1.01])
    add("decay_far_negative", pre + list(range(200, 800)), P, fix={STOP: -9.3}, decay=[5, 1.01], theta=10.0)
    add("everything", pre + [3, 4, 3], P, theta=10.0, table=[[[3], 1.0], [[4, 3, 11], -2.0]], n=2, bad_words=[[3, 12]], min_new=2, decay=[1, 1.2],
        suppress=[13])
    return cases


def warper_cases():
    """EpsilonLogitsWarper / EtaLogitsWarper behind Temperature / TopK / TopP / MinP, min_tokens_to_keep 1 (no beams) and 2
    (beams); LogitNormalization behind warpers."""
    sys.path.insert(0, os.path.dirname(HERE))
    import gen_processors_ref as R

    out = []
    seed = 300
    table = (
        # name, scale, T, top_k, top_p, min_p, epsilon, eta, keep, renorm, which eta term must be the smaller
        ("eps_k30_keep1", 2.0, 1.5, 30, 1.0, 0.0, 0.02, 0.0, 1, False, None),
        ("eps_k0_keep1", 2.0, 1.0, 0, 1.0, 0.0, 3e-3, 0.0, 1, False, None),
        ("eps_k30_keep2", 6.0, 1.0, 30, 1.0, 0.0, 0.4, 0.0, 2, False, None),
        ("eps_k0_keep2", 6.0, 1.0, 0, 1.0, 0.0, 0.4, 0.0, 2, False, None),
        ("eta_k30_keep1_peaked", 6.0, 1.0, 30, 1.0, 0.0, 0.0, 0.02, 1, False, "eps"),
        ("eta_k0_keep1_flat", 0.5, 1.0, 0, 1.0, 0.0, 0.0, 0.09, 1, False, "entropy"),
        ("eta_k30_keep2_flat", 1.0, 1.0, 30, 1.0, 0.0, 0.0, 0.6, 2, False, "entropy"),
        ("eta_k0_keep2_peaked", 6.0, 1.0, 0, 1.0, 0.0, 0.0, 0.3, 2, False, "eps"),
        ("eps_eta_all_warpers", 2.0, 1.3, 30, 0.9, 0.05, 0.03, 0.06, 1, False, None),
        ("renorm_after_warpers", 2.0, 1.5, 30, 0.9, 0.0, 0.03, 0.0, 1, True, None),
    )
    for name, scale, T, k, p, mp, eps, eta, keep, renorm, term in table:
        cfg = dict(sampling=True, temperature=T, top_k=k, top_p=p, min_p=mp, epsilon=eps, eta=eta, renorm=renorm)
        while True:  # a condition on the INPUTS: no live probability within GUARD (relative) of a cutoff's threshold
            g = torch.Generator().manual_seed(seed)
            seed += 1
            logits = torch.randn(1, V, generator=g) * scale
            before = run(chain(dict(cfg, epsilon=0.0, eta=0.0, renorm=False), 2, STOP, keep), [1, START], logits)[0]
            ok = True
            if eps:
                ok = ok and R.cut_margin(before, eps) > GUARD
                before = run(chain(dict(cfg, eta=0.0, renorm=False), 2, STOP, keep), [1, START], logits)[0]
            if eta:
                thr = float(R.eta_threshold(before, eta))
                ok = ok and R.cut_margin(before, thr) > GUARD
                if term is not None:
                    ok = ok and (thr == np.float32(eta)) == (term == "eps")
            if ok:
                break
        s = run(chain(cfg, 2, STOP, keep), [1, START], logits)[0]
        n_before, n_after = int(torch.isfinite(before).sum()), int(torch.isfinite(s).sum())
        uncut = run(chain(dict(cfg, epsilon=0.0, eta=0.0), 2, STOP, keep), [1, START], logits)[0]
        assert keep <= n_after < int(torch.isfinite(uncut).sum()), (name, n_after)
        print(name, "kept", n_after, "of", int(torch.isfinite(uncut).sum()), "(eta sees", n_before, ")")
        out.append(dict(name=name, cfg=json.dumps(cfg), min_keep=keep, logits=logits[0].numpy(), scores=s.numpy()))
    return out


def beam_case(stop_bias, rng_seed, cfg, nb=3, max_new=12):
    """Beam search proper through the reference's BeamSearchScorer + model forward (make_golden.py::_gen_beam_case) under
    `chain(cfg)`; ForcedEOS is given max_length = P + max_new here."""
    from indextts.gpt.transformers_beam_search import BeamSearchScorer

    gcfg = WR.tiny_gpt_cfg(model_dim=128, layers=2, heads=2)
    W = WR.make_gpt_weights(gcfg, seed=31, head_scale=50.0)
    W["mel_head.bias"] = W["mel_head.bias"].clone()
    W["mel_head.bias"][8193] += stop_bias
    uv = MG.build_ref_gpt(gcfg, W)
    g = torch.Generator().manual_seed(rng_seed)
    D = gcfg["model_dim"]
    conds_latent = torch.randn(34, D, generator=g) * 0.5
    text = torch.randint(2, 200, (10,), generator=g).to(torch.int32)
    VV = 8194
    input_ids, embeds, mask = uv.prepare_gpt_inputs(conds_latent.unsqueeze(0), text.unsqueeze(0))
    P = input_ids.shape[1]
    model = uv.inference_model
    model.store_mel_emb(embeds)
    cfg = dict(cfg)
    if cfg.get("forced"):
        cfg["max_length"] = P + max_new
    procs = chain(cfg, P, 8193)
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
    return dict(stop_bias=stop_bias, cfg=json.dumps({k: v for k, v in cfg.items() if k != "max_length"}), conds_latent=conds_latent, text=text, max_new=max_new,
                picks=torch.stack(all_picks), next_scores=torch.stack(all_ns), next_tokens=torch.stack(all_nt), next_indices=torch.stack(all_ni),
                sequence=fin["sequences"][0, P:], sequence_score=fin["sequence_scores"], done=int(bool(scorer.is_done)))


def main():
    out = dict(V=V, start=START, stop=STOP)
    for group, cases in (("cases", processor_cases()), ("warper_cases", warper_cases())):
        for c in cases:
            out.update({f"{c['name']}_{k}": v for k, v in c.items() if k != "name"})
        out[group] = np.array([c["name"] for c in cases if c["name"] != "row"])
        print(group, len(cases))
    plain = beam_case(4.0, 93, dict(theta=10.0))
    seq = [int(t) for t in plain["sequence"]]
    assert 8193 not in seq and len(seq) == 12 and not plain["done"], "the free trace must run past every cap below"
    traces = {}
    # a two-id bad word on the free trace's best beam, a one-id bias on a later token of it, a two-id bias that matches after its first token
    third = int(plain["next_tokens"][1][2])
    traces["bias_bad_words"] = beam_case(4.0, 93, dict(theta=10.0, table=[[[seq[3]], -6.0], [[seq[0], third], 3.0]], bad_words=[[seq[0], seq[1]], [8193]]))
    assert traces["bias_bad_words"]["next_tokens"].tolist() != plain["next_tokens"].tolist(), "the table must change the trace"
    traces["forced_eos"] = beam_case(4.0, 93, dict(theta=10.0, forced=[8193]), max_new=7)
    assert traces["forced_eos"]["sequence"].tolist() == seq[:6] + [8193], traces["forced_eos"]["sequence"].tolist()
    traces["renorm"] = beam_case(4.0, 93, dict(theta=10.0, renorm=True))
    assert not np.allclose(traces["renorm"]["next_scores"].numpy(), plain["next_scores"].numpy(), atol=1e-2), "renormalisation must move the beam scores"
    for tag, r in traces.items():
        print(tag, "steps", r["picks"].shape[0], "done", r["done"], "seq", r["sequence"].tolist())
        out.update({f"beam_{tag}_{k}": v for k, v in r.items()})
    out["beam_cases"] = np.array(list(traces))
    out["beam_seed"] = 31
    path = os.path.join(HERE, "gen_processors.npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()})
    print(f"wrote gen_processors.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
