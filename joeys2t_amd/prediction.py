"""Decode / validation driver: the numerically relevant part of the reference's `predict` batch loop
(joeynmt/prediction.py:154-245): sort by source length -> [validation loss | reference scoring] -> search -> un-sort (n-best
expanded) -> ids to tokens (cut at EOS).  Dataset plumbing, logging, BLEU/chrF and checkpoint handling are out of scope.

The validation leg (prediction.py:165-200): the model runs "as during training" under no_grad, the batch loss, the number of
correct tokens and the token count are summed over ranks (`ddp_reduce`) and over batches; with `return_prob="ref"` no search runs -
the log-probabilities of the reference tokens are looked up instead (`ddp_merge` of log-probs and targets, `Batch.score`).
Reference quirks, stated rather than copied:
  * its loop asks the model for return_type="loss" also when it goes on to score the references - that 4-tuple carries the loss
    components in slots 1-2, not log-probabilities (model.py:133-150), so `Batch.score` cannot have worked there; this driver asks
    for "loss_probs" when it needs log-probabilities.  tests/golden/predict_loss.npz holds both calls' outputs of the reference model.
  * it computes the normaliser of the validation loss and then drops it: its valid_scores keep loss / acc / ppl at NaN.  `totals`
    below are what it accumulates; `valid_scores` are upstream JoeyNMT's formulas over them (flagged: not this reference's output)."""
import math
from typing import Dict, Iterable

import numpy as np
import torch

from joeys2t_amd.batch import Batch
from joeys2t_amd.helpers import expand_reverse_index
from joeys2t_amd.helpers_for_ddp import ddp_merge, ddp_reduce, use_ddp
from joeys2t_amd.ctc_search import (confidence_args, context_args, ctc_attention_rescore, ctc_beam_search, decision_args, lm_fusion_arg,
                                     lm_given)
from joeys2t_amd.sampling import MBR_MAX_SAMPLES, sample_args, sample_search
from joeys2t_amd.search import search


def predict(model, batches: Iterable[Batch], *, beam_size: int = 1, beam_alpha: float = -1.0, n_best: int = 1,
            max_output_length: int = -1, min_output_length: int = 1, generate_unk: bool = True,
            return_prob: str = "none", repetition_penalty: float = -1, no_repeat_ngram_size: int = -1,
            return_attention: bool = False, compute_loss: bool = False, normalization: str = "batch", n_gpu: int = 1,
            decoder: str = "attention", ctc_candidates: int = 8, ctc_weight: float = 0.3, lm=None, lm_weight: float = 0.0,
            length_bonus: float = 0.0, lm_fusion: str = "rescore", decision: str = "map", mbr_scale: float = 1.0,
            confidence: bool = False, confidence_scale: float = 1.0, n_samples: int = 1, temperature: float = 1.0, top_k: int = 0,
            top_p: float = 1.0, epsilon: float = 0.0, seed: int = 0, context=None, context_weight: float = 0.0):
    """Returns (id arrays in the ORIGINAL batch order, decoded token lists, scores or None); with `return_attention` a fourth
    element: the attention arrays of greedy search (prediction.py:205-218 hands the same options to `search`, which derives
    `encoder_input` / the forced prefix from the batch); with `compute_loss` a last element, the validation record
    {"totals": {loss, n_correct, ntokens, nseqs}, "normalizer", "valid_scores": {loss, acc, ppl}}.
    return_prob="ref": ids are the reference tokens and scores their log-probabilities (one array per sentence), no search.
    Under a process group every rank passes ITS batches; totals are sums over ranks, and rank 0's outputs hold all ranks'
    sentences in dataset order (`batch.indices`), as in the reference (prediction.py:222-231, 250-257).
    decoder="ctc" (EXTENSION): hypotheses come from the CTC output layer alone - `search.ctc_beam_search` with a beam of `beam_size`
    (any value >= 1) over the `ctc_candidates` best labels of every frame; scores (with return_prob="hyp") are the log-probabilities
    of the labellings; the options of the attention decoder (beam_alpha, output lengths, penalties, attention) do not apply.
    decoder="ctc-attention" (EXTENSION): two-pass decoding - `search.ctc_attention_rescore`: the `beam_size` best CTC hypotheses are
    scored by the attention decoder in one teacher-forced pass and re-ranked by ctc_weight * ctc + (1 - ctc_weight) * attention;
    scores are the combined ones.  `ctc_weight` is read by this decoder only.
    lm / lm_weight / length_bonus (EXTENSION): an n-gram LM over the target vocabulary (joeys2t_amd.lm.NGramLM) and a bonus per label,
    handed to the two CTC decoders, which re-rank their n-best list with them on the device; the attention decoder has no place
    for them and refuses them.  lm_fusion="search" (EXTENSION; default "rescore") applies them inside the CTC beam of either CTC
    decoder instead (shallow fusion, `search.ctc_beam_search`); the attention decoder refuses it too.
    decision="mbr" / mbr_scale (EXTENSION; default "map"): the two CTC decoders rank their n-best list by minimum Bayes risk - the
    smallest expected edit distance to the list under the softmax of mbr_scale * score - instead of by score (`search.ctc_beam_search`);
    the hypotheses of a sentence then come in ascending risk, each with its model score.  The attention decoder refuses them.
    context / context_weight (EXTENSION): contextual biasing - a joeys2t_amd.biasing.ContextGraph of phrases that matter for these
    batches and the boost per matched token, applied inside the CTC beam of either CTC decoder (`search.ctc_beam_search`); a phrase
    token outside a frame's `ctc_candidates` best labels is still not proposed.  The attention decoder refuses them; a weight that is
    not finite, or non-zero without a graph, is refused before a model is touched.
    confidence / confidence_scale (EXTENSION): token confidence from the n-best list of the two CTC decoders
    (`search.ctc_beam_search`): the return value gains a LAST element {"token": [one np.float32 array per returned hypothesis, its
    tokens' confidences, in the original order of the ids], "hypothesis": np.float32 array, each hypothesis' own posterior}.  It
    says how much of the list's mass agrees with a token; it is no calibrated probability.  The attention decoder has no such list
    and refuses them, return_prob="ref" runs no search and refuses them, and under a process group confidence=True is refused:
    merging ragged per-token arrays across ranks is out of scope here.
    decoder="sample" (EXTENSION) / n_samples, temperature, top_k, top_p, epsilon, seed: `search.sample_search` - n_samples draws per
    sentence from the attention decoder under temperature / top-k / nucleus / epsilon truncation, from ONE device generator seeded
    with `seed` and carried across the batches.  decision="map" (the default) returns the draws in draw order and needs n_best ==
    n_samples; decision="mbr" returns the n_best draws of smallest expected edit distance to the sentence's draws (sampled MBR, uniform
    posterior: mbr_scale has nothing to scale).  Scores (return_prob="hyp") are the draws' log-probabilities under the model.  The
    options of the other decoders (lm*, lm_fusion, context*, confidence*, ctc_*, beam_alpha, repetition_penalty, no_repeat_ngram_size,
    return_attention) are refused, the six sampling options are refused with any other decoder unless at their defaults, and under a
    process group the decoder is refused: merging is out of scope, as for confidence."""
    if decoder not in ("attention", "ctc", "ctc-attention", "sample"):
        raise ValueError(f"predict: decoder '{decoder}' is none of 'attention', 'ctc', 'ctc-attention', 'sample'")
    sample = decoder == "sample"
    n_samples, temperature, top_k, top_p, epsilon = sample_args("predict", n_samples, temperature, top_k, top_p, epsilon)
    if not sample and (n_samples, temperature, top_k, top_p, epsilon, int(seed)) != (1, 1.0, 0, 1.0, 0.0, 0):
        raise ValueError(f"predict: n_samples / temperature / top_k / top_p / epsilon / seed belong to decoder='sample', not to "
                         f"decoder='{decoder}'")
    if decoder == "attention" and lm_given(lm, lm_weight, length_bonus):
        raise ValueError("predict: lm / lm_weight / length_bonus re-rank the n-best list of decoder='ctc' or 'ctc-attention'; "
                         "decoder='attention' cannot apply them")
    lm_fusion_arg("predict", lm_fusion)  # (the value alone: without an lm or a bonus the decoder refuses "search")
    if decoder == "attention" and lm_fusion != "rescore":
        raise ValueError("predict: lm_fusion applies to the CTC beam of decoder='ctc' or 'ctc-attention'; decoder='attention' has none")
    mbr, mbr_scale = decision_args("predict", decision, mbr_scale)
    biased, context_weight = context_args("predict", context, context_weight)
    if decoder == "attention" and (context is not None or biased):
        raise ValueError("predict: context / context_weight bias the CTC beam of decoder='ctc' or 'ctc-attention'; decoder='attention' has none")
    if decoder == "attention" and mbr:
        raise ValueError("predict: decision='mbr' ranks the n-best list of decoder='ctc' or 'ctc-attention'; decoder='attention' has "
                         "no such list")
    confidence, confidence_scale = confidence_args("predict", confidence, confidence_scale)
    if decoder == "attention" and confidence:
        raise ValueError("predict: confidence=True votes over the n-best list of decoder='ctc' or 'ctc-attention'; decoder='attention' has "
                         "no such list")
    if confidence and return_prob == "ref":
        raise ValueError("predict: confidence=True with return_prob='ref' (no search runs: there is no n-best list to vote)")
    if confidence and use_ddp():
        raise ValueError("predict: confidence=True under a process group (per-token arrays are not merged across ranks)")
    if sample:
        other = {"lm / lm_weight / length_bonus": lm_given(lm, lm_weight, length_bonus), "lm_fusion": lm_fusion != "rescore",
                 "context / context_weight": context is not None or biased, "confidence": confidence,
                 "ctc_candidates / ctc_weight": ctc_candidates != 8 or ctc_weight != 0.3, "beam_alpha": beam_alpha != -1.0,
                 "mbr_scale": mbr_scale != 1.0, "repetition_penalty": repetition_penalty != -1,
                 "no_repeat_ngram_size": no_repeat_ngram_size != -1, "return_attention": bool(return_attention)}
        for name, given in other.items():
            if given:
                raise ValueError(f"predict: {name} belongs to another decoder; decoder='sample' draws from the attention decoder and "
                                 f"has no place for it")
        if not mbr and n_best != n_samples:
            raise ValueError(f"predict: decoder='sample' with decision='map' returns the draws in draw order: n_best {n_best} must equal "
                             f"n_samples {n_samples}")
        if mbr and not (2 <= n_samples <= MBR_MAX_SAMPLES and 1 <= n_best <= n_samples):
            raise ValueError(f"predict: decoder='sample' with decision='mbr' ranks 2..{MBR_MAX_SAMPLES} samples and returns 1..n_samples "
                             f"of them, got n_samples {n_samples}, n_best {n_best}")
        if use_ddp():
            raise ValueError("predict: decoder='sample' under a process group (the draws are not merged across ranks)")
    sample_gen = None
    lm_kw = {} if not lm_given(lm, lm_weight, length_bonus) else \
        dict(lm=lm, lm_weight=lm_weight, length_bonus=length_bonus)  # nothing given: the decoders are called as they always were
    if lm_fusion != "rescore":
        lm_kw = dict(lm_kw, lm_fusion=lm_fusion)  # (without an lm or a bonus the decoder refuses it)
    if mbr:
        lm_kw = dict(lm_kw, decision="mbr", mbr_scale=mbr_scale)
    if biased:
        lm_kw = dict(lm_kw, context=context, context_weight=context_weight)
    if confidence:
        lm_kw = dict(lm_kw, confidence=True, confidence_scale=confidence_scale)
    tok_conf, hyp_conf = [], []
    ctc = decoder in ("ctc", "ctc-attention")  # hypotheses of this rank's rows, whatever beam_size is
    model.eval()
    all_ids, all_scores, all_att, by_index = [], [], [], {}
    totals: Dict[str, float] = {"loss": 0.0, "n_correct": 0, "ntokens": 0, "nseqs": 0}
    ddp = use_ddp()
    for batch in batches:
        device = batch.src.device
        batch_nseqs = int(ddp_reduce(batch.nseqs, device, torch.long).item())  # = all ranks' sentences under DDP
        sort_reverse_index = expand_reverse_index(batch.sort_by_src_length(), n_best)
        ids = scores = att = None
        if compute_loss and batch.has_trg:
            assert model.loss_function is not None
            with torch.no_grad():  # run as during training to get the validation loss; log-probabilities only when they are used
                batch_loss, slot1, _, n_correct = model(return_type="loss_probs" if return_prob == "ref" else "loss",
                                                        return_prob=return_prob, return_attention=return_attention, **vars(batch))
            batch_loss, n_correct = ddp_reduce(batch_loss.detach().float()), ddp_reduce(n_correct)
            batch_ntokens = ddp_reduce(int(batch.ntokens), device, torch.long)
            batch_loss = batch.normalize(batch_loss, "sum", n_gpu=n_gpu)  # sum over multiple GPUs (DataParallel's vector of losses)
            n_correct = batch.normalize(n_correct, "sum", n_gpu=n_gpu)
            if return_prob == "ref":
                log_probs = ddp_merge(slot1, 0.0)
                batch_trg = ddp_merge(batch.trg, model.pad_index)
                scores = Batch.score(log_probs, batch_trg, model.pad_index)
                ids = batch_trg.detach().cpu().numpy()
            totals["loss"] += float(batch_loss.sum().item())
            totals["n_correct"] += int(n_correct.sum().item())
            totals["ntokens"] += int(batch_ntokens.sum().item())
        if return_prob != "ref" and decoder == "ctc-attention":
            ids, scores, lens, *parts = ctc_attention_rescore(model, batch, beam_size=beam_size, n_best=n_best, candidates=ctc_candidates,
                                                              ctc_weight=ctc_weight, **lm_kw)
            scores = scores if return_prob == "hyp" else None
        elif return_prob != "ref" and ctc:
            ids, scores, lens, *parts = ctc_beam_search(model, batch, beam_size=beam_size, n_best=n_best, candidates=ctc_candidates, **lm_kw)
            scores = scores if return_prob == "hyp" else None
        elif return_prob != "ref" and sample:
            if sample_gen is None:  # one generator for all batches: a later batch continues the stream
                sample_gen = torch.Generator(device=device)
                sample_gen.manual_seed(int(seed))
            ids, scores, lens = sample_search(model, batch, n_samples=n_samples, max_output_length=max_output_length,
                                              min_output_length=min_output_length, temperature=temperature, top_k=top_k, top_p=top_p,
                                              epsilon=epsilon, generate_unk=generate_unk, decision="mbr" if mbr else "none", n_best=n_best,
                                              generator=sample_gen)
            scores = scores if return_prob == "hyp" else None
        elif return_prob != "ref":
            ids, scores, att = search(model=model, batch=batch, beam_size=beam_size, beam_alpha=beam_alpha, n_best=n_best,
                                      max_output_length=max_output_length, min_output_length=min_output_length,
                                      generate_unk=generate_unk, return_prob=return_prob,
                                      repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                      return_attention=return_attention)
        if ddp:
            # Hypotheses are merged ONCE: greedy search returns all ranks' rows already (its tail merges ids, scores and attention as
            # the reference's does, search.py:333-335); beam search returns this rank's rows, so they are merged here (extension: the
            # reference's beam search does not merge, and its assert below then fails for world_size > 1).  The order of merged
            # outputs is unknown: they are put back by `indices` after the loop (prediction.py:222-231).
            if return_prob != "ref" and (beam_size >= 2 or ctc):
                ids = ddp_merge(torch.as_tensor(np.asarray(ids), device=device), model.pad_index).cpu().numpy()
                if scores is not None:
                    scores = ddp_merge(torch.as_tensor(np.asarray(scores), device=device), 0.0).cpu().numpy()
            batch_indices = ddp_merge(batch.indices.to(device).unsqueeze(1), -1).squeeze(1)
            assert bool(torch.all(batch_indices >= 0)) and len(batch_indices) * n_best == len(ids) == batch_nseqs * n_best, \
                (len(batch_indices), len(ids), batch_nseqs)
            have_scores = scores is not None and len(scores) == len(ids)
            for k, index in enumerate(batch_indices.cpu().tolist()):
                # keyed by dataset index: a sentence the sampler handed out twice (its padding to a multiple of the world size)
                # is kept once, the later copy overwriting the earlier one as in the reference (`_all_outputs[i] = row`, :250-257)
                rows = slice(k * n_best, (k + 1) * n_best)
                by_index[int(index)] = (list(ids[rows]), list(scores[rows]) if have_scores else None,
                                        att[k] if att is not None else None)
        else:
            all_ids.extend(ids[sort_reverse_index])  # either hypotheses or references
            if confidence:
                tok_conf.extend(parts[0]["token_confidence"][i, :int(lens[i])].copy() for i in sort_reverse_index)
                hyp_conf.extend(parts[0]["confidence"][sort_reverse_index])
            if att is not None:
                all_att.extend(att[sort_reverse_index])
            if scores is not None and len(scores) == len(sort_reverse_index):
                all_scores.extend(scores[sort_reverse_index])
        totals["nseqs"] += batch_nseqs
    if ddp:
        for index in sorted(by_index):  # dataset order; the n-best rows of a sentence stay together
            rows, row_scores, row_att = by_index[index]
            all_ids.extend(rows)
            if row_scores is not None:
                all_scores.extend(row_scores)
            if row_att is not None:
                all_att.append(row_att)
    sentences = model.trg_vocab.arrays_to_sentences(all_ids, cut_at_eos=True)
    out = [all_ids, sentences, (all_scores if len(all_scores) else None)]
    if return_attention:
        out.append(all_att if all_att else None)
    if compute_loss:
        normalizer = {"batch": totals["nseqs"], "tokens": totals["ntokens"], "none": 1}[normalization]
        assert normalizer > 0 and totals["ntokens"] > 0, (normalizer, totals)
        valid_scores = {"loss": totals["loss"] / normalizer, "acc": totals["n_correct"] / totals["ntokens"],
                        "ppl": math.exp(totals["loss"] / totals["ntokens"])}  # upstream JoeyNMT; this reference leaves them NaN
        out.append({"totals": totals, "normalizer": normalizer, "valid_scores": valid_scores})
    if confidence:
        out.append({"token": tok_conf, "hypothesis": np.asarray(hyp_conf, dtype=np.float32)})
    return tuple(out)
