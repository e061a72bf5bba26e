"""The decoders over the CTC output layer (EXTENSION; the reference hands out ctc_out, model.py:162-166, without a consumer):
`ctc_greedy`, `ctc_beam_search` (the n-best list of CTC prefix beam search) and `ctc_attention_rescore` (that list re-scored by the
attention decoder).  search.py re-exports the three.

The two n-best decoders are one chain of stages over one list, each stage one function here and each ops call made once:
    first pass -> [attention] -> [n-gram] -> [context] -> [MBR] -> row selection -> parts -> [confidence]
`NBestOptions` (built and checked once per call) says which of the optional stages run and documents the options; `NBest`
carries the list between the stages.  Where the two decoders differ it shows in the stages they call and the arguments they pass
- which Lp the list carries, whether the n-gram stage runs behind a fused search, when the model rank is taken - never in a stage
asking who called it."""
import math

import numpy as np
import torch

from joeys2t_amd import ops
from joeys2t_amd.helpers import tile


def ctc_greedy(model, batch):
    """CTC best-path decoding of the encoder-side output layer (the reference's `decode_ctc` return type hands
    out ctc_out, model.py:162-166, without a consumer): encode once, project with `decoder.ctc_output_layer`, take the
    frame-wise arg-max inside each utterance's sub-sampled length (model.py:125), merge repeats, drop blanks
    (blank = BOS, model.py:84).  Returns NumPy (ids i64[B, T'] pad-filled, lengths i64[B])."""
    layer = getattr(model.decoder, "ctc_output_layer", None)
    if layer is None:
        raise ValueError("ctc_greedy: the model has no CTC output layer (loss: crossentropy-ctc)")
    with torch.no_grad():
        encoder_output, _, src_mask, _ = model(return_type="encode", **vars(batch))
        ctc_out = model.decoder.project(layer, encoder_output, model.runtime.compute_dtype)  # [B, T', V]
        B, T, V = ctc_out.shape
        _, best = ops.row_lse(ctc_out.reshape(B * T, V), want_argmax=True)
        in_len = src_mask.squeeze(1).sum(dim=1)
        ids, n = ops.ctc_collapse(best.view(B, T), in_len, model.bos_index, model.pad_index)
    return ids.cpu().numpy(), n.cpu().numpy()


# ---------------------------------------------------------------- the options
def ngram_args(who, lm, lm_weight, length_bonus):
    """(re-rank at all?, lm_weight, length_bonus) of the LM options"""
    lm_weight, length_bonus = float(lm_weight), float(length_bonus)
    if not (math.isfinite(lm_weight) and math.isfinite(length_bonus)):
        raise ValueError(f"{who}: lm_weight {lm_weight} / length_bonus {length_bonus} not finite")
    if lm is None and lm_weight != 0.0:
        raise ValueError(f"{who}: lm_weight {lm_weight} without an lm")
    return lm is not None or length_bonus != 0.0, lm_weight, length_bonus


def lm_given(lm, lm_weight, length_bonus) -> bool:
    """is any of the LM options set? (none: a caller leaves all three out of the call)"""
    return lm is not None or float(lm_weight) != 0.0 or float(length_bonus) != 0.0


def lm_fusion_arg(who, lm_fusion, rerank=True):
    """is the LM fused into the beam ("search") instead of re-ranking its n-best list ("rescore", the default)?  (rerank left out: the
    value alone is checked)"""
    if lm_fusion not in ("rescore", "search"):
        raise ValueError(f"{who}: lm_fusion '{lm_fusion}' is neither 'rescore' nor 'search'")
    if lm_fusion == "search" and not rerank:
        raise ValueError(f"{who}: lm_fusion='search' without an lm or a length_bonus")
    return lm_fusion == "search"


def context_args(who, context, context_weight):
    """(bias at all?, context_weight) of the contextual-biasing options"""
    context_weight = float(context_weight)
    if not math.isfinite(context_weight):
        raise ValueError(f"{who}: context_weight {context_weight} not finite")
    if context is None and context_weight != 0.0:
        raise ValueError(f"{who}: context_weight {context_weight} without a context graph")
    return context is not None and context_weight != 0.0, context_weight


def decision_args(who, decision, mbr_scale):
    """(rank by minimum Bayes risk?, mbr_scale) of the decision options"""
    if decision not in ("map", "mbr"):
        raise ValueError(f"{who}: decision '{decision}' is neither 'map' nor 'mbr'")
    mbr_scale = float(mbr_scale)
    if not (math.isfinite(mbr_scale) and mbr_scale > 0.0):
        raise ValueError(f"{who}: mbr_scale {mbr_scale} not finite and above 0")
    if decision == "map" and mbr_scale != 1.0:
        raise ValueError(f"{who}: mbr_scale {mbr_scale} with decision='map' (it scales the posterior of decision='mbr')")
    return decision == "mbr", mbr_scale


def confidence_args(who, confidence, confidence_scale):
    """(token confidence wanted?, confidence_scale) of the confidence options"""
    confidence_scale = float(confidence_scale)
    if not (math.isfinite(confidence_scale) and confidence_scale > 0.0):
        raise ValueError(f"{who}: confidence_scale {confidence_scale} not finite and above 0")
    if not confidence and confidence_scale != 1.0:
        raise ValueError(f"{who}: confidence_scale {confidence_scale} without confidence=True (it scales the posterior of the votes)")
    return bool(confidence), confidence_scale


class NBestOptions:
    """The ten options the two n-best decoders share, checked (every refusal is a ValueError raised before the model is touched, with
    `who` in front of its message; the checks run in the order n-gram, context, fusion, decision, confidence) and reduced to what the
    stages ask; nothing changes it afterwards.  Each decoder's docstring says what a stage's base score is there.

    lm / lm_weight / length_bonus (`rerank`: an lm, or a non-zero bonus): the list is re-ranked on the device by
        base + lm_weight * lm + length_bonus * n, lm = the log-probability a joeys2t_amd.lm.NGramLM over the target vocabulary gives
        the labels and EOS behind them (js2t_ngram_rescore).  Refused: a weight or bonus that is not finite; a weight without an lm.
    lm_fusion ("rescore", the default, is the line above; `fused`: "search"): the LM and the bonus act INSIDE the beam instead
        (shallow fusion, js2t_ctc_beam_search_lm): every frame prunes by ctc + lm_weight * lm + length_bonus * n, so a labelling the
        LM prefers survives where the CTC score alone would have dropped it.  Refused: another value; "search" without `rerank`.
    context / context_weight (`biased`: a joeys2t_amd.biasing.ContextGraph of phrases that matter for this batch, and a non-zero
        boost per matched token): the search is js2t_ctc_beam_search_ctx - every frame prunes by ctc + context_weight * m, m = the
        tokens of the prefix inside completed phrases or the partial match at its end, and the final score counts completed phrases
        only.  Biasing acts inside the beam, always: there is no "rescore" mode for it.  The LM and the bonus take part in that kernel
        only when `fused`.  Biasing adds no candidates: a phrase token that is not among a frame's `candidates` (<= 8) best labels is
        still not proposed.  The parts gain "context" i32, the matched tokens of every row.  Refused: a weight that is not finite, or
        non-zero without a graph.
    decision / mbr_scale (`mbr`: "mbr"; the default "map" returns the best-scored rows): the whole list of n_rescore slots is scored
        as with "map" and then ranked on the device by the expected edit distance to the list under the posterior
        softmax(mbr_scale * score) (js2t_mbr_rescore); the n_best first are returned.  The rows of an utterance are then in ASCENDING
        RISK, not in descending score; the scores column keeps each row's model score, the value the row would carry with "map".  A
        hypothesis of more than ops.edit_max_len() labels takes no part (it is ranked last).  The parts gain "risk" and "posterior"
        f32 and "map_rank" i64, the row's rank within its utterance by the model score.  Refused: another decision; a scale that is not
        finite and above 0, or one other than 1 with "map".
    confidence / confidence_scale (`confidence`; token confidence from the list, js2t_nbest_confidence): the whole list of n_rescore
        slots is searched for and scored as under "mbr", the ranking stays whatever `decision` says, and every token of the returned
        rows gets the posterior mass, under softmax(confidence_scale * score), of the list entries whose Levenshtein alignment with
        the row matches it.  The call then returns the parts dict as with return_parts=True, with two more entries:
        "token_confidence" f32 [B * n_best, L], 0 behind each row's length, and "confidence" f32 [B * n_best], the row's own
        posterior.  Ids, scores and lengths are those of the same call without it.  It says how much of the LIST's mass agrees with a
        token: it is no calibrated probability.  Refused: a scale that is not finite and above 0, or one other than 1 without it.
    `wide`: mbr or confidence - the whole list of n_rescore slots is wanted, not the n_best first alone."""
    def __init__(self, who, lm, lm_weight, length_bonus, lm_fusion, decision, mbr_scale, confidence, confidence_scale, context, context_weight):
        self.lm = lm
        self.rerank, self.lm_weight, self.length_bonus = ngram_args(who, lm, lm_weight, length_bonus)
        self.biased, self.context_weight = context_args(who, context, context_weight)
        self.context = context if self.biased else None
        self.fused = lm_fusion_arg(who, lm_fusion, self.rerank)
        self.mbr, self.mbr_scale = decision_args(who, decision, mbr_scale)
        self.confidence, self.confidence_scale = confidence_args(who, confidence, confidence_scale)
        self.wide = self.mbr or self.confidence


# ---------------------------------------------------------------- the list and its stages (all inside the caller's no_grad)
class NBest:
    """The n-best list between the stages.  ids i64 [B, N, T] as the beam kernel wrote it, n i32 [R] (R = B * N), ctc f32 [R] the pure
    CTC score, score f32 [R] the last stage's score, order i32 [B, N] the last stage's ranking (None: the list as the search left it,
    best first), ctx i32 [R] the context counts of whichever stage counted last (None: no graph), Lp: the bound on lengths + 1 the
    stages pass on - the table's width + 1 unless the caller has read the lengths.  The stages add what the parts need: tok_lp / att,
    lm_tok / lm_score, map_rank, posterior / risk."""

    def __init__(self, ids, n, ctc, score, ctx):
        self.B, self.N, self.T = ids.shape
        R = self.B * self.N
        self.ids, self.n, self.ctc, self.score = ids, n.reshape(R), ctc.reshape(R), score.reshape(R)
        self.ctx = None if ctx is None else ctx.reshape(R)
        self.order, self.Lp = None, self.T + 1
        self.tok_lp = self.att = self.lm_tok = self.lm_score = self.map_rank = self.posterior = self.risk = None

    def ranking(self):
        """order, or the slots themselves where no stage ranked"""
        return self.order if self.order is not None else torch.arange(self.N, device=self.ids.device, dtype=torch.int32).expand(self.B, self.N)


def _to(thing, dev):
    if thing is not None and thing.device != dev:
        thing.to(dev)
    return thing


def _search(model, logits, in_len, pack, beam_size, N, candidates, opt: NBestOptions):
    """The n-best search over CTC logits that are there already - [B, T, V], or with `pack` (ops.PackedRows) packed rows [pack.rows, V];
    in_len i64 [B] - for both callers, the utterance decoders through `_first_pass` and long_form.transcribe_long over its segments:
    pick the candidates of every frame and search for the N best prefixes (blank = BOS) with the plain kernel, the LM-fused one when
    opt.fused, the biased one whenever opt.biased (the LM in it only when fused), the lm and the graph moved to the device if need
    be.  The list's score is the search's own: ctc itself unless fused or biased."""
    V = logits.shape[-1]
    logits = logits.float().contiguous()  # js2t_beam_pick reads f32
    cand_id, cand_lp, lse = ops.ctc_beam_candidates(logits.view(-1, V), min(int(candidates), V - 1), model.bos_index)
    search = (logits, lse, cand_id, cand_lp, in_len, beam_size, N, model.bos_index, model.pad_index)
    in_beam = (_to(opt.lm, logits.device), model.bos_index, model.eos_index, opt.lm_weight, opt.length_bonus) if opt.fused else \
        (None, model.bos_index, model.eos_index, 0.0, 0.0)  # lm_fusion="rescore": the LM stays behind the search
    ctx = None
    if opt.biased:
        ids, n, score, ctc, _, ctx = ops.ctc_beam_search_ctx(*search, *in_beam, _to(opt.context, logits.device), opt.context_weight, pack=pack)
    elif opt.fused:
        ids, n, score, ctc, _ = ops.ctc_beam_search_lm(*search, *in_beam, pack=pack)
    else:
        ids, n, ctc = ops.ctc_beam_search(*search, pack=pack)
        score = ctc
    return NBest(ids, n, ctc, score, ctx)


def _first_pass(model, batch, who, beam_size, N, candidates, opt: NBestOptions, want_encoder=False):
    """Encode once, project, and search (`_search`).  Returns (list, [encoder output, its mask] with want_encoder)."""
    from joeys2t_amd.alignment import _ctc_frames
    ctc_out, _, in_len, *enc = _ctc_frames(model, batch, who=who, want_lse=False, want_encoder=want_encoder)
    return _search(model, ctc_out, in_len, None, beam_size, N, candidates, opt), enc


def _attention_stage(model, lst: NBest, encoder_output, src_mask, ctc_weight):
    """The list scored by the attention decoder in one teacher-forced pass over its R rows and ranked by ctc_weight * ctc +
    (1 - ctc_weight) * attention (js2t_rescore); lst.Lp says how long the pass is.  The decoder input is [BOS, labels...] with the
    target mask made from the LENGTHS (a hypothesis may contain pad or EOS as labels)."""
    R, N, Lp, dev = lst.B * lst.N, lst.N, lst.Lp, lst.ids.device
    trg_input = torch.cat([torch.full((R, 1), model.bos_index, dtype=torch.int64, device=dev), lst.ids.view(R, lst.T)[:, :Lp - 1]], dim=1).contiguous()
    trg_mask = (torch.arange(Lp, device=dev)[None, :] <= lst.n.view(R, 1)).unsqueeze(1)  # [R, 1, Lp] from the lengths, not from pad ids
    dec_logits, _, _, _ = model(return_type="decode", trg_input=trg_input, encoder_output=tile(encoder_output.contiguous(), N, dim=0),
                                encoder_hidden=None, src_mask=tile(src_mask, N, dim=0), unroll_steps=None, decoder_hidden=None,
                                trg_mask=trg_mask)
    lst.tok_lp, lst.att, lst.score, lst.order = ops.rescore(dec_logits.contiguous(), lst.ids, lst.n, lst.ctc, N, model.eos_index, ctc_weight)


def _ngram_stage(model, lst: NBest, opt: NBestOptions, want_tokens=False):
    """the list re-ranked by the n-gram LM and the length bonus over the model's vocabulary on top of lst.score"""
    lst.lm_tok, lst.lm_score, lst.score, lst.order = ops.ngram_rescore(
        lst.ids, lst.n, lst.score, lst.N, _to(opt.lm, lst.ids.device), model.bos_index, model.eos_index, opt.lm_weight, opt.length_bonus,
        Lp=lst.Lp, want_tokens=want_tokens, V=len(model.trg_vocab))


def _context_stage(lst: NBest, opt: NBestOptions):
    """the context term counted over the list as it is and added on top of lst.score (a search that was biased kept these labellings
    alive; its own count gives way to this one)"""
    lst.ctx, lst.score, lst.order = ops.context_rescore(lst.ids, lst.n, lst.score, lst.N, opt.context, opt.context_weight, Lp=lst.Lp)


def _map_rank_stage(lst: NBest):
    """i64 [R]: the rank of every slot by the model score - the inverse of the ranking so far"""
    slots = torch.arange(lst.N, device=lst.ids.device, dtype=torch.int64).expand(lst.B, lst.N)
    rank = slots if lst.order is None else torch.empty((lst.B, lst.N), dtype=torch.int64, device=slots.device).scatter_(1, lst.order.to(torch.int64), slots)
    lst.map_rank = rank.reshape(lst.B * lst.N)


def _mbr_stage(lst: NBest, opt: NBestOptions, Lp):
    """the same list and scores, ranked by the expected edit distance instead"""
    _, lst.posterior, lst.risk, lst.order = ops.mbr_rescore(lst.ids, lst.n, lst.score, lst.N, opt.mbr_scale, Lp=Lp)


def _ragged(tok, out_n):
    tok = tok.cpu().numpy()
    return [tok[i, :int(out_n[i]) + 1].copy() for i in range(len(out_n))]


def _parts(lst: NBest, rows, slot, out_n) -> dict:
    """per-returned-row NumPy data of whatever the stages that ran left on the list (each decoder's docstring names its keys)"""
    parts = {}
    if lst.att is not None:
        parts.update({"ctc": lst.ctc[rows].cpu().numpy(), "attention": lst.att[rows].cpu().numpy(), "token_log_probs": _ragged(lst.tok_lp[rows], out_n),
                      "ctc_rank": slot.reshape(-1).cpu().numpy()})
    if lst.lm_tok is not None:
        parts["lm"], parts["lm_token_log_probs"] = lst.lm_score[rows].cpu().numpy(), _ragged(lst.lm_tok[rows], out_n)
    if lst.map_rank is not None:
        parts["map_rank"] = lst.map_rank[rows].cpu().numpy()
    if lst.risk is not None:
        parts["risk"], parts["posterior"] = lst.risk[rows].cpu().numpy(), lst.posterior[rows].cpu().numpy()
    if lst.ctx is not None:
        parts["context"] = lst.ctx[rows].cpu().numpy()
    return parts


def _confidence_stage(lst: NBest, opt: NBestOptions, n_best, parts, L):
    """adds "token_confidence" f32 [B * n_best, L] (0 behind each row's length) and "confidence" f32 [B * n_best] to `parts`: the
    votes of the whole list of N slots for the tokens of the returned rows"""
    Lp = min(lst.Lp, ops.edit_max_len() + 1)  # what an edit table takes: a longer hypothesis is dead to it
    _, conf, hyp = ops.nbest_confidence(lst.ids, lst.n, lst.score, lst.N, lst.ranking()[:, :n_best].contiguous(), opt.confidence_scale, Lp=Lp)
    conf = conf.reshape(lst.B * n_best, Lp - 1).cpu().numpy()
    tok = np.zeros((lst.B * n_best, L), dtype=np.float32)
    tok[:, :min(L, Lp - 1)] = conf[:, :L]
    parts["token_confidence"], parts["confidence"] = tok, hyp.reshape(lst.B * n_best).cpu().numpy()


def _finish(lst: NBest, opt: NBestOptions, n_best, return_parts):
    """Row selection - the n_best first of every utterance by the ranking, or the list as it is where it is those rows already - and
    the decoders' return layout: NumPy ids i64 [B * n_best, L] cut to the longest hypothesis (L at least 1), scores f32 [B * n_best, 1],
    lengths i64 [B * n_best]; with return_parts the parts, and the confidence votes in them."""
    rows, slot = slice(None), None  # (a view: no gather)
    if lst.order is not None or lst.N != n_best:
        slot = lst.ranking()[:, :n_best].to(torch.int64)
        rows = (slot + torch.arange(lst.B, device=slot.device)[:, None] * lst.N).reshape(lst.B * n_best)
    n = lst.n[rows].cpu().numpy().astype(np.int64)
    L = max(int(n.max()) if n.size else 0, 1)
    out = np.ascontiguousarray(lst.ids.view(lst.B * lst.N, lst.T)[rows].cpu().numpy()[:, :L]), lst.score[rows].cpu().numpy().reshape(n.size, 1), n
    if not return_parts:
        return out
    parts = _parts(lst, rows, slot, n)
    if opt.confidence:
        _confidence_stage(lst, opt, n_best, parts, L)
    return (*out, parts)


# ---------------------------------------------------------------- the two decoders
def nbest_slots(who, opt: NBestOptions, beam_size, n_best, n_rescore):
    """(beam_size, n_best, the slots to search for) of the encoder-only decoder - `ctc_beam_search`, and long_form.transcribe_long
    over its segments - with that decoder's refusals of n_best / n_rescore (its docstring states them)"""
    if not 1 <= n_best <= beam_size:
        raise ValueError(f"{who}: n_best {n_best} outside 1..beam_size ({beam_size})")
    if opt.fused and not opt.wide:
        if n_rescore is not None:
            raise ValueError(f"{who}: n_rescore with lm_fusion='search' (the LM is in the beam: there is no list to re-rank)")
    elif opt.rerank or opt.wide:
        n_rescore = int(beam_size if n_rescore is None else n_rescore)
        if not n_best <= n_rescore <= beam_size:
            raise ValueError(f"{who}: n_best {n_best} <= n_rescore {n_rescore} <= beam_size {beam_size} expected")
    elif n_rescore is not None:
        raise ValueError(f"{who}: n_rescore without an lm or a length_bonus")
    beam_size, n_best = int(beam_size), int(n_best)
    return beam_size, n_best, n_rescore if opt.wide or (opt.rerank and not opt.fused) else n_best


def ctc_stages(model, lst: NBest, opt: NBestOptions, n_best, return_parts):
    """the stages of the encoder-only decoder behind its search, and its return layout (inside the caller's no_grad)"""
    if opt.rerank and not opt.fused:  # (a fused search has applied the LM already)
        _ngram_stage(model, lst, opt)
    if return_parts:
        _map_rank_stage(lst)
    if opt.mbr:
        _mbr_stage(lst, opt, min(lst.Lp, ops.edit_max_len() + 1))  # nobody has read the lengths: one above the limit is dead, not refused
    return _finish(lst, opt, n_best, return_parts)


def ctc_beam_search(model, batch, beam_size: int = 10, n_best: int = 1, candidates: int = 8, lm=None, lm_weight: float = 0.0,
                    length_bonus: float = 0.0, n_rescore: int = None, lm_fusion: str = "rescore", decision: str = "map",
                    mbr_scale: float = 1.0, return_parts: bool = False, confidence: bool = False, confidence_scale: float = 1.0,
                    context=None, context_weight: float = 0.0):
    """CTC prefix beam search over the encoder-side output layer alone (EXTENSION; no decoder runs): encode once, project with
    `decoder.ctc_output_layer`, pick the `candidates` (<= 8) most probable labels of every frame and search over them with a beam of
    `beam_size` (<= 32) prefixes, summing over all alignments of a prefix (js2t_ctc_beam_search; blank = BOS, model.py:84).
    Returns NumPy in the row layout of `beam_search`: ids i64 [B * n_best, L] pad-filled (L = the longest hypothesis, at least 1),
    scores f32 [B * n_best, 1] (log-probability of the labelling under the truncated distribution; -inf with an all-pad row where
    an utterance has fewer than n_best prefixes) and lengths i64 [B * n_best].  The options are `NBestOptions`'; here:
    the stages and their base scores: the search's own score (ctc; with lm_fusion="search" the kernel's final score, EOS term
    included; with a graph the biased kernel's final score) is the base of the n-gram stage, which runs under lm_fusion="rescore"
    only, and whatever that leaves is the model score the MBR stage and the confidence votes take.  Lp is the table's width + 1
    throughout: there is no host read between the encoder and the final copy.
    n_rescore (default: beam_size): the slots searched for and re-ranked, n_best <= n_rescore <= beam_size, of which the n_best first
    are returned.  It needs a list to re-rank: it is refused without an lm or a length_bonus, and with lm_fusion="search" (the LM is
    in the beam) - unless decision="mbr" or confidence=True want the whole list, where it is accepted without an LM too and under
    lm_fusion="search" is the fused search's n_best.
    return_parts (confidence=True implies it): a fourth element, a dict of per-returned-row NumPy data: "map_rank" i64 [B * n_best]
    (the row's rank within its utterance by the model score); with decision="mbr" "risk" and "posterior" f32 [B * n_best]; with a graph
    "context" i32 [B * n_best], the beam's own count; with confidence "token_confidence" and "confidence"."""
    opt = NBestOptions("ctc_beam_search", lm, lm_weight, length_bonus, lm_fusion, decision, mbr_scale, confidence, confidence_scale, context,
                        context_weight)
    return_parts = return_parts or opt.confidence
    beam_size, n_best, N = nbest_slots("ctc_beam_search", opt, beam_size, n_best, n_rescore)
    with torch.no_grad():
        lst, _ = _first_pass(model, batch, "ctc_beam_search", beam_size, N, candidates, opt)
        return ctc_stages(model, lst, opt, n_best, return_parts)


def ctc_attention_rescore(model, batch, beam_size: int = 10, n_best: int = 1, candidates: int = 8, ctc_weight: float = 0.3,
                          n_rescore: int = None, return_parts: bool = False, lm=None, lm_weight: float = 0.0,
                          length_bonus: float = 0.0, lm_fusion: str = "rescore", decision: str = "map", mbr_scale: float = 1.0,
                          confidence: bool = False, confidence_scale: float = 1.0, context=None, context_weight: float = 0.0):
    """Two-pass decoding (EXTENSION; the reference has no consumer of ctc_out): the `n_rescore` (default: beam_size; n_best <= n_rescore
    <= beam_size <= 32) best hypotheses of CTC prefix beam search (`ctc_beam_search`: beam_size, candidates) are scored by the
    attention decoder in ONE teacher-forced pass over B * n_rescore rows - no step loop - and re-ranked by ctc_weight * ctc +
    (1 - ctc_weight) * attention, attention = the sum of the log-probabilities of the hypothesis' labels and of EOS behind them
    (js2t_rescore; ctc_weight in [0, 1]).  The encoder runs once; the n-best list, the decoder input and the scores stay on the
    device, with one host read (the longest hypothesis) to size the decoder pass: it sets the Lp every later stage takes.  The
    encoder output and its mask are tiled n_rescore times as `beam_search` does - the padded path: packed encoder rows are not handed
    to the decoder here.
    Returns NumPy in `ctc_beam_search`'s layout: ids i64 [B * n_best, L] pad-filled, scores f32 [B * n_best, 1] (the final score;
    -inf with an all-pad row where an utterance has fewer than n_best prefixes), lengths i64 [B * n_best].  The options are
    `NBestOptions`'; here:
    the stages and their base scores: the first pass is the plain, the LM-fused or the biased search with n_best = n_rescore;
    js2t_rescore takes its pure CTC score, whatever the search pruned by.  The combined score is the base of the n-gram stage, which
    runs with an lm or a bonus under either lm_fusion (under "search" the list that is re-scored already holds the labellings the LM
    prefers); the context term, context_weight * the matched tokens of completed phrases, is added behind it (js2t_context_rescore);
    the MBR stage and the confidence votes take the final score.  Each stage's ranking replaces the one before.
    return_parts (confidence=True implies it): a fourth element, a dict of per-returned-row NumPy data: "ctc" and "attention" f32
    [B * n_best] (the two scores), "token_log_probs" (a list of f32 arrays of n + 1 values, the last one EOS's) and "ctc_rank" i64
    [B * n_best] (the slot of the row in the first pass's list); with an lm or a bonus "lm" f32 [B * n_best] and
    "lm_token_log_probs"; with decision="mbr" "risk", "posterior" and "map_rank"; with a graph "context" i32 [B * n_best]; with
    confidence "token_confidence" and "confidence"."""
    opt = NBestOptions("ctc_attention_rescore", lm, lm_weight, length_bonus, lm_fusion, decision, mbr_scale, confidence, confidence_scale,
                        context, context_weight)
    return_parts = return_parts or opt.confidence
    n_rescore = beam_size if n_rescore is None else n_rescore
    beam_size, n_best, n_rescore, ctc_weight = int(beam_size), int(n_best), int(n_rescore), float(ctc_weight)
    if not 1 <= n_best <= n_rescore <= beam_size <= 32:
        raise ValueError(f"ctc_attention_rescore: n_best {n_best} <= n_rescore {n_rescore} <= beam_size {beam_size} <= 32 expected "
                         "(all at least 1)")
    if not 0.0 <= ctc_weight <= 1.0:  # (a NaN fails too)
        raise ValueError(f"ctc_attention_rescore: ctc_weight {ctc_weight} outside [0, 1]")
    with torch.no_grad():
        lst, (encoder_output, src_mask) = _first_pass(model, batch, "ctc_attention_rescore", beam_size, n_rescore, candidates, opt,
                                                      want_encoder=True)
        lst.Lp = int(lst.n.max().item()) + 1 if lst.n.numel() else 1  # the one host read: it sizes the decoder pass
        _attention_stage(model, lst, encoder_output, src_mask, ctc_weight)
        if opt.rerank:
            _ngram_stage(model, lst, opt, want_tokens=return_parts)
        if opt.biased:
            _context_stage(lst, opt)
        if opt.mbr:
            if return_parts:
                _map_rank_stage(lst)
            _mbr_stage(lst, opt, lst.Lp)  # the lengths were read: Lp is exact, and one the edit table cannot take is refused
        return _finish(lst, opt, n_best, return_parts)
