"""Sampling from the attention decoder (EXTENSION: the reference's decoder takes the arg-max or runs a beam, search.py:162-825; it
has no sampling): N draws per utterance under temperature / top-k / nucleus / epsilon truncation, and the minimum-Bayes-risk choice
among them (epsilon sampling + MBR, the usual recipe of MT / ST).

The step is `IncrementalDecoder.step` (one replayed graph over N rows per utterance and ONE copy of the encoder keys / values) followed
by ONE launch of js2t_sample_step, which truncates, renormalises, draws and keeps ids / finished / score / length on the device.  The
rule of a draw is the kernel's contract (include/joeys2t_hip.h) and is restated in float64 in tests/sampling_reference.py."""
import math

import numpy as np
import torch

from joeys2t_amd import ops
from joeys2t_amd.incremental import IncrementalDecoder

MBR_MAX_SAMPLES = 32  # the list kernels' N (js2t_mbr_rescore)


def sample_args(who, n_samples, temperature, top_k, top_p, epsilon):
    """The five sampling options, checked: -> (n_samples, temperature, top_k, top_p, epsilon).  Every refusal is a ValueError with
    `who` in front."""
    if int(n_samples) != n_samples or n_samples < 1:
        raise ValueError(f"{who}: n_samples {n_samples} below 1")
    temperature, top_p, epsilon = float(temperature), float(top_p), float(epsilon)
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"{who}: temperature {temperature} not finite and above 0")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"{who}: top_k {top_k} is no count (0 switches it off)")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"{who}: top_p {top_p} outside (0, 1] (1 switches it off)")
    if not 0.0 <= epsilon < 1.0:
        raise ValueError(f"{who}: epsilon {epsilon} outside [0, 1) (0 switches it off)")
    return int(n_samples), temperature, int(top_k), top_p, epsilon


def sample_search(model, batch, n_samples: int = 1, max_output_length: int = -1, min_output_length: int = 1, temperature: float = 1.0,
                  top_k: int = 0, top_p: float = 1.0, epsilon: float = 0.0, seed: int = 0, generate_unk: bool = True,
                  decision: str = "none", n_best: int = None, return_parts: bool = False, generator=None):
    """Draw `n_samples` hypotheses per utterance from the attention decoder.  Encode once; row b * n_samples + k is sample k of
    utterance b; all rows advance together through `IncrementalDecoder` (n_samples in {2, 4, 5, 8} takes its grouped cross-attention
    path, which reads an utterance's keys / values once for all its samples; other values take the ungrouped one).  Per step: the
    decoder's graph, `torch.rand(rows)` from a device generator, one js2t_sample_step.  The ids table, finished flags, scores and
    lengths live on the device; the host looks at `finished.all()` every `search.SYNC_EVERY` steps and cuts off the steps past the
    stopping point, as the greedy loop does.  max_output_length < 0: `search()`'s rule (1.5 x the longest source).
    temperature / top_k / top_p / epsilon: js2t_sample_step's rule - the kept set is the prefix (raw logit descending, id ascending)
    that survives epsilon (probability under the temperature >= epsilon, at least one), top-k and then the nucleus of what is left;
    the draw is from its renormalised masses.  Forbidden ids are `search()`'s greedy list (BOS, SEP, language tags, UNK without
    generate_unk, EOS below min_output_length).
    Random numbers: a `torch.Generator` on the device seeded with `seed`; a caller's `generator` wins (predict passes one across its
    batches).  Same seed, same bits.
    Returns NumPy (ctc_beam_search's layout): ids i64 [B * n_best, L] - labels only, pad behind each length, no EOS stored, L = the
    longest row and at least 1; scores f32 [B * n_best, 1] - the sum of the drawn tokens' log-probabilities under the MODEL (whatever
    the truncation), the EOS term included when EOS was drawn; lengths i64 [B * n_best].
    decision="none": all n_samples rows of an utterance in draw order (n_best None or n_samples).
    decision="mbr": sampled MBR - js2t_mbr_rescore over the table with ALL-ZERO scores, i.e. the uniform Monte-Carlo posterior over
    the draws: a hypothesis drawn twice counts twice, which is the model's probability entering by multiplicity; weighting by the
    model score as well would count it twice.  The n_best (default 1) first rows come in ascending risk, ties in draw order.  It
    needs 2 <= n_samples <= 32; lengths beyond ops.edit_max_len() are refused once they are known.
    return_parts: a fourth element, per returned row: "sampling_log_prob" f32 (the sum of the log-probabilities under the
    distribution drawn from), "slot" i64 (the draw index), with mbr "risk" f32.
    Not built: best-of-N by model score, confidence votes over samples, repetition penalty / n-gram blocking in the sampler, prompted
    batches."""
    who = "sample_search"
    n_samples, temperature, top_k, top_p, epsilon = sample_args(who, n_samples, temperature, top_k, top_p, epsilon)
    if decision not in ("none", "mbr"):
        raise ValueError(f"{who}: decision '{decision}' is neither 'none' nor 'mbr'")
    mbr = decision == "mbr"
    if n_best is None:
        n_best = 1 if mbr else n_samples
    if int(n_best) != n_best or not 1 <= n_best <= n_samples:
        raise ValueError(f"{who}: n_best {n_best} outside 1..n_samples = {n_samples}")
    if not mbr and n_best != n_samples:
        raise ValueError(f"{who}: n_best {n_best} with decision='none', which returns all n_samples = {n_samples} draws")
    if mbr and not 2 <= n_samples <= MBR_MAX_SAMPLES:
        raise ValueError(f"{who}: decision='mbr' ranks 2..{MBR_MAX_SAMPLES} samples, got n_samples {n_samples}")
    if batch is not None and getattr(batch, "trg_prompt_mask", None) is not None:
        raise ValueError(f"{who}: a prompted batch (trg_prompt_mask) needs forced decoding, which the sampler does not do")
    if not hasattr(model.decoder, "layers") or not hasattr(model.decoder, "pe"):
        raise ValueError(f"{who}: the model's decoder is no Transformer decoder (the incremental decoder runs that one only)")
    n_best = int(n_best)
    with torch.no_grad():
        encoder_output, _, src_mask, _ = model(return_type="encode", **vars(batch))
    src_mask = src_mask if batch.src_mask is None else batch.src_mask
    if max_output_length < 0:
        max_output_length = int(max(batch.src_length.cpu().numpy()) * 1.5)
    from joeys2t_amd.search import SYNC_EVERY, _forbidden
    dev = encoder_output.device
    B, V, N = encoder_output.shape[0], model.decoder.output_size, n_samples
    rows, max_len = B * N, max(int(max_output_length), 1)
    eos, pad = model.eos_index, model.pad_index
    if generator is None:
        generator = torch.Generator(device=dev)
        generator.manual_seed(int(seed))
    inc = IncrementalDecoder(model, encoder_output, src_mask, N, max_len)
    table = torch.full((rows, max_len), pad, dtype=torch.int64, device=dev)
    finished = torch.zeros((rows, ), dtype=torch.uint8, device=dev)
    score = torch.zeros((rows, ), dtype=torch.float32, device=dev)
    length = torch.zeros((rows, ), dtype=torch.int32, device=dev)
    logp = torch.empty((rows, ), dtype=torch.float32, device=dev)
    q_steps = torch.zeros((max_len, rows), dtype=torch.float32, device=dev)
    done = torch.zeros((max_len, ), dtype=torch.uint8, device=dev)  # has every row ended after step s?
    last = torch.full((rows, ), model.bos_index, dtype=torch.int64, device=dev)
    n_steps = max_len
    for step in range(max_len):
        logits = inc.step(last)
        u = torch.rand((rows, ), generator=generator, device=dev, dtype=torch.float32)
        ops.sample_step(logits, u, table, step, _forbidden(model, False, generate_unk, step, min_output_length, V), eos, pad,
                        temperature=temperature, top_k=top_k, top_p=top_p, epsilon=epsilon, finished=finished, score=score,
                        length=length, out=(logp, q_steps[step], None, None))
        last = table[:, step]
        done[step:step + 1].copy_(finished.min().view(1))
        if (step + 1) % SYNC_EVERY == 0 or step + 1 == max_len:  # the one host read of the loop
            flags = done[:step + 1].cpu()
            if bool(flags.any()):
                n_steps = int(torch.nonzero(flags)[0]) + 1  # what ran past the stopping point drew nothing: finished rows write pad
                break
    lens_dev = length
    n_host = length.cpu().numpy().astype(np.int64)
    longest = max(int(n_host.max()) if rows else 0, 1)
    keep = torch.arange(rows, device=dev)
    parts = {}
    if mbr:
        if longest > ops.edit_max_len():
            raise ValueError(f"{who}: decision='mbr' with a sample of {longest} labels, beyond the edit-distance kernel's {ops.edit_max_len()}")
        tab = table[:, :longest].contiguous()
        _, _, risk, order = ops.mbr_rescore(tab, lens_dev, torch.zeros_like(score), N)
        slot = order[:, :n_best].to(torch.int64)
        keep = (torch.arange(B, device=dev).unsqueeze(1) * N + slot).reshape(-1)
        parts["risk"] = risk[keep].cpu().numpy()
    keep_host = keep.cpu().numpy()
    lengths = n_host[keep_host]
    L = max(int(lengths.max()) if len(lengths) else 0, 1)
    ids = table[keep, :max(L, 1)].cpu().numpy()
    if ids.shape[1] < L:  # (a table shorter than one column cannot be: max_len >= 1)
        ids = np.pad(ids, ((0, 0), (0, L - ids.shape[1])), constant_values=pad)
    ids[np.arange(L)[None, :] >= lengths[:, None]] = pad  # the EOS a row drew is not stored
    scores = score[keep].cpu().numpy().reshape(-1, 1)
    if not return_parts:
        return ids, scores, lengths
    parts["sampling_log_prob"] = q_steps[:n_steps].sum(0)[keep].cpu().numpy()
    parts["slot"] = (keep_host % N).astype(np.int64)
    return ids, scores, lengths, parts
