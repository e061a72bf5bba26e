"""Word confidence from token confidence (EXTENSION; the reference has neither): the per-token figures of
`search.ctc_beam_search(..., confidence=True)` - the posterior mass of the n-best list that agrees with each token
(js2t_nbest_confidence) - merged into one figure per word.  Pure host code.

It says how much of the LIST's mass agrees with a word; whether that is a calibrated probability on real data has not been measured.
"""
from typing import List, Sequence, Tuple

import numpy as np

from joeys2t_amd.alignment import WORD_MARKER

HOW = ("min", "mean", "prod")


def word_confidence(pieces: Sequence[str], token_conf, how: str = "min") -> List[Tuple[str, float]]:
    """Merge `token_conf`, one value per token, into words: `pieces` are the sentence pieces of the tokens, a piece that begins with
    the word marker opens a new word (so does the first piece) - `alignment.word_segments`' rule.  Returns (word, confidence) per
    word, the confidence being the smallest ("min", the default: a word is as sure as its least sure piece), the mean or the product
    ("prod") of its pieces' values.  Values beyond the pieces list (EOS, padding) are left out."""
    if how not in HOW:
        raise ValueError(f"word_confidence: how '{how}' is none of 'min', 'mean', 'prod'")
    conf = np.asarray(token_conf, dtype=np.float64).reshape(-1)
    if len(pieces) > conf.size:
        raise ValueError(f"word_confidence: {len(pieces)} pieces for {conf.size} token confidences")
    words = []
    for i, piece in enumerate(pieces):
        if i == 0 or piece.startswith(WORD_MARKER):
            words.append([piece.lstrip(WORD_MARKER), []])
        else:
            words[-1][0] += piece
        words[-1][1].append(conf[i])
    merge = {"min": np.min, "mean": np.mean, "prod": np.prod}[how]
    return [(w, float(merge(v))) for w, v in words]
