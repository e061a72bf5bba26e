"""Back-off n-gram language model over the target vocabulary (EXTENSION; the reference has no language model): an ARPA reader and
the builder of the device table that js2t_ngram_rescore reads (include/joeys2t_hip.h states the layout, joeys2t_amd/csrc/ngram.hpp
is its device side).  Plain Python and NumPy; torch is touched only by `.to(device)`.

The LM's "words" are the vocabulary's tokens (SentencePiece pieces, BPE units, characters or words - whatever trg_vocab holds), so
a hypothesis' ids are looked up as they are.  Layout:
    uni   f32 [V, 2]          (logp, backoff) of every id, natural logarithms
    table ENTRY [capacity]    {u64 key, f32 logp, f32 backoff}: the 2-grams .. order-grams, open addressing, linear probing with
                              wrap-around, home slot fmix(key) & (capacity - 1), capacity a power of two
    key of (w1 .. wk)         field j (0 = newest = wk) = id + 1 in bits 16j .. 16j+15; 0 = empty
    max_probe                 the largest distance of a stored key from its home, plus 1: a lookup may stop after that many slots
"""
import math
import os
from typing import Dict, Iterable, NamedTuple, Tuple, Union

import numpy as np

MAX_ORDER = 4
MAX_V = 65535
ENTRY = np.dtype([("key", "<u8"), ("logp", "<f4"), ("backoff", "<f4")])  # 16 bytes
LN10 = math.log(10.0)


class Arpa(NamedTuple):
    order: int
    counts: Dict[int, int]
    ngrams: Dict[Tuple[str, ...], Tuple[float, float]]  # (w1 .. wk) -> (log10 p, log10 backoff; 0 where the file has none)


def read_arpa(path_or_lines: Union[str, os.PathLike, Iterable[str]]) -> Arpa:
    """Parse the ARPA text format: `\\data\\`, the `ngram k=count` lines, the `\\k-grams:` sections of tab or space separated
    `log10p w1 .. wk [log10 backoff]` lines, `\\end\\`.  Text in front of `\\data\\` is skipped.  ValueError (with the line number)
    for a line with too few or too many fields, a section that was not announced, a count that disagrees with its section and a
    missing `\\end\\`."""
    if isinstance(path_or_lines, (str, os.PathLike)):
        with open(path_or_lines, encoding="utf-8") as f:
            lines = f.read().splitlines()
    else:
        lines = [ln.rstrip("\n") for ln in path_or_lines]
    counts, count_line, seen, ngrams = {}, {}, {}, {}
    state, k, ended = "head", 0, False
    for no, raw in enumerate(lines, 1):
        line = raw.strip()
        if not line:
            continue
        if state == "head":
            if line == "\\data\\":
                state = "data"
            continue
        if line == "\\end\\":
            ended = True
            break
        if line.startswith("\\") and line.endswith("-grams:"):
            try:
                k = int(line[1:-len("-grams:")])
            except ValueError:
                raise ValueError(f"ARPA line {no}: bad section header '{line}'") from None
            if k not in counts or k in seen:
                raise ValueError(f"ARPA line {no}: section '{line}' was not announced by an 'ngram {k}=' line (or is repeated)")
            state, seen[k] = "grams", 0
            continue
        if state == "data":
            if not line.startswith("ngram ") or "=" not in line:
                raise ValueError(f"ARPA line {no}: 'ngram k=count' expected, got '{line}'")
            a, b = line[len("ngram "):].split("=", 1)
            try:
                counts[int(a)] = int(b)
            except ValueError:
                raise ValueError(f"ARPA line {no}: 'ngram k=count' expected, got '{line}'") from None
            count_line[int(a)] = (no, line)
            continue
        f = line.split()
        if len(f) not in (k + 1, k + 2):
            raise ValueError(f"ARPA line {no}: a {k}-gram line has {k + 1} or {k + 2} fields, got {len(f)}: '{line}'")
        try:
            lp, bo = float(f[0]), float(f[k + 1]) if len(f) == k + 2 else 0.0
        except ValueError:
            raise ValueError(f"ARPA line {no}: bad number in '{line}'") from None
        ngrams[tuple(f[1:k + 1])] = (lp, bo)
        seen[k] += 1
    if state == "head":
        raise ValueError("ARPA: no \\data\\ section")
    if not ended:
        raise ValueError("ARPA: the file ends without \\end\\")
    for kk, c in sorted(counts.items()):
        if seen.get(kk, 0) != c:
            no, line = count_line[kk]
            raise ValueError(f"ARPA line {no}: '{line}' announces {c} {kk}-grams, the section holds {seen.get(kk, 0)}")
    if not counts or sorted(counts) != list(range(1, max(counts) + 1)):
        raise ValueError(f"ARPA: orders {sorted(counts)} are not 1 .. K")
    return Arpa(max(counts), counts, ngrams)


def fmix(z: np.ndarray) -> np.ndarray:
    """the splitmix64 finaliser on u64 arrays (wrapping arithmetic)"""
    z = np.asarray(z, dtype=np.uint64).copy()
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def pack_keys(ids: np.ndarray) -> np.ndarray:
    """u64 keys of the k-grams in the rows of ids [n, k] (oldest word first)"""
    ids = np.asarray(ids, dtype=np.int64)
    n, k = ids.shape
    key = np.zeros(n, dtype=np.uint64)
    for j in range(k):  # field j = the j-th newest word
        key |= (ids[:, k - 1 - j] + 1).astype(np.uint64) << np.uint64(16 * j)
    return key


def build_table(keys: np.ndarray, logp: np.ndarray, backoff: np.ndarray, max_load: float = 0.5):
    """(table ENTRY [capacity], max_probe) for distinct non-zero u64 keys: capacity = the smallest power of two with
    n <= max_load * capacity and n < capacity.  Vectorised: the keys are sorted by home slot, slot_i = max(home_i, slot_{i-1} + 1)
    is a running maximum, and the entries that run past the last slot wrap to the first ones, which are reserved for them by
    repeating the pass until their number is stable (at most a few passes: an empty slot ends every run)."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = keys.shape[0]
    if not 0.0 < max_load <= 1.0:
        raise ValueError(f"build_table: max_load {max_load} outside (0, 1]")
    if n == 0:
        raise ValueError("build_table: no entries")
    if (keys == 0).any() or np.unique(keys).shape[0] != n:
        raise ValueError("build_table: keys must be distinct and non-zero")
    cap = 2
    while cap * max_load < n or cap <= n:
        cap *= 2
    home = (fmix(keys) & np.uint64(cap - 1)).astype(np.int64)
    by_home = np.argsort(home, kind="stable")
    h, idx = home[by_home], np.arange(n, dtype=np.int64)
    carry = 0
    while True:
        pos = idx + np.maximum.accumulate(np.maximum(h, carry) - idx)
        over = int((pos >= cap).sum())
        if over == carry:
            break
        carry = over
    table = np.zeros(cap, dtype=ENTRY)
    slot = pos % cap
    assert np.unique(slot).shape[0] == n
    table["key"][slot] = keys[by_home]
    table["logp"][slot] = np.asarray(logp, dtype=np.float32)[by_home]
    table["backoff"][slot] = np.asarray(backoff, dtype=np.float32)[by_home]
    return table, int((pos - h).max()) + 1


class NGramLM:
    """A back-off n-gram LM of order 1 .. 4 over V <= 65535 ids in the layout js2t_ngram_rescore reads.  Build it with from_arpa,
    from_ngrams or from_arrays; `.to(device)` puts `uni` and `table` on the device (`uni_dev` f32 [V, 2], `table_dev` i64
    [capacity, 2], the 16-byte entries as they are)."""

    def __init__(self, uni: np.ndarray, table: np.ndarray, order: int, n_entries: int, max_probe: int, dropped: int = 0,
                 dropped_tokens=()):
        uni = np.ascontiguousarray(uni, dtype=np.float32)
        if uni.ndim != 2 or uni.shape[1] != 2 or not 2 <= uni.shape[0] <= MAX_V:
            raise ValueError(f"NGramLM: uni f32 [V, 2] with 2 <= V <= {MAX_V} expected, got {uni.shape}")
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NGramLM: order {order} outside 1..{MAX_ORDER}")
        table = np.ascontiguousarray(table, dtype=ENTRY)
        cap = table.shape[0]
        if (order == 1) != (cap == 0) or cap & (cap - 1) or (cap and not 1 <= max_probe <= cap):
            raise ValueError(f"NGramLM: order {order} with capacity {cap}, max_probe {max_probe}")
        self.uni, self.table, self.order, self.n_entries, self.max_probe = uni, table, int(order), int(n_entries), int(max_probe)
        self.dropped, self.dropped_tokens = int(dropped), tuple(dropped_tokens)
        self.device = self.uni_dev = self.table_dev = None

    V = property(lambda self: self.uni.shape[0])
    capacity = property(lambda self: self.table.shape[0])

    # ------------------------------------------------------------ builders
    @classmethod
    def from_arrays(cls, uni, grams, device=None, max_load: float = 0.5, **kw) -> "NGramLM":
        """uni f32 [V, 2]; grams: {k: (ids i64 [n_k, k] oldest word first, logp [n_k], backoff [n_k])} for k >= 2, natural
        logarithms.  The vectorised route for large models."""
        grams = {int(k): g for k, g in grams.items() if len(g[0])}
        V = np.asarray(uni).shape[0]
        order = max(grams, default=1)
        if grams and (min(grams) < 2 or order > MAX_ORDER):
            raise ValueError(f"NGramLM: n-gram orders {sorted(grams)} outside 2..{MAX_ORDER}")
        keys, lps, bos = [], [], []
        for k, (ids, lp, bo) in sorted(grams.items()):
            ids = np.asarray(ids, dtype=np.int64).reshape(-1, k)
            if ids.size and (ids.min() < 0 or ids.max() >= V):
                raise ValueError(f"NGramLM: a {k}-gram holds an id outside 0..{V - 1}")
            keys.append(pack_keys(ids)), lps.append(np.asarray(lp, dtype=np.float32)), bos.append(np.asarray(bo, dtype=np.float32))
        if keys:
            keys = np.concatenate(keys)
            table, max_probe = build_table(keys, np.concatenate(lps), np.concatenate(bos), max_load)
        else:
            keys, table, max_probe = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=ENTRY), 1
        lm = cls(uni, table, order, keys.shape[0], max_probe, **kw)
        return lm.to(device) if device is not None else lm

    @classmethod
    def from_ngrams(cls, ngrams: Dict[Tuple[int, ...], Tuple[float, float]], V: int, device=None, max_load: float = 0.5,
                    unk_index: int = None, oov_log10: float = -100.0, **kw) -> "NGramLM":
        """{(id, ..): (logp, backoff)} in natural logarithms (float64 values are rounded to f32 once, here).  An id without a
        unigram gets unk_index's log-probability if that has one, else oov_log10 * ln 10, with back-off 0."""
        fill = ngrams[(unk_index, )][0] if unk_index is not None and (unk_index, ) in ngrams else oov_log10 * LN10
        uni = np.empty((V, 2), dtype=np.float64)
        uni[:, 0], uni[:, 1] = fill, 0.0
        by_k = {}
        for gram, (lp, bo) in ngrams.items():
            if not 1 <= len(gram) <= MAX_ORDER or any(not 0 <= int(g) < V for g in gram):
                raise ValueError(f"NGramLM: n-gram {gram} longer than {MAX_ORDER} or outside 0..{V - 1}")
            if len(gram) == 1:
                uni[gram[0]] = (lp, bo)
            else:
                by_k.setdefault(len(gram), []).append((gram, lp, bo))
        grams = {k: (np.array([g for g, _, _ in v], dtype=np.int64), np.array([lp for _, lp, _ in v], dtype=np.float64),
                     np.array([bo for _, _, bo in v], dtype=np.float64)) for k, v in by_k.items()}
        return cls.from_arrays(uni.astype(np.float32), grams, device=device, max_load=max_load, **kw)

    @classmethod
    def from_arpa(cls, path_or_lines, vocab, device=None, max_load: float = 0.5, oov_log10: float = -100.0) -> "NGramLM":
        """The ARPA file's tokens are the vocabulary's: `<s>`, `</s>` and `<unk>` are its bos / eos / unk ids, every other token
        goes through vocab.lookup.  A token the vocabulary does not hold is dropped with every n-gram that contains it
        (`.dropped` counts those n-grams, `.dropped_tokens` names the tokens)."""
        arpa = read_arpa(path_or_lines)
        special = {"<s>": vocab.bos_index, "</s>": vocab.eos_index, "<unk>": vocab.unk_index}
        ids, missing = {}, set()

        def tid(tok):
            if tok not in ids:
                i = special[tok] if tok in special else vocab.lookup(tok)
                if tok not in special and i == vocab.unk_index and tok != vocab.specials[0]:
                    i = -1
                    missing.add(tok)
                ids[tok] = i
            return ids[tok]

        ngrams, dropped = {}, 0
        for gram, (lp, bo) in arpa.ngrams.items():
            g = tuple(tid(t) for t in gram)
            if min(g) < 0 or len(g) > MAX_ORDER:
                dropped += 1
                continue
            ngrams[g] = (lp * LN10, bo * LN10)
        if arpa.order > MAX_ORDER:
            raise ValueError(f"NGramLM: ARPA order {arpa.order} above {MAX_ORDER}")
        return cls.from_ngrams(ngrams, len(vocab), device=device, max_load=max_load, unk_index=vocab.unk_index, oov_log10=oov_log10,
                               dropped=dropped, dropped_tokens=sorted(missing))

    # ------------------------------------------------------------ storage
    def save(self, path) -> None:
        """an .npz of the arrays and the scalars: a large model is parsed and laid out once"""
        with open(path, "wb") as f:
            np.savez(f, uni=self.uni, table=self.table.view(np.uint64).reshape(-1, 2), order=self.order, n_entries=self.n_entries,
                     max_probe=self.max_probe, dropped=self.dropped, dropped_tokens=np.array(self.dropped_tokens, dtype=np.str_))

    @classmethod
    def load(cls, path, device=None) -> "NGramLM":
        with np.load(path, allow_pickle=False) as z:
            lm = cls(z["uni"], np.ascontiguousarray(z["table"]).view(ENTRY).reshape(-1), int(z["order"]), int(z["n_entries"]),
                     int(z["max_probe"]), int(z["dropped"]), [str(t) for t in z["dropped_tokens"]])
        return lm.to(device) if device is not None else lm

    def to(self, device) -> "NGramLM":
        """put uni and the table on `device` (a torch device); returns self"""
        import torch
        device = torch.device(device)
        self.uni_dev = torch.from_numpy(self.uni).to(device)
        self.table_dev = torch.from_numpy(self.table.view(np.int64).reshape(-1, 2).copy()).to(device)
        self.device = device
        return self
