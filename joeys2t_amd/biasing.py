"""Contextual biasing of the CTC beam search (EXTENSION; the reference has no hot words): the phrase automaton that
js2t_ctc_beam_search_ctx and js2t_context_rescore read (include/joeys2t_hip.h states the rule and the layout,
joeys2t_amd/csrc/context.hpp is its device side).  Plain Python and NumPy; torch is touched only by `.to(device)`.

A set of phrases, each a sequence of target-vocabulary ids, becomes an Aho-Corasick automaton over the trie of the phrases:
    nodes i32 [n_nodes, 4]   {fail, depth, keep, 0} per node, node 0 = the root.  fail(u) = the node of the longest proper suffix of
                             u's string that is a trie node (the root if none); keep(u) = the depth of the deepest node on the path
                             root .. u, u included, at which a phrase ends (0 if none)
    edges ENTRY [capacity]   the n-gram table's entry format and probing rule (lm.build_table): the key of the edge (node, token) is
                             lm.pack_keys of the row (node, token), the `logp` word holds the child's id as i32 bits
    max_probe                as in lm.py
    max_fail                 the largest number of fail links between a node and the root: what bounds a step of the walk

Biasing adds no candidates: a phrase token that is not among a frame's `candidates` (<= 8) best labels is still not proposed.
"""
from collections import deque
from typing import Iterable, Sequence

import numpy as np

from joeys2t_amd.lm import ENTRY, build_table, pack_keys

MAX_NODES = 65535   # JS2T_CONTEXT_MAX_NODES
MAX_LEN = 32        # JS2T_CONTEXT_MAX_LEN
MAX_FAIL = 32       # JS2T_CONTEXT_MAX_FAIL
MAX_V = 65535       # JS2T_CONTEXT_MAX_V


def phrase_ids(phrases: Iterable, vocab):
    """phrases: strings of whitespace-separated pieces, or sequences of pieces, in the vocabulary's own tokens.  Returns (the id
    lists of the phrases kept, in order; the number dropped): a phrase with a piece the vocabulary does not hold is dropped."""
    ids, dropped = [], 0
    for p in phrases:
        pieces = p.split() if isinstance(p, str) else list(p)
        row = [vocab.lookup(tok) for tok in pieces]
        if any(i == vocab.unk_index and tok != vocab.specials[0] for i, tok in zip(row, pieces)):
            dropped += 1
            continue
        ids.append(row)
    return ids, dropped


class ContextGraph:
    """The automaton of a phrase set over V <= 65535 ids in the layout js2t_ctc_beam_search_ctx reads.  Build it with from_phrases
    or from_text; `.to(device)` puts the tables on the device (`nodes_dev` i32 [n_nodes, 4], `edges_dev` i64 [capacity, 2], the
    16-byte entries as they are).  Attributes: n_nodes, n_phrases, max_len, max_fail, V, capacity, max_probe, dropped."""

    def __init__(self, nodes: np.ndarray, edges: np.ndarray, V: int, n_phrases: int, max_len: int, max_fail: int, max_probe: int,
                 dropped: int = 0):
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        edges = np.ascontiguousarray(edges, dtype=ENTRY)
        cap = edges.shape[0]
        if nodes.ndim != 2 or nodes.shape[1] != 4 or not 2 <= nodes.shape[0] <= MAX_NODES:
            raise ValueError(f"ContextGraph: nodes i32 [n, 4] with 2 <= n <= {MAX_NODES} expected, got {nodes.shape}")
        if not 1 <= int(V) <= MAX_V:
            raise ValueError(f"ContextGraph: V {V} outside 1..{MAX_V}")
        if cap < 1 or cap & (cap - 1) or not 1 <= max_probe <= cap:
            raise ValueError(f"ContextGraph: capacity {cap}, max_probe {max_probe}")
        if not 1 <= max_len <= MAX_LEN or not 1 <= max_fail <= MAX_FAIL:
            raise ValueError(f"ContextGraph: max_len {max_len} outside 1..{MAX_LEN} or max_fail {max_fail} outside 1..{MAX_FAIL}")
        self.nodes, self.edges, self.V = nodes, edges, int(V)
        self.n_phrases, self.max_len, self.max_fail, self.max_probe = int(n_phrases), int(max_len), int(max_fail), int(max_probe)
        self.dropped = int(dropped)
        self.device = self.nodes_dev = self.edges_dev = None

    n_nodes = property(lambda self: self.nodes.shape[0])
    capacity = property(lambda self: self.edges.shape[0])

    # ------------------------------------------------------------ builders
    @classmethod
    def from_phrases(cls, phrases: Iterable[Sequence[int]], V: int, device=None, max_load: float = 0.5, dropped: int = 0) -> "ContextGraph":
        """phrases: sequences of ids in 0 .. V-1; duplicates are merged.  ValueError for no phrase, an empty phrase, an id outside
        the vocabulary, a phrase of more than 32 tokens and a trie of more than 65535 nodes."""
        V = int(V)
        if not 1 <= V <= MAX_V:
            raise ValueError(f"ContextGraph: V {V} outside 1..{MAX_V}")
        uniq = []
        seen = set()
        for p in phrases:
            p = tuple(int(t) for t in p)
            if not p:
                raise ValueError("ContextGraph: an empty phrase")
            if len(p) > MAX_LEN:
                raise ValueError(f"ContextGraph: a phrase of {len(p)} tokens, at most {MAX_LEN} are supported")
            if min(p) < 0 or max(p) >= V:
                raise ValueError(f"ContextGraph: phrase {p} holds an id outside 0..{V - 1}")
            if p not in seen:
                seen.add(p)
                uniq.append(p)
        if not uniq:
            raise ValueError("ContextGraph: no phrases")
        # the trie, nodes numbered in order of creation (a parent before its children)
        child, depth, ends, parent = [{}], [0], [False], [0]
        for p in uniq:
            u = 0
            for t in p:
                v = child[u].get(t)
                if v is None:
                    v = len(child)
                    if v >= MAX_NODES:
                        raise ValueError(f"ContextGraph: the phrases need more than {MAX_NODES} nodes")
                    child[u][t] = v
                    child.append({}), depth.append(depth[u] + 1), ends.append(False), parent.append(u)
                u = v
            ends[u] = True
        n = len(child)
        fail, hops, keep = [0] * n, [0] * n, [0] * n
        queue = deque([0])
        while queue:  # breadth first: fail(u) is known before u's children are looked at
            u = queue.popleft()
            for t, v in child[u].items():
                keep[v] = depth[v] if ends[v] else keep[u]
                w = fail[u]
                while u and t not in child[w] and w:
                    w = fail[w]
                f = child[w].get(t, 0) if u else 0
                fail[v], hops[v] = f, (hops[f] + 1 if f else 1)
                queue.append(v)
        nodes = np.zeros((n, 4), dtype=np.int32)
        nodes[:, 0], nodes[:, 1], nodes[:, 2] = fail, depth, keep
        src = np.array([(u, t) for u in range(n) for t in child[u]], dtype=np.int64).reshape(-1, 2)
        dst = np.array([v for u in range(n) for v in child[u].values()], dtype=np.int32)
        edges, max_probe = build_table(pack_keys(src), dst.view(np.float32), np.zeros(dst.shape[0], dtype=np.float32), max_load)
        g = cls(nodes, edges, V, len(uniq), max(len(p) for p in uniq), max(hops), max_probe, dropped)
        return g.to(device) if device is not None else g

    @classmethod
    def from_text(cls, phrases: Iterable, vocab, device=None, max_load: float = 0.5) -> "ContextGraph":
        """phrases: strings of whitespace-separated pieces, or sequences of pieces, in the vocabulary's own tokens (what
        NGramLM.from_arpa looks up).  A phrase with a piece the vocabulary does not hold is dropped; `.dropped` counts them."""
        ids, dropped = phrase_ids(phrases, vocab)
        return cls.from_phrases(ids, len(vocab), device=device, max_load=max_load, dropped=dropped)

    # ------------------------------------------------------------ storage
    def save(self, path) -> None:
        with open(path, "wb") as f:
            np.savez(f, nodes=self.nodes, edges=self.edges.view(np.uint64).reshape(-1, 2), V=self.V, n_phrases=self.n_phrases,
                     max_len=self.max_len, max_fail=self.max_fail, max_probe=self.max_probe, dropped=self.dropped)

    @classmethod
    def load(cls, path, device=None) -> "ContextGraph":
        with np.load(path, allow_pickle=False) as z:
            g = cls(z["nodes"], np.ascontiguousarray(z["edges"]).view(ENTRY).reshape(-1), int(z["V"]), int(z["n_phrases"]), int(z["max_len"]),
                    int(z["max_fail"]), int(z["max_probe"]), int(z["dropped"]))
        return g.to(device) if device is not None else g

    def to(self, device) -> "ContextGraph":
        """put the two tables on `device` (a torch device); returns self"""
        import torch
        device = torch.device(device)
        self.nodes_dev = torch.from_numpy(self.nodes).to(device)
        self.edges_dev = torch.from_numpy(self.edges.view(np.int64).reshape(-1, 2).copy()).to(device)
        self.device = device
        return self
