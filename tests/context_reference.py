"""Plain-Python reference of the contextual-biasing rule (js2t_ctc_beam_search_ctx / js2t_context_rescore, include/joeys2t_hip.h):
a dict trie, breadth-first fail links and the walk, written from the header's statement and independently of joeys2t_amd/biasing.py.
No GPU, no torch.

Rule.  Per trie node u: depth(u); fail(u) = the node of the longest proper suffix of u's string that is a trie node (root if none);
keep(u) = the depth of the deepest node on the path root .. u, u included, at which a phrase ends (0 if none).  A prefix y carries
(node, bank), the empty one (root, 0).  Extending by c from u = node(y):
    u has a child by c: node = that child, bank unchanged
    else: bank += keep(u); w = fail(u); while w has no child by c and w != root: w = fail(w); node = child(w, c) if any, else root
    c outside 0 .. V-1: root, bank += keep(u)
m(y) = bank + depth(node) (the in-beam value), ctx(y) = bank + keep(node) (the final value).

rescore: score = base + context_weight * ctx, a weight of exactly 0 left out (ctx = 0 then, nothing read); dead slots (base = -inf,
n < 0, n > Lp - 1): ctx 0, score -inf; order by rescore_reference.rank.
"""
import numpy as np

from ctc_beam_reference import DECIDABLE, bound  # noqa: F401  (one statement of the tolerance)
from rescore_reference import margin, rank  # noqa: F401  (one statement of the tie and NaN rules)

NEG = -np.inf
ROOT = 0


class Automaton:
    def __init__(self, phrases, V):
        self.V = V
        self.child = [{}]
        self.depth = [0]
        self.ends = [False]
        self.path = [()]
        for p in phrases:
            u = ROOT
            for t in p:
                if t not in self.child[u]:
                    self.child[u][t] = len(self.child)
                    self.child.append({})
                    self.depth.append(self.depth[u] + 1)
                    self.ends.append(False)
                    self.path.append(self.path[u] + (t, ))
                u = self.child[u][t]
            self.ends[u] = True
        index = {s: u for u, s in enumerate(self.path)}
        n = len(self.child)
        self.fail = [ROOT] * n
        self.keep = [0] * n
        for u in range(n):  # straight from the definitions: no breadth-first cleverness to get wrong
            s = self.path[u]
            for k in range(1, len(s)):
                if s[k:] in index:
                    self.fail[u] = index[s[k:]]
                    break
            self.keep[u] = max([d for d in range(1, len(s) + 1) if self.ends[index[s[:d]]]], default=0)

    def max_fail(self):
        def hops(u):
            h = 0
            while u != ROOT:
                u, h = self.fail[u], h + 1
            return h
        return max(hops(u) for u in range(len(self.child)))

    def step(self, node, bank, c):
        if not 0 <= c < self.V:
            return ROOT, bank + self.keep[node]
        if c in self.child[node]:
            return self.child[node][c], bank
        bank += self.keep[node]
        w = self.fail[node]
        while c not in self.child[w] and w != ROOT:
            w = self.fail[w]
        return self.child[w].get(c, ROOT), bank

    def walk(self, y):
        """[(node, bank)] after every token of y"""
        node, bank, out = ROOT, 0, []
        for c in y:
            node, bank = self.step(node, bank, int(c))
            out.append((node, bank))
        return out

    def state(self, y):
        node, bank = ROOT, 0
        for c in y:
            node, bank = self.step(node, bank, int(c))
        return node, bank

    def m(self, y):
        node, bank = self.state(y)
        return bank + self.depth[node]

    def ctx(self, y):
        node, bank = self.state(y)
        return bank + self.keep[node]


def combine(base, ctx, context_weight):
    s = float(base)
    if context_weight != 0:
        s = s + context_weight * float(ctx)
    return s


def rescore(ids, n, base, N, Lp, auto, context_weight):
    """(ctx i64 [R], score f64 [R], order i64 [B, N]); reads the ids of live slots at positions < n only"""
    n, base = np.asarray(n).reshape(-1), np.asarray(base, dtype=np.float64).reshape(-1)
    R = n.shape[0]
    assert R % N == 0
    ids = np.asarray(ids).reshape(R, -1)
    dead = (base == NEG) | (n < 0) | (n > Lp - 1)
    ctx, score = np.zeros(R, dtype=np.int64), np.full(R, NEG)
    for r in range(R):
        if dead[r]:
            continue
        if context_weight != 0:
            ctx[r] = auto.ctx([int(v) for v in ids[r, :n[r]]])
        score[r] = combine(base[r], ctx[r], context_weight)
    order = np.array([rank(score[b * N:(b + 1) * N].tolist()) for b in range(R // N)], dtype=np.int64).reshape(R // N, N)
    return ctx, score, order


# ---------------------------------------------------------------- phrase sets
def random_phrases(rs, V, count, lengths=(1, 6), share=0.5, lo=0):
    """`count` phrases over ids lo .. V-1: with probability `share` a phrase starts with a prefix of an earlier one (shared prefixes
    and nested phrases), else it is drawn afresh; lengths uniform in `lengths`"""
    out = []
    for _ in range(count):
        L = int(rs.randint(lengths[0], lengths[1] + 1))
        if out and rs.rand() < share:
            base = out[rs.randint(len(out))]
            k = int(rs.randint(1, len(base) + 1))
            p = list(base[:k])[:L]
        else:
            p = []
        while len(p) < L:
            p.append(int(rs.randint(lo, V)))
        out.append(tuple(p))
    return out


def occurrences(y, phrases):
    """sum of the lengths of all occurrences of all (distinct) phrases in y, by plain substring search"""
    y = tuple(y)
    return sum(len(p) for p in set(map(tuple, phrases)) for i in range(len(y) - len(p) + 1) if y[i:i + len(p)] == tuple(p))


def pending(y, phrases):
    """the length of the longest suffix of y that is a proper prefix of a phrase"""
    y = tuple(y)
    best = 0
    for p in phrases:
        for k in range(1, min(len(p) - 1, len(y)) + 1):
            if y[len(y) - k:] == tuple(p[:k]):
                best = max(best, k)
    return best
