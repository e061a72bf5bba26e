"""CPU: the contextual-biasing rule (include/joeys2t_hip.h at js2t_ctc_beam_search_ctx).  The header's examples; the plain-Python
reference of tests/context_reference.py pinned by brute force; joeys2t_amd.biasing.ContextGraph's tables against the reference,
walked in NumPy AND by the library's own walk (csrc/context.hpp through js2t_context_walk_host - the statement the two kernels
share, run on the host); max_fail, save / load and every refusal."""
import ctypes
import itertools
import re

import numpy as np
import pytest

import context_reference as X
from joeys2t_amd import _lib, biasing
from joeys2t_amd.biasing import ContextGraph
from joeys2t_amd.lm import fmix

A, B_, C, D, XX = 0, 1, 2, 3, 4  # the header's letters; x = 4

EXAMPLES = [  # (phrases, y, m, ctx); None = the header does not state it
    ([(A, B_, C), (C, D)], (A, B_), 2, 0),
    ([(A, B_, C), (C, D)], (A, B_, C), 3, 3),
    ([(A, B_, C), (C, D)], (A, B_, C, D), 5, 5),
    ([(A, B_, C), (C, D)], (A, B_, XX), 0, None),
    ([(A, B_, C), (C, D)], (A, A, B_, C), None, 3),
    ([(A, B_), (A, B_, C, D)], (A, B_, C), 3, 2),
    ([(A, B_), (A, B_, C, D)], (A, B_, C, XX), 2, None),
    ([(A, B_, C, D), (B_, C)], (A, B_, C, XX), 0, None),  # the stated limitation
]


# ---------------------------------------------------------------- two walks over ContextGraph's arrays
def np_child(g, u, c):
    """child of node u by token c from the edge table, by the probing rule of the header, or -1"""
    key = np.uint64(((u + 1) << 16) | (c + 1))
    home = int(fmix(np.array([key]))[0]) & (g.capacity - 1)
    for i in range(g.max_probe):
        e = g.edges[(home + i) & (g.capacity - 1)]
        if e["key"] == key:
            return int(np.array([e["logp"]], dtype=np.float32).view(np.int32)[0])
        if e["key"] == 0:
            return -1
    return -1


def np_walk(g, y):
    """[(node, bank, m, ctx)] after every token of y, by the five steps of the rule over g.nodes / g.edges"""
    fail, depth, keep = g.nodes[:, 0], g.nodes[:, 1], g.nodes[:, 2]
    node, bank, out = 0, 0, []
    for c in y:
        u = node
        if not 0 <= c < g.V:
            node, bank = 0, bank + int(keep[u])
        else:
            ch = np_child(g, u, c)
            if ch >= 0:
                node = ch
            else:
                bank += int(keep[u])
                w = int(fail[u])
                hops = 0
                while np_child(g, w, c) < 0 and w != 0:
                    w, hops = int(fail[w]), hops + 1
                    assert hops <= g.max_fail
                node = max(np_child(g, w, c), 0)
        out.append((node, bank, bank + int(depth[node]), bank + int(keep[node])))
    return out


def lib_walk(g, y):
    """the same through js2t_context_walk_host: csrc/context.hpp compiled for the host"""
    n = len(y)
    ids = np.asarray(y, dtype=np.int64)
    outs = [np.full(max(n, 1), -7, dtype=np.int32) for _ in range(4)]
    edges = np.ascontiguousarray(g.edges)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert g.nodes.ctypes.data % 16 == 0 and edges.ctypes.data % 16 == 0
    rc = _lib.lib().js2t_context_walk_host(ptr(ids), n, ptr(g.nodes), ptr(edges), g.capacity, g.max_probe, g.n_nodes, g.max_fail, g.V,
                                           *(ptr(o) for o in outs))
    assert rc == 0, _lib.lib().js2t_last_error()
    return [tuple(int(o[i]) for o in outs) for i in range(n)]


def aligned(g):
    """the graph with its two tables at 16-byte aligned addresses (NumPy promises no more than the item size)"""
    def al(a):
        raw = np.zeros(a.nbytes + 16, dtype=np.uint8)
        off = (-raw.ctypes.data) % 16
        out = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        out[...] = a
        return out
    g.nodes, g.edges = al(g.nodes), al(g.edges)
    return g


def same_as_reference(g, auto, y):
    """both walks over the tables give the reference's (node string, bank, m, ctx) after every token of y"""
    want = auto.walk(y)
    paths = graph_paths(g)
    for got in (np_walk(g, y), lib_walk(g, y)):
        assert len(got) == len(want)
        for (node, bank, m, ctx), (rn, rb) in zip(got, want):
            assert paths[node] == auto.path[rn] and bank == rb, (y, got, want)
            assert m == rb + auto.depth[rn] and ctx == rb + auto.keep[rn], (y, got, want)


def graph_paths(g):
    """node id -> its string, recovered from the edge table (node numbering is the builder's business)"""
    paths = {0: ()}
    for e in g.edges[g.edges["key"] != 0]:
        key = int(e["key"])
        u, c, v = (key >> 16) - 1, (key & 0xFFFF) - 1, int(np.array([e["logp"]], dtype=np.float32).view(np.int32)[0])
        paths[v] = (u, c)
    def full(v):
        s = []
        while v != 0:
            v, c = paths[v]
            s.append(c)
        return tuple(reversed(s))
    return {v: full(v) for v in list(paths)}


# ---------------------------------------------------------------- the pinned examples
@pytest.mark.parametrize("phrases, y, m, ctx", EXAMPLES)
def test_the_headers_examples(phrases, y, m, ctx):
    auto = X.Automaton(phrases, 5)
    g = aligned(ContextGraph.from_phrases(phrases, 5))
    for mm, cc in ((auto.m(y), auto.ctx(y)), np_walk(g, y)[-1][2:], lib_walk(g, y)[-1][2:]):
        assert m is None or mm == m
        assert ctx is None or cc == ctx


def test_the_header_states_the_examples_and_the_limits():
    text = " ".join(_lib.HEADER_PATH.read_text().split())
    for piece in ('"a b" m 2, ctx 0', '"a b c" m 3, ctx 3', '"a b c d" m 5, ctx 5', '"a b x" m 0', '"a a b c" ctx 3', '"a b c" m 3, ctx 2',
                  '"a b c x" m 2', '"a b c x" m 0'):
        assert piece in text, piece
    defs = dict(re.findall(r"#define (JS2T_CONTEXT_\w+) (\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {"JS2T_CONTEXT_MAX_NODES": biasing.MAX_NODES, "JS2T_CONTEXT_MAX_LEN": biasing.MAX_LEN,
                                                   "JS2T_CONTEXT_MAX_FAIL": biasing.MAX_FAIL, "JS2T_CONTEXT_MAX_V": biasing.MAX_V}


# ---------------------------------------------------------------- the reference, pinned by brute force
DISJOINT = [[(0, 1, 2), (3, 4)], [(0, 1), (2, 3, 4)], [(4, 3, 2, 1, 0)], [(0, ), (1, 2), (3, 4)], [(2, 0, 4, 1)]]


@pytest.mark.parametrize("phrases", DISJOINT)
def test_reference_counts_occurrences_on_disjoint_alphabets(phrases):
    """phrases over pairwise disjoint alphabets, no token repeated inside one: for EVERY y in V^<=6 at V = 5, ctx(y) = the summed
    lengths of all occurrences by substring search and m(y) - ctx(y) = the longest suffix of y that is a proper prefix of a phrase.
    The library's walk over ContextGraph's tables gives the same two numbers."""
    V = 5
    auto = X.Automaton(phrases, V)
    g = aligned(ContextGraph.from_phrases(phrases, V))
    count = 0
    for L in range(0, 7):
        for y in itertools.product(range(V), repeat=L):
            ctx, m = auto.ctx(y), auto.m(y)
            assert ctx == X.occurrences(y, phrases), (phrases, y)
            assert m - ctx == X.pending(y, phrases), (phrases, y)
            if L == 6:  # (its prefixes are the shorter ones)
                got = lib_walk(g, y)
                assert got[-1][2:] == (m, ctx), (phrases, y, got)
            count += 1
    assert count == sum(5**L for L in range(7))


# ---------------------------------------------------------------- ContextGraph against the reference
def check_graph(phrases, V, ys, **kw):
    auto = X.Automaton(phrases, V)
    g = aligned(ContextGraph.from_phrases(phrases, V, **kw))
    assert g.n_nodes == len(auto.child) and g.n_phrases == len(set(phrases)) and g.max_len == max(len(p) for p in phrases)
    assert g.max_fail == auto.max_fail() and g.V == V
    paths = graph_paths(g)
    assert sorted(paths.values()) == sorted(auto.path)
    index = {s: u for u, s in enumerate(auto.path)}
    for v, s in paths.items():  # every record: fail, depth, keep by the node's string
        assert paths[int(g.nodes[v, 0])] == auto.path[auto.fail[index[s]]]
        assert (int(g.nodes[v, 1]), int(g.nodes[v, 2]), int(g.nodes[v, 3])) == (len(s), auto.keep[index[s]], 0)
    for y in ys:
        same_as_reference(g, auto, y)
    return g, auto


@pytest.mark.parametrize("seed", range(6))
def test_graph_tables_on_random_phrase_sets(seed):
    """shared prefixes, nested phrases, tokens outside the vocabulary in the walked sequences; small alphabets so that suffixes recur"""
    rs = np.random.RandomState(seed)
    V = int(rs.randint(2, 6))
    phrases = X.random_phrases(rs, V, int(rs.randint(1, 12)), lengths=(1, 6), share=0.6)
    ys = [tuple(int(v) for v in rs.randint(-1, V + 1, size=int(rs.randint(0, 24)))) for _ in range(40)]
    ys += [p + p for p in phrases] + [p[:-1] + p for p in phrases]
    check_graph(phrases, V, ys, max_load=(0.5, 0.95, 1.0)[seed % 3])


def test_self_overlapping_phrases_and_the_fail_chain():
    """`a a a b`: after a a a a the walk must stay at depth 3; a a a a b against a a a a a a b is the chain case of the GPU test"""
    g, auto = check_graph([(0, 0, 0, 1)], 3, [(0, ) * 6 + (1, ), (0, 0, 1, 0, 0, 0, 1), (0, 0, 0, 0, 1, 1)])
    assert auto.ctx((0, ) * 6 + (1, )) == 4 and auto.m((0, ) * 5) == 3 and g.max_fail == 3
    g, auto = check_graph([(0, 0, 0, 0, 1)], 2, [(0, ) * 6 + (1, ), (0, ) * 9])
    assert auto.ctx((0, ) * 6 + (1, )) == 5 and g.max_fail == 4
    # the longest chain a phrase allows: 32 equal tokens
    g, auto = check_graph([(1, ) * 32], 2, [(1, ) * 40, (1, ) * 31 + (0, )])
    assert g.max_fail == 32 == g.max_len and auto.ctx((1, ) * 40) == 9 * 32


def test_large_graph_at_high_load():
    """about 2000 phrases at V = 5000 and max_load 0.95: long probe chains; every phrase is found, a near miss is not"""
    rs = np.random.RandomState(7)
    phrases = X.random_phrases(rs, 5000, 2000, lengths=(2, 6), share=0.3)
    ys = [phrases[i] for i in range(0, 2000, 50)] + [phrases[i][:-1] + (4999, ) + phrases[i + 1] for i in range(0, 2000, 100)]
    g, _ = check_graph(phrases, 5000, ys, max_load=0.95)
    assert g.max_probe > 4 and g.capacity < 2 * (g.n_nodes - 1) / 0.95 + 2


def test_duplicates_merge_and_save_load(tmp_path):
    g = ContextGraph.from_phrases([(1, 2), (1, 2), [1, 2, 3], (4, )], 6)
    assert g.n_phrases == 3 and g.n_nodes == 5 and g.max_len == 3 and g.max_fail == 1 and g.dropped == 0
    g.save(tmp_path / "g.npz")
    h = ContextGraph.load(tmp_path / "g.npz")
    assert np.array_equal(h.nodes, g.nodes) and np.array_equal(h.edges, g.edges)
    assert (h.V, h.n_phrases, h.max_len, h.max_fail, h.max_probe, h.dropped) == (g.V, g.n_phrases, g.max_len, g.max_fail, g.max_probe, g.dropped)
    assert g.nodes.dtype == np.int32 and g.nodes.shape == (5, 4) and g.edges.dtype.itemsize == 16
    d = g.to("cpu")
    assert d is g and d.nodes_dev.shape == (5, 4) and d.edges_dev.shape == (g.capacity, 2) and str(d.device) == "cpu"


def test_from_text():
    from joeys2t_amd.vocabulary import Vocabulary
    vocab = Vocabulary.synthetic(20)
    toks = ["tok1", "tok2", "tok3"]  # ids 5, 6, 7 behind the four specials
    assert [vocab.lookup(t) for t in toks] == [5, 6, 7]
    g = ContextGraph.from_text([" ".join(toks), [toks[0], toks[2]], toks[1] + " no-such-piece"], vocab)
    assert g.dropped == 1 and g.n_phrases == 2 and g.V == len(vocab)
    auto = X.Automaton([(5, 6, 7), (5, 7)], len(vocab))
    assert sorted(graph_paths(g).values()) == sorted(auto.path)


def test_refusals():
    ok = [(1, 2)]
    for phrases, V, msg in (([], 5, "no phrases"), ([()], 5, "an empty phrase"), ([(1, 5)], 5, "outside 0..4"), ([(-1, )], 5, "outside 0..4"),
                            ([(1, ) * 33], 5, "33 tokens"), (ok, 0, "V 0 outside"), (ok, 65536, "V 65536 outside")):
        with pytest.raises(ValueError, match=msg):
            ContextGraph.from_phrases(phrases, V)
    with pytest.raises(ValueError, match="max_load"):
        ContextGraph.from_phrases(ok, 5, max_load=0.0)
    # 2048 phrases of 32 tokens that share nothing cross the node limit
    with pytest.raises(ValueError, match="more than 65535 nodes"):
        ContextGraph.from_phrases([(i, ) + (0, ) * 31 for i in range(2048)], 4096)
    ContextGraph.from_phrases([(1, ) * 32], 5)  # the limit itself is fine


def test_host_walk_refuses_bad_graph_arguments():
    """the checks the two kernels' entry points share (context.hpp's context_args), reached without a device"""
    g = aligned(ContextGraph.from_phrases([(1, 2), (2, 3)], 5))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    ids = np.array([1, 2, 3], dtype=np.int64)
    outs = [np.zeros(3, dtype=np.int32) for _ in range(4)]
    good = dict(ids=ptr(ids), n=3, nodes=ptr(g.nodes), edges=ptr(g.edges), capacity=g.capacity, max_probe=g.max_probe, n_nodes=g.n_nodes,
                max_fail=g.max_fail, V=5)
    L = _lib.lib()

    def call(**change):
        return L.js2t_context_walk_host(*dict(good, **change).values(), *(ptr(o) for o in outs))

    assert call() == 0 and outs[3].tolist() == [0, 2, 4]
    for change, msg in ((dict(nodes=None), b"null pointer (context graph"), (dict(edges=None), b"null pointer (context graph"),
                        (dict(n_nodes=1), b"1 context nodes outside"), (dict(n_nodes=65536), b"65536 context nodes outside"),
                        (dict(capacity=12), b"capacity 12 is no power"), (dict(capacity=0), b"capacity 0 is no power"),
                        (dict(max_probe=0), b"max_probe 0 outside"), (dict(max_probe=g.capacity + 1), b"max_probe"),
                        (dict(max_fail=0), b"max_fail 0 outside"), (dict(max_fail=33), b"max_fail 33 outside"), (dict(V=65536), b"V 65536 outside"),
                        (dict(nodes=ctypes.c_void_p(g.nodes.ctypes.data + 8)), b"not 16-byte aligned"), (dict(n=-1), b"below 0")):
        assert call(**change) < 0 and msg in L.js2t_last_error(), (change, L.js2t_last_error())
