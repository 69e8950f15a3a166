"""TEST INFRASTRUCTURE ONLY: irregular graphs for the tests of the graph consumers.

Every GPU test used to build its graph with ``build_spatial_graph`` on a square grid: in-degree 3..6, no
isolated node, no duplicate, no self loop, A_hat almost symmetric. These fixtures are what ``build_ell``
(api.cpp) and ``model.GCNConv`` promise beyond that. All are deterministic (seeded numpy generator), int64
``edge_index`` [2, E] with ``edge_index[0]`` the sources and ``edge_index[1]`` the targets.

=========  ====  =========================================================================================
 name       N    what it holds
=========  ====  =========================================================================================
 mixed37     37  a random directed multigraph: node 0 with in-degree 7 (its self loop lands in the last of
                 the 8 ELL slots); nodes 20 and 36 with no edge at all (so edge_index.max() + 1 < N); one
                 edge twice; one self loop in the input; one self loop twice; the other nodes with
                 in-degree 0..5; the columns shuffled
 chain37     37  i -> i + 1 only: A_hat differs from A_hat^T at every node
 fan150     150  node 149 feeds nodes 1..100 (a row of 101 entries in the CSR of A_hat^T); node 0 has
                 in-degree 7, all from nodes 140..146 (edges across the 128-row tile of k_gcn_layer); the
                 other nodes have in-degree 0..3
 empty37     37  no edge: A_hat = I
 over        37  mixed37 plus one more edge into node 0 (in-degree 8): must be rejected
=========  ====  =========================================================================================

``dense_ahat`` is a dense float64 restatement of PyG's ``gcn_norm`` (D^-1/2 (A + I) D^-1/2, parallel edges add,
input self loops replaced by one of weight 1, rows past N the identity), written independently of
``refcpu.gcn_conv`` and of ``graph.gcn_ell``.
"""
from __future__ import annotations

import numpy as np

MIXED_SEED = 2024
FAN_SEED = 7
ISOLATED = (20, 36)      # mixed37: neither in- nor out-edges
DUPLICATE = (5, 9)       # mixed37: this edge is present twice, and is node 9's only in-edge
SELF_ONCE, SELF_TWICE = 11, 23
FAN_SOURCE, FAN_TARGETS = 149, 100
FAN_FULL_SOURCES = tuple(range(140, 147))  # node 0's seven in-edges, all from rows >= 128


def _random_in_edges(rng, targets, sources, lo, hi, taken):
    """For every target a random number in [lo, hi] of distinct random sources (never the target itself,
    never an edge of `taken`)."""
    out = []
    for t in targets:
        cand = [s for s in sources if s != t and (s, t) not in taken]
        k = int(rng.integers(lo, hi + 1))
        for s in rng.choice(cand, size=min(k, len(cand)), replace=False):
            out.append((int(s), int(t)))
    return out


def mixed37():
    n = 37
    rng = np.random.default_rng(MIXED_SEED)
    live = [i for i in range(n) if i not in ISOLATED]
    edges = [(int(s), 0) for s in rng.choice([i for i in live if i != 0], size=7, replace=False)]
    edges += [DUPLICATE, DUPLICATE]
    others = [t for t in live if t not in (0, DUPLICATE[1])]
    edges += _random_in_edges(rng, others, live, 0, 5, set(edges))
    for i in live:  # only the two ISOLATED nodes stay without an edge: a node the draw left out feeds the next one
        if not any(i in e for e in edges):
            edges.append((i, next(t for t in others if t != i and sum(e[1] == t for e in edges) < 5)))
    edges += [(SELF_ONCE, SELF_ONCE), (SELF_TWICE, SELF_TWICE), (SELF_TWICE, SELF_TWICE)]
    ei = np.asarray(edges, np.int64).T
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def chain37():
    i = np.arange(36, dtype=np.int64)
    return np.stack([i, i + 1])


def fan150():
    n = 150
    rng = np.random.default_rng(FAN_SEED)
    edges = [(s, 0) for s in FAN_FULL_SOURCES]
    edges += [(FAN_SOURCE, t) for t in range(1, FAN_TARGETS + 1)]
    plain = [i for i in range(n) if i != FAN_SOURCE]  # node 149 feeds exactly its 100 targets
    edges += _random_in_edges(rng, range(1, FAN_TARGETS + 1), plain, 0, 2, set(edges))
    edges += _random_in_edges(rng, range(FAN_TARGETS + 1, n), plain, 0, 3, set(edges))
    ei = np.asarray(edges, np.int64).T
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def empty37():
    return np.zeros((2, 0), np.int64)


def over():
    """mixed37 plus one more edge into node 0, from a node that does not feed it yet: in-degree 8."""
    ei = mixed37()
    feeds = set(ei[0][ei[1] == 0].tolist())
    s = next(i for i in range(1, 37) if i not in feeds and i not in ISOLATED)
    return np.concatenate([ei, np.asarray([[s], [0]], np.int64)], axis=1)


NUM_NODES = {"mixed37": 37, "chain37": 37, "fan150": 150, "empty37": 37}
_BUILD = {"mixed37": mixed37, "chain37": chain37, "fan150": fan150, "empty37": empty37}
ACCEPTED = tuple(NUM_NODES)
_CACHE = {}


def get(name):
    """(edge_index, N) of an accepted fixture (built once; every call returns its own copy)."""
    if name not in _CACHE:
        _CACHE[name] = _BUILD[name]()
    return _CACHE[name].copy(), NUM_NODES[name]


def reverse(ei):
    """Every edge turned round: A becomes A^T."""
    return np.ascontiguousarray(np.asarray(ei)[::-1])


def dedup(ei):
    """The same graph with every parallel edge (self loops too) kept once, first occurrence first."""
    ei = np.asarray(ei)
    seen, keep = set(), []
    for e, (s, t) in enumerate(zip(ei[0].tolist(), ei[1].tolist())):
        if (s, t) not in seen:
            seen.add((s, t))
            keep.append(e)
    return np.ascontiguousarray(ei[:, keep])


def in_degrees(ei, n):
    """In-degree as PyG counts it: parallel edges each, self loops not."""
    ei = np.asarray(ei)
    deg = np.zeros(n, np.int64)
    for s, t in zip(ei[0].tolist(), ei[1].tolist()):
        if s != t:
            deg[t] += 1
    return deg


def dense_ahat(ei, n, rows=None):
    """float64 [rows, rows]: D^-1/2 (A + I) D^-1/2 over the n graph nodes (A[t, s] = number of edges s -> t with
    s != t), the identity on the rows past n."""
    rows = n if rows is None else rows
    assert rows >= n
    ei = np.asarray(ei)
    a = np.zeros((n, n), np.float64)
    for s, t in zip(ei[0].tolist(), ei[1].tolist()):
        if s != t:
            a[t, s] += 1.0
    a += np.eye(n)
    dinv = 1.0 / np.sqrt(a.sum(axis=1))
    out = np.eye(rows, dtype=np.float64)
    out[:n, :n] = dinv[:, None] * a * dinv[None, :]
    return out
