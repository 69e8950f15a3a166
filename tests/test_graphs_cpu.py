"""CPU checks behind tests/test_gpu_graphs.py: the irregular graph fixtures (oracle/graphs.py), the two ELL
builders on them, the transpose ``smaml_set_graph`` uploads, and the oracle itself.

1. The fixtures hold what their table says (in-degrees, isolated nodes, duplicates, self loops, the long row of
   A_hat^T, the edges across the 128-row tile).
2. ``refcpu.gcn_conv`` (run in float64) equals ``graphs.dense_ahat``, an independent dense float64 restatement
   of D^-1/2 (A + I) D^-1/2, to 1e-12 on every fixture: the reference of every GPU comparison is right on
   graphs with parallel edges, input self loops and isolated nodes.
3. ``_capi.graph_ell`` (C, ``build_ell``) and ``graph.gcn_ell`` (Python) agree with each other and with the
   dense matrix; a numpy restatement of ``smaml_set_graph``'s transpose gives A_hat^T; in-degree 7 is accepted
   with the self loop in the eighth slot, in-degree 8 and any index outside [0, N) in either row are rejected
   by both builders.
4. The fixtures discriminate: swapping a graph for its reverse (A_hat^T where A_hat belongs), removing the
   duplicate edges, or dropping the eighth ELL slot changes the oracle's operator outputs by more than 1e-2
   rel-L2 (1e-3 for the one row the eighth slot touches, against the operators' 1e-5) -- at least 100 x the
   tolerance of the GPU comparison, so such a kernel cannot pass it. Through the hybrid model (one time block of
   three aggregates) the reverse graph still moves predictions and gradients by more than 1e-2, the one
   duplicate edge the predictions by more than 1e-4 (10 x their tolerance).
"""
import numpy as np
import pytest
import torch

from oracle import graphs, refcpu
from weatherforecast_stgcn_maml_amd import _capi, graph

import test_gpu_graphs as tg

W = graph.ELL_WIDTH


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def ell_dense(cols, vals, n):
    out = np.zeros((n, n), np.float64)
    for i in range(n):
        for c, v in zip(cols[i], vals[i]):
            out[i, c] += v
    return out


def transpose_csr(cols, vals):
    """smaml_set_graph's transpose restated: entry (t, e) of the ELL with a non-zero value becomes an entry of
    row cols[t][e], rows filled in ascending t, slots in ascending e."""
    n = cols.shape[0]
    rows = [[] for _ in range(n)]
    for t in range(n):
        for e in range(W):
            if vals[t, e] != 0.0:
                rows[cols[t, e]].append((t, vals[t, e]))
    ptr = np.zeros(n + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.asarray([t for r in rows for t, _ in r], np.int32)
    val = np.asarray([v for r in rows for _, v in r], np.float32)
    return ptr, col, val


# ----------------------------------------------------------------------------- 1. the fixtures
def test_fixtures_hold_what_they_promise():
    ei, n = graphs.get("mixed37")
    deg = graphs.in_degrees(ei, n)
    assert n == 37 and deg[0] == 7 and deg.max() == 7 and sorted(set(deg[1:])) != [0]
    used = set(ei.ravel().tolist())
    assert [i for i in range(n) if i not in used] == list(graphs.ISOLATED) and graphs.ISOLATED[1] == n - 1
    assert int(ei.max()) + 1 < n  # the module path sizes its context from edge_index.max() + 1
    pairs = list(zip(ei[0].tolist(), ei[1].tolist()))
    twice = sorted({p for p in pairs if pairs.count(p) == 2})
    assert twice == sorted([graphs.DUPLICATE, (graphs.SELF_TWICE, graphs.SELF_TWICE)]) and max(map(pairs.count, pairs)) == 2
    assert pairs.count((graphs.SELF_ONCE, graphs.SELF_ONCE)) == 1
    assert sum(s == t for s, t in pairs) == 3
    assert pairs != sorted(pairs) and pairs != sorted(pairs, key=lambda p: p[::-1])  # the columns are shuffled
    assert graphs.dedup(ei).shape[1] == ei.shape[1] - 2

    ei, n = graphs.get("chain37")
    assert n == 37 and ei.T.tolist() == [[i, i + 1] for i in range(36)]

    ei, n = graphs.get("fan150")
    deg = graphs.in_degrees(ei, n)
    assert n == 150 and deg[0] == 7 and deg[1:].max() == 3 and deg[1:].min() == 0
    assert sorted(ei[0][ei[1] == 0].tolist()) == list(graphs.FAN_FULL_SOURCES) and min(graphs.FAN_FULL_SOURCES) >= 128
    assert sorted(ei[1][ei[0] == graphs.FAN_SOURCE].tolist()) == list(range(1, graphs.FAN_TARGETS + 1))
    ptr, _, _ = transpose_csr(*graph.gcn_ell(ei, n))
    lens = np.diff(ptr)
    assert lens[graphs.FAN_SOURCE] == graphs.FAN_TARGETS + 1 == lens.max()
    pairs = list(zip(ei[0].tolist(), ei[1].tolist()))
    assert len(set(pairs)) == len(pairs) and all(s != t for s, t in pairs)

    ei, n = graphs.get("empty37")
    assert ei.shape == (2, 0) and ei.dtype == np.int64 and n == 37
    ov = graphs.over()
    assert ov.shape[1] == graphs.get("mixed37")[0].shape[1] + 1 and graphs.in_degrees(ov, 37)[0] == 8
    assert np.array_equal(ov[:, :-1], graphs.get("mixed37")[0])
    for name in graphs.ACCEPTED:  # deterministic
        assert np.array_equal(graphs.get(name)[0], graphs.get(name)[0])


# ----------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("name", graphs.ACCEPTED)
def test_oracle_gcn_conv_is_the_dense_normalised_adjacency(name):
    """refcpu.gcn_conv in float64 on rows = 3 N + 7 against dense_ahat @ x @ W^T + b: 1e-12."""
    ei, n = graphs.get(name)
    rows = 3 * n + 7
    rng = np.random.default_rng(3)
    x, w, b = rng.standard_normal((rows, 8)), rng.standard_normal((40, 8)), rng.standard_normal(40)
    got = refcpu.gcn_conv(torch.from_numpy(x), torch.from_numpy(ei), torch.from_numpy(w), torch.from_numpy(b)).numpy()
    want = graphs.dense_ahat(ei, n, rows) @ x @ w.T + b
    e = rel(got, want)
    print(f"{name}: refcpu.gcn_conv (f64) against the dense restatement: rel-L2 {e:.3g}")
    assert got.dtype == np.float64 and e < 1e-12
    a = graphs.dense_ahat(ei, n, rows)
    assert np.array_equal(a[n:, n:], np.eye(rows - n)) and not a[:n, n:].any() and not a[n:, :n].any()


# ----------------------------------------------------------------------------- 3. the builders
@pytest.mark.parametrize("name", graphs.ACCEPTED)
def test_ell_builders_agree_and_match_the_dense_matrix(name):
    ei, n = graphs.get(name)
    c_cols, c_vals = _capi.graph_ell(ei, n)
    p_cols, p_vals = graph.gcn_ell(ei, n)
    np.testing.assert_array_equal(c_cols, p_cols)
    np.testing.assert_allclose(c_vals, p_vals, rtol=1e-7)
    dense = graphs.dense_ahat(ei, n)
    np.testing.assert_allclose(ell_dense(c_cols, c_vals, n), dense, rtol=1e-6, atol=1e-7)
    # as test_ell_matches_python_restatement_and_pyg_norm: the oracle's f32 matrix too
    eye = torch.eye(n)
    ora = refcpu.gcn_conv(eye, torch.from_numpy(ei), eye, torch.zeros(n)).numpy()
    np.testing.assert_allclose(ell_dense(c_cols, c_vals, n).astype(np.float32), ora, rtol=1e-6, atol=1e-7)
    # every row: its in-edges in input order, then the self loop, then (row, 0) padding
    deg = graphs.in_degrees(ei, n)
    for i in range(n):
        assert c_cols[i, deg[i]] == i and abs(c_vals[i, deg[i]] * (deg[i] + 1.0) - 1.0) < 1e-6  # d_i^-1/2 squared, in f32
        assert np.all(c_cols[i, deg[i]:] == i) and not c_vals[i, deg[i] + 1:].any()
        assert c_cols[i, :deg[i]].tolist() == [s for s, t in zip(ei[0].tolist(), ei[1].tolist()) if t == i and s != i]


@pytest.mark.parametrize("name", graphs.ACCEPTED)
def test_transpose_restatement_gives_ahat_transposed(name):
    ei, n = graphs.get(name)
    cols, vals = _capi.graph_ell(ei, n)
    ptr, col, val = transpose_csr(cols, vals)
    assert ptr[0] == 0 and ptr[-1] == len(col) == int((vals != 0).sum())
    dense_t = np.zeros((n, n), np.float64)
    for j in range(n):
        seg = col[ptr[j]:ptr[j + 1]]
        assert np.all(np.diff(seg) >= 0)  # ascending targets: the fixed summation order of the CSR gathers
        for t, v in zip(seg, val[ptr[j]:ptr[j + 1]]):
            dense_t[j, t] += v
    assert np.array_equal(dense_t, ell_dense(cols, vals, n).T)
    np.testing.assert_allclose(dense_t, graphs.dense_ahat(ei, n).T, rtol=1e-6, atol=1e-7)
    if name == "empty37":
        assert np.array_equal(dense_t, np.eye(n))


def test_in_degree_seven_fills_the_row_and_eight_is_rejected():
    ei, n = graphs.get("mixed37")
    for cols, vals in (_capi.graph_ell(ei, n), graph.gcn_ell(ei, n)):
        assert np.all(vals[0] != 0) and cols[0, 7] == 0 and abs(vals[0, 7] - 0.125) < 1e-7
        assert 0 not in cols[0, :7].tolist()
        for i in graphs.ISOLATED:  # the self loop alone, weight 1
            assert cols[i].tolist() == [i] * W and vals[i].tolist() == [1.0] + [0.0] * (W - 1)
    with pytest.raises(_capi.SmamlError, match="EINVAL.*in-degree exceeds the ELL width"):
        _capi.graph_ell(graphs.over(), 37)
    with pytest.raises(ValueError, match="in-degree of node 0 exceeds ELL width 7"):
        graph.gcn_ell(graphs.over(), 37)
    # a self loop does not count: node 0 with 7 in-edges and a self loop is still accepted
    looped = np.concatenate([ei, np.asarray([[0], [0]], np.int64)], axis=1)
    np.testing.assert_array_equal(_capi.graph_ell(looped, n)[0], _capi.graph_ell(ei, n)[0])
    np.testing.assert_array_equal(graph.gcn_ell(looped, n)[1], graph.gcn_ell(ei, n)[1])


@pytest.mark.parametrize("row", [0, 1], ids=["source", "target"])
@pytest.mark.parametrize("value", [-1, 3, -(1 << 40)], ids=["minus-one", "num-nodes", "very-negative"])
def test_index_outside_the_graph_is_rejected_by_both_builders(row, value):
    bad = np.asarray([[0, 1], [1, 2]], np.int64)
    bad[row, 1] = value
    with pytest.raises(_capi.SmamlError, match="EINVAL.*outside"):
        _capi.graph_ell(bad, 3)
    with pytest.raises(ValueError, match="outside"):
        graph.gcn_ell(bad, 3)
    loop = np.asarray([[0, value], [1, value]], np.int64)  # an out-of-range self loop is no exception
    with pytest.raises(_capi.SmamlError, match="EINVAL.*outside"):
        _capi.graph_ell(loop, 3)
    with pytest.raises(ValueError, match="outside"):
        graph.gcn_ell(loop, 3)


# ----------------------------------------------------------------------------- 4. discrimination
@pytest.mark.parametrize("cin,cout", tg.OP_SHAPES)
@pytest.mark.parametrize("name", ["mixed37", "chain37", "fan150"])
def test_operator_outputs_tell_a_graph_from_its_reverse(name, cin, cout):
    """The operator tests' own inputs: gcn_conv, and the three gradients of sum(out * R), under the graph and
    under its reverse (= a kernel that gathers with A_hat^T where A_hat belongs, or the reverse)."""
    ei, n = graphs.get(name)
    a, b = tg.operator_oracle(name, cin, cout), tg.operator_oracle(name, cin, cout, edge_fn=graphs.reverse)
    for k in ("out", "relu", "dx", "dW"):
        e = rel(b[k], a[k])
        print(f"{name} {cin}->{cout} {k}: reverse graph changes it by {e:.3g}")
        assert e > 1e-2, (k, e)
    assert np.array_equal(a["db"], b["db"])  # (the bias gradient sees no graph)


@pytest.mark.parametrize("cin,cout", tg.OP_SHAPES)
def test_operator_outputs_tell_duplicates_and_the_eighth_slot(cin, cout):
    a = tg.operator_oracle("mixed37", cin, cout)
    b = tg.operator_oracle("mixed37", cin, cout, edge_fn=graphs.dedup)
    for k in ("out", "relu", "dx", "dW"):
        e = rel(b[k], a[k])
        print(f"mixed37 {cin}->{cout} {k}: without the duplicates it changes by {e:.3g}")
        assert e > 1e-2, (k, e)
    # a gather that stops after seven slots loses node 0's self loop: x_0 / 8 is missing from row 0
    for name in ("mixed37", "fan150"):
        ei, n = graphs.get(name)
        x, w, bias, _ = tg.operator_inputs(name, cin, cout)
        cols, vals = _capi.graph_ell(ei, n)
        vals7 = vals.copy()
        vals7[:, 7] = 0.0
        assert int((vals7 != vals).sum()) == 1
        full = ell_dense(cols, vals, n) @ x[:n].astype(np.float64) @ w.astype(np.float64).T + bias
        cut = ell_dense(cols, vals7, n) @ x[:n].astype(np.float64) @ w.astype(np.float64).T + bias
        whole = tg.operator_oracle(name, cin, cout)["out"]
        e = float(np.linalg.norm(cut - full) / np.linalg.norm(whole))
        print(f"{name} {cin}->{cout}: without the eighth slot the output changes by {e:.3g}")
        assert e > 1e-3, e  # one row of 3 N + 7; 100 x the operator tolerance (1e-5)


@pytest.mark.parametrize("name", ["mixed37", "chain37", "fan150"])
def test_hybrid_outputs_tell_a_graph_from_its_reverse(name):
    """The hybrid cases of the GPU file (T = 3: one time block of three aggregates): predictions, the conv
    gradients and dx under the graph and under its reverse."""
    a, b = tg.hybrid_oracle(name, 0.0), tg.hybrid_oracle(name, 0.0, edge_fn=graphs.reverse)
    e = rel(np.stack(b[0]), np.stack(a[0]))
    print(f"{name}: predictions change by {e:.3g}")
    assert e > 1e-2
    for k in a[1]:
        if k.startswith("base_stgcn.conv") and k.endswith("weight"):
            e = rel(b[1][k], a[1][k])
            print(f"{name}: {k} gradient changes by {e:.3g}")
            assert e > 1e-2, (k, e)
    e = rel(np.stack(b[2]), np.stack(a[2]))
    print(f"{name}: dx changes by {e:.3g}")
    assert e > 1e-2


def test_hybrid_outputs_tell_duplicates():
    a, b = tg.hybrid_oracle("mixed37", 0.0), tg.hybrid_oracle("mixed37", 0.0, edge_fn=graphs.dedup)
    e = rel(np.stack(b[0]), np.stack(a[0]))
    print(f"mixed37: predictions change by {e:.3g} without the duplicates")
    assert e > 1e-4  # 10 x the prediction tolerance (1e-5): one duplicate edge, seen through one time block of three
