"""CPU checks of the CSR form of the graph: the fixtures of ``weighted_graph_fixtures.py``, ``smaml_graph_csr``
against a dense float64 matrix and against the ELL, ``graph.gcn_csr``, the rules (self loops, zero weights, degree 0),
the rejections, ``build_distance_weighted_graph``, the weighted oracle itself and that it tells the graphs apart by at
least 100 x the GPU tolerances (1e-5 on operator outputs and predictions), so a wrong table cannot pass on the GPU.
"""
import ctypes
import re

import numpy as np
import pytest
import torch

from oracle import graphs, refcpu
from weatherforecast_stgcn_maml_amd import _capi, graph

import weighted_graph_fixtures as wg

ELL_GRAPHS = ("mixed37", "chain37", "fan150", "empty37")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ----------------------------------------------------------------------------- fixtures
def test_fixtures_hold_what_they_promise():
    ei, ew, n = wg.get("over37")
    assert ew is None and n == 37 and graphs.in_degrees(ei, n)[0] == 8
    ei, ew, n = wg.get("knn8_49")
    assert ew is None and n == 49 and ei.shape == (2, 8 * 49) and graphs.in_degrees(ei, n).max() >= 8
    ei, ew, n = wg.get("hub150")
    src0 = ei[0][ei[1] == 0]
    assert ew is None and n == 150 and len(src0) == len(set(src0.tolist())) == wg.HUB_IN_DEGREE
    assert (src0 < 128).sum() >= 100 and (src0 >= 128).sum() >= 7
    rowptr, _, _ = _capi.graph_csr(ei, n)
    assert np.diff(rowptr).max() == np.diff(rowptr)[0] == 141
    ei, ew, n = wg.get("int37")
    assert np.array_equal(ei, graphs.get("mixed37")[0]) and set(ew.tolist()) == {1.0, 2.0, 3.0}
    assert np.all(ew[ei[0] == ei[1]] == 1.0)  # (the multigraph's loops are replaced by one of weight 1)
    assert wg.multigraph(ei, ew).shape[1] == int(ew.sum())
    ei, ew, n = wg.get("frac37")
    assert np.array_equal(ei, graphs.get("mixed37")[0]) and ew.dtype == np.float32
    loops = np.flatnonzero(ei[0] == ei[1])
    assert sorted(zip(ei[0][loops].tolist(), ew[loops].tolist())) == [(11, 2.5), (23, 0.5), (23, 3.0)]
    l23 = [e for e in loops if ei[0][e] == 23]
    assert ew[l23[0]] == 0.5 and ew[l23[1]] == 3.0  # in edge order: 3.0 is the one that stays
    zero = np.flatnonzero(ew == 0)
    assert len(zero) == 1 and ei[0][zero[0]] != ei[1][zero[0]]
    rest = np.delete(ew, np.concatenate([loops, zero]))
    assert rest.min() >= 0.25 and rest.max() <= 4.0 and len(set(rest.tolist())) == len(rest)
    ei, ew, n = wg.get("dist36")
    assert n == 36 and graphs.in_degrees(ei, n).max() == 8 and graphs.in_degrees(ei, n).min() == 3
    assert sorted(set(ew.tolist())) == [float(np.float32(1 / np.sqrt(2.0))), 1.0]
    for name in wg.NAMES:
        a, b = wg.get(name), wg.get(name)
        assert np.array_equal(a[0], b[0]) and (a[1] is None or np.array_equal(a[1], b[1]))


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", wg.NAMES)
def test_weighted_oracle_is_the_dense_matrix_and_agrees_with_the_unchanged_one(name):
    """weighted_gcn_conv in float64 against dense_ahat_w @ x @ W^T + b: 1e-12. On the unweighted fixtures (weights
    of ones) and on int37-as-multigraph it agrees with the unchanged refcpu.gcn_conv to 1e-12 too."""
    ei, ew, n = wg.get(name)
    rows = 3 * n + 7
    rng = np.random.default_rng(3)
    x, w, b = (torch.from_numpy(a) for a in (rng.standard_normal((rows, 8)), rng.standard_normal((40, 8)),
                                             rng.standard_normal(40)))
    ones = np.ones(ei.shape[1], np.float32)
    got = wg.weighted_gcn_conv(ones if ew is None else ew)(x, torch.from_numpy(ei), w, b).numpy()
    want = wg.dense_ahat_w(ei, ew, n, rows) @ x.numpy() @ w.numpy().T + b.numpy()
    assert got.dtype == np.float64 and rel(got, want) < 1e-12
    if name not in wg.FRACTIONAL:
        plain = refcpu.gcn_conv(x, torch.from_numpy(wg.oracle_edges(name)), w, b).numpy()
        e = rel(got, plain)
        print(f"{name}: weighted restatement against the unchanged oracle: {e:.3g}")
        assert e < 1e-12
        assert np.allclose(wg.dense_ahat_w(ei, ew, n), graphs.dense_ahat(wg.oracle_edges(name), n), rtol=1e-13, atol=0)


def test_patch_oracle_reaches_the_composed_functions(monkeypatch):
    ei, ew, n = wg.get("frac37")
    d = wg.hybrid_dims("frac37")
    from weatherforecast_stgcn_maml_amd import synth
    P = refcpu.to_torch(synth.init_params(1, d, gcn_bias_scale=0.1))
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((3 * n, d.input_channels)).astype(np.float32))
    with torch.no_grad():
        before = refcpu.stgcn_features(x, torch.from_numpy(ei), P).numpy()
        wg.patch_oracle(monkeypatch, "frac37")
        after = refcpu.stgcn_features(x, torch.from_numpy(ei), P).numpy()
    assert rel(after, before) > 1e-3


# ----------------------------------------------------------------------------- smaml_graph_csr
@pytest.mark.parametrize("name", wg.NAMES + ELL_GRAPHS)
def test_graph_csr_matches_the_dense_matrix(name):
    """Every entry within 1e-6 relative of the float64 matrix (seven f32 roundings of 2^-24 bound it at 4.2e-7) and
    the rows sum into the dense matrix with nothing left over; graph.gcn_csr gives the same arrays."""
    if name in wg.NAMES:
        ei, ew, n = wg.get(name)
    else:
        (ei, n), ew = graphs.get(name), None
    rowptr, cols, vals = _capi.graph_csr(ei, n, ew)
    dense = wg.dense_ahat_w(ei, ew, n)
    assert rowptr[0] == 0 and rowptr[-1] == len(cols) == len(vals) and np.all(np.diff(rowptr) >= 0)
    assert cols.min() >= 0 and cols.max() < n and np.all(vals > 0)
    got = wg.csr_dense(rowptr, cols, vals, n)
    nz = dense != 0
    assert np.array_equal(got != 0, nz)  # nothing left over, nothing missing
    single = np.ones_like(dense, bool)  # entries that one stored value makes up (parallel edges add several)
    for t in range(n):
        seg = cols[rowptr[t]:rowptr[t + 1]].tolist()
        for c in set(seg):
            if seg.count(c) > 1:
                single[t, c] = False
    for t in range(n):
        for e in range(rowptr[t], rowptr[t + 1]):
            if single[t, cols[e]]:
                assert abs(float(vals[e]) - dense[t, cols[e]]) <= 1e-6 * dense[t, cols[e]], (t, e)
    np.testing.assert_allclose(got[nz], dense[nz], rtol=1e-6, atol=0)
    # row t: its in-edges in input order, then its self loop last
    w = np.ones(ei.shape[1], np.float32) if ew is None else ew
    for t in range(n):
        seg = cols[rowptr[t]:rowptr[t + 1]].tolist()
        want = [s for s, tt, x in zip(ei[0].tolist(), ei[1].tolist(), w.tolist()) if tt == t and s != t and x != 0]
        assert seg == want + [t], t
    p_rowptr, p_cols, p_vals = graph.gcn_csr(ei, n, ew)
    assert np.array_equal(p_rowptr, rowptr) and np.array_equal(p_cols, cols) and np.array_equal(bits(p_vals), bits(vals))
    assert p_rowptr.dtype == np.int32 and p_cols.dtype == np.int32 and p_vals.dtype == np.float32


@pytest.mark.parametrize("name", ELL_GRAPHS)
def test_csr_rows_are_the_ell_rows_bitwise(name):
    """On a graph the ELL accepts: the CSR rows are the ELL's non-padding entries, in order, bit for bit; weights of
    1.0 are NULL weights bit for bit."""
    ei, n = graphs.get(name)
    ec, ev = _capi.graph_ell(ei, n)
    rowptr, cols, vals = _capi.graph_csr(ei, n)
    for t in range(n):
        m = ev[t] != 0
        assert np.array_equal(ec[t][m], cols[rowptr[t]:rowptr[t + 1]]), t
        assert np.array_equal(bits(ev[t][m]), bits(vals[rowptr[t]:rowptr[t + 1]])), t
    r1, c1, v1 = _capi.graph_csr(ei, n, np.ones(ei.shape[1], np.float32))
    assert np.array_equal(r1, rowptr) and np.array_equal(c1, cols) and np.array_equal(bits(v1), bits(vals))
    for a, b in zip(graph.gcn_csr(ei, n), (rowptr, cols, vals)):
        assert np.array_equal(a, b)


def test_self_loop_rule_zero_weights_and_degree_zero():
    ei, ew, n = wg.get("frac37")
    rowptr, cols, vals = _capi.graph_csr(ei, n, ew)
    dense = wg.csr_dense(rowptr, cols, vals, n)
    deg = {t: (3.0 if t == 23 else 2.5 if t == 11 else 1.0) +
           float(sum(w for s, tt, w in zip(ei[0].tolist(), ei[1].tolist(), ew.astype(np.float64).tolist()) if tt == t and s != t))
           for t in (11, 23, 5)}
    assert abs(dense[11, 11] - 2.5 / deg[11]) < 1e-6 and abs(dense[23, 23] - 3.0 / deg[23]) < 1e-6
    assert abs(dense[5, 5] - 1.0 / deg[5]) < 1e-6  # no input loop: weight 1
    z = int(np.flatnonzero(ew == 0)[0])
    s, t = int(ei[0][z]), int(ei[1][z])
    others = [e for e in range(ei.shape[1]) if e != z and ei[0][e] == s and ei[1][e] == t]
    assert not others and dense[t, s] == 0.0  # the zero-weight edge left no entry
    assert len(cols) == ei.shape[1] - 3 - 1 + n  # 3 input loops and the zero edge out, one loop per node in
    # a node whose only weight is a zero self loop has degree 0: its row and its column vanish (PyG: inf -> 0)
    e3 = np.asarray([[0, 1, 1, 2], [1, 1, 2, 0]], np.int64)
    w3 = np.asarray([2.0, 0.0, 3.0, 1.5], np.float32)
    w3[0] = 0.0  # node 1: loop 0 and a zero in-edge -> degree 0
    rp, c, v = _capi.graph_csr(e3, 3, w3)
    assert rp.tolist() == [0, 2, 2, 3] and c.tolist() == [2, 0, 2]  # row 1 empty; 1 -> 2 dropped, 2's loop stays
    np.testing.assert_allclose(v, [1.5 / np.sqrt(2.5 * 4.0), 1 / 2.5, 1 / 4.0], rtol=1e-6)  # degrees 2.5, 0, 4
    for a, b in zip(graph.gcn_csr(e3, 3, w3), (rp, c, v)):
        assert np.array_equal(a, b)


def _raw_graph_csr(ei, ew, n, cap):
    L = _capi.lib()
    ei = np.ascontiguousarray(ei, np.int64)
    rowptr = np.full(n + 1, -5, np.int32)
    cols, vals = np.full(max(cap, 1), -5, np.int32), np.full(max(cap, 1), -5.0, np.float32)
    nnz = ctypes.c_int64(-1)
    rc = L.smaml_graph_csr(ei.ctypes.data_as(_capi.PI64), None if ew is None else ew.ctypes.data_as(_capi.PF32),
                           ei.shape[1], n, rowptr.ctypes.data_as(_capi.PI32), cols.ctypes.data_as(_capi.PI32),
                           vals.ctypes.data_as(_capi.PF32), cap, ctypes.byref(nnz))
    return rc, nnz.value, rowptr, cols, vals, L.smaml_last_error().decode()


def test_rejections_name_the_edge_and_cap_too_small_still_writes_nnz():
    ei = np.asarray([[0, 1, 2], [1, 2, 0]], np.int64)
    for bad, what in ((-1.0, "negative"), (np.nan, "NaN"), (np.inf, "infinite")):
        w = np.asarray([1.0, bad, 1.0], np.float32)
        with pytest.raises(_capi.SmamlError, match=r"EINVAL.*edge 1 \(1 -> 2\).*" + what):
            _capi.graph_csr(ei, 3, w)
        with pytest.raises(ValueError, match="finite and non-negative"):
            graph.gcn_csr(ei, 3, w)
    for row in (0, 1):
        for value in (-1, 3, -(1 << 40)):
            b = ei.copy()
            b[row, 2] = value
            with pytest.raises(_capi.SmamlError, match=r"EINVAL.*edge 2 .*outside"):
                _capi.graph_csr(b, 3)
            with pytest.raises(ValueError, match="outside"):
                graph.gcn_csr(b, 3)
    with pytest.raises(ValueError, match="edge_weight has 2 entries for 3 edges"):
        _capi.graph_csr(ei, 3, np.ones(2, np.float32))
    rc, nnz, rowptr, cols, vals, msg = _raw_graph_csr(ei, None, 3, 5)
    assert rc == 1 and nnz == 6 and re.search(r"cap \(5\).*6 entries", msg)
    assert np.all(cols == -5) and np.all(vals == -5.0) and np.all(rowptr == -5)
    rc, nnz, rowptr, cols, vals, _ = _raw_graph_csr(ei, None, 3, 6)
    assert rc == 0 and nnz == 6 and rowptr.tolist() == [0, 2, 4, 6] and cols.tolist() == [2, 0, 0, 1, 1, 2]
    rc, nnz, *_ = _raw_graph_csr(np.asarray([[0], [7]], np.int64), None, 3, 8)
    assert rc == 1 and nnz == 0


# ----------------------------------------------------------------------------- build_distance_weighted_graph
@pytest.mark.parametrize("lats,lons,thr", [(np.arange(6.0), np.arange(6.0), 1.6),
                                           (np.linspace(50, 52, 4), np.linspace(8, 11, 5), 1.2),
                                           (np.arange(3.0), np.arange(4.0), 100.0)])
def test_distance_weighted_graph_against_the_double_loop(lats, lons, thr):
    ei, ew, n = graph.build_distance_weighted_graph(lats, lons, thr)
    pos = [(la, lo) for la in lats for lo in lons]  # the ij meshgrid, ravelled
    edges, weights = [], []
    for i in range(len(pos)):
        for j in range(i + 1, len(pos)):
            dist = float(np.hypot(pos[i][0] - pos[j][0], pos[i][1] - pos[j][1]))
            if 0 < dist < thr:
                edges += [(i, j), (j, i)]
                weights += [1.0 / dist] * 2
    assert n == len(pos) and ei.dtype == np.int64 and ew.dtype == np.float32
    assert ei.T.tolist() == [list(e) for e in edges]
    np.testing.assert_allclose(ew, np.asarray(weights, np.float32), rtol=1e-6)
    if thr == 100.0:
        assert ei.shape[1] == n * (n - 1)  # the complete graph


# ----------------------------------------------------------------------------- discrimination
def _operator_oracle(ei, conv):
    n = 37
    rng = np.random.default_rng(77)
    cin, cout = 8, 40
    x, w, b, R = (torch.from_numpy(a) for a in (rng.standard_normal((3 * n + 7, cin)).astype(np.float32),
                                                rng.uniform(-0.35, 0.35, (cout, cin)).astype(np.float32),
                                                rng.uniform(-0.1, 0.1, cout).astype(np.float32),
                                                rng.standard_normal((3 * n + 7, cout)).astype(np.float32)))
    for t in (x, w):
        t.requires_grad_(True)
    out = conv(x, torch.from_numpy(np.ascontiguousarray(ei)), w, b)
    (out * R).sum().backward()
    return {"out": out.detach().numpy(), "dx": x.grad.numpy(), "dW": w.grad.numpy()}


def test_the_oracle_tells_the_weighted_graphs_apart():
    """100 x the operator tolerance of the GPU tests (1e-5): frac37 from its unweighted graph and from its reverse;
    over37 from its reverse and from over37 without the eighth in-edge (= mixed37, what an ELL would keep)."""
    ei, ew, _ = wg.get("frac37")
    a = _operator_oracle(ei, wg.weighted_gcn_conv(ew))
    over = wg.get("over37")[0]
    b = _operator_oracle(over, refcpu.gcn_conv)
    others = {"frac37 unweighted": (a, _operator_oracle(ei, refcpu.gcn_conv)),
              "frac37 reversed": (a, _operator_oracle(graphs.reverse(ei), wg.weighted_gcn_conv(ew))),
              "over37 reversed": (b, _operator_oracle(graphs.reverse(over), refcpu.gcn_conv)),
              "over37 without the eighth in-edge": (b, _operator_oracle(over[:, :-1], refcpu.gcn_conv))}
    for what, (x, y) in others.items():
        for k in ("out", "dx", "dW"):
            e = rel(y[k], x[k])
            print(f"{what}: {k} changes by {e:.3g}")
            assert e > 1e-3, (what, k, e)


# ----------------------------------------------------------------------------- the ABI
def test_exports_and_abi_version():
    L = _capi.lib()
    for name in ("smaml_graph_csr", "smaml_set_graph_weighted", "smaml_graph_stats"):
        assert name in _capi.EXPORTS and name in _capi._SIGS and hasattr(L, name)
    assert L.smaml_abi_version() == _capi.ABI_VERSION
    assert _capi.GRAPH_STATS == ("form", "entries", "longest_row", "csr_layer_launches", "csr_gather_launches")
    header = open(__import__("os").path.join(__import__("os").path.dirname(_capi.HERE), "include", "smaml.h")).read()
    for rule in ("LAST input entry", "summed in double", "(dinv[s] * w) * dinv[t]", "2^31 - 1"):
        assert rule in header, rule
