"""k-NN spatial graph (input producer) and the normalised t=0 adjacency.

``build_spatial_graph`` follows ``graphBuilder.py:9-47``: an ``ij`` meshgrid of
(lat, lon), a cKDTree k+1 query, drop the first hit (self), edges ``[node, neighbour]``
(source = node, target = neighbour in PyG's ``source_to_target`` flow). E = k*N, the
graph is not symmetric (border tie-breaking).

``gcn_ell`` restates PyG 2.x ``gcn_norm`` for the t=0 block: self-loops are
added for every row, ``deg = 1 + in-degree`` (counted at the target), ``norm(s->d) =
deg_s^-1/2 deg_d^-1/2``. Rows >= N (t >= 1) have only their self-loop and degree 1, so
their aggregation is the identity; only the first N rows of each sample need the ELL.
"""
from __future__ import annotations

import numpy as np

ELL_WIDTH = 8


def build_spatial_graph(lats, lons, k_neighbors: int = 4):
    from scipy.spatial import cKDTree

    lat_grid, lon_grid = np.meshgrid(np.asarray(lats), np.asarray(lons), indexing="ij")
    pos = np.c_[lat_grid.ravel(), lon_grid.ravel()]
    tree = cKDTree(pos)
    _, nbr = tree.query(pos, k=k_neighbors + 1)
    src = np.repeat(np.arange(len(pos), dtype=np.int64), k_neighbors)
    dst = nbr[:, 1:].reshape(-1).astype(np.int64)
    return np.stack([src, dst]), len(pos), pos


def gcn_ell(edge_index: np.ndarray, num_nodes: int, width: int = ELL_WIDTH):
    """Return ``(cols int32 [N, width], vals float32 [N, width])``: row ``d`` of the
    normalised ``D^-1/2 (A+I) D^-1/2`` restricted to the t=0 block, padded with
    (d, 0.0). Edges in the input are assumed free of self loops (graphBuilder drops
    self); any present are replaced, as PyG's ``add_remaining_self_loops`` does."""
    ei = np.asarray(edge_index, dtype=np.int64)
    src, dst = ei[0], ei[1]
    # both rows, self loops included, before anything is indexed (numpy would wrap a negative target)
    if ei.size and (ei.max() >= num_nodes or ei.min() < 0):
        raise ValueError("edge_index references nodes outside [0, num_nodes)")
    keep = src != dst
    src, dst = src[keep], dst[keep]
    deg = np.ones(num_nodes, dtype=np.float64)
    np.add.at(deg, dst, 1.0)
    dinv = np.float32(1.0) / np.sqrt(deg.astype(np.float32))
    cols = np.tile(np.arange(num_nodes, dtype=np.int32)[:, None], (1, width))
    vals = np.zeros((num_nodes, width), dtype=np.float32)
    fill = np.zeros(num_nodes, dtype=np.int64)
    for s, d in zip(src.tolist(), dst.tolist()):
        j = fill[d]
        if j >= width - 1:
            raise ValueError(f"in-degree of node {d} exceeds ELL width {width - 1}")
        cols[d, j] = s
        vals[d, j] = dinv[s] * dinv[d]
        fill[d] += 1
    for d in range(num_nodes):
        cols[d, fill[d]] = d
        vals[d, fill[d]] = dinv[d] * dinv[d]
    return cols, vals


def build_distance_weighted_graph(lats, lons, distance_threshold: float = 5.0):
    """``graphBuilder.py:50-84`` without its double loop: every pair ``i < j`` of grid nodes with
    ``0 < dist < distance_threshold`` (Euclidean, in degrees), in lexicographic order of ``(i, j)``, gives the
    edges ``(i, j)`` then ``(j, i)``, both of weight ``1 / dist``. Returns ``(edge_index int64 [2, E],
    edge_weight float32 [E], num_nodes)``. The in-degree has no bound: the graph goes to
    ``smaml_set_graph_weighted`` (``gcn_csr``), not to the ELL."""
    lat_grid, lon_grid = np.meshgrid(np.asarray(lats, dtype=np.float64), np.asarray(lons, dtype=np.float64),
                                     indexing="ij")
    pos = np.c_[lat_grid.ravel(), lon_grid.ravel()]
    n = len(pos)
    i, j = np.triu_indices(n, k=1)  # row-major: lexicographic in (i, j)
    dist = np.linalg.norm(pos[i] - pos[j], axis=1)
    keep = (dist < distance_threshold) & (dist > 0)
    i, j, dist = i[keep].astype(np.int64), j[keep].astype(np.int64), dist[keep]
    edge_index = np.stack([np.stack([i, j], axis=1).reshape(-1), np.stack([j, i], axis=1).reshape(-1)])
    edge_weight = np.repeat(1.0 / dist, 2).astype(np.float32)
    return np.ascontiguousarray(edge_index), edge_weight, n


def gcn_csr(edge_index: np.ndarray, num_nodes: int, edge_weight=None):
    """``(rowptr int32 [N + 1], cols int32 [nnz], vals float32 [nnz])``: the normalised adjacency of PyG 2.x
    ``gcn_norm(edge_index, edge_weight)`` for any in-degree (the rules of ``smaml_graph_csr`` in ``smaml.h``). Input
    self loops are replaced by one loop per node, whose weight is that of the node's last input loop (1 without
    one, or without weights); ``deg`` = loop + in-edge weights, accumulated in float64 in edge order and rounded
    once to float32; an entry is ``(dinv[s] * w) * dinv[t]`` in float32; row ``t`` lists its in-edges in input
    order, then its loop; entries that come out 0 are dropped. Without weights and with in-degree <= 7 the rows are
    ``gcn_ell``'s non-padding entries."""
    ei = np.asarray(edge_index, dtype=np.int64)
    src, dst = ei[0], ei[1]
    if ei.size and (ei.max() >= num_nodes or ei.min() < 0):
        raise ValueError("edge_index references nodes outside [0, num_nodes)")
    if edge_weight is None:
        w = np.ones(src.shape[0], np.float32)
    else:
        w = np.asarray(edge_weight, dtype=np.float32).reshape(-1)
        if w.shape[0] != src.shape[0]:
            raise ValueError(f"edge_weight has {w.shape[0]} entries for {src.shape[0]} edges")
        if not np.all(np.isfinite(w) & (w >= 0)):
            raise ValueError("edge_weight must be finite and non-negative")
    loop = np.ones(num_nodes, np.float32)
    is_loop = src == dst
    loop[src[is_loop]] = w[is_loop]  # numpy assigns in order: the last entry of a node wins
    keep = ~is_loop
    src, dst, w = src[keep], dst[keep], w[keep]
    deg = loop.astype(np.float64)
    np.add.at(deg, dst, w.astype(np.float64))  # unbuffered, in edge order
    deg = deg.astype(np.float32)
    with np.errstate(divide="ignore"):
        dinv = np.where(deg > 0, np.float32(1.0) / np.sqrt(deg), np.float32(0.0)).astype(np.float32)
    order = np.argsort(dst, kind="stable")  # rows in input order
    nodes = np.arange(num_nodes, dtype=np.int64)
    rows = np.concatenate([dst[order], nodes])
    cols = np.concatenate([src[order], nodes])
    wts = np.concatenate([w[order], loop])
    last = np.argsort(rows, kind="stable")  # every row's loop after its in-edges
    rows, cols, wts = rows[last], cols[last], wts[last]
    vals = (dinv[cols] * wts) * dinv[rows]
    nz = vals != 0
    rows, cols, vals = rows[nz], cols[nz], vals[nz]
    rowptr = np.zeros(num_nodes + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=num_nodes))
    return rowptr, cols.astype(np.int32), vals.astype(np.float32)
