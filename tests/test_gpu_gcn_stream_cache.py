"""The meta-step's per-stream GCN feature cache (option ``gcn_stream_cache``; DESIGN.md "Per-stream GCN feature
cache") against the path it replaces: the same meta-steps with the option 1 and 0 must agree BITWISE in ``losses``,
``norms``, ``meta_grad`` and ``theta`` -- the cache recomputes nothing differently, it only computes each stream
row once. What was served and filled is asserted from the ``gcn_cache`` / ``gcn_cache_rows`` counters and the
``gcn_layer`` timing category, never from time.

Shapes: N = 9 (3 x 3 grid, 4 neighbours), H = 32, L = 2, T = 3, B = 3, K = 2 -- M = B N = 27 puts the boundary
between the t = 0 rows and the later stream rows of a task's compact features inside the first row tile -- with
Hc = 256 (the fused ``k_gcn_mlp`` fill) or Hc = 16 (the per-layer fill), 3 tasks in task groups of 2 (the cache
must survive the ``set_tasks`` rotation of every meta-step), two consecutive meta-steps. ``big`` forces the
bench's kernels as tests/test_gpu_shapes.py does, which is what makes the features compact (``f_compact``).

The last section runs ``smaml_meta_step_base`` the same way (two tasks in one pass, order 2, ``big``): its base stage
masks by the features as the cache gather laid them out, so ``gcn_meta_grad`` must be bitwise equal too.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import params, synth
from weatherforecast_stgcn_maml_amd.config import MamlConfig, ModelDims
from weatherforecast_stgcn_maml_amd.maml import MetaLearner, stream_len_for

import base_meta_oracle as bmo
import test_gpu_base_meta as bm
from test_gpu_parity import DEV, grid_edges, split

pytestmark = pytest.mark.gpu

K, B, NT = 2, 3, 3
BIG_OPTS = (("wgrad_group_max_rows", 0), ("bwd_big_min", 0), ("bwdd_big_min", 0), ("split_max", 1))


def dims(hc):
    return ModelDims(num_nodes=9, window_size=3, hidden_channels=hc, lstm_hidden_size=32, lstm_num_layers=2)


def edge_weights(ei):
    return np.random.default_rng(5).uniform(0.5, 1.5, ei.shape[1]).astype(np.float32)


def learner(hc, order, cache, big, weighted=False, dropout=(0.0, 0.0), batch=B, task_group=2, options=(), tasks=NT):
    d = dims(hc)
    cfg = MamlConfig(inner_steps=K, batch=batch, order=order)
    theta, gcn, _ = split(synth.init_params(31, d, gcn_bias_scale=0.1))
    ei = grid_edges(d)
    ml = MetaLearner(d, cfg, gcn, theta, ei, device=DEV, task_group=task_group, dropout=dropout, dropout_seed=3,
                     edge_weight=edge_weights(ei) if weighted else None)
    ml.ctx.set_option("gcn_stream_cache", cache)
    for k, v in (BIG_OPTS if big else ()) + tuple(options):
        ml.ctx.set_option(k, v)
    # (B = 3 streams whatever the batch under test: the window tables below index them alike)
    n = stream_len_for(MamlConfig(inner_steps=K, batch=B, order=order), d) + 6
    ml.set_tasks([synth.make_features(900 + j, d.num_nodes, n) for j in range(tasks)])
    return ml


def snapshot(ml, res):
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy() for t in (res.losses, res.norms, ml.meta_grad, ml.theta)]


def run(ml, steps=2, windows=None, between=None):
    """`steps` meta-steps; per step its (losses, norms, meta_grad, theta) and the variant counters it added."""
    out = []
    for i in range(steps):
        if i and between:
            between(ml)
        ml.ctx.variant_counts(reset=True)
        res = ml.meta_step(windows=windows)
        out.append((snapshot(ml, res), ml.ctx.variant_counts()))
    return out


def assert_bitwise(a, b, what):
    for i, ((sa, _), (sb, _)) in enumerate(zip(a, b)):
        for name, x, y in zip(("losses", "norms", "meta_grad", "theta"), sa, sb):
            assert np.all(np.isfinite(x)), (what, i, name)
            assert x.tobytes() == y.tobytes(), (what, "meta-step", i, name, float(np.max(np.abs(x - y))))


def served(vc):
    return vc["gcn_cache"], vc["gcn_cache_rows"]


# ----------------------------------------------------------------------------- parity and structure
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("case", ["fused-big", "fused-default", "layer-big", "layer-default", "weighted-fused-big",
                                  "weighted-layer-default"])
def test_cached_meta_steps_are_bitwise_the_uncached(case, order):
    """Two meta-steps over 3 tasks in groups of 2, the default (consecutive) windows: bitwise, and the structure --
    every forward of a consecutive-window step is served (K + 1 per group, and the K steps of a second-order
    sweep, which has no per-step feature store to read any more), the first meta-step fills exactly the distinct
    rows its windows touch, the second fills none and launches no GCN kernel at all."""
    hc = 256 if "fused" in case else 16
    big, weighted = case.endswith("big"), case.startswith("weighted")
    on = learner(hc, order, 1, big, weighted)
    on.ctx.timing(True)
    a = [run(on, 1)[0]]
    t1 = on.ctx.timing_collect()
    a.append(run(on, 1)[0])
    t2 = on.ctx.timing_collect()
    b = run(learner(hc, order, 0, big, weighted))
    assert_bitwise(a, b, case)
    d = on.dims
    w = on.default_windows()  # [K + 1][tasks][B], each row consecutive
    rows = 0
    for z in range(NT):
        w0 = sorted({int(x) for x in w[:, z, 0]})
        rows += len({r for s in w0 for r in range(s, s + B)})                         # as t = 0 rows
        rows += len({r for s in w0 for r in range(s + 1, s + B + d.window_size - 1)})  # as later rows
    groups = len(on._groups)
    assert groups == 2
    fwd = groups * (K + 1 + (K if order == 2 else 0))  # (no per-step feature store: the sweep is served too)
    assert served(a[0][1]) == (fwd, rows), a[0][1]
    assert served(a[1][1]) == (fwd, 0), a[1][1]
    assert t1["gcn_layer"]["launches"] > 0 and t2["gcn_layer"]["launches"] == 0, (t1["gcn_layer"], t2["gcn_layer"])
    if big:
        assert a[1][1]["f_compact"] == groups * (K + 1), a[1][1]  # (once per step: the sweep's visit is not counted)
    else:
        assert a[1][1]["f_compact"] == 0, a[1][1]
    assert served(b[1][1]) == (0, 0), b[1][1]


@pytest.mark.parametrize("hc", [256, 16])
def test_second_order_sweep_without_the_feature_store_reads_the_cache(hc):
    """`so_f_store` 0 takes the per-step feature store from the uncached run too: its sweep recomputes each step's
    features, the cached one is served them (K more forwards per group, no row filled twice) -- bitwise equal.
    `keep` 0 in both arms: without a feature store the uncached run keeps no primal, and a sweep over kept primal
    equals a recomputing one only up to f32 rounding, cache or no cache (the primal gate kernel adds layer 0's
    projection in its epilogue, the tangent one starts its accumulators from it; 6e-11 in meta_grad here)."""
    opts = (("so_f_store", 0), ("keep", 0))
    a = run(learner(hc, 2, 1, True, options=opts))
    b = run(learner(hc, 2, 0, True, options=opts))
    assert_bitwise(a, b, "so_f_store 0")
    assert served(a[1][1]) == (2 * (2 * K + 1), 0), a[1][1]


# ----------------------------------------------------------------------------- window tables
def window_tables(ml):
    """Overlapping, repeated and reordered consecutive batches (tests/test_gpu_windows.py's style), so the lazy
    fill meets ranges that are partly filled, filled in the middle only, and already complete."""
    d = ml.dims
    n = min(synth.num_samples(f.shape[0], d.window_size, d.forecast_horizon) for f in ml.tasks)
    assert n >= 12, n
    starts = np.array([[4, 5, 0],      # step 0: tasks start apart
                       [2, 5, 1],      # step 1: overlaps step 0 from below / repeats it / overlaps from above
                       [n - B, 3, 4]])  # query: the last window of the stream / inside the union / above
    return (starts[:, :, None] + np.arange(B)[None, None, :]).astype(np.int32)


@pytest.mark.parametrize("case", ["fused-big", "layer-default"])
def test_overlapping_and_repeated_batches(case):
    hc, big = (256, True) if case == "fused-big" else (16, False)
    on, off = learner(hc, 2, 1, big), learner(hc, 2, 0, big)
    w = window_tables(on)
    a, b = run(on, windows=w), run(off, windows=w)
    assert_bitwise(a, b, case)
    d, rows = on.dims, 0
    for z in range(NT):
        w0 = sorted({int(x) for x in w[:, z, 0]})
        rows += len({r for s in w0 for r in range(s, s + B)})
        rows += len({r for s in w0 for r in range(s + 1, s + B + d.window_size - 1)})
    assert served(a[0][1]) == (2 * (2 * K + 1), rows) and served(a[1][1]) == (2 * (2 * K + 1), 0), (a[0][1], a[1][1])


# ----------------------------------------------------------------------------- invalidation
def _changed_gcn(ml):
    ml.gcn.mul_(1.25)
    torch.cuda.synchronize()
    ml.ctx.set_gcn_params(ml.gcn)  # same pointer, new values: the call is the signal


def _changed_graph(ml):
    ei = grid_edges(ml.dims)
    ml.ctx.set_graph(np.ascontiguousarray(ei[:, : ei.shape[1] // 2 * 2 - 4]))


def _rewritten_stream(ml):
    ml.tasks[1].mul_(0.5)
    torch.cuda.synchronize()
    ml.ctx.gcn_cache_invalidate()


def _rewritten_stream_unannounced(ml):
    ml.tasks[1].mul_(0.5)
    torch.cuda.synchronize()


@pytest.mark.parametrize("change", [_changed_gcn, _changed_graph, _rewritten_stream])
@pytest.mark.parametrize("hc", [256, 16])
def test_invalidation(hc, change):
    """After new GCN values behind the kept pointer, a new graph, or a stream written in place and announced, the
    second meta-step refills what it reads and equals the uncached run bitwise."""
    a = run(learner(hc, 2, 1, True), between=change)
    b = run(learner(hc, 2, 0, True), between=change)
    assert_bitwise(a, b, change.__name__)
    assert a[1][1]["gcn_cache_rows"] > 0, a[1][1]
    if change is not _rewritten_stream:
        assert a[1][1]["gcn_cache_rows"] == a[0][1]["gcn_cache_rows"], (a[0][1], a[1][1])


def test_unannounced_rewrite_shows_the_cache_is_read():
    """A stream written in place WITHOUT the invalidate call: the cached rows are served, so the second meta-step
    differs from the uncached one (which reads the new values) -- the cache is what the kernels read."""
    a = run(learner(256, 1, 1, True), between=_rewritten_stream_unannounced)
    b = run(learner(256, 1, 0, True), between=_rewritten_stream_unannounced)
    assert_bitwise(a[:1], b[:1], "first meta-step")
    assert a[1][1]["gcn_cache_rows"] == 0, a[1][1]
    assert a[1][0][0].tobytes() != b[1][0][0].tobytes(), "losses equal: the cached rows were not read"


# ----------------------------------------------------------------------------- bypass
def _scattered(ml):
    w = ml.default_windows().copy()
    w[:, :, 1:] = w[:, :, 1:] + 1  # b, b + 2, b + 3: no batch is consecutive
    return w


@pytest.mark.parametrize("case", ["p_gcn", "scattered", "batch1", "budget0"])
def test_bypass(case):
    """GCN dropout, non-consecutive windows, a batch of one and a byte budget of zero: nothing is served or
    filled, and the results are bitwise those of option 0."""
    kw = {"p_gcn": dict(dropout=(0.2, 0.0)), "batch1": dict(batch=1), "scattered": {},
          "budget0": dict(options=(("gcn_stream_cache_mb", 0),))}[case]
    on, off = learner(256, 2, 1, True, **kw), learner(256, 2, 0, True, **kw)
    w = _scattered(on) if case == "scattered" else None
    a, b = run(on, windows=w), run(off, windows=w)
    assert_bitwise(a, b, case)
    for _, vc in a:
        assert served(vc) == (0, 0), vc


# ----------------------------------------------------------------------------- under smaml_meta_step_base
BASE_OUT = ("mg", "gmg", "losses", "norms", "fast")


def base_learner(hc, cache):
    """Two tasks in one pass, order 2, the big knobs, the unclipped setting of test_base_meta_cpu.py (inner_lr 0.1,
    max_norm 10: the sweep's share of the base gradient is well above the tolerance)."""
    ml = learner(hc, 2, cache, True, task_group=None, tasks=2)
    ml.cfg = dataclasses.replace(ml.cfg, inner_lr=0.1, max_norm=10.0)
    return ml


def base_calls(ml, n=2, between=None):
    """`n` smaml_meta_step_base calls on output buffers of their own; per call (outputs, variant counters)."""
    w = ml.default_windows()
    out = []
    for i in range(n):
        if i and between:
            between(ml)
        ml.ctx.variant_counts(reset=True)
        o, _ = bm.call(ml, w)
        out.append(({k: o[k].cpu().numpy().copy() for k in BASE_OUT}, ml.ctx.variant_counts()))
    return out


def assert_base_bitwise(a, b, what):
    for i, ((oa, _), (ob, _)) in enumerate(zip(a, b)):
        for k in BASE_OUT:
            assert np.all(np.isfinite(oa[k])), (what, i, k)
            assert oa[k].tobytes() == ob[k].tobytes(), (what, "call", i, k, float(np.max(np.abs(oa[k] - ob[k]))))


@pytest.mark.parametrize("hc", [256, 16])
def test_base_stage_cached_is_bitwise_the_uncached(hc):
    """Every inner step served, so no per-step feature store: the base stage masks by ``w.F`` as the cache gather
    laid it out. All five outputs, ``gcn_meta_grad`` among them, bitwise those of option 0. The first cached call
    counts every forward and sweep visit (2K + 1) and fills rows, the second fills none; what its ``gcn_layer``
    category still holds is the base stage's own work, never a fill: per stage (K + 1), task (2) and block (t = 0
    and the rows past it) conv1..conv3 recomputed (3 launches) and the three layer-to-layer gradients of
    ``gcn_backward_chain`` (3 timed regions), which carry the same category."""
    on = base_learner(hc, 1)
    on.ctx.timing(True)
    a = base_calls(on, 1)
    t1 = on.ctx.timing_collect()
    a += base_calls(on, 1)
    t2 = on.ctx.timing_collect()
    off = base_learner(hc, 0)
    off.ctx.timing(True)
    b = base_calls(off, 1)
    u1 = off.ctx.timing_collect()
    b += base_calls(off, 1)
    assert_base_bitwise(a, b, f"Hc {hc}")
    assert served(a[0][1])[0] == 2 * K + 1 and served(a[0][1])[1] > 0, a[0][1]
    assert served(a[1][1]) == (2 * K + 1, 0), a[1][1]
    assert served(b[0][1]) == (0, 0) and served(b[1][1]) == (0, 0), (b[0][1], b[1][1])
    stage = 2 * (K + 1) * 2 * (3 + 3)
    print(f"Hc {hc}: gcn_layer launches cached {t1['gcn_layer']['launches']} then {t2['gcn_layer']['launches']}, "
          f"uncached {u1['gcn_layer']['launches']}; the base stage's own {stage}")
    assert t2["gcn_layer"]["launches"] == stage, t2["gcn_layer"]
    assert t1["gcn_layer"]["launches"] > stage and u1["gcn_layer"]["launches"] > stage
    assert not np.array_equal(a[0][0]["gmg"], np.zeros_like(a[0][0]["gmg"]))


@pytest.mark.parametrize("hc", [256, 16])
def test_base_stage_refills_after_new_gcn_values(hc):
    """The base scaled in place and announced by ``set_gcn_params`` between two calls: the cached arm refills what
    the first call filled, stays bitwise the uncached arm, and its ``gcn_meta_grad`` meets the float64 oracle at
    the scaled base (1e-4) -- stale rows would show there."""
    on, off = base_learner(hc, 1), base_learner(hc, 0)
    a, b = base_calls(on, between=_changed_gcn), base_calls(off, between=_changed_gcn)
    assert_base_bitwise(a, b, f"Hc {hc} scaled base")
    assert a[1][1]["gcn_cache_rows"] == a[0][1]["gcn_cache_rows"] > 0, (a[0][1], a[1][1])
    assert a[0][0]["gmg"].tobytes() != a[1][0]["gmg"].tobytes()
    d = on.dims
    names = list(params.unpack(on.theta, d, 0))
    Pt = {k: v.cpu().clone() for k, v in params.unpack(on.theta, d, 0).items()}
    Pg = {k: v.cpu().clone() for k, v in params.unpack(on.gcn, d, 1).items()}  # the scaled values, as the device holds them
    ei = grid_edges(d)
    tasks = [refcpu.TaskData(f.cpu().numpy(), ei, d) for f in on.tasks]
    ref = bmo.meta_step(Pt, Pg, tasks, on.default_windows(), on.cfg.inner_lr, on.cfg.max_norm, 2)
    got = dict(gmg=torch.from_numpy(a[1][0]["gmg"]), mg=torch.from_numpy(a[1][0]["mg"]),
               fast=torch.from_numpy(a[1][0]["fast"]), losses=torch.from_numpy(a[1][0]["losses"]))
    bm.check_base_grad(f"Hc {hc} scaled base", d, got["gmg"], ref)
    bm.check_theta_part(f"Hc {hc} scaled base", d, names, got, ref)
