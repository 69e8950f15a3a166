"""What the graph's form and density cost, timed on one MI355X at config-2 shapes (N = 441 on a 21 x 21 grid,
T = 24, Hc = 256, LSTM 4 x 128). For each graph:

  gcn_ms        the GCN category (smaml_timing category 0, k_gcn_layer / k_gcn_mlp launches) of one second-order
                meta-step (`--tasks` tasks, `--inner-steps` inner steps of `--batch` samples)
  forecast_ms   smaml_forecast over `--windows` consecutive windows in passes of `--fc-batch`, host-timed with a
                device synchronise

The graphs: k = 4 through the ELL (smaml_set_graph) and the same graph through the CSR form
(smaml_set_graph_weighted, NULL weights: bitwise the same results), k = 8 and k = 16 (CSR), and
build_distance_weighted_graph on the unit grid at a threshold that gives about 50 neighbours and at one that
gives the complete graph. `--reps` repetitions after `--warmup`, reported as min - max with the median. ONE JSON
line last.

Usage: python tools/bench_graph.py [--reps 5] [--warmup 1] [--tasks 2] [--inner-steps 5] [--batch 32]
                                   [--windows 1200] [--fc-batch 64] [--graphs k4_ell,k4_csr,...]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIDE = 21
NEAR_THRESHOLD, COMPLETE_THRESHOLD = 4.1, 100.0  # unit grid: 4.1 reaches about 50 neighbours, 100 every node


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--tasks", type=int, default=2)
    p.add_argument("--inner-steps", type=int, default=5)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--windows", type=int, default=1200)
    p.add_argument("--fc-batch", type=int, default=64)
    p.add_argument("--graphs", default="k4_ell,k4_csr,k8,k16,dist_near,dist_complete")
    a = p.parse_args()
    import torch

    from weatherforecast_stgcn_maml_amd import _capi, params, synth
    from weatherforecast_stgcn_maml_amd.config import CONFIG2, SEED, MamlConfig
    from weatherforecast_stgcn_maml_amd.graph import build_distance_weighted_graph, build_spatial_graph
    from weatherforecast_stgcn_maml_amd.maml import MetaLearner, stream_len_for

    if not torch.cuda.is_available():
        raise SystemExit("bench_graph needs a HIP device (no CPU fallback)")
    d = CONFIG2
    assert d.num_nodes == SIDE * SIDE
    grid = np.arange(float(SIDE))
    knn = {k: build_spatial_graph(grid, grid, k)[0] for k in (4, 8, 16)}
    near = build_distance_weighted_graph(grid, grid, NEAR_THRESHOLD)
    complete = build_distance_weighted_graph(grid, grid, COMPLETE_THRESHOLD)
    # name -> (edge_index, edge_weight, force the CSR form)
    graphs = {"k4_ell": (knn[4], None, False), "k4_csr": (knn[4], None, True), "k8": (knn[8], None, True),
              "k16": (knn[16], None, True), "dist_near": (near[0], near[1], True),
              "dist_complete": (complete[0], complete[1], True)}
    cfg = MamlConfig(inner_steps=a.inner_steps, batch=a.batch, order=2)
    P = synth.init_params(SEED, d)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    feats = [synth.make_features(synth.task_seed(j), d.num_nodes, stream_len_for(cfg, d)) for j in range(a.tasks)]
    dev = torch.device("cuda:0")
    fc_stream = torch.from_numpy(synth.make_features(synth.task_seed(7), d.num_nodes, synth.t_total_for(a.windows))).to(dev)
    windows = np.arange(a.windows, dtype=np.int32)
    st = _capi.stream_ptr(torch)
    print(f"build: {_capi.build_info()}")
    print(f"meta-step: order 2, {a.tasks} tasks, {a.inner_steps} inner steps, batch {a.batch}; forecast: {a.windows} "
          f"windows in passes of {a.fc_batch}; {a.reps} repetitions after {a.warmup}")
    result = {"dims": d.as_dict(), "reps": a.reps, "graphs": {}}
    for name in a.graphs.split(","):
        ei, ew, csr = graphs[name]
        ml = MetaLearner(d, cfg, {k: v for k, v in P.items() if k not in names}, {k: P[k] for k in names}, ei,
                         device="cuda:0", task_group=None, edge_weight=ew)
        ctx = ml.ctx
        if csr:
            ctx.set_graph_weighted(ei, ew)
        ml.set_tasks(feats)
        gs = ctx.graph_stats()
        assert gs["form"] == (2 if csr else 1), gs
        gcn_ms, step_ms = [], []
        for rep in range(a.warmup + a.reps):
            if rep == a.warmup:
                ctx.timing_collect()
                ctx.timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ml.meta_step(sync=False)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                step_ms.append((time.perf_counter() - t0) * 1e3)
                gcn_ms.append(ctx.timing_collect()["gcn_layer"]["ms"])
        ctx.timing(False)
        # the forecast on the same context (the meta-step's tasks are replaced by the long stream)
        ctx.set_tasks([fc_stream])
        pred = torch.empty(a.windows, d.num_nodes * d.forecast_horizon, d.output_channels, device=dev)
        fc_ms = []
        for rep in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.forecast(st, ml.theta, windows, a.fc_batch, pred=pred)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                fc_ms.append((time.perf_counter() - t0) * 1e3)
        gs = ctx.graph_stats()
        r = {"form": gs["form"], "entries": gs["entries"], "longest_row": gs["longest_row"], "gcn_ms": stats(gcn_ms),
             "meta_step_ms": stats(step_ms), "forecast_ms": stats(fc_ms)}
        result["graphs"][name] = r
        print(f"{name:14s} form {gs['form']} entries {gs['entries']:7d} longest row {gs['longest_row']:4d} | "
              f"GCN of one meta-step {r['gcn_ms']['min']:8.3f} - {r['gcn_ms']['max']:8.3f} ms (median "
              f"{r['gcn_ms']['median']:8.3f}) | meta-step {r['meta_step_ms']['min']:8.1f} - {r['meta_step_ms']['max']:8.1f} ms | "
              f"forecast {r['forecast_ms']['min']:8.2f} - {r['forecast_ms']['max']:8.2f} ms (median "
              f"{r['forecast_ms']['median']:8.2f})", flush=True)
        ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
