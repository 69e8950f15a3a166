"""What the weighted loss and the weighted scores cost, timed on one MI355X at config-2 shapes (N = 441, T = 24,
Hc = 256, LSTM 4 x 128). Three measurements, each with its arms interleaved repetition by repetition on one context
(set / clear between repetitions, so drift hits every arm alike):

  meta_step_ms   one second-order meta-step (`--tasks` tasks, `--inner-steps` inner steps of `--batch` samples, as
                 tools/bench_graph.py measures it), host-timed with a device synchronise: no table, one shared
                 table, one table per task
  forecast_ms    smaml_forecast's skill sums over `--windows` consecutive windows in passes of `--fc-batch`, with
                 and without node weights
  adapt_step_ms  tools/bench_adapt.py's later-epoch step (batch 1, every window's GCN features cached): ms per
                 step of an epoch of `--adapt-steps` steps, with and without a table

`--reps` repetitions after `--warmup`, reported as min - max with the median; the lines are appended to `--log`.
ONE JSON line last.

Usage: python tools/bench_loss.py [--reps 5] [--warmup 1] [--tasks 2] [--inner-steps 5] [--batch 32]
                                  [--windows 1200] [--fc-batch 64] [--adapt-steps 240]
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


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def fmt(s):
    return f"{s['min']:9.3f} - {s['max']:9.3f} ms (median {s['median']:9.3f})"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--tasks", type=int, default=2)
    p.add_argument("--inner-steps", type=int, default=5)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--windows", type=int, default=1200)
    p.add_argument("--fc-batch", type=int, default=64)
    p.add_argument("--adapt-steps", type=int, default=240)
    p.add_argument("--log", default=os.path.join(REPO, "profiles", "weighted_loss_bench.log"))
    a = p.parse_args()
    import torch

    from weatherforecast_stgcn_maml_amd import _capi, adapt, loss, params, synth
    from weatherforecast_stgcn_maml_amd.config import CONFIG2, SEED, MamlConfig
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph
    from weatherforecast_stgcn_maml_amd.maml import MetaLearner, stream_len_for

    if not torch.cuda.is_available():
        raise SystemExit("bench_loss needs a HIP device (no CPU fallback)")
    d = CONFIG2
    lats, lons = synth.region_grid(n_lat=21, n_lon=21)
    ei, _, pos = build_spatial_graph(lats, lons, 4)  # pos [N, 2]: each node's (lat, lon)
    P = synth.init_params(SEED, d)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    gcn, theta = {k: v for k, v in P.items() if k not in names}, {k: P[k] for k in names}
    dev = torch.device("cuda:0")
    st = _capi.stream_ptr(torch)
    rng = np.random.default_rng(SEED)
    node_w = loss.latitude_weights(pos[:, 0])
    tables = [loss.make_loss_weights(d, node=node_w, variable=rng.uniform(0.25, 4.0, d.output_channels),
                                     lead=rng.uniform(0.25, 4.0, d.forecast_horizon)) for _ in range(a.tasks)]
    log = open(a.log, "a")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")

    say(f"build: {_capi.build_info()}")
    result = {"dims": d.as_dict(), "reps": a.reps}

    # ---- second-order meta-step
    cfg = MamlConfig(inner_steps=a.inner_steps, batch=a.batch, order=2)
    feats = [synth.make_features(synth.task_seed(j), d.num_nodes, stream_len_for(cfg, d)) for j in range(a.tasks)]
    ml = MetaLearner(d, cfg, gcn, theta, ei, device="cuda:0", task_group=None)
    ml.set_tasks(feats)
    arms = {"none": None, "shared": tables[0], "per_task": np.stack(tables)}
    ms = {k: [] for k in arms}
    for rep in range(a.warmup + a.reps):
        for name, tab in arms.items():
            ml.ctx.set_loss_weights(tab)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ml.meta_step(sync=False)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    ml.ctx.set_loss_weights(None)
    result["meta_step_ms"] = {k: stats(v) for k, v in ms.items()}
    say(f"meta-step: order 2, {a.tasks} tasks, {a.inner_steps} inner steps, batch {a.batch}; {a.reps} repetitions after "
        f"{a.warmup}, arms interleaved")
    for k, v in result["meta_step_ms"].items():
        say(f"  {k:9s} {fmt(v)}")

    # ---- forecast skill sums
    ctx = ml.ctx
    fc_stream = torch.from_numpy(synth.make_features(synth.task_seed(7), d.num_nodes, synth.t_total_for(a.windows))).to(dev)
    ctx.set_tasks([fc_stream])
    windows = np.arange(a.windows, dtype=np.int32)
    sums = torch.empty(3, d.forecast_horizon, d.output_channels, device=dev, dtype=torch.float64)
    arms = {"none": None, "node_weights": node_w}
    ms = {k: [] for k in arms}
    for rep in range(a.warmup + a.reps):
        for name, v in arms.items():
            ctx.set_score_weights(v)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.forecast(st, ml.theta, windows, a.fc_batch, skill=sums)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    ctx.set_score_weights(None)
    result["forecast_ms"] = {k: stats(v) for k, v in ms.items()}
    say(f"forecast: skill sums of {a.windows} windows in passes of {a.fc_batch}")
    for k, v in result["forecast_ms"].items():
        say(f"  {k:12s} {fmt(v)}")
    ctx.close()

    # ---- the later-epoch adaptation step (batch 1, features cached)
    n = a.adapt_steps
    stream_t = torch.from_numpy(synth.make_features(synth.task_seed(0), d.num_nodes, synth.t_total_for(n))).to(dev)
    ctx = _capi.Context(d, 0)
    ctx.set_graph(ei)
    gflat = params.pack({k: v for k, v in gcn.items() if k.startswith("base_stgcn.conv")}, d, which=1, device=dev)
    ctx.set_gcn_params(gflat)
    th = params.pack(theta, d, which=0, device=dev)
    ctx.set_tasks([stream_t])
    ctx.set_task_ids([0])
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    lr, wd = adapt.climate_optimizer_config("Amazon", 0.0006)
    lr_dev = torch.full((n,), lr, device=dev, dtype=torch.float32)
    losses = torch.empty(n, device=dev)
    arms = {"none": None, "table": tables[0]}
    ms = {k: [] for k in arms}
    step = 0
    for rep in range(a.warmup + 1 + a.reps):  # (the first epoch fills the feature cache)
        for name, tab in arms.items():
            ctx.set_loss_weights(tab)
            order = rng.permutation(n).astype(np.int32).reshape(n, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.adapt_steps(st, th, m, v, step, order, lr_dev, (0.9, 0.999), 1e-8, wd, adapt.MAX_GRAD_NORM, losses)
            torch.cuda.synchronize()
            step += n
            if rep >= a.warmup + 1:
                ms[name].append((time.perf_counter() - t0) * 1e3 / n)
    result["adapt_step_ms"] = {k: stats(v) for k, v in ms.items()}
    say(f"adaptation: later-epoch step, batch 1, epochs of {n} steps")
    for k, v in result["adapt_step_ms"].items():
        say(f"  {k:9s} {fmt(v)}")
    ctx.close()
    log.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
