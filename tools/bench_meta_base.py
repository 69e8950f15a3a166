"""What the base meta-gradient costs: smaml_meta_step against smaml_meta_step_base in its two row forms, on one
MI355X, at the setting of the README's GCN-share figures -- config-2 shapes (N = 441), 2 tasks, K = 5 inner steps,
B = 32, order 2, the default (consecutive) window table, synthetic streams (seeds 1000..), random-init weights.

Arms, interleaved in one process, each repetition --steps calls timed on the host around a device synchronise
(every buffer and the per-stream feature cache warm: the base does not move here, so all arms see the same cache):
  plain    smaml_meta_step
  dedup1   smaml_meta_step_base, option meta_base_dedup = 1 (distinct-row form on the consecutive steps)
  dedup0   smaml_meta_step_base, option meta_base_dedup = 0 (per-sample form on every step)
Reports min / median / max ms per call over --reps repetitions after --warmup, the stage counters of the base
arms, and the largest rel-L2 difference of a conv tensor between the two forms (they differ in summation order).
--arms picks a subset; --repo measures another tree's package with this tool (the parent commit's `plain`).
The lines go to stdout and are appended to --log (default profiles/meta_base_bench.log); ONE JSON line last.

Usage: python tools/bench_meta_base.py [--reps 5] [--steps 3] [--warmup 1] [--arms plain,dedup1,dedup0]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--steps", type=int, default=3, help="calls per timed repetition")
    p.add_argument("--warmup", type=int, default=1, help="untimed repetitions of every arm")
    p.add_argument("--arms", default="plain,dedup1,dedup0")
    p.add_argument("--tasks", type=int, default=2)
    p.add_argument("--inner-steps", type=int, default=5)
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--nodes", type=int, default=0, help="0: config 2's 441 (a square number otherwise)")
    p.add_argument("--repo", default=HERE, help="the tree whose package is measured (default: this one)")
    p.add_argument("--label", default="")
    p.add_argument("--log", default=os.path.join(HERE, "profiles", "meta_base_bench.log"))
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))

    import dataclasses

    import torch

    from weatherforecast_stgcn_maml_amd import _capi, params, synth
    from weatherforecast_stgcn_maml_amd.config import CONFIG2, MamlConfig
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph
    from weatherforecast_stgcn_maml_amd.maml import MetaLearner, stream_len_for

    if not torch.cuda.is_available():
        raise SystemExit("bench_meta_base needs a HIP device (no CPU fallback)")
    d = CONFIG2 if not a.nodes else dataclasses.replace(CONFIG2, num_nodes=a.nodes)
    side = int(round(d.num_nodes ** 0.5))
    assert side * side == d.num_nodes
    cfg = MamlConfig(inner_steps=a.inner_steps, batch=a.batch, order=2)
    lats, lons = synth.region_grid(n_lat=side, n_lon=side)
    ei = build_spatial_graph(lats, lons, 4)[0]
    P = synth.init_params(3, d, gcn_bias_scale=0.1)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    feats = [synth.make_features(1000 + j, d.num_nodes, stream_len_for(cfg, d)) for j in range(a.tasks)]
    arms = [x for x in a.arms.split(",") if x]
    st = _capi.stream_ptr(torch)

    def learner(dedup):
        ml = MetaLearner(d, cfg, {k: v for k, v in P.items() if k not in names}, {k: P[k] for k in names}, ei,
                         device="cuda:0", task_group=None)
        ml.set_tasks(feats)
        if dedup is not None:
            ml.ctx.set_option("meta_base_dedup", dedup)
        return ml

    ctx = {arm: learner({"plain": None, "dedup1": 1, "dedup0": 0}[arm]) for arm in arms}
    w = next(iter(ctx.values())).default_windows()
    bufs = {arm: (torch.zeros_like(ml.theta), torch.zeros_like(ml.gcn)) for arm, ml in ctx.items()}

    def run(arm, n):
        ml = ctx[arm]
        mg, gmg = bufs[arm]
        args = (st, ml.theta, 2, cfg.inner_steps, cfg.batch, w, cfg.inner_lr, cfg.max_norm, cfg.query_loss_scale)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            if arm == "plain":
                ml.ctx.meta_step(*args, meta_grad=mg)
            else:
                ml.ctx.meta_step_base(*args, mg, gmg)
        ml.ctx.sync(st)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    for _ in range(a.warmup):
        for arm in arms:
            run(arm, 1)
    ms = {arm: [] for arm in arms}
    for _ in range(a.reps):
        for arm in arms:  # interleaved: every repetition visits every arm
            ms[arm].append(run(arm, a.steps))
    out = {"tool": "bench_meta_base", "label": a.label, "nodes": d.num_nodes, "tasks": a.tasks, "K": cfg.inner_steps,
           "B": cfg.batch, "order": 2, "reps": a.reps, "steps": a.steps, "arms": {}}
    lines = []
    for arm in arms:
        v = sorted(ms[arm])
        out["arms"][arm] = {"min_ms": round(v[0], 3), "median_ms": round(float(np.median(v)), 3), "max_ms": round(v[-1], 3)}
        line = f"{a.label or 'tree'} {arm}: ms per call min {v[0]:.3f} median {np.median(v):.3f} max {v[-1]:.3f} ({a.reps} x {a.steps})"
        if arm != "plain":
            s = ctx[arm].ctx.meta_base_stats()
            out["arms"][arm]["stats"] = s
            line += f"; stages {s['stages']} distinct {s['distinct']} per_sample {s['per_sample']} rows {s['rows']} bytes {s['bytes']}"
        lines.append(line)
    if "dedup1" in arms and "dedup0" in arms:
        g1, g0 = params.unpack(bufs["dedup1"][1], d, 1), params.unpack(bufs["dedup0"][1], d, 1)
        diff = max(float((g1[k] - g0[k]).norm() / g0[k].norm()) for k in g0)
        same = all(torch.equal(bufs["dedup1"][0], bufs[x][0]) for x in arms)
        out["forms_max_rel_l2"] = diff
        out["meta_grad_bitwise_equal_across_arms"] = same
        lines.append(f"distinct-row vs per-sample form: largest rel-L2 difference of a conv tensor {diff:.3e}; "
                     f"meta_grad bitwise equal across arms: {same}")
        r1, r0 = out["arms"]["dedup1"]["stats"]["rows"], out["arms"]["dedup0"]["stats"]["rows"]
        lines.append(f"rows through the GCN backward: per-sample {r0}, distinct-row {r1} ({r0 / max(r1, 1):.2f}x)")
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "a") as f:
        for line in lines:
            print(line)
            f.write(line + "\n")
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
