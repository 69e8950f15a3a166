"""Rolling forecast (smaml_forecast) against the training-forward way of scoring the same windows, timed
on one MI355X: config-2 dims, one region of N = 441 nodes, the reference's 1,200-window cap
(adapt_hybrid_v5.py:152), consecutive windows.

Arms, alternating in one process, each repetition timed on the host with a device synchronise inside:
  forecast_32 / forecast_128  ctx.forecast(skill sums only) in passes of 32 / 128 windows
  meta_step_32                the yardstick: adapt.evaluate's loop of smaml_meta_step(order=0, steps=0,
                              batch=32) over the same windows, one scalar MSE per pass
The forecast arms run on one context, the yardstick on another (their buffers are reported apart). After
the timed repetitions one more repetition per arm runs with the per-category event timing on
(smaml_timing_collect), outside the timed region.

Prints the arms' median and min-max, windows/s, the ratio to the yardstick, smaml_forecast_bytes against
smaml_workspace_bytes, the per-category kernel times, and ONE JSON line last.

With --members E the tool times the MC-dropout ensemble (smaml_forecast_ensemble) instead: E members over the
same windows in passes of --batch (32), scores only, in four arms -- p_gcn = 0 (features, layer 0's projection
and LSTM layer 0 shared by the members) and p_gcn = 0.2 (per-member GCN), each with option ens_share 1 and 0 --
against the arm `deterministic`: smaml_forecast of the same windows at the same pass size in the same run,
whose median times E is the yardstick (E separate eval forecasts). p_lstm = 0.2 throughout. Optional
--group G sets option ens_group for every ensemble arm.

With --rollout R the tool times the autoregressive rollout (smaml_forecast_rollout) instead: --origins (32)
origins, R cycles of Hf + 1 steps, one pass, the trajectory only, in three arms:
  rollout           the library call as shipped (option roll_reuse at its default)
  rollout_reuse_1/0 the option forced on / off (the A/B of keeping layer 0's projection across cycles)
  python_loop       the way without the entry point: per cycle ctx.forecast() of every origin's current window
                    and torch ops on the device that assemble the next windows (gap row, fed-back rows, exogenous
                    channels) into a new stream for set_tasks
and prints smaml_rollout_stats of the reuse arms and how far the loop's trajectory is from the library's.

With --rollout R --members E the tool times the ensemble rollout (smaml_forecast_rollout_ensemble) instead: E
members over --origins (32) origins, R cycles, one pass, p_lstm = 0.2, the statistics only (scores), against the
arm `deterministic`: smaml_forecast_rollout of the same origins (skill sums only) in the same run, whose median
times E is the yardstick (E separate deterministic rollouts). Arms:
  ens                 the library call as shipped (p_gcn = 0, every option at its default)
  ens_group_1/4/8/all option ens_group forced (all = 0; a budget large enough for E members plans the same groups)
  ens_budget_2048     option roll_ens_budget_mb at the 2 GiB of smaml_forecast_ensemble's plan (default grouping)
  ens_share_0         ens_share 0 at ens_group all: LSTM layer 0 of cycle 0 per member
  ens_reuse_0         roll_reuse 0 at ens_group all: every row of every window per member and cycle
  ens_pgcn0.2         p_gcn = 0.2 (per-member GCN on the per-layer kernels), default grouping
and prints smaml_rollout_ensemble_stats and smaml_forecast_bytes of every arm.

Usage: python tools/bench_forecast.py [--reps 5] [--warmup 1] [--windows 1200] [--members E [--batch 32] [--group G]]
       python tools/bench_forecast.py --rollout 15 [--origins 32] [--members 16]
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5, help="timed repetitions per arm (>= 5 for the spread)")
    p.add_argument("--warmup", type=int, default=1, help="untimed repetitions per arm first")
    p.add_argument("--windows", type=int, default=1200)
    p.add_argument("--members", type=int, default=0, help="time the E-member ensemble instead (see above)")
    p.add_argument("--batch", type=int, default=32, help="--members: windows per pass")
    p.add_argument("--group", type=int, default=-1, help="--members: option ens_group (-1: the default plan)")
    p.add_argument("--rollout", type=int, default=0, help="time the R-cycle autoregressive rollout instead (see above)")
    p.add_argument("--origins", type=int, default=32, help="--rollout: origins (one pass)")
    a = p.parse_args()
    if a.rollout > 0:  # the stream holds every origin's R cycles and their targets
        a.windows = a.origins + a.rollout * 9
    import torch

    from weatherforecast_stgcn_maml_amd import _capi, adapt, params, synth
    from weatherforecast_stgcn_maml_amd.config import SEED, ModelDims
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph

    d = ModelDims(num_nodes=441, hidden_channels=256)
    lats, lons = synth.region_grid(n_lat=21, n_lon=21)
    ei, _, _ = build_spatial_graph(lats, lons, 4)
    P = synth.init_params(SEED, d)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    dev = torch.device("cuda:0")
    gflat = params.pack({k: v for k, v in P.items() if k not in names}, d, which=1, device=dev)
    theta = params.pack({k: P[k] for k in names}, d, which=0, device=dev)
    t_total = a.windows + d.window_size + d.forecast_horizon
    stream_t = torch.from_numpy(synth.make_features(synth.task_seed(0), d.num_nodes, t_total)).to(dev)
    windows = list(range(a.windows))
    st = _capi.stream_ptr(torch)

    def context():
        ctx = _capi.Context(d, 0)
        ctx.set_graph(ei)
        ctx.set_gcn_params(gflat)
        ctx.set_tasks([stream_t])
        return ctx

    if a.rollout > 0 and a.members > 0:
        return rollout_ensemble_main(a, d, context, theta, st, torch)
    if a.rollout > 0:
        return rollout_main(a, d, context, theta, stream_t, st, torch)
    if a.members > 0:
        return ensemble_main(a, d, context, theta, windows, st, torch)
    fc_ctx, ms_ctx = context(), context()
    sums = torch.zeros(3, d.forecast_horizon, d.output_channels, device=dev, dtype=torch.float64)
    out = {}

    def forecast_arm(batch):
        def run():
            fc_ctx.forecast(st, theta, windows, batch, skill=sums)
            torch.cuda.synchronize()
            out[f"forecast_{batch}"] = float(sums[0].sum().item()) / (a.windows * d.num_nodes * d.head_out)
        return run

    def meta_arm():
        out["meta_step_32"] = adapt.evaluate(ms_ctx, theta, windows, 32)  # (each pass ends with loss.item(): a sync)
        torch.cuda.synchronize()

    arms = {"forecast_32": (forecast_arm(32), fc_ctx), "forecast_128": (forecast_arm(128), fc_ctx),
            "meta_step_32": (meta_arm, ms_ctx)}
    times = {k: [] for k in arms}
    arms["forecast_32"][0]()  # (untimed) the forecast's buffers at pass size 32, before the 128-window passes grow them
    fb32 = fc_ctx.forecast_bytes()
    for _ in range(a.warmup):
        for fn, _ in arms.values():
            fn()
    for _ in range(a.reps):
        for k, (fn, _) in arms.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    cats = {}
    for k, (fn, ctx) in arms.items():  # where the time goes: one more repetition with event timing on
        ctx.timing(True)
        ctx.timing_collect()
        fn()
        cats[k] = {c: v for c, v in ctx.timing_collect().items() if v["launches"]}
        ctx.timing(False)

    # the same quantity from both paths: the mean squared error over the windows (unscaled)
    assert np.isfinite(list(out.values())).all(), out
    assert abs(out["forecast_32"] - out["meta_step_32"]) <= 1e-4 * out["meta_step_32"], out
    res = {}
    for k, ts in times.items():
        ms = np.asarray(ts) * 1e3
        res[k] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                  "windows_per_s": a.windows / float(np.median(ts))}
        print(f"{k:13s} median {res[k]['median_ms']:8.1f} ms  (min {res[k]['min_ms']:.1f} - max {res[k]['max_ms']:.1f}, "
              f"{a.reps} reps)  {res[k]['windows_per_s']:8.0f} windows/s  mse {out[k]:.6f}")
    base = res["meta_step_32"]
    for k in ("forecast_32", "forecast_128"):
        res[k]["vs_meta_step_32"] = base["median_ms"] / res[k]["median_ms"]
        inside = res[k]["median_ms"] <= base["max_ms"]
        print(f"{k}: {res[k]['vs_meta_step_32']:.2f}x the yardstick's median; median "
              f"{'within or below' if inside else 'ABOVE'} the yardstick's max ({base['max_ms']:.1f} ms); "
              f"ranges {'overlap' if res[k]['max_ms'] >= base['min_ms'] else 'do not overlap'}")
    fb, wb = fc_ctx.forecast_bytes(), ms_ctx.workspace_bytes()
    print(f"smaml_forecast_bytes {fb32} ({fb32 / 2**20:.0f} MiB) at pass size 32, {fb} ({fb / 2**20:.0f} MiB) after "
          f"the passes of 128 (workspace of that context: {fc_ctx.workspace_bytes()} B); smaml_workspace_bytes of the "
          f"yardstick {wb} ({wb / 2**20:.0f} MiB, batch 32): ratio {fb32 / wb:.3f} at equal pass size")
    for k, c in cats.items():
        print(f"{k} kernel ms by category: " +
              ", ".join(f"{n} {v['ms']:.1f} ({v['launches']})" for n, v in c.items()))
    print(json.dumps({
        "metric": "rolling forecast + skill sums, windows/sec (N=441, T=24, config-2 dims)",
        "value": res["forecast_32"]["windows_per_s"], "unit": "windows/s", "higher_is_better": True,
        "windows": a.windows, "reps": a.reps, "warmup": a.warmup, "arms": res,
        "forecast_bytes_pass32": fb32, "forecast_bytes": fb, "yardstick_workspace_bytes": wb,
        "kernel_ms": {k: {n: v["ms"] for n, v in c.items()} for k, c in cats.items()}}))


def ensemble_main(a, d, context, theta, windows, st, torch):
    E, B = a.members, a.batch
    dev = theta.device
    skill = torch.zeros(3, d.forecast_horizon, d.output_channels, device=dev, dtype=torch.float64)
    scores = torch.zeros(4, d.forecast_horizon, d.output_channels, device=dev, dtype=torch.float64)
    out = {}
    det_ctx = context()

    def det():
        det_ctx.forecast(st, theta, windows, B, skill=skill)
        torch.cuda.synchronize()
        out["deterministic"] = skill.cpu().numpy()

    arms = {"deterministic": (det, det_ctx)}
    for p_gcn in (0.0, 0.2):
        for share in (1, 0):
            ctx = context()
            ctx.set_option("ens_share", share)
            ctx.set_option("ens_group", a.group)

            def run(ctx=ctx, p_gcn=p_gcn, key=f"ens_pgcn{p_gcn:g}_share{share}"):
                ctx.forecast_ensemble(st, theta, windows, B, E, p_gcn, 0.2, 12345, scores=scores)
                torch.cuda.synchronize()
                out[key] = scores.cpu().numpy()

            arms[f"ens_pgcn{p_gcn:g}_share{share}"] = (run, ctx)
    times = {k: [] for k in arms}
    for _ in range(a.warmup):
        for fn, _ in arms.values():
            fn()
    for _ in range(a.reps):
        for k, (fn, _) in arms.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    cats = {}
    for k, (fn, ctx) in arms.items():
        ctx.timing(True)
        ctx.timing_collect()
        fn()
        cats[k] = {c: v for c, v in ctx.timing_collect().items() if v["launches"]}
        ctx.timing(False)
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    for p_gcn in ("0", "0.2"):  # sharing changes no bit
        assert np.array_equal(out[f"ens_pgcn{p_gcn}_share1"], out[f"ens_pgcn{p_gcn}_share0"]), p_gcn
    # the persistence sums are the deterministic forecast's (same targets, same blocks)
    assert np.allclose(out["ens_pgcn0_share1"][3], out["deterministic"][2], rtol=1e-6)
    res = {}
    for k, ts in times.items():
        ms = np.asarray(ts) * 1e3
        res[k] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}
    yard = E * res["deterministic"]["median_ms"]
    print(f"{E} members, {a.windows} windows in passes of {B}, ens_group {a.group}, {a.reps} reps after {a.warmup} warm-up")
    for k, r in res.items():
        line = f"{k:22s} median {r['median_ms']:9.1f} ms  (min {r['min_ms']:.1f} - max {r['max_ms']:.1f})"
        if k != "deterministic":
            r["vs_E_x_deterministic"] = r["median_ms"] / yard
            line += f"  = {r['vs_E_x_deterministic']:.3f} x ({E} x deterministic = {yard:.1f} ms)"
        print(line)
    for p_gcn in ("0", "0.2"):
        on, off = res[f"ens_pgcn{p_gcn}_share1"], res[f"ens_pgcn{p_gcn}_share0"]
        print(f"p_gcn {p_gcn}: ens_share 1 / ens_share 0 = {on['median_ms'] / off['median_ms']:.3f} "
              f"(ranges {'overlap' if on['max_ms'] >= off['min_ms'] and off['max_ms'] >= on['min_ms'] else 'do not overlap'})")
    fbytes = {k: ctx.forecast_bytes() for k, (_, ctx) in arms.items()}
    for k, b in fbytes.items():
        print(f"smaml_forecast_bytes {k}: {b} ({b / 2**20:.0f} MiB)")
    for k, c in cats.items():
        print(f"{k} kernel ms by category: " + ", ".join(f"{n} {v['ms']:.1f} ({v['launches']})" for n, v in c.items()))
    best = res["ens_pgcn0_share1"]
    print(json.dumps({
        "metric": f"{E}-member MC-dropout ensemble + scores, member-windows/sec (N=441, T=24, config-2 dims, p_gcn=0)",
        "value": E * a.windows / (best["median_ms"] * 1e-3), "unit": "member-windows/s", "higher_is_better": True,
        "members": E, "windows": a.windows, "batch": B, "ens_group": a.group, "reps": a.reps, "warmup": a.warmup,
        "arms": res, "forecast_bytes": fbytes,
        "kernel_ms": {k: {n: v["ms"] for n, v in c.items()} for k, c in cats.items()}}))


def rollout_main(a, d, context, theta, stream_t, st, torch):
    R, B = a.rollout, a.origins
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    s = Hf + 1
    dev = theta.device
    origins = list(range(B))
    out, stats = {}, {}

    def lib_arm(key, reuse):
        ctx = context()
        if reuse is not None:
            ctx.set_option("roll_reuse", reuse)
        traj = torch.zeros(B, R, s, N, C, device=dev)

        def run():
            ctx.forecast_rollout(st, theta, origins, B, R, 1, traj=traj)
            torch.cuda.synchronize()
            out[key] = traj
            stats[key] = ctx.rollout_stats()
        return run, ctx

    lp_ctx = context()
    wins = [i * T for i in range(B)]
    pred = torch.zeros(B, N * Hf, C, device=dev)
    traj_lp = torch.zeros(B, R, s, N, C, device=dev)

    def loop_arm():
        W = torch.stack([stream_t[o:o + T] for o in origins])  # [B, T, N, Cin]
        for j in range(R):
            lp_ctx.set_tasks([W.reshape(B * T, N, -1).contiguous()])
            lp_ctx.forecast(st, theta, wins, B, pred=pred)
            P = pred.view(B, Hf, N, C)  # the F4 view
            gaprow = 0.5 * (W[:, T - 1, :, :C] + P[:, 0])
            blk = torch.cat([gaprow[:, None], P], dim=1)
            traj_lp[:, j] = blk
            exo = torch.stack([stream_t[o + T + j * s:o + T + (j + 1) * s, :, C:] for o in origins])
            W = torch.cat([W[:, s:], torch.cat([blk, exo], dim=-1)], dim=1)
        torch.cuda.synchronize()
        out["python_loop"] = traj_lp

    arms = {"rollout": lib_arm("rollout", None), "rollout_reuse_1": lib_arm("rollout_reuse_1", 1),
            "rollout_reuse_0": lib_arm("rollout_reuse_0", 0), "python_loop": (loop_arm, lp_ctx)}
    times = {k: [] for k in arms}
    for _ in range(a.warmup):
        for fn, _ in arms.values():
            fn()
    for _ in range(a.reps):
        for k, (fn, _) in arms.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    cats = {}
    for k, (fn, ctx) in arms.items():
        ctx.timing(True)
        ctx.timing_collect()
        fn()
        cats[k] = {c: v for c, v in ctx.timing_collect().items() if v["launches"]}
        ctx.timing(False)
    ref = out["rollout"]
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(out["rollout_reuse_1"], out["rollout_reuse_0"]) and torch.equal(out["rollout_reuse_1"], ref)
    drift = float((out["python_loop"] - ref).norm() / ref.norm())
    res = {}
    for k, ts in times.items():
        ms = np.asarray(ts) * 1e3
        res[k] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}
    print(f"{B} origins x {R} cycles of {s} steps (N = {N}, T = {T}), one pass, {a.reps} reps after {a.warmup} warm-up")
    for k, r in res.items():
        print(f"{k:16s} median {r['median_ms']:8.2f} ms  (min {r['min_ms']:.2f} - max {r['max_ms']:.2f})  "
              f"{r['median_ms'] / R:.2f} ms per cycle")

    def apart(x, y):
        return x["max_ms"] < y["min_ms"] or y["max_ms"] < x["min_ms"]

    on, off, lp = res["rollout_reuse_1"], res["rollout_reuse_0"], res["python_loop"]
    print(f"roll_reuse 1 / roll_reuse 0 = {on['median_ms'] / off['median_ms']:.3f} "
          f"(ranges {'do not overlap' if apart(on, off) else 'overlap'}); rollout / python_loop = "
          f"{res['rollout']['median_ms'] / lp['median_ms']:.3f} (ranges "
          f"{'do not overlap' if apart(res['rollout'], lp) else 'overlap'})")
    for k in ("rollout_reuse_1", "rollout_reuse_0"):
        print(f"smaml_rollout_stats {k}: {stats[k]}")
    print(f"python_loop trajectory against the library's: rel-L2 {drift:.3g} (the loop's windows are not consecutive, "
          f"so smaml_forecast forms layer 0's projection in its K loop: another rounding, fed back {R - 1} times)")
    for k, c in cats.items():
        print(f"{k} kernel ms by category: " + ", ".join(f"{n} {v['ms']:.1f} ({v['launches']})" for n, v in c.items()))
    print(json.dumps({
        "metric": f"{R}-cycle autoregressive rollout, origin-cycles/sec (N=441, T=24, config-2 dims, {B} origins)",
        "value": B * R / (res["rollout"]["median_ms"] * 1e-3), "unit": "origin-cycles/s", "higher_is_better": True,
        "origins": B, "cycles": R, "reps": a.reps, "warmup": a.warmup, "arms": res, "rollout_stats": stats,
        "python_loop_rel_l2": drift,
        "kernel_ms": {k: {n: v["ms"] for n, v in c.items()} for k, c in cats.items()}}))


def rollout_ensemble_main(a, d, context, theta, st, torch):
    R, B, E = a.rollout, a.origins, a.members
    s, N, C = d.forecast_horizon + 1, d.num_nodes, d.output_channels
    dev = theta.device
    origins = list(range(B))
    out, stats = {}, {}
    det_ctx = context()
    skill = torch.zeros(3, R * s, C, device=dev, dtype=torch.float64)

    def det():
        det_ctx.forecast_rollout(st, theta, origins, B, R, 1, skill=skill)
        torch.cuda.synchronize()
        out["deterministic"] = skill.cpu().numpy()

    def ens_arm(key, p_gcn=0.0, **opts):
        ctx = context()
        for k, v in opts.items():
            ctx.set_option(k, v)
        scores = torch.zeros(4, R * s, C, device=dev, dtype=torch.float64)

        def run():
            ctx.forecast_rollout_ensemble(st, theta, origins, B, R, E, p_gcn, 0.2, 12345, scores=scores)
            torch.cuda.synchronize()
            out[key] = scores.cpu().numpy()
            stats[key] = ctx.rollout_ensemble_stats()
        return run, ctx

    arms = {"deterministic": (det, det_ctx), "ens": ens_arm("ens")}
    for g, name in ((1, "1"), (4, "4"), (8, "8"), (0, "all")):
        arms[f"ens_group_{name}"] = ens_arm(f"ens_group_{name}", ens_group=g)
    arms["ens_budget_2048"] = ens_arm("ens_budget_2048", roll_ens_budget_mb=2048)
    arms["ens_share_0"] = ens_arm("ens_share_0", ens_group=0, ens_share=0)
    arms["ens_reuse_0"] = ens_arm("ens_reuse_0", ens_group=0, roll_reuse=0)
    arms["ens_pgcn0.2"] = ens_arm("ens_pgcn0.2", p_gcn=0.2)
    times = {k: [] for k in arms}
    for _ in range(a.warmup):
        for fn, _ in arms.values():
            fn()
    for _ in range(a.reps):
        for k, (fn, _) in arms.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t0)
    cats = {}
    for k, (fn, ctx) in arms.items():
        ctx.timing(True)
        ctx.timing_collect()
        fn()
        cats[k] = {c: v for c, v in ctx.timing_collect().items() if v["launches"]}
        ctx.timing(False)
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    for k in out:  # grouping, sharing and reuse change no bit
        if k not in ("deterministic", "ens", "ens_pgcn0.2"):
            assert np.array_equal(out[k], out["ens"]), k
    # the persistence sums are the deterministic rollout's (same targets, same blocks)
    assert np.allclose(out["ens"][3], out["deterministic"][2], rtol=1e-6)
    res = {}
    for k, ts in times.items():
        ms = np.asarray(ts) * 1e3
        res[k] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}
    yard = E * res["deterministic"]["median_ms"]
    print(f"{E} members x {B} origins x {R} cycles of {s} steps (N = {N}, T = {d.window_size}), one pass, scores only, "
          f"{a.reps} reps after {a.warmup} warm-up")
    for k, r in res.items():
        line = f"{k:16s} median {r['median_ms']:9.2f} ms  (min {r['min_ms']:.2f} - max {r['max_ms']:.2f})"
        if k != "deterministic":
            r["vs_E_x_deterministic"] = r["median_ms"] / yard
            line += f"  = {r['vs_E_x_deterministic']:.3f} x ({E} x deterministic = {yard:.1f} ms)"
        print(line)

    def apart(x, y):
        return x["max_ms"] < y["min_ms"] or y["max_ms"] < x["min_ms"]

    al = res["ens_group_all"]
    for k in ("ens_group_1", "ens_group_4", "ens_group_8", "ens_budget_2048", "ens_share_0", "ens_reuse_0"):
        print(f"ens_group_all / {k} = {al['median_ms'] / res[k]['median_ms']:.3f} "
              f"(ranges {'do not overlap' if apart(al, res[k]) else 'overlap'})")
    for k, v in stats.items():
        print(f"smaml_rollout_ensemble_stats {k}: {v}")
    fbytes = {k: ctx.forecast_bytes() for k, (_, ctx) in arms.items()}
    for k, b in fbytes.items():
        print(f"smaml_forecast_bytes {k}: {b} ({b / 2**20:.0f} MiB)")
    for k, c in cats.items():
        print(f"{k} kernel ms by category: " + ", ".join(f"{n} {v['ms']:.1f} ({v['launches']})" for n, v in c.items()))
    print(json.dumps({
        "metric": f"{E}-member {R}-cycle ensemble rollout + scores, member-origin-cycles/sec (N=441, T=24, config-2 "
                  f"dims, {B} origins, p_gcn=0)",
        "value": E * B * R / (res["ens"]["median_ms"] * 1e-3), "unit": "member-origin-cycles/s",
        "higher_is_better": True, "members": E, "origins": B, "cycles": R, "reps": a.reps, "warmup": a.warmup,
        "arms": res, "stats": stats, "forecast_bytes": fbytes,
        "kernel_ms": {k: {n: v["ms"] for n, v in c.items()} for k, c in cats.items()}}))


if __name__ == "__main__":
    main()
