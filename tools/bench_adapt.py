"""BASELINE config 4 (regional adaptation, adapt_hybrid_v5.py:65-257): the 15-epoch fine-tune of the
pretrained init on one region -- epochs of 960 shuffled batch-1 train steps (fwd + bwd + clip +
Adam(L2)), then the no-grad validation pass over the 240 held-out windows -- timed on one MI355X.

Prints ONE JSON line: sample-steps/s over a full 15-epoch adaptation from a cold context (inputs
resident in HBM, each epoch is one smaml_adapt_steps call; GCN features are computed on a window's
first use and reused by later epochs), the first / later epoch and validation times, and the reference's CPU path
(oracle.refcpu.ReferencePort, batch-1 per-node nn.LSTM loop) timed on a bounded sample of the same
sample-steps on this host. Synthetic ERA5-shaped stream (seed 1000), random-init weights.

Usage: python tools/bench_adapt.py [--epochs 15] [--warmup 1] [--cpu-sample-steps 4]

--regions R: R regions (R streams, seeds 1000..) adapted in lockstep (smaml_adapt_steps_multi, one call per
epoch) against the same R regions adapted one after another on the single-region path (smaml_adapt_steps,
a fresh context per region, as main.py's loop pays it), in the same process. One JSON line: ms per lockstep
step and region-sample-steps/s of the first epoch and of the later epochs (min / median / max over the
later epochs: each is one repetition; --epochs 6 gives five), the set-up time (workspace + feature caches,
smaml_adapt_prepare[_multi]), the bytes the set-up took, the ratio sequential / lockstep, and with
--timing the per-category kernel time of one more lockstep epoch. --adapt-group g runs g regions per
launch set (option adapt_group); --no-sequential skips the yardstick.

--train-base: whole-model adaptation (smaml_adapt_steps_full: the GCN base trained inside the step) at config-4
shapes, batch 1, no dropout, later epochs (every buffer and cache warm), ms per step. Arms, alternating in one
process, each repetition --steps steps timed on the host around a device synchronise:
  full                smaml_adapt_steps_full, default options
  full_keep0          ... option gcn_keep = 0 (frozen-base forward + recompute of conv1..conv3)
  full_dz_fused       ... option gcn_dz_fused = 1 (k_gcn_dz instead of GEMM + gather + mask per layer)
  module              yardstick (a): the same steps through HybridSTGCN_LSTM(base_grad=True) with MSE,
                      clip_grad_norm_(1.0) and torch.optim.Adam(weight_decay), windows already on the device
  frozen              yardstick (b): smaml_adapt_steps (frozen base, feature cache warm): what training the base
                      costs on top of it, not a race
Medians of --reps repetitions after --warmup, with min and max; then the event time per timing category of one
more repetition of each library arm (gcn_layer: the GCN forward and recompute; misc: k_lstm_dx0, k_gcn_dz or its
composed form, the weight re-split, k_sqsum + k_adam_l2). The lines go to stdout and to --log
(default profiles/adapt_full_bench.log); ONE JSON line last.
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
    p.add_argument("--epochs", type=int, default=15, help="timed epochs (the reference adapts for 15)")
    p.add_argument("--warmup", type=int, default=1, help="untimed one-epoch runs on a separate context")
    p.add_argument("--max-samples", type=int, default=1200)
    p.add_argument("--cpu-sample-steps", type=int, default=4)
    p.add_argument("--region", default="Amazon")
    p.add_argument("--regions", type=int, default=0, help="R > 0: lockstep adaptation of R regions vs sequential")
    p.add_argument("--adapt-group", type=int, default=-1, help="option adapt_group of the lockstep run (-1: the default plan)")
    p.add_argument("--no-sequential", action="store_true")
    p.add_argument("--timing", action="store_true", help="one more lockstep epoch with per-category kernel timing")
    p.add_argument("--train-base", action="store_true", help="whole-model adaptation arms and yardsticks (see above)")
    p.add_argument("--steps", type=int, default=48, help="--train-base: steps per timed repetition")
    p.add_argument("--reps", type=int, default=5, help="--train-base: timed repetitions per arm")
    p.add_argument("--log", default=os.path.join(REPO, "profiles", "adapt_full_bench.log"))
    a = p.parse_args()
    if a.train_base:
        return train_base_main(a)
    if a.regions > 0:
        return regions_main(a)
    import torch

    from weatherforecast_stgcn_maml_amd import _capi, adapt, params, synth
    from weatherforecast_stgcn_maml_amd.config import SEED, ModelDims
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph

    d = ModelDims(num_nodes=441, hidden_channels=256)
    lats, lons = synth.region_grid(n_lat=21, n_lon=21)
    ei, _, _ = build_spatial_graph(lats, lons, 4)
    P = synth.init_params(SEED, d)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    gcn = {k: v for k, v in P.items() if k not in names}
    theta = {k: P[k] for k in names}
    T_total = a.max_samples + d.window_size + d.forecast_horizon
    feats = synth.make_features(synth.task_seed(0), d.num_nodes, T_total)
    dev = torch.device("cuda:0")
    n_all = synth.num_samples(T_total, d.window_size, d.forecast_horizon)
    n_max = min(a.max_samples, n_all)
    n_train = int(0.8 * n_max)
    lr, wd = adapt.climate_optimizer_config(a.region, 0.0006)
    stream_t = torch.from_numpy(np.ascontiguousarray(feats)).to(dev)
    stream = _capi.stream_ptr(torch)

    def run(n_epochs, per_epoch=None):
        """A fresh context (cold GCN feature cache) adapting the pretrained init for n_epochs."""
        ctx = _capi.Context(d, 0)
        ctx.set_graph(ei)
        gflat = params.pack(gcn, d, which=1, device=dev)
        ctx.set_gcn_params(gflat)
        th = params.pack(theta, d, which=0, device=dev)
        ctx.set_tasks([stream_t])
        ctx.set_task_ids([0])
        m = torch.zeros_like(th)
        v = torch.zeros_like(th)
        losses = torch.empty(n_train, device=dev)
        step = 0
        torch.cuda.synchronize()
        for _ in range(n_epochs):
            t0 = time.perf_counter()
            order = adapt.random_sampler_order(n_train).numpy().astype(np.int32)
            lr_dev = torch.full((n_train,), lr, device=dev, dtype=torch.float32)
            ctx.adapt_steps(stream, th, m, v, step, order.reshape(n_train, 1), lr_dev, (0.9, 0.999), 1e-8, wd,
                            adapt.MAX_GRAD_NORM, losses)
            step += n_train
            if per_epoch is not None:
                torch.cuda.synchronize()
                per_epoch.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        return ctx, th, gflat, float(losses.double().mean().item())

    for _ in range(a.warmup):
        run(1)  # module load, first-touch of the workspace
    epochs_s = []
    t0 = time.perf_counter()
    ctx, th, gflat, loss = run(a.epochs, epochs_s)
    t_total = time.perf_counter() - t0
    t_epoch = t_total / a.epochs
    t0 = time.perf_counter()
    val = adapt.evaluate(ctx, th, list(range(n_train, n_max)), 32)
    torch.cuda.synchronize()
    t_val = time.perf_counter() - t0
    assert np.isfinite(loss) and np.isfinite(val), (loss, val)

    out = {
        "metric": "regional adaptation sample-steps/sec (batch-1 fwd+bwd+clip+Adam, N=441, T=24)",
        "value": n_train / t_epoch,
        "unit": "sample-steps/s",
        "n_gpus": 1,
        "epochs": a.epochs,
        "warmup": a.warmup,
        "ms_per_epoch": t_epoch * 1e3,
        "first_epoch_ms": epochs_s[0] * 1e3,
        "later_epoch_ms": float(np.mean(epochs_s[1:])) * 1e3 if len(epochs_s) > 1 else None,
        "ms_per_sample_step": t_epoch / n_train * 1e3,
        "val_ms": t_val * 1e3,
        "higher_is_better": True,
        "dtype": "f32",
        "data": "synthetic ERA5-shaped feature stream (numpy PCG64 seed 1000), random-init weights",
        "config": {"workload": f"BASELINE config 4: {a.epochs}-epoch adaptation (adapt_hybrid_v5), epochs of "
                               f"{n_train} shuffled batch-1 train steps + {n_max - n_train}-window validation, "
                               f"N=441, Hc=256, LSTM 4x128, Adam(L2) lr {lr:g} wd {wd:g} ({a.region}); GCN "
                               f"features computed once per window (frozen GCN, no GCN dropout: F2)",
                   "train_samples": n_train, "val_samples": n_max - n_train},
        "train_loss": loss,
        "val_loss": val,
    }
    if a.cpu_sample_steps > 0:
        from bench import cpu_baseline
        t_cpu, cores = cpu_baseline(d, a.cpu_sample_steps, P, ei, feats)
        out["cpu_baseline"] = {"value": 1.0 / t_cpu, "unit": "sample-steps/s", "cores": cores, "kind": "port",
                               "sample": f"{a.cpu_sample_steps} batch-1 sample-steps of the reference's per-node "
                                         f"nn.LSTM CPU path at N=441, {t_cpu:.3f} s each"}
        out["vs_cpu_baseline"] = out["value"] * t_cpu
    print(json.dumps(out))


REGION_NAMES = ("Amazon", "Thailand", "Moscow", "Delhi", "Indonesia", "NorthSiberia", "Sahara", "QueensAustralia",
                "Afghanistan", "Alps", "Andes", "Congo", "Gobi", "Iberia", "Japan", "Kalahari", "Patagonia", "Texas")


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "n": len(xs)} if xs else None


def train_base_main(a):
    import torch

    from weatherforecast_stgcn_maml_amd import _capi, adapt, params, synth
    from weatherforecast_stgcn_maml_amd.config import SEED, ModelDims
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph
    from weatherforecast_stgcn_maml_amd.hybrid_model import HybridSTGCN_LSTM
    from weatherforecast_stgcn_maml_amd.model import STGCN

    if not torch.cuda.is_available():
        raise SystemExit("bench_adapt --train-base needs a HIP device (no CPU fallback)")
    d = ModelDims(num_nodes=441, hidden_channels=256)
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    lats, lons = synth.region_grid(n_lat=21, n_lon=21)
    ei, _, _ = build_spatial_graph(lats, lons, 4)
    P = synth.init_params(SEED, d, gcn_bias_scale=0.1)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    conv = [k for k in P if k.startswith("base_stgcn.conv")]
    dev = torch.device("cuda:0")
    n_steps = a.steps
    T_total = n_steps + T + Hf
    stream_t = torch.from_numpy(np.ascontiguousarray(synth.make_features(synth.task_seed(0), N, T_total))).to(dev)
    lr, wd = adapt.climate_optimizer_config(a.region, 0.0006)
    st = _capi.stream_ptr(torch)
    rng = np.random.default_rng(SEED)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"build: {_capi.build_info()}")
    say(f"config-4 shapes N={N} T={T} Hc={d.hidden_channels} LSTM {d.lstm_num_layers}x{d.lstm_hidden_size}, batch 1, "
        f"p = 0, {n_steps} steps per repetition, {a.reps} repetitions after {a.warmup} warm-up, Adam lr {lr:g} wd {wd:g}")

    class LibArm:
        def __init__(self, full, options=()):
            self.full = full
            self.ctx = _capi.Context(d, 0)
            for k, v in options:
                self.ctx.set_option(k, v)
            self.ctx.set_graph(ei)
            self.g = params.pack({k: P[k] for k in conv}, d, which=1, device=dev)
            self.ctx.set_gcn_params(self.g)
            self.th = params.pack({k: P[k] for k in names}, d, which=0, device=dev)
            self.ctx.set_tasks([stream_t])
            self.ctx.set_task_ids([0])
            self.vecs = [torch.zeros_like(self.th), torch.zeros_like(self.th), torch.zeros_like(self.g),
                         torch.zeros_like(self.g)]
            self.losses = torch.empty(n_steps, device=dev)
            self.lr_dev = torch.full((n_steps,), lr, device=dev, dtype=torch.float32)
            self.step = 0

        def run(self, order):
            m, v, gm, gv = self.vecs
            w = order.reshape(n_steps, 1)
            if self.full:
                self.ctx.adapt_steps_full(st, self.th, m, v, self.g, gm, gv, self.step, w, self.lr_dev, (0.9, 0.999),
                                          1e-8, wd, adapt.MAX_GRAD_NORM, self.losses)
            else:
                self.ctx.adapt_steps(st, self.th, m, v, self.step, w, self.lr_dev, (0.9, 0.999), 1e-8, wd,
                                     adapt.MAX_GRAD_NORM, self.losses)
            self.step += n_steps

    class ModuleArm:
        def __init__(self):
            base = STGCN(d.input_channels, d.hidden_channels, C, T, Hf, dropout_rate=0.0)
            self.m = HybridSTGCN_LSTM(base, d.lstm_hidden_size, d.lstm_num_layers, 0.0, C, Hf, freeze_base=False,
                                      base_grad=True)
            self.m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
            self.m = self.m.to(dev).train()
            self.eig = torch.from_numpy(np.ascontiguousarray(ei)).to(dev)
            self.ps = [q for q in self.m.parameters() if q.requires_grad]
            self.opt = torch.optim.Adam(self.ps, lr=lr, weight_decay=wd)
            self.losses = torch.empty(n_steps, device=dev)

        def run(self, order):
            for k, i in enumerate(order):
                i = int(i)
                x = stream_t[i:i + T].reshape(T * N, -1)
                y = stream_t[i + T + 1:i + T + 1 + Hf, :, :C].reshape(Hf * N, C)
                self.opt.zero_grad()
                loss = torch.nn.functional.mse_loss(self.m(x, self.eig), y)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(self.ps, adapt.MAX_GRAD_NORM)
                self.opt.step()
                self.losses[k] = loss.detach()

    arms = {"full": LibArm(True), "full_keep0": LibArm(True, (("gcn_keep", 0),)),
            "full_dz_fused": LibArm(True, (("gcn_dz_fused", 1),)), "module": ModuleArm(), "frozen": LibArm(False)}
    times = {k: [] for k in arms}
    first_loss = {}
    for rep in range(a.warmup + a.reps):
        order = rng.permutation(n_steps).astype(np.int32)
        for k, arm in arms.items():  # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            arm.run(order)
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3 / n_steps)
            if rep == 0:
                first_loss[k] = float(arm.losses.double().mean().item())

    def stats(v):
        return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    res = {k: stats(v) for k, v in times.items()}
    say("--- ms per step (host time around a device synchronise)")
    for k, s_ in res.items():
        say(f"  {k:18s} {s_['median']:9.4f}  (min {s_['min']:.4f}, max {s_['max']:.4f})   first-repetition mean loss "
            f"{first_loss[k]:.6f}")

    def outside(fast, slow):  # the faster arm's worst repetition still beats the slower arm's best
        return bool(res[fast]["max"] < res[slow]["min"])

    verdict = {
        "full_vs_module": {"ratio": res["module"]["median"] / res["full"]["median"], "outside_spread": outside("full", "module")},
        "keep_vs_recompute": {"ratio": res["full_keep0"]["median"] / res["full"]["median"],
                              "outside_spread": outside("full", "full_keep0")},
        "dz_fused_vs_composed": {"ratio": res["full"]["median"] / res["full_dz_fused"]["median"],
                                 "outside_spread": outside("full_dz_fused", "full")},
        "base_training_costs_x_frozen": res["full"]["median"] / res["frozen"]["median"],
    }
    for k, v in verdict.items():
        say(f"  {k}: {v}")
    # event time per category, one more repetition of each library arm
    cats = {}
    order = rng.permutation(n_steps).astype(np.int32)
    for k, arm in arms.items():
        if k == "module":
            continue
        arm.ctx.timing(True)
        arm.run(order)
        cats[k] = {c: {"us_per_step": t["ms"] * 1e3 / n_steps, "launches_per_step": t["launches"] / n_steps}
                   for c, t in arm.ctx.timing_collect().items() if t["launches"]}
        arm.ctx.timing(False)
        say(f"--- event time per step, {k}: " + ", ".join(f"{c} {t['us_per_step']:.1f} us ({t['launches_per_step']:.1f} launches)"
                                                         for c, t in cats[k].items()))
    stats_full = arms["full"].ctx.adapt_full_stats()
    say(json.dumps({"metric": "whole-model adaptation, ms per batch-1 step at config-4 shapes (median)",
                    "value": res["full"]["median"], "unit": "ms/step", "higher_is_better": False, "steps": n_steps,
                    "reps": a.reps, "ms_per_step": res, "verdict": verdict, "event_us_per_step": cats,
                    "adapt_full_stats": stats_full, "first_repetition_mean_loss": first_loss}))
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "w") as f:
        f.write("\n".join(lines) + "\n")


def regions_main(a):
    import torch

    from weatherforecast_stgcn_maml_amd import _capi, adapt, params, synth
    from weatherforecast_stgcn_maml_amd.config import SEED, ModelDims
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph

    R = a.regions
    d = ModelDims(num_nodes=441, hidden_channels=256)
    lats, lons = synth.region_grid(n_lat=21, n_lon=21)
    ei, _, _ = build_spatial_graph(lats, lons, 4)
    P = synth.init_params(SEED, d)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    gcn = {k: v for k, v in P.items() if k not in names}
    theta = {k: P[k] for k in names}
    T_total = a.max_samples + d.window_size + d.forecast_horizon
    dev = torch.device("cuda:0")
    n_max = min(a.max_samples, synth.num_samples(T_total, d.window_size, d.forecast_horizon))
    n_train = int(0.8 * n_max)
    regions = [REGION_NAMES[r % len(REGION_NAMES)] for r in range(R)]
    cfgs = [adapt.climate_optimizer_config(n, 0.0006) for n in regions]
    streams = [torch.from_numpy(np.ascontiguousarray(synth.make_features(synth.task_seed(r), d.num_nodes, T_total))).to(dev)
               for r in range(R)]
    stream = _capi.stream_ptr(torch)
    gflat = params.pack(gcn, d, which=1, device=dev)
    th0 = params.pack(theta, d, which=0, device=dev)
    torch.manual_seed(SEED)
    orders = [[adapt.random_sampler_order(n_train).numpy().astype(np.int32) for _ in range(a.epochs + 1)]
              for _ in range(R)]
    cache_bytes = T_total * d.window_size * d.num_nodes * d.hidden_channels * 4

    def context(tasks):
        ctx = _capi.Context(d, 0)
        ctx.set_graph(ei)
        ctx.set_gcn_params(gflat)
        ctx.set_tasks(tasks)
        ctx.set_task_ids([0] * len(tasks))
        return ctx

    def used():
        free, total = torch.cuda.mem_get_info()
        return total - free

    def lockstep(n_epochs, n_steps=n_train, timing=False):
        """A fresh context adapting all R regions in lockstep -> (setup s, bytes, per-epoch s, mean last loss)."""
        ctx = context(streams)
        ctx.set_option("adapt_group", a.adapt_group)
        torch.cuda.synchronize()
        u0, t0 = used(), time.perf_counter()
        ctx.adapt_prepare_multi(stream, list(range(R)), 1)
        torch.cuda.synchronize()
        setup, took = time.perf_counter() - t0, used() - u0
        th = th0.unsqueeze(0).repeat(R, 1).contiguous()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        losses = torch.empty(n_steps, R, device=dev)
        lr_dev = torch.tensor([c[0] for c in cfgs], dtype=torch.float32).to(dev).repeat(n_steps, 1).contiguous()
        per, cats = [], None
        for ep in range(n_epochs + (1 if timing else 0)):
            w = np.stack([orders[r][ep][:n_steps] for r in range(R)], axis=1).reshape(n_steps, R, 1)
            timed = timing and ep == n_epochs
            if timed:
                ctx.timing(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.adapt_steps_multi(stream, list(range(R)), th, m, v, ep * n_steps, w, lr_dev, (0.9, 0.999), 1e-8,
                                  [c[1] for c in cfgs], adapt.MAX_GRAD_NORM, losses)
            torch.cuda.synchronize()
            if timed:
                cats = {k: {"us_per_step": c["ms"] * 1e3 / n_steps, "launches_per_step": c["launches"] / n_steps}
                        for k, c in ctx.timing_collect().items() if c["launches"]}
                ctx.timing(False)
            else:
                per.append(time.perf_counter() - t0)
        loss = losses.double().mean(dim=0).cpu().numpy()
        vc = {k: n for k, n in ctx.variant_counts().items() if n}
        ctx.close()
        return setup, took, per, loss, cats, vc

    def sequential(n_epochs, n_steps=n_train):
        """Each region on a fresh single-region context, one after another -> the same, summed over regions."""
        setup, took, per, loss = 0.0, 0, [0.0] * n_epochs, []
        for r in range(R):
            ctx = context([streams[r]])
            torch.cuda.synchronize()
            u0, t0 = used(), time.perf_counter()
            ctx.adapt_prepare(stream, 1)
            torch.cuda.synchronize()
            setup += time.perf_counter() - t0
            took = max(took, used() - u0)
            th = th0.clone()
            m, v = torch.zeros_like(th), torch.zeros_like(th)
            losses = torch.empty(n_steps, device=dev)
            lr_dev = torch.full((n_steps,), cfgs[r][0], device=dev, dtype=torch.float32)
            for ep in range(n_epochs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.adapt_steps(stream, th, m, v, ep * n_steps, orders[r][ep][:n_steps].reshape(n_steps, 1), lr_dev,
                                (0.9, 0.999), 1e-8, cfgs[r][1], adapt.MAX_GRAD_NORM, losses)
                torch.cuda.synchronize()
                per[ep] += time.perf_counter() - t0
            loss.append(float(losses.double().mean().item()))
            ctx.close()
        return setup, took, per, np.asarray(loss)

    for _ in range(a.warmup):  # module load, first touch: a short epoch of each path
        lockstep(1, min(16, n_train))
        if not a.no_sequential:
            sequential(1, min(16, n_train))

    def report(setup, took, per):
        later = [t / n_train * 1e3 for t in per[1:]]
        return {"setup_ms": setup * 1e3, "setup_bytes": took, "first_epoch_ms": per[0] * 1e3,
                "first_epoch_ms_per_step": per[0] / n_train * 1e3, "later_ms_per_step": spread(later),
                "later_region_sample_steps_per_s": spread([R * 1e3 / t for t in later])}

    setup, took, per, loss, cats, vc = lockstep(a.epochs, timing=a.timing)
    out = {
        "metric": "lockstep regional adaptation, region-sample-steps/s of the later epochs (median)",
        "regions": R, "adapt_group": a.adapt_group, "epochs": a.epochs, "train_samples": n_train,
        "cache_bytes_per_region": cache_bytes, "lockstep": report(setup, took, per),
        "caches_fit": bool(took >= R * cache_bytes), "train_loss_last_epoch": loss.tolist(), "variants": vc,
        "config": "N=441, Hc=256, LSTM 4x128, batch-1 steps, GCN features cached per (region, window)",
    }
    assert np.isfinite(loss).all(), loss
    if out["lockstep"]["later_region_sample_steps_per_s"]:
        out["value"] = out["lockstep"]["later_region_sample_steps_per_s"]["median"]
        out["unit"] = "region-sample-steps/s"
    if cats:
        out["timing_us_per_lockstep_step"] = cats
    if not a.no_sequential:
        setup, took, sper, sloss = sequential(a.epochs)
        out["sequential"] = report(setup, took, sper)
        out["loss_rel_diff_vs_sequential"] = float(np.max(np.abs(loss - sloss) / np.abs(sloss)))
        lo, sq = out["lockstep"]["later_ms_per_step"], out["sequential"]["later_ms_per_step"]
        if lo and sq:
            out["speedup_later"] = {"median": sq["median"] / lo["median"], "worst": sq["min"] / lo["max"],
                                    "best": sq["max"] / lo["min"],
                                    "beats_by_more_than_both_spreads": bool(
                                        sq["median"] - lo["median"] > (sq["max"] - sq["min"]) + (lo["max"] - lo["min"]))}
        out["speedup_first_epoch_with_setup"] = ((out["sequential"]["first_epoch_ms"] + out["sequential"]["setup_ms"]) /
                                                 (out["lockstep"]["first_epoch_ms"] + out["lockstep"]["setup_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
