"""What the gradient through the GCN base costs (smaml_backward_base), timed on one MI355X at config-2 shapes
(N = 441, T = 24, Hc = 256, LSTM 4 x 128) with 1 and 32 samples.

1. End to end, arms alternating in one process, each repetition `--inner` forward + backward pairs timed on the
   host with a device synchronise inside (default: max(40, 200 / samples) pairs, a few tenths of a second):
     backward        smaml_forward + smaml_backward        (LSTM / head gradients only)
     backward_base   smaml_forward + smaml_backward_base   (+ gcn_grad and every dx)
2. The layer-0 input gradient alone, from the library's event timing (category misc, which in
   smaml_backward_base holds nothing else), the two forms alternating:
     fused      k_lstm_dx0 (option dx0_fused = 1)
     composed   launch_gemm_nn_plain + relu_mask + T strided copies per sample (dx0_fused = 0)
   and whether the two forms' results are bitwise equal.

Medians of `--reps` repetitions after `--warmup`, with min and max (the run-to-run spread). ONE JSON line last.

Usage: python tools/bench_base_grad.py [--reps 5] [--warmup 2] [--inner 0] [--samples 1,32]
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5, help="timed repetitions per arm (>= 5 for the spread)")
    p.add_argument("--warmup", type=int, default=2, help="untimed repetitions per arm first")
    p.add_argument("--inner", type=int, default=0, help="forward + backward pairs per timed repetition (0: see above)")
    p.add_argument("--samples", default="1,32")
    a = p.parse_args()
    import torch

    from weatherforecast_stgcn_maml_amd import _capi, params, synth
    from weatherforecast_stgcn_maml_amd.config import SEED, ModelDims
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph

    if not torch.cuda.is_available():
        raise SystemExit("bench_base_grad needs a HIP device (no CPU fallback)")
    d = ModelDims(num_nodes=441, hidden_channels=256)
    lats, lons = synth.region_grid(n_lat=21, n_lon=21)
    ei, _, _ = build_spatial_graph(lats, lons, 4)
    P = synth.init_params(SEED, d, gcn_bias_scale=0.1)
    names = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    dev = torch.device("cuda:0")
    gflat = params.pack({k: v for k, v in P.items() if k.startswith("base_stgcn.conv")}, d, which=1, device=dev)
    theta = params.pack({k: P[k] for k in names}, d, which=0, device=dev)
    st = _capi.stream_ptr(torch)
    print(f"build: {_capi.build_info()}")
    result = {"dims": d.as_dict(), "reps": a.reps, "samples": {}}
    for B in [int(s) for s in a.samples.split(",")]:
        inner = a.inner or max(40, 200 // B)
        ctx = _capi.Context(d, 0)
        ctx.set_graph(ei)
        ctx.set_gcn_params(gflat)
        feats = synth.make_features(synth.task_seed(0), d.num_nodes, synth.t_total_for(B))
        xs = [torch.from_numpy(np.ascontiguousarray(synth.sample_xy(feats, i)[0])).to(dev) for i in range(B)]
        g = torch.Generator().manual_seed(B)
        dpred = torch.randn(B, d.num_nodes * d.forecast_horizon, d.output_channels, generator=g).to(dev)
        pred = torch.empty_like(dpred)
        grad = torch.empty_like(theta)
        gg = torch.empty_like(gflat)
        dxs = [torch.empty_like(x) for x in xs]

        def plain():
            ctx.forward(st, theta, xs, pred)
            ctx.backward(st, theta, dpred, grad)

        def base():
            ctx.forward(st, theta, xs, pred)
            ctx.backward_base(st, theta, xs, dpred, grad, gg, dxs)

        arms = {"backward": plain, "backward_base": base}
        times = {k: [] for k in arms}
        for _ in range(a.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for k, fn in arms.items():  # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3 / inner)
        e2e = {k: stats(v) for k, v in times.items()}
        # the layer-0 input gradient alone: event time of category misc inside smaml_backward_base
        ctx.timing(True)
        ktimes = {"fused": [], "composed": []}
        outs = {}
        for rep in range(a.warmup + a.reps):
            for form, opt in (("fused", 1), ("composed", 0)):  # alternating
                ctx.set_option("dx0_fused", opt)
                ctx.forward(st, theta, xs, pred)
                ctx.timing_collect()  # (synchronises and resets: the forward's launches are not counted)
                ctx.backward_base(st, theta, xs, dpred, grad, gg, dxs)
                ms = ctx.timing_collect()["misc"]["ms"]
                if rep >= a.warmup:
                    ktimes[form].append(ms)
                outs[form] = (gg.clone(), [x.clone() for x in dxs])
        ctx.timing(False)
        ctx.set_option("dx0_fused", 1)
        same = bool(torch.equal(outs["fused"][0], outs["composed"][0])
                    and all(torch.equal(u, v) for u, v in zip(outs["fused"][1], outs["composed"][1])))
        kern = {k: stats(v) for k, v in ktimes.items()}
        rows = B * d.window_size * d.num_nodes
        flops = 2.0 * rows * 4 * d.lstm_hidden_size * d.hidden_channels
        print(f"--- {B} sample(s): {rows} rows, {inner} pairs per repetition")
        for k, s in e2e.items():
            print(f"  {k:14s} {s['median']:9.3f} ms per forward + backward  (min {s['min']:.3f}, max {s['max']:.3f})")
        extra = e2e["backward_base"]["median"] - e2e["backward"]["median"]
        print(f"  base gradient on top: {extra:.3f} ms (+{100 * extra / e2e['backward']['median']:.1f} %)")
        for k, s in kern.items():
            print(f"  dx0 {k:9s} {s['median']:9.4f} ms  (min {s['min']:.4f}, max {s['max']:.4f})"
                  f"  {flops / (s['median'] * 1e-3) / 1e12:.2f} TFLOP/s algorithmic")
        print(f"  fused and composed results bitwise equal: {same}")
        result["samples"][str(B)] = {"rows": rows, "inner": inner, "end_to_end_ms": e2e, "dx0_ms": kern, "bitwise_equal": same}
        ctx.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
