"""The CPU oracle of the weighted loss (test infrastructure; imported by test_weighted_loss_cpu.py and
test_gpu_weighted_loss.py).

``oracle/refcpu.py`` hard-codes ``mse`` and is not edited: ``weighted_mse`` swaps ``refcpu.mse`` for a closure
over ONE table for the duration of a ``with`` block (every caller in refcpu and in the existing adapt oracles
looks the name up at call time). Per-task tables therefore run ``refcpu.meta_step`` once per task
(``tasks=[task_j]``, ``task_ids=[j]``) and sum the meta-gradients, which is what ``refcpu.meta_step`` itself does
over its task loop.

The table multiplies ``(pred - y)**2`` elementwise: both are ``[Hf*N, C]`` rows as the loss sees them (F4), and
the table is in the layout of ``y``. With all ones the closure computes bitwise what ``refcpu.mse`` computes.
"""
import contextlib

import numpy as np
import torch

from oracle import refcpu


def draw_tables(dims, seed):
    """(separable, random) float32 ``[Hf*N, C]``, each scaled to mean 1. Entries from [0.25, 4] with about 10 %
    zeros: the separable one is lead x node x variable with the cube roots of such draws as factors and about
    10 % of its NODES zero (every lead and variable of a masked node); the random one draws every entry on its
    own, so a transposed or mis-strided index cannot reproduce it."""
    Hf, N, C = dims.forecast_horizon, dims.num_nodes, dims.output_channels
    rng = np.random.default_rng(seed)
    f = lambda n: rng.uniform(0.25, 4.0, n) ** (1.0 / 3.0)  # noqa: E731
    node = f(N)
    node[rng.choice(N, max(1, round(0.1 * N)), replace=False)] = 0.0
    sep = f(Hf)[:, None, None] * node[None, :, None] * f(C)[None, None, :]
    rnd = rng.uniform(0.25, 4.0, (Hf, N, C))
    rnd[rng.random((Hf, N, C)) < 0.1] = 0.0
    out = []
    for w in (sep, rnd):
        w = (w / w.mean()).reshape(Hf * N, C).astype(np.float32)
        assert 0.05 < float((w == 0).mean()) < 0.2 and abs(float(w.astype(np.float64).mean()) - 1.0) < 1e-6
        out.append(w)
    return tuple(out)


@contextlib.contextmanager
def weighted_mse(W):
    """``refcpu.mse`` := ``mean(W * (pred - y)**2)`` inside the block (None: unchanged)."""
    if W is None:
        yield
        return
    Wt = torch.as_tensor(np.asarray(W))
    orig = refcpu.mse

    def wmse(pred, y):
        return (Wt.to(pred.dtype) * (pred - y) ** 2).mean()

    refcpu.mse = wmse
    try:
        yield
    finally:
        refcpu.mse = orig


def meta_step(Pt, Pg, tasks, tables, windows, steps, batch, lr, max_norm, order, query_scale=0.5, dropout=None,
              task_ids=None):
    """``refcpu.meta_step`` over ``windows [steps + 1][tasks][B]`` with task j's loss weighted by ``tables[j]``
    (one table: ``tables`` of length 1 serves every task; None: unweighted). Same result dict."""
    windows = np.asarray(windows)
    Z = len(tasks)
    ids = list(range(Z)) if task_ids is None else list(task_ids)
    names = list(Pt.keys())
    out = dict(meta_loss=0.0, query_losses=[], meta_grad={k: torch.zeros_like(Pt[k]) for k in names},
               step_records=[], adapted=[])
    for j in range(Z):
        W = None if tables is None else tables[j if len(tables) > 1 else 0]
        with weighted_mse(W):
            r = refcpu.meta_step(Pt, Pg, [tasks[j]], None, steps, batch, None, lr, max_norm, order, query_scale,
                                 dropout=dropout, task_ids=[ids[j]], windows=windows[:, j:j + 1])
        out["meta_loss"] += r["meta_loss"]
        out["query_losses"] += r["query_losses"]
        out["step_records"] += r["step_records"]
        out["adapted"] += r["adapted"]
        for k in names:
            out["meta_grad"][k] += r["meta_grad"][k]
    return out


def to_dtype(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def adam_steps(d, P, feats, ei, windows, lrs, W, wd, max_norm=1.0, train_base=False, dtype=torch.float32):
    """The adaptation steps of the existing adapt oracles (test_gpu_adapt_full.oracle_steps; refcpu.adapt_reference's
    loop) with the weighted loss: step k runs the batch ``windows[k]`` -- forward, ``mean W (pred - y)^2`` averaged over
    the batch, backward, ``clip_grad_norm_(max_norm)``, ``torch.optim.Adam(lr=lrs[k], weight_decay=wd)`` from zero
    moments -- on the trainable vector alone, or with ``train_base`` on the GCN convolutions too (features outside
    ``no_grad``, one joint clip). Returns ({name: array}, step losses)."""
    tr = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    gc = [k for k in P if k.startswith("base_stgcn.conv")]
    Pt = {k: v.clone().to(dtype) for k, v in refcpu.to_torch(P).items()}
    names = tr + gc if train_base else tr
    for k in names:
        Pt[k].requires_grad_(True)
    leaves = [Pt[k] for k in names]
    task = refcpu.TaskData(np.asarray(feats, np.float64 if dtype == torch.float64 else np.float32), ei, d)
    opt = torch.optim.Adam(leaves, lr=float(lrs[0]), weight_decay=wd)
    losses = []
    with weighted_mse(W):
        for k in range(len(windows)):
            for pg in opt.param_groups:
                pg["lr"] = float(lrs[k])
            opt.zero_grad()
            with torch.enable_grad() if train_base else torch.no_grad():
                fs = [refcpu.stgcn_features(task.xy(int(i))[0], task.edge_index, Pt) for i in windows[k]]
            preds = refcpu.batched_forward(Pt, fs, d)
            loss = torch.stack([refcpu.mse(q, task.xy(int(i))[1]) for q, i in zip(preds, windows[k])]).mean()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(leaves, max_norm)
            opt.step()
            losses.append(float(loss.detach()))
    return {k: v.detach().numpy() for k, v in Pt.items()}, np.array(losses)


def weighted_val_loss(d, P, feats, ei, sample_ids, W):
    """Mean over ``sample_ids`` of the per-sample weighted loss (no gradients): what ``adapt``'s validation computes."""
    Pt = refcpu.to_torch(P)
    task = refcpu.TaskData(np.asarray(feats, np.float32), ei, d)
    with weighted_mse(W), torch.no_grad():
        vals = [float(refcpu.batch_loss({k: v for k, v in Pt.items() if not k.startswith("base_stgcn")},
                                        {k: v for k, v in Pt.items() if k.startswith("base_stgcn")}, task, [i])[0])
                for i in sample_ids]
    return sum(vals) / max(len(vals), 1)
