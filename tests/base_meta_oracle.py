"""The CPU oracle of the base meta-gradient (test infrastructure; imported by test_base_meta_cpu.py and
test_gpu_base_meta.py).

``oracle/refcpu.py`` computes its GCN features under ``no_grad`` (F2) and is not edited. Here
``refcpu.stgcn_features`` is called with the base tensors as autograd leaves, outside ``no_grad``, and
``refcpu.batched_forward``, ``refcpu.mse`` and ``refcpu.clip_coef`` run on top of it, in float64 by default.
The inner loop is ``refcpu.inner_loop``'s: clip + SGD on ``theta`` alone, the base shared and not adapted.

order 2: the inner steps run with ``create_graph=True`` and the gradients are taken with respect to ``theta0``
and the base leaves -- the total derivative, mixed terms and the clip's derivative included.
order 1: the inner steps run detached; the gradients are taken with respect to the adapted parameters and the base
leaves at the query batch alone -- the partial derivative with ``fast_K`` held constant.

The per-step ``Dropout(seed, 0, p_lstm, task id, k)`` goes to ``batched_forward`` only (GCN dropout with base
gradients is not supported by the library).
"""
import numpy as np
import torch

from oracle import refcpu


def base_names(P):
    return [k for k in P if k.startswith("base_stgcn.conv")]


def _loss(P, task, feats, idx, drop, table):
    preds = refcpu.batched_forward(P, feats, task.dims, drop)
    ls = []
    for p, i in zip(preds, idx):
        y = task.xy(i)[1].to(p.dtype)
        ls.append(refcpu.mse(p, y) if table is None else (table.to(p.dtype) * (p - y) ** 2).mean())
    return torch.stack(ls).mean()


def meta_step(Pt0, Pg, tasks, windows, lr, max_norm, order, query_scale=0.5, dtype=torch.float64, dropout=None,
              task_ids=None, tables=None):
    """One meta-step over ``windows [K + 1][tasks][B]`` with the base differentiated. ``dropout`` = (seed, p_lstm);
    ``tables``: None, or loss-weight tables ``[Hf*N, C]`` (one for all tasks, or one per task).
    Returns dict(meta_grad, gcn_grad (per name, summed over tasks), query_losses, step_records, adapted)."""
    assert order in (1, 2)
    windows = np.asarray(windows)
    K = windows.shape[0] - 1
    names, gnames = list(Pt0.keys()), base_names(Pg)
    base = {k: Pg[k].detach().to(dtype).clone().requires_grad_(True) for k in gnames}
    meta_grad = {k: torch.zeros_like(Pt0[k], dtype=dtype) for k in names}
    gcn_grad = {k: torch.zeros_like(base[k]) for k in gnames}
    qlosses, records, adapted_all = [], [], []
    for j, task in enumerate(tasks):
        tid = task_ids[j] if task_ids is not None else j
        table = None if tables is None else torch.as_tensor(np.asarray(tables[j if len(tables) > 1 else 0]))
        cache = {}

        def feats_of(i, attached):
            if i not in cache:
                x = task.xy(i)[0].to(dtype)
                cache[i] = refcpu.stgcn_features(x, task.edge_index, base)
            return cache[i] if attached else cache[i].detach()

        theta0 = [Pt0[k].detach().to(dtype).clone().requires_grad_(True) for k in names]
        params, rec = theta0, []
        for k in range(K):
            idx = [int(i) for i in windows[k, j]]
            drop = refcpu.Dropout(dropout[0], 0.0, dropout[1], tid, k) if dropout else None
            P = dict(zip(names, params))
            loss = _loss(P, task, [feats_of(i, order == 2) for i in idx], idx, drop, table)
            grads = torch.autograd.grad(loss, params, create_graph=order == 2)
            coef, total = refcpu.clip_coef(grads, max_norm)
            rec.append((float(loss.detach()), float(total.detach()), float(coef.detach())))
            params = [p - lr * coef * g for p, g in zip(params, grads)]
            if order == 1:
                params = [p.detach().requires_grad_(True) for p in params]
        qidx = [int(i) for i in windows[K, j]]
        qdrop = refcpu.Dropout(dropout[0], 0.0, dropout[1], tid, K) if dropout else None
        qloss = _loss(dict(zip(names, params)), task, [feats_of(i, True) for i in qidx], qidx, qdrop, table)
        wrt = (theta0 if order == 2 else params) + [base[k] for k in gnames]
        g = torch.autograd.grad(qloss * query_scale, wrt)
        for k, gi in zip(names, g[:len(names)]):
            meta_grad[k] += gi.detach()
        for k, gi in zip(gnames, g[len(names):]):
            gcn_grad[k] += gi.detach()
        qlosses.append(float(qloss.detach()))
        records.append(rec)
        adapted_all.append({k: v.detach() for k, v in zip(names, params)})
    return dict(meta_grad=meta_grad, gcn_grad=gcn_grad, query_losses=qlosses, step_records=records,
                adapted=adapted_all)


def query_objective(Pt0, Pg, tasks, windows, lr, max_norm, query_scale=0.5, dtype=torch.float64):
    """sum over tasks of query_scale * L_q(fast_K(theta0, g), g) as a float, no autograd (finite differences)."""
    windows = np.asarray(windows)
    K = windows.shape[0] - 1
    names = list(Pt0.keys())
    base = {k: v.detach().to(dtype) for k, v in Pg.items()}
    total = 0.0
    for j, task in enumerate(tasks):
        params = [Pt0[k].detach().to(dtype).clone().requires_grad_(True) for k in names]
        feats = lambda i: refcpu.stgcn_features(task.xy(i)[0].to(dtype), task.edge_index, base)  # noqa: E731
        for k in range(K):
            idx = [int(i) for i in windows[k, j]]
            loss = _loss(dict(zip(names, params)), task, [feats(i) for i in idx], idx, None, None)
            grads = torch.autograd.grad(loss, params)
            coef, _ = refcpu.clip_coef(grads, max_norm)
            params = [(p - lr * coef * g).detach().requires_grad_(True) for p, g in zip(params, grads)]
        qidx = [int(i) for i in windows[K, j]]
        with torch.no_grad():
            total += float(_loss(dict(zip(names, params)), task, [feats(i) for i in qidx], qidx, None, None)) * query_scale
    return total


def train_loop(Pt0, Pg, tasks, windows, cfg, nsteps, dtype=torch.float64):
    """``nsteps`` outer steps of MetaLearner(train_base=True) in float64: the meta-step above at cfg.order, the
    gradients of theta and of the base clipped jointly (cfg.outer_max_norm), ``torch.optim.AdamW`` over both sets.
    Returns (theta, base, per-step query losses [nsteps][tasks])."""
    names, gnames = list(Pt0.keys()), base_names(Pg)
    theta = {k: Pt0[k].detach().to(dtype).clone().requires_grad_(True) for k in names}
    base = {k: Pg[k].detach().to(dtype).clone().requires_grad_(True) for k in gnames}
    leaves = [theta[k] for k in names] + [base[k] for k in gnames]
    opt = torch.optim.AdamW(leaves, lr=cfg.outer_lr, betas=tuple(cfg.outer_betas), eps=cfg.outer_eps,
                            weight_decay=cfg.outer_weight_decay)
    qlosses = []
    for _ in range(nsteps):
        r = meta_step({k: v.detach() for k, v in theta.items()}, {k: v.detach() for k, v in base.items()}, tasks,
                      windows, cfg.inner_lr, cfg.max_norm, cfg.order, cfg.query_loss_scale, dtype)
        for k in names:
            theta[k].grad = r["meta_grad"][k].clone()
        for k in gnames:
            base[k].grad = r["gcn_grad"][k].clone()
        torch.nn.utils.clip_grad_norm_(leaves, cfg.outer_max_norm)
        opt.step()
        qlosses.append(r["query_losses"])
    return ({k: v.detach() for k, v in theta.items()}, {k: v.detach() for k, v in base.items()}, qlosses)
