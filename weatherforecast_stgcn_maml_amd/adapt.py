"""Regional adaptation (BASELINE config 4) over libsmaml.so.

Mirrors ``adapt_hybrid_v5.adaptModel`` (adapt_hybrid_v5.py:65-271): a 1,200-sample cap split
80/20 into train/validation (:152-159), 15 epochs of shuffled batch-1 fine-tuning — forward,
MSE, backward, ``clip_grad_norm_(1.0)``, ``torch.optim.Adam`` with the climate learning rate
and L2 weight decay (:168-203) — the ``ClimateAwareLRScheduler`` stepped once per epoch on
the epoch's mean loss (:208), a no-grad validation MSE (:216-231) and the adapted checkpoint
(:240-257). Each epoch's steps run inside the library (``smaml_adapt_steps``); Python only
draws the shuffle order and steps the scheduler. Data loading from ERA5 (:30-62) is out of
scope: callers pass a feature stream.

``ClimateAwareLRScheduler`` / ``create_climate_optimizer`` are restated from
adaptive_scheduler.py:7-94 (host-side scalars).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from . import _capi, params, synth
from .config import MAX_GRAD_NORM, ModelDims

TROPICAL = ("Indonesia", "Thailand", "QueensAustralia")
COLD = ("Moscow", "NorthSiberia", "Afghanistan")
CLIMATE_MULT = {"tropical": 0.9, "temperate": 1.0, "cold": 1.1}
CLIMATE_WD = {"tropical": 1e-5, "temperate": 1e-4, "cold": 5e-5}


def climate_zone(region_name: str) -> str:
    if region_name in TROPICAL:
        return "tropical"
    if region_name in COLD:
        return "cold"
    return "temperate"


def climate_optimizer_config(region_name: str, base_lr: float = 0.0006):
    """(lr, weight_decay) of create_climate_optimizer (adaptive_scheduler.py:68-94)."""
    z = climate_zone(region_name)
    return base_lr * CLIMATE_MULT[z], CLIMATE_WD[z]


class ClimateAwareLRScheduler:
    """adaptive_scheduler.py:7-66: cosine with 5-epoch cycles times the climate multiplier,
    nudged by the epoch loss after epoch 3."""

    def __init__(self, region_name: str, base_lr: float = 0.0006):
        self.region_name = region_name
        self.base_lr = base_lr
        self.current_epoch = 0
        self.lr_multiplier = CLIMATE_MULT[climate_zone(region_name)]

    def step(self, epoch_loss: Optional[float] = None) -> float:
        self.current_epoch += 1
        cycle_length = 5
        cycle_progress = (self.current_epoch - 1) % cycle_length / cycle_length
        cosine_factor = 0.5 * (1 + np.cos(np.pi * cycle_progress))
        lr = self.base_lr * self.lr_multiplier * cosine_factor
        if epoch_loss is not None and self.current_epoch > 3:
            if epoch_loss > 1.0:
                lr *= 1.1
            elif epoch_loss < 0.2:
                lr *= 0.95
        return lr


def random_sampler_order(n: int) -> torch.Tensor:
    """The order a ``DataLoader(ds, batch_size=1, shuffle=True)`` (adapt_hybrid_v5.py:179; PyG's
    loader is torch's) yields in one epoch, drawing from the global torch RNG as it does: the
    iterator first draws its ``_base_seed`` (one int64), then ``RandomSampler`` draws its own seed
    (one int64) and runs ``randperm`` on a generator seeded with it. This reproduces the
    reference's order for its first epoch, and for every epoch only when the adaptation is
    dropout-free: ``adaptModel`` trains in train mode, where each step's ``nn.Dropout`` also draws
    from the global RNG, so from epoch 2 its shuffle depends on draws this path does not make.
    Parity with train-mode adaptation therefore replays recorded orders (``adapt(orders=...)``)."""
    torch.empty((), dtype=torch.int64).random_()  # _BaseDataLoaderIter._base_seed
    seed = int(torch.empty((), dtype=torch.int64).random_().item())
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


@dataclass
class AdaptResult:
    theta: torch.Tensor
    epoch_losses: List[float] = field(default_factory=list)
    lrs: List[float] = field(default_factory=list)
    val_loss: float = float("nan")
    n_train: int = 0
    n_val: int = 0
    gcn: Optional[torch.Tensor] = None  # train_base: the adapted GCN vector (params.unpack(gcn, dims, 1))


def adapt(dims: ModelDims, features, edge_index, gcn: dict, theta: dict, region_name: str, epochs: int = 15,
          max_samples: int = 1200, train_frac: float = 0.8, base_lr: float = 0.0006, device="cuda",
          val_batch: int = 32, ctx: Optional[_capi.Context] = None, dropout=(0.0, 0.0),
          dropout_seed: int = 0, orders=None, train_base: bool = False, edge_weight=None,
          loss_weights=None) -> AdaptResult:
    """``dropout`` = (STGCN dropout_rate, lstm_dropout) of the train-mode steps (the reference
    adapts in train mode: (0.2, 0.2)); validation runs without dropout (eval mode).
    ``orders``: optional per-epoch sample permutations of the training windows (default: drawn
    from the global torch RNG as the reference's shuffling DataLoader draws them).
    ``train_base``: fine-tune the GCN base too, as the reference's ``freeze_base=False`` and its optimiser
    "for ALL parameters" announce and its ``no_grad`` withholds (F2): each epoch is one
    ``smaml_adapt_steps_full`` call, one Adam state and one joint gradient clip over both vectors, no
    per-window feature cache; ``AdaptResult.gcn`` is the adapted flat GCN vector and the validation runs on
    the adapted base. ``edge_weight`` [E] (optional): the graph's edge weights, as PyG's ``GCNConv`` takes them.
    ``loss_weights`` ``[Hf*N, C]`` (``loss.make_loss_weights``): the training steps and the validation loss are
    ``mean W (pred - y)^2`` (``smaml_set_loss_weights``); the context's table is cleared again before returning."""
    dev = torch.device(device)
    ctx = ctx or _capi.Context(dims, dev.index or 0)
    ei = edge_index.detach().cpu().numpy() if torch.is_tensor(edge_index) else np.asarray(edge_index)
    ew = edge_weight.detach().cpu().numpy() if torch.is_tensor(edge_weight) else edge_weight
    _capi.set_graph_auto(ctx, ei, ew)  # the ELL, or the CSR form for a weighted graph or an in-degree above 7
    gflat = params.pack(gcn, dims, which=1, device=dev)
    ctx.set_gcn_params(gflat)
    th = params.pack(theta, dims, which=0, device=dev)
    stream_t = features if torch.is_tensor(features) else torch.from_numpy(np.ascontiguousarray(features))
    stream_t = stream_t.to(dev, torch.float32).contiguous()
    ctx.set_tasks([stream_t])
    if loss_weights is not None and _capi._loss_table(dims, loss_weights).shape[0] != 1:
        raise ValueError("adapt takes one loss weight table [Hf*N, C]")
    if loss_weights is not None:
        ctx.set_loss_weights(loss_weights)
    try:
        return _adapt_epochs(dims, ctx, stream_t, th, gflat, region_name, epochs, max_samples, train_frac, base_lr, dev,
                             val_batch, dropout, dropout_seed, orders, train_base)
    finally:
        if loss_weights is not None:
            ctx.set_loss_weights(None)


def _adapt_epochs(dims, ctx, stream_t, th, gflat, region_name, epochs, max_samples, train_frac, base_lr, dev, val_batch,
                  dropout, dropout_seed, orders, train_base) -> AdaptResult:
    """``adapt``'s epochs and validation on a prepared context (graph, parameters, task and loss weights set)."""
    n_all = synth.num_samples(stream_t.shape[0], dims.window_size, dims.forecast_horizon)
    n_max = min(max_samples, n_all)
    n_train = int(train_frac * n_max)
    lr0, wd = climate_optimizer_config(region_name, base_lr)
    sched = ClimateAwareLRScheduler(region_name, lr0)
    m = torch.zeros_like(th)
    v = torch.zeros_like(th)
    res = AdaptResult(theta=th, n_train=n_train, n_val=n_max - n_train)
    stream = _capi.stream_ptr(torch)
    lr = lr0
    step = 0
    losses = torch.empty(max(n_train, 1), device=dev)
    ctx.set_task_ids([0])
    ctx.set_dropout(dropout[0], dropout[1], dropout_seed)
    if train_base:
        gm, gv = torch.zeros_like(gflat), torch.zeros_like(gflat)
        res.gcn = gflat
        ctx.reserve(1, 1)  # the workspace before the first epoch (a trained base has no feature cache)
    else:
        ctx.adapt_prepare(stream, 1)  # workspace + feature cache before the first epoch (setup, no compute)
    for _ in range(epochs):
        ctx.set_dropout(dropout[0], dropout[1], dropout_seed)  # masks keyed by the global step index
        ep = len(res.epoch_losses)
        order = np.asarray(orders[ep] if orders is not None else random_sampler_order(n_train).numpy(), np.int32)
        assert order.shape == (n_train,), order.shape
        lr_dev = torch.full((n_train,), lr, device=dev, dtype=torch.float32)
        if train_base:
            ctx.adapt_steps_full(stream, th, m, v, gflat, gm, gv, step, order.reshape(n_train, 1), lr_dev,
                                 (0.9, 0.999), 1e-8, wd, MAX_GRAD_NORM, losses)
        else:
            ctx.adapt_steps(stream, th, m, v, step, order.reshape(n_train, 1), lr_dev, (0.9, 0.999), 1e-8, wd,
                            MAX_GRAD_NORM, losses)
        step += n_train
        avg = float(losses[:n_train].double().mean().item())
        res.epoch_losses.append(avg)
        res.lrs.append(lr)
        lr = sched.step(avg)
    ctx.set_dropout(0.0, 0.0, 0)
    res.val_loss = evaluate(ctx, th, list(range(n_train, n_max)), val_batch)
    return res


def lockstep_groups(n_trains) -> List[List[int]]:
    """Regions that can run in lockstep: equal numbers of training windows (equal step counts per
    epoch). Groups in order of their first region, regions in order inside a group."""
    groups = {}
    for r, n in enumerate(n_trains):
        groups.setdefault(int(n), []).append(r)
    return list(groups.values())


def check_orders(orders, n_trains, epochs: int) -> List[np.ndarray]:
    """``orders[r][epoch]``: region r's permutation of its training windows for that epoch, as int32
    arrays ``[epochs, n_train_r]`` per region. Raises ValueError naming the region on any other shape."""
    if len(orders) != len(n_trains):
        raise ValueError(f"orders has {len(orders)} entries for {len(n_trains)} regions")
    out = []
    for r, (o, n) in enumerate(zip(orders, n_trains)):
        try:
            a = np.asarray(o, np.int32)[:epochs]  # (later epochs' orders may be given and go unused)
        except ValueError:  # ragged: epochs of different lengths
            a = np.zeros((0,), np.int32)
        if a.shape != (epochs, n):
            raise ValueError(f"orders[{r}] has shape {a.shape}, expected ({epochs}, {n}): one permutation of the "
                             f"region's {n} training windows per epoch")
        out.append(a)
    return out


def adapt_many(dims: ModelDims, streams, edge_index, gcn: dict, theta: dict, region_names, epochs: int = 15,
               max_samples: int = 1200, train_frac: float = 0.8, base_lr: float = 0.0006, device="cuda",
               val_batch: int = 32, ctx: Optional[_capi.Context] = None, dropout=(0.0, 0.0),
               dropout_seed: int = 0, orders=None, edge_weight=None, loss_weights=None) -> List[AdaptResult]:
    """``adapt`` for several regions at once (main.py adapts its regions one after another): every region
    starts from the same meta-trained ``theta`` and keeps its own stream, climate optimiser settings,
    ``ClimateAwareLRScheduler`` (stepped on its own epoch mean), shuffle orders and Adam state, and each
    step of all regions of a group runs as one set of launches (``smaml_adapt_steps_multi``). Regions
    are grouped by their number of training windows (lockstep needs equal step counts); the groups run
    one after another. Region r computes what ``adapt`` computes on its stream alone.
    ``orders[r][epoch]``: optional shuffle orders; default: drawn from the global torch RNG region by
    region, each region's epochs in turn -- the draws of one ``adapt`` call per region in that order.
    ``loss_weights``: one table ``[Hf*N, C]`` for every region or one per region ``[R, Hf*N, C]``, as in ``adapt``
    (the validation loss is then the weighted mean too, formed from ``smaml_forecast``'s predictions)."""
    dev = torch.device(device)
    R = len(streams)
    if len(region_names) != R or R == 0:
        raise ValueError(f"{len(region_names)} region names for {R} streams")
    ctx = ctx or _capi.Context(dims, dev.index or 0)
    ei = edge_index.detach().cpu().numpy() if torch.is_tensor(edge_index) else np.asarray(edge_index)
    ew = edge_weight.detach().cpu().numpy() if torch.is_tensor(edge_weight) else edge_weight
    _capi.set_graph_auto(ctx, ei, ew)  # the ELL, or the CSR form for a weighted graph or an in-degree above 7
    gflat = params.pack(gcn, dims, which=1, device=dev)
    ctx.set_gcn_params(gflat)
    th0 = params.pack(theta, dims, which=0, device=dev)
    stream_ts = []
    for f in streams:
        t = f if torch.is_tensor(f) else torch.from_numpy(np.ascontiguousarray(f))
        stream_ts.append(t.to(dev, torch.float32).contiguous())
    ctx.set_tasks(stream_ts)
    ctx.set_task_ids([0] * R)  # every region draws the dropout masks of a single-region adapt()
    lw = None
    if loss_weights is not None:
        lw = _capi._loss_table(dims, loss_weights)
        if lw.shape[0] not in (1, R):
            raise ValueError(f"{lw.shape[0]} loss weight tables for {R} regions (one table, or one per region)")
        ctx.set_loss_weights(lw)
    try:
        return _adapt_many_groups(dims, ctx, stream_ts, th0, region_names, epochs, max_samples, train_frac, base_lr,
                                  dev, val_batch, dropout, dropout_seed, orders, lw)
    finally:
        if lw is not None:
            ctx.set_loss_weights(None)


def _adapt_many_groups(dims, ctx, stream_ts, th0, region_names, epochs, max_samples, train_frac, base_lr, dev,
                       val_batch, dropout, dropout_seed, orders, lw) -> List[AdaptResult]:
    """``adapt_many``'s lockstep groups on a prepared context (graph, parameters, tasks and loss weights set)."""
    R = len(stream_ts)
    n_maxs = [min(max_samples, synth.num_samples(t.shape[0], dims.window_size, dims.forecast_horizon))
              for t in stream_ts]
    n_trains = [int(train_frac * n) for n in n_maxs]
    if orders is not None:
        orders = check_orders(orders, n_trains, epochs)
    else:
        orders = [np.stack([random_sampler_order(n).numpy().astype(np.int32) for _ in range(epochs)])
                  if epochs > 0 else np.zeros((0, n), np.int32) for n in n_trains]
    stream = _capi.stream_ptr(torch)
    results: List[Optional[AdaptResult]] = [None] * R
    for group in lockstep_groups(n_trains):
        G, n_train = len(group), n_trains[group[0]]
        th = th0.unsqueeze(0).repeat(G, 1).contiguous()
        m, v = torch.zeros_like(th), torch.zeros_like(th)
        cfgs = [climate_optimizer_config(region_names[r], base_lr) for r in group]
        scheds = [ClimateAwareLRScheduler(region_names[r], lr0) for r, (lr0, _) in zip(group, cfgs)]
        lrs = [lr0 for lr0, _ in cfgs]
        wds = [wd for _, wd in cfgs]
        res = [AdaptResult(theta=th[i], n_train=n_train, n_val=n_maxs[r] - n_train) for i, r in enumerate(group)]
        losses = torch.empty(max(n_train, 1), G, device=dev)
        ctx.set_dropout(dropout[0], dropout[1], dropout_seed)
        ctx.adapt_prepare_multi(stream, group, 1)
        step = 0
        for ep in range(epochs):
            ctx.set_dropout(dropout[0], dropout[1], dropout_seed)  # masks keyed by the global step index
            windows = np.stack([orders[r][ep] for r in group], axis=1).reshape(n_train, G, 1)
            lr_dev = torch.tensor(lrs, dtype=torch.float32).to(dev).repeat(n_train, 1).contiguous()
            ctx.adapt_steps_multi(stream, group, th, m, v, step, windows, lr_dev, (0.9, 0.999), 1e-8, wds,
                                  MAX_GRAD_NORM, losses)
            step += n_train
            avgs = losses[:n_train].double().mean(dim=0).cpu().numpy()
            for i in range(G):
                res[i].epoch_losses.append(float(avgs[i]))
                res[i].lrs.append(lrs[i])
                lrs[i] = scheds[i].step(float(avgs[i]))
        ctx.set_dropout(0.0, 0.0, 0)
        for i, r in enumerate(group):
            res[i].val_loss = evaluate_region(ctx, th[i], r, list(range(n_train, n_maxs[r])), val_batch,
                                              loss_weights=None if lw is None else lw[r if lw.shape[0] > 1 else 0],
                                              features=stream_ts[r])
            results[r] = res[i]
    return results


def evaluate_region(ctx: _capi.Context, theta: torch.Tensor, task: int, sample_ids, batch: int = 32,
                    loss_weights=None, features=None) -> float:
    """Mean per-sample MSE over the given windows of task ``task`` (no gradients, no dropout): the
    squared-error sum of ``smaml_forecast`` over the element count. With ``loss_weights [Hf*N, C]`` the weighted
    mean ``mean W (pred - y)^2``, formed in torch from ``smaml_forecast``'s predictions and the targets in
    ``features`` (the task's stream on the device)."""
    if len(sample_ids) == 0:
        return 0.0
    d = ctx.dims
    if loss_weights is not None:
        from .loss import weighted_mse_reference

        T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
        ids = np.asarray(sample_ids, np.int32)
        W = torch.as_tensor(np.asarray(loss_weights, np.float32), device=theta.device)
        total = 0.0
        for i in range(0, len(ids), batch):
            chunk = ids[i:i + batch]
            pred = torch.empty(len(chunk), N * Hf, C, device=theta.device)
            ctx.forecast(_capi.stream_ptr(torch), theta, chunk, batch, task=task, pred=pred)
            y = torch.stack([features[int(w) + T + 1:int(w) + T + 1 + Hf, :, :C].reshape(Hf * N, C) for w in chunk])
            total += float(weighted_mse_reference(pred.double(), y.double(), W.double()).item()) * len(chunk)
        return total / len(ids)
    sums = torch.empty(3, d.forecast_horizon, d.output_channels, device=theta.device, dtype=torch.float64)
    ctx.forecast(_capi.stream_ptr(torch), theta, np.asarray(sample_ids, np.int32), batch, task=task, skill=sums)
    return float(sums[0].sum().item()) / (len(sample_ids) * d.num_nodes * d.forecast_horizon * d.output_channels)


def evaluate(ctx: _capi.Context, theta: torch.Tensor, sample_ids, batch: int = 32) -> float:
    """Mean per-sample MSE over the given windows of task 0 (no gradients, no dropout)."""
    ctx.set_dropout(0.0, 0.0, 0)
    total, n = 0.0, 0
    stream = _capi.stream_ptr(torch)
    for i in range(0, len(sample_ids), batch):
        chunk = sample_ids[i:i + batch]
        w = np.asarray(chunk, np.int32).reshape(1, 1, len(chunk))
        loss = torch.empty(1, 1, device=theta.device)
        ctx.meta_step(stream, theta, 0, 0, len(chunk), w, 0.0, 1.0, 1.0, losses=loss)
        total += float(loss.item()) * len(chunk)
        n += len(chunk)
    return total / max(n, 1)
