"""Rolling forecast of an adapted model over a region's feature stream, with per-lead-time,
per-variable skill in physical units (``smaml_forecast``).

What the reference stops short of: ``validate_hybrid_v5.validateAdapted`` (validate_hybrid_v5.py:189-237)
scores ``min(3, n)`` windows and ``adaptModel``'s validation loop (adapt_hybrid_v5.py:216-231) gives one
scalar MSE. ``forecast`` runs every window of the stream -- including, without scoring, the windows whose
targets lie past its end -- through the inference-only forward of the library and returns the predictions
and RMSE / MAE per target lead and variable, beside the persistence baseline (the last observed value
held for every lead) and the skill ``1 - SSE / SSE_persistence``.

The pairing of predictions and targets is the one the model was trained with and the reference's
evaluation uses (validate_hybrid_v5.py:224-237): the flat prediction rows ``[N*Hf]`` are
viewed as ``[Hf, N]``, so flat row ``r`` meets target ``(h' = r // N, n' = r % N)``. Kept, not fixed.

``skill_reference`` states the sums in numpy (float64) from given predictions; the GPU tests hold the
library to it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

SUMS = ("sse", "sae", "persistence_sse")  # order of smaml_forecast's skill sums


def default_windows(t_total: int, window: int, horizon: int, score: bool) -> np.ndarray:
    """Window starts of a ``t_total``-step stream: with ``score`` every window whose targets
    ``stream[w+T+1 .. w+T+Hf]`` exist (``len(WeatherGraphDataset)``, dataset.py:25), else every window
    whose inputs exist (``w + T <= t_total``; the last ``Hf + 1`` forecast past the end of the stream)."""
    n = max(0, t_total - window - horizon) if score else max(0, t_total - window + 1)
    return np.arange(n, dtype=np.int32)


def node_weight_vector(node_weights, N: int):
    """``node_weights`` as a float64 ``[N]`` vector (finite, >= 0, at least one positive), or None."""
    if node_weights is None:
        return None
    if hasattr(node_weights, "detach"):
        node_weights = node_weights.detach().cpu()
    v = np.asarray(node_weights, np.float64).reshape(-1)
    if v.size != N:
        raise ValueError(f"node_weights has {v.size} entries, expected {N}")
    if not np.all(np.isfinite(v)) or np.any(v < 0) or not np.any(v > 0):
        raise ValueError("node_weights must be finite and >= 0 with at least one positive entry")
    return v


def _node_sum(a, v):
    """Sum of ``a [K, N, C]`` over its node axis, each node times ``v[n]`` (None: unweighted); a node of weight
    0 contributes exactly 0 whatever ``a`` holds there (NaN targets of masked nodes)."""
    if v is None:
        return a.sum(axis=1)
    vb = v[None, :, None]
    with np.errstate(invalid="ignore"):
        return np.where(vb > 0, a * vb, 0.0).sum(axis=1)


def score_count(n: int, N: int, node_weights=None) -> float:
    """What the score sums of ``n`` windows (origins) divide by: ``n * N``, or ``n * sum(v)`` with node weights."""
    v = node_weight_vector(node_weights, N)
    return int(n) * N if v is None else int(n) * float(v.sum())


def skill_reference(pred_norm, features, windows: Sequence[int], dims, scale=None, node_weights=None) -> np.ndarray:
    """The three skill sums ``[3, Hf, C]`` (float64; order ``SUMS``) of normalised predictions
    ``pred_norm [nwin, N*Hf, C]`` for the windows ``windows`` of ``features [t_total, N, >= C]``:
    ``sum (s_c (p - y))^2``, ``sum |s_c (p - y)|`` and ``sum (s_c (y_last - y))^2`` over windows and
    nodes, with ``y = features[w+T+1+h', n', c]``, ``y_last = features[w+T-1, n', c]`` and the F4 pairing
    (module docstring). ``node_weights [N]``: every summand times the weight of its target node ``n'``
    (``smaml_set_score_weights``; latitude weighting, masks). Pure numpy; needs no GPU."""
    T, Hf, N, C = dims.window_size, dims.forecast_horizon, dims.num_nodes, dims.output_channels
    v = node_weight_vector(node_weights, N)
    p_all = np.asarray(pred_norm, np.float64).reshape(len(windows), Hf, N, C)  # flat rows seen as [Hf, N]
    f = np.asarray(features)
    s = np.ones(C) if scale is None else np.asarray(scale, np.float64).reshape(C)
    out = np.zeros((3, Hf, C))
    for p, w in zip(p_all, windows):
        w = int(w)
        if w < 0 or w + T + Hf >= f.shape[0]:
            raise ValueError(f"window {w} has no targets in a stream of {f.shape[0]} steps")
        y = f[w + T + 1:w + T + 1 + Hf, :, :C].astype(np.float64)
        y_last = f[w + T - 1, :, :C].astype(np.float64)[None]
        e = (p - y) * s
        q = (y_last - y) * s
        out[0] += _node_sum(e * e, v)
        out[1] += _node_sum(np.abs(e), v)
        out[2] += _node_sum(q * q, v)
    return out


@dataclass
class ForecastResult:
    pred: Optional[np.ndarray]              # [nwin, Hf, N, C], physical units over the first len(std) variables
    rmse: Optional[np.ndarray]              # [Hf, C]
    mae: Optional[np.ndarray]               # [Hf, C]
    persistence_rmse: Optional[np.ndarray]  # [Hf, C]
    skill: Optional[np.ndarray]             # [Hf, C]: 1 - SSE / SSE_persistence, NaN where the baseline error is 0
    n_windows: int
    windows: np.ndarray                     # the window starts that were run


def skill_metrics(sums: np.ndarray, count: int):
    """(rmse, mae, persistence_rmse, skill) ``[Hf, C]`` from the sums ``[3, Hf, C]`` over ``count``
    (window, node) pairs per entry."""
    sums = np.asarray(sums, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        skill = np.where(sums[2] > 0, 1.0 - sums[0] / sums[2], np.nan)
    return np.sqrt(sums[0] / count), sums[1] / count, np.sqrt(sums[2] / count), skill


def _stats(stats, C):
    """(mean, std) of the adaptation checkpoint's ``stats`` padded to C variables with (0, 1)."""
    mean, std = np.zeros(C), np.ones(C)
    if stats is not None:
        m = np.asarray(stats["mean"] if isinstance(stats, dict) else stats[0], np.float64).reshape(-1)[:C]
        s = np.asarray(stats["std"] if isinstance(stats, dict) else stats[1], np.float64).reshape(-1)[:C]
        mean[:len(m)] = m
        std[:len(s)] = s
    return mean, std


class _score_weights:
    """Context manager: ``ctx.set_score_weights(v)`` for the call inside, cleared on the way out (a shared
    context is left as found). None: nothing to do."""

    def __init__(self, ctx, node_weights, N):
        self.ctx, self.v = ctx, node_weight_vector(node_weights, N)

    def __enter__(self):
        if self.v is not None:
            self.ctx.set_score_weights(self.v)
        return self

    def __exit__(self, *exc):
        if self.v is not None:
            self.ctx.set_score_weights(None)
        return False


def _setup(who, model, features, edge_index, edge_weight, stats, ctx, entries, default_entries, device_only=True,
           prepare_empty=False):
    """What the four forecast calls share before their library call: the device check, ``features`` as a float32
    device tensor, the window starts or origins (``entries``, or ``default_entries(t_total, T, Hf)``) and -- unless
    there are none: nothing is asked of a context then, but for its graph and parameters with ``prepare_empty``,
    which ``forecast`` has always set -- the context (``ctx``, or the model's own) holding the
    graph, the GCN parameters and the stream as task 0, ``theta``, and the ``stats`` as ``std`` (numpy) and the
    device tensors ``units() = (scale_t, shift_t)`` that take normalised output to physical units."""
    import torch
    from types import SimpleNamespace

    from . import _capi
    from .model import _set_graph

    dev = next(model.parameters()).device
    if device_only and dev.type != "cuda":
        raise _capi.SmamlError(-1, f"{who} runs on a HIP device only")
    f = features if torch.is_tensor(features) else torch.from_numpy(np.ascontiguousarray(features))
    f = f.to(dev, torch.float32).contiguous()
    T = model.base_stgcn.window_size
    Hf, C = model.forecast_horizon, model.out_channels
    t_total, N = int(f.shape[0]), int(f.shape[1])
    ei = edge_index if torch.is_tensor(edge_index) else torch.from_numpy(np.asarray(edge_index))
    ew = edge_weight  # (optional: a weighted graph, or an in-degree above 7, runs in the library's CSR form)
    if ew is not None and not torch.is_tensor(ew):
        ew = torch.from_numpy(np.asarray(ew, dtype=np.float32))
    e = default_entries(t_total, T, Hf) if entries is None else np.asarray(entries, np.int32).reshape(-1)
    c = SimpleNamespace(dev=dev, N=N, Hf=Hf, C=C, entries=e)
    if e.size == 0 and not prepare_empty:
        return c
    if ctx is None:
        ctx, dims, theta = model._prepare(f[:T].reshape(T * N, -1), ei, ew)
    else:
        dims = model.dims(N)
        _set_graph(ctx, ei, ew)
        gflat, _ = model._packed(1, model._gcn_params(), dims, dev)
        ctx.set_gcn_params(gflat)
        theta, _ = model._packed(0, model._trainable_params(), dims, dev)
    if e.size == 0:
        return c
    ctx.set_tasks([f])
    mean, c.std = _stats(stats, C)
    c.ctx, c.theta = ctx, theta
    c.units = lambda: (torch.from_numpy(c.std.astype(np.float32)).to(dev),
                       torch.from_numpy(mean.astype(np.float32)).to(dev))
    return c


def forecast(model, features, edge_index, stats=None, windows=None, batch: int = 64, score: bool = True,
             return_pred: bool = True, ctx=None,
             edge_weight=None, node_weights=None) -> ForecastResult:
    """``model``: the drop-in ``HybridSTGCN_LSTM`` (its weights, prepared as ``evaluate_regional``
    prepares it); ``features``: the region's normalised ``[T_total, N, 24]`` stream (a tensor on the HIP
    device or a numpy array); ``stats``: ``{"mean": [..], "std": [..]}`` of the adaptation checkpoint
    (None: normalised units). ``windows``: window starts (default: ``default_windows``). The windows
    run in passes of ``batch``; consecutive windows share their GCN features and input projections.
    ``score=False`` forecasts only (windows may then reach the end of the stream); ``return_pred=False``
    keeps the predictions on the device pass by pass and returns the metrics alone. ``ctx``: a
    ``_capi.Context`` of the model's shape to run on (default: the model's own cached one). ``node_weights
    [N]``: weights of the score sums per target node (``loss.latitude_weights`` for an area-weighted RMSE; 0
    masks a node, whose targets may then be NaN); the metrics divide by ``nwin * sum(v)``. The context's score
    weights are cleared again before returning."""
    import torch

    from . import _capi

    if not score and not return_pred:
        raise ValueError("forecast(score=False, return_pred=False) has nothing to return")
    c = _setup("forecast", model, features, edge_index, edge_weight, stats, ctx, windows,
               lambda t_total, T, Hf: default_windows(t_total, T, Hf, score), prepare_empty=True)
    w, N, Hf, C = c.entries, c.N, c.Hf, c.C
    if w.size == 0:
        return ForecastResult(None, None, None, None, None, 0, w)
    pred = torch.empty(w.size, N * Hf, C, device=c.dev) if return_pred else None
    sums = torch.empty(3, Hf, C, device=c.dev, dtype=torch.float64) if score else None
    with torch.no_grad(), _score_weights(c.ctx, node_weights if score else None, N):
        c.ctx.forecast(_capi.stream_ptr(torch), c.theta, w, batch, scale=c.std if score else None, pred=pred,
                       skill=sums)
        out = None
        if pred is not None:
            scale_t, shift_t = c.units()
            out = (pred * scale_t + shift_t).view(w.size, Hf, N, C).cpu().numpy()
    if not score:
        return ForecastResult(out, None, None, None, None, int(w.size), w)
    rmse, mae, prmse, skill = skill_metrics(sums.cpu().numpy(), score_count(w.size, N, node_weights))
    return ForecastResult(out, rmse, mae, prmse, skill, int(w.size), w)


# ---- autoregressive rollout (smaml_forecast_rollout) ----------------------------------------------------
# The model predicts Hf steps; feeding the forecast back in reaches day-scale leads. Stride s = Hf + 1: the
# targets of a window skip t + 0 (dataset.py:40-48), so each cycle appends a gap row no forecast
# covers, then the Hf predicted rows. The first C input channels are the predicted variables (dataset.py:
# targets are stream[..., :C]); the others are calendar / Koppen features known in advance and are taken
# from the stream row of the same absolute time.
GAPS = {"persistence": 0, "midpoint": 1}


def _gap_code(gap) -> int:
    if isinstance(gap, str):
        if gap not in GAPS:
            raise ValueError(f"gap must be one of {sorted(GAPS)} (or 0 / 1), got {gap!r}")
        return GAPS[gap]
    if int(gap) not in (0, 1):
        raise ValueError(f"gap must be 0 (persistence) or 1 (midpoint), got {gap!r}")
    return int(gap)


def rollout_origins(t_total: int, window: int, horizon: int, cycles: int, score: bool) -> np.ndarray:
    """Every origin the range rule of ``smaml_forecast_rollout`` admits: ``o + T + (R-1) s <= t_total``, with
    ``score`` ``o + T + R s <= t_total`` (``s = Hf + 1``). ``cycles = 1`` gives ``default_windows``."""
    s, R = horizon + 1, int(cycles)
    if R < 1:
        raise ValueError(f"cycles must be >= 1, got {cycles}")
    n = t_total - window - (R if score else R - 1) * s + 1
    return np.arange(max(0, n), dtype=np.int32)


def extend_stream(features, exo) -> np.ndarray:
    """``features [t, N, Cin]`` followed by ``len(exo)`` rows past the last observation: their exogenous
    channels are ``exo [k, N, Cin - C]`` (C is inferred from its width), their weather channels NaN -- the
    rollout never reads those as inputs. For forecasting past the end of the observations (``score=False``)."""
    f = np.asarray(features.detach().cpu() if hasattr(features, "detach") else features, np.float32)
    e = np.asarray(exo.detach().cpu() if hasattr(exo, "detach") else exo, np.float32)
    if f.ndim != 3 or e.ndim != 3 or e.shape[1] != f.shape[1] or not 0 < e.shape[2] <= f.shape[2]:
        raise ValueError(f"exo {e.shape} does not extend features {f.shape}: want [k, N, Cin - C]")
    C = f.shape[2] - e.shape[2]
    tail = np.full((e.shape[0],) + f.shape[1:], np.nan, np.float32)
    tail[:, :, C:] = e
    return np.concatenate([f, tail], axis=0)


def rollout_reference(forward, features, origins: Sequence[int], dims, cycles: int, gap="midpoint") -> np.ndarray:
    """The definition of ``smaml_forecast_rollout`` in numpy: ``traj [norig, R s, N, C]`` (float32,
    normalised) of the origins ``origins`` of ``features [t_total, N, Cin]``, with ``forward`` a callable
    ``window [T*N, Cin] -> [N*Hf, C]`` (the model's eval-mode output, flat rows as the model writes them).

    Per origin ``o`` a private sequence ``X[rho] = S[o + rho]``, ``rho < T``; cycle ``j`` runs the window
    ``X[j s : j s + T]``, reads the flat output as ``P [Hf, N, C]`` (F4), and appends at ``rho0 = j s + T`` the
    gap row (``X[rho0 - 1]`` held, or its float32 midpoint with ``P[0]``) and ``P``; the channels ``>= C`` of
    appended rows are those of ``S[o + rho]``. Weather channels of stream rows ``>= o + T`` are never read."""
    T, Hf, N, C = dims.window_size, dims.forecast_horizon, dims.num_nodes, dims.output_channels
    s, R, g = Hf + 1, int(cycles), _gap_code(gap)
    if R < 1:
        raise ValueError(f"cycles must be >= 1, got {cycles}")
    f = np.asarray(features)
    rows = T + (R - 1) * s
    out = np.empty((len(origins), R * s, N, C), np.float32)
    for i, o in enumerate(origins):
        o = int(o)
        if o < 0 or o + rows > f.shape[0]:
            raise ValueError(f"origin {o} does not fit {R} cycles in a stream of {f.shape[0]} steps")
        X = np.zeros((rows, N, f.shape[2]), np.float32)
        X[:T] = f[o:o + T]
        X[T:, :, C:] = f[o + T:o + rows, :, C:]
        for j in range(R):
            P = np.asarray(forward(X[j * s:j * s + T].reshape(T * N, -1)), np.float32).reshape(Hf, N, C)
            prev = X[j * s + T - 1, :, :C]
            first = np.float32(0.5) * (prev + P[0]) if g else prev
            blk = np.concatenate([first[None].astype(np.float32), P], axis=0)
            out[i, j * s:(j + 1) * s] = blk
            if j + 1 < R:
                X[j * s + T:(j + 1) * s + T, :, :C] = blk
    return out


def rollout_skill_reference(traj, features, origins: Sequence[int], dims, scale=None, node_weights=None) -> np.ndarray:
    """The three sums ``[3, R s, C]`` (float64; order ``SUMS``) of a normalised trajectory ``traj
    [norig, R s, N, C]`` per absolute lead ``k`` and variable, over origins and nodes: every row (gap rows
    included) against ``y = features[o + T + k]``, and the persistence ``y_last = features[o + T - 1]``.
    ``node_weights``: as ``skill_reference``."""
    T, N, C = dims.window_size, dims.num_nodes, dims.output_channels
    v = node_weight_vector(node_weights, N)
    x = np.asarray(traj, np.float64)
    x = x.reshape(len(origins), -1, N, C)
    K = x.shape[1]
    f = np.asarray(features)
    sc = np.ones(C) if scale is None else np.asarray(scale, np.float64).reshape(C)
    out = np.zeros((3, K, C))
    for xi, o in zip(x, origins):
        o = int(o)
        if o < 0 or o + T + K > f.shape[0]:
            raise ValueError(f"origin {o} has no targets for {K} leads in a stream of {f.shape[0]} steps")
        y = f[o + T:o + T + K, :, :C].astype(np.float64)
        y_last = f[o + T - 1, :, :C].astype(np.float64)[None]
        e = (xi - y) * sc
        q = (y_last - y) * sc
        out[0] += _node_sum(e * e, v)
        out[1] += _node_sum(np.abs(e), v)
        out[2] += _node_sum(q * q, v)
    return out


@dataclass
class RolloutResult:
    traj: Optional[np.ndarray]              # [norig, R s, N, C], physical units over the first len(std) variables
    is_gap: np.ndarray                      # [R s] bool: the rows no forecast covers (filled by the gap rule)
    rmse: Optional[np.ndarray]              # [R s, C] per absolute lead (hours on an hourly stream: k + 1 ahead)
    mae: Optional[np.ndarray]               # [R s, C]
    persistence_rmse: Optional[np.ndarray]  # [R s, C]
    skill: Optional[np.ndarray]             # [R s, C]: 1 - SSE / SSE_persistence
    n_origins: int
    origins: np.ndarray
    cycles: int
    gap: str


def rollout(model, features, edge_index, stats=None, origins=None, cycles: int = 3, gap="midpoint", batch: int = 32,
            score: bool = True, ctx=None,
            edge_weight=None, node_weights=None) -> RolloutResult:
    """Autoregressive forecast of ``cycles`` x ``(Hf + 1)`` steps from every origin (``smaml_forecast_rollout``):
    each cycle's prediction is fed back as the weather channels of the next window, the exogenous channels
    come from ``features`` (use ``extend_stream`` to forecast past the last observation, with ``score=False``).
    Arguments as ``forecast``; ``origins`` defaults to ``rollout_origins``; ``gap``: "midpoint" or
    "persistence" fills the row between a window and its first target. Returns the trajectory in physical
    units and, with ``score``, RMSE / MAE / persistence RMSE / skill per absolute lead and variable (count per
    lead: ``norig * N``, or ``norig * sum(v)`` with ``node_weights``, which weigh the sums as in ``forecast``)."""
    import torch

    from . import _capi

    g = _gap_code(gap)
    R = int(cycles)
    c = _setup("rollout", model, features, edge_index, edge_weight, stats, ctx, origins,
               lambda t_total, T, Hf: rollout_origins(t_total, T, Hf, R, score))
    o, N, C, s = c.entries, c.N, c.C, c.Hf + 1
    is_gap = (np.arange(R * s) % s) == 0
    gname = "midpoint" if g else "persistence"
    if o.size == 0:
        return RolloutResult(None, is_gap, None, None, None, None, 0, o, R, gname)
    traj = torch.empty(o.size, R, s, N, C, device=c.dev)
    sums = torch.empty(3, R * s, C, device=c.dev, dtype=torch.float64) if score else None
    with torch.no_grad(), _score_weights(c.ctx, node_weights if score else None, N):
        c.ctx.forecast_rollout(_capi.stream_ptr(torch), c.theta, o, batch, R, g, scale=c.std if score else None,
                               traj=traj, skill=sums)
        scale_t, shift_t = c.units()
        out = (traj * scale_t + shift_t).view(o.size, R * s, N, C).cpu().numpy()
    if not score:
        return RolloutResult(out, is_gap, None, None, None, None, int(o.size), o, R, gname)
    rmse, mae, prmse, skill = skill_metrics(sums.cpu().numpy(), score_count(o.size, N, node_weights))
    return RolloutResult(out, is_gap, rmse, mae, prmse, skill, int(o.size), o, R, gname)


# ---- MC-dropout ensemble (smaml_forecast_ensemble) -----------------------------------------------------
ENSEMBLE_SUMS =("mean_sse", "variance", "crps", "persistence_sse")  # order of smaml_forecast_ensemble's scores


def ensemble_reference(member_pred, features, windows: Sequence[int], dims, scale=None, node_weights=None):
    """``(mean, spread, sums)`` in float64 of the members ``member_pred [E, nwin, N*Hf, C]`` (normalised):
    ``mean`` / ``spread [nwin, N*Hf, C]`` -- the member mean and the unbiased standard deviation about it
    (0 at E = 1) -- and ``sums [4, Hf, C]`` (order ``ENSEMBLE_SUMS``) over windows and nodes with
    ``skill_reference``'s pairing, targets and scale: ``sum (s (mu - y))^2``, ``sum s^2 sigma^2``,
    ``sum s CRPS`` with ``CRPS = (1/E) sum_i |x_i - y| - (1/(2 E^2)) sum_ij |x_i - x_j|`` and the persistence
    ``sum (s (y_last - y))^2``. ``node_weights``: as ``skill_reference`` (the sums only; mean and spread are
    not affected). Pure numpy; needs no GPU."""
    T, Hf, N, C = dims.window_size, dims.forecast_horizon, dims.num_nodes, dims.output_channels
    v = node_weight_vector(node_weights, N)
    x = np.asarray(member_pred, np.float64)
    E, nwin = x.shape[0], len(windows)
    x = x.reshape(E, nwin, N * Hf, C)
    mean = x.sum(axis=0) / E
    var = ((x - mean) ** 2).sum(axis=0) / (E - 1) if E > 1 else np.zeros_like(mean)
    f = np.asarray(features)
    s = np.ones(C) if scale is None else np.asarray(scale, np.float64).reshape(C)
    xv, mv, vv = x.reshape(E, nwin, Hf, N, C), mean.reshape(nwin, Hf, N, C), var.reshape(nwin, Hf, N, C)
    sums = np.zeros((4, Hf, C))
    for i, w in enumerate(windows):
        w = int(w)
        if w < 0 or w + T + Hf >= f.shape[0]:
            raise ValueError(f"window {w} has no targets in a stream of {f.shape[0]} steps")
        y = f[w + T + 1:w + T + 1 + Hf, :, :C].astype(np.float64)
        y_last = f[w + T - 1, :, :C].astype(np.float64)[None]
        xi = xv[:, i]
        crps = np.abs(xi - y).sum(axis=0) / E - np.abs(xi[:, None] - xi[None, :]).sum(axis=(0, 1)) / (2.0 * E * E)
        sums[0] += _node_sum(((mv[i] - y) * s) ** 2, v)
        sums[1] += _node_sum(vv[i] * s * s, v)
        sums[2] += _node_sum(crps * s, v)
        sums[3] += _node_sum(((y_last - y) * s) ** 2, v)
    return mean, np.sqrt(var), sums


def ensemble_metrics(sums: np.ndarray, count: int, members: int):
    """(rmse of the mean, rms spread, spread-skill ratio, mean CRPS, persistence rmse) ``[Hf, C]`` from the
    sums ``[4, Hf, C]`` over ``count`` (window, node) pairs per entry, of an ensemble of ``members`` = E.
    The ratio ``sqrt(((E + 1) / E) variance / mean_sse)`` is 1 for a statistically consistent E-member
    ensemble (NaN where the mean's error is 0). E is required: the sums do not carry it, and the finite-size
    factor ``(E + 1) / E`` is 1.06 at E = 16."""
    sums = np.asarray(sums, np.float64)
    if int(members) < 1:
        raise ValueError(f"members must be >= 1, got {members}")
    fac = (int(members) + 1) / int(members)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sums[0] > 0, np.sqrt(fac * sums[1] / sums[0]), np.nan)
    return np.sqrt(sums[0] / count), np.sqrt(sums[1] / count), ratio, sums[2] / count, np.sqrt(sums[3] / count)


@dataclass
class EnsembleResult:
    mean: Optional[np.ndarray]              # [nwin, Hf, N, C], physical units over the first len(std) variables
    spread: Optional[np.ndarray]            # [nwin, Hf, N, C], physical units (spread * std)
    members: Optional[np.ndarray]           # [E, nwin, Hf, N, C] with return_members
    rmse: Optional[np.ndarray]              # [Hf, C]: of the ensemble mean
    rms_spread: Optional[np.ndarray]        # [Hf, C]
    spread_skill: Optional[np.ndarray]      # [Hf, C]
    crps: Optional[np.ndarray]              # [Hf, C]: mean CRPS
    persistence_rmse: Optional[np.ndarray]  # [Hf, C]
    n_windows: int
    n_members: int
    windows: np.ndarray
    seed: int
    p_gcn: float
    p_lstm: float


def ensemble_forecast(model, features, edge_index, stats=None, members: int = 16, p_gcn=None, p_lstm=None,
                      seed=None, windows=None, batch: int = 32, score: bool = True, return_members: bool = False,
                      ctx=None,
                      edge_weight=None, node_weights=None) -> EnsembleResult:
    """MC-dropout ensemble of ``forecast``: ``members`` stochastic forwards per window, member ``e`` under the
    library's masks of ``(seed, step e)`` (what ``model.train()``'s forward under ``no_grad`` computes), in
    lockstep over the member axis. ``p_gcn`` / ``p_lstm`` default to the model's own dropout rates
    (``base_stgcn.dropout.p``, ``dropout.p``), ``seed`` to ``draw_dropout_seed()``. Returns the ensemble mean
    (``mean * std + mean_stat``) and spread (``spread * std``) in physical units, optionally every member, and
    with ``score`` the metrics of ``ensemble_metrics``; ``score=False`` forecasts only (windows may then reach
    the end of the stream). Other arguments as ``forecast`` (``node_weights`` included: the four sums are
    weighted, the metrics divide by ``nwin * sum(v)``).

    Cost: with ``p_gcn == 0`` the GCN features, layer 0's projection and LSTM layer 0 are computed once for all
    members (16 members measured 0.69 x 16 deterministic ``forecast`` runs at N = 441). With ``p_gcn > 0`` --
    the default for a model trained with GCN dropout, since the default is the model's own rate -- nothing
    below the LSTM is shared and every member runs its own GCN on the per-layer kernels: 2.5 x the time of
    ``p_gcn = 0`` there (1.73 x 16 deterministic runs). Pass ``p_gcn=0.0`` for LSTM-only MC dropout when that
    is acceptable."""
    import torch

    from . import _capi
    from .hybrid_model import draw_dropout_seed

    # (a caller's context may live elsewhere than the model: only the model's own needs the device)
    c = _setup("ensemble_forecast", model, features, edge_index, edge_weight, stats, ctx, windows,
               lambda t_total, T, Hf: default_windows(t_total, T, Hf, score), device_only=ctx is None)
    p_gcn = float(model.base_stgcn.dropout.p) if p_gcn is None else float(p_gcn)
    p_lstm = float(model.dropout.p) if p_lstm is None else float(p_lstm)
    seed = draw_dropout_seed() if seed is None else int(seed) & 0xFFFFFFFF
    E = int(members)
    w, N, Hf, C, dev = c.entries, c.N, c.Hf, c.C, c.dev
    if w.size == 0:
        return EnsembleResult(None, None, None, None, None, None, None, None, 0, E, w, seed, p_gcn, p_lstm)
    mean = torch.empty(w.size, N * Hf, C, device=dev)
    spread = torch.empty(w.size, N * Hf, C, device=dev)
    mem = torch.empty(E, w.size, N * Hf, C, device=dev) if return_members else None
    sums = torch.empty(4, Hf, C, device=dev, dtype=torch.float64) if score else None
    with torch.no_grad(), _score_weights(c.ctx, node_weights if score else None, N):
        c.ctx.forecast_ensemble(_capi.stream_ptr(torch), c.theta, w, batch, E, p_gcn, p_lstm, seed,
                                scale=c.std if score else None, mean=mean, spread=spread, member_pred=mem, scores=sums)
        scale_t, shift_t = c.units()
        mean_o = (mean * scale_t + shift_t).view(w.size, Hf, N, C).cpu().numpy()
        spread_o = (spread * scale_t).view(w.size, Hf, N, C).cpu().numpy()
        mem_o = (mem * scale_t + shift_t).view(E, w.size, Hf, N, C).cpu().numpy() if mem is not None else None
    if not score:
        return EnsembleResult(mean_o, spread_o, mem_o, None, None, None, None, None, int(w.size), E, w, seed, p_gcn,
                              p_lstm)
    rmse, rms, ratio, crps, prmse = ensemble_metrics(sums.cpu().numpy(), score_count(w.size, N, node_weights), E)
    return EnsembleResult(mean_o, spread_o, mem_o, rmse, rms, ratio, crps, prmse, int(w.size), E, w, seed, p_gcn, p_lstm)


# ---- ensemble rollout (smaml_forecast_rollout_ensemble) -------------------------------------------------
# Every MC-dropout member feeds its OWN forecast back in: how the spread grows with lead time, and whether it
# keeps pace with the error of the ensemble mean. Cycle j of member e runs under the masks of step 64 j + e, so
# cycle 0 is ``ensemble_forecast``'s member e and a member does not depend on E, R or the pass size.
def ensemble_rollout_reference(member_traj, features, origins: Sequence[int], dims, scale=None, node_weights=None):
    """``(mean, spread, sums)`` in float64 of the member trajectories ``member_traj [E, norig, R s, N, C]``
    (normalised; any shape that reshapes to it): ``mean`` / ``spread [norig, R s, N, C]`` -- the member mean and
    the unbiased standard deviation about it (0 at E = 1) -- and ``sums [4, R s, C]`` (order ``ENSEMBLE_SUMS``) per
    absolute lead ``k`` and variable over origins and nodes, every row (gap rows included) against
    ``y = features[o + T + k]`` and the persistence ``y_last = features[o + T - 1]``: ``sum (s (mu - y))^2``,
    ``sum s^2 sigma^2``, ``sum s CRPS`` with ``CRPS = (1/E) sum_i |x_i - y| - (1/(2 E^2)) sum_ij |x_i - x_j|``,
    ``sum (s (y_last - y))^2``. Rows are ``[N, C]`` already: no F4 pairing. ``node_weights``: as
    ``skill_reference``. Pure numpy; needs no GPU."""
    T, N, C = dims.window_size, dims.num_nodes, dims.output_channels
    v = node_weight_vector(node_weights, N)
    x = np.asarray(member_traj, np.float64)
    E, norig = x.shape[0], len(origins)
    x = x.reshape(E, norig, -1, N, C)
    K = x.shape[2]
    mean = x.sum(axis=0) / E
    var = ((x - mean) ** 2).sum(axis=0) / (E - 1) if E > 1 else np.zeros_like(mean)
    f = np.asarray(features)
    s = np.ones(C) if scale is None else np.asarray(scale, np.float64).reshape(C)
    sums = np.zeros((4, K, C))
    for i, o in enumerate(origins):
        o = int(o)
        if o < 0 or o + T + K > f.shape[0]:
            raise ValueError(f"origin {o} has no targets for {K} leads in a stream of {f.shape[0]} steps")
        y = f[o + T:o + T + K, :, :C].astype(np.float64)
        y_last = f[o + T - 1, :, :C].astype(np.float64)[None]
        xi = x[:, i]
        crps = np.abs(xi - y).sum(axis=0) / E - np.abs(xi[:, None] - xi[None, :]).sum(axis=(0, 1)) / (2.0 * E * E)
        sums[0] += _node_sum(((mean[i] - y) * s) ** 2, v)
        sums[1] += _node_sum(var[i] * s * s, v)
        sums[2] += _node_sum(crps * s, v)
        sums[3] += _node_sum(((y_last - y) * s) ** 2, v)
    return mean, np.sqrt(var), sums


def ensemble_rollout_metrics(sums: np.ndarray, count: int):
    """(rmse of the mean, rms spread, spread-skill ratio ``rms_spread / rmse``, mean CRPS, persistence rmse, skill
    ``1 - mean_sse / persistence_sse``) ``[R s, C]`` from the sums ``[4, R s, C]`` over ``count`` (origin, node)
    pairs per entry; the ratios are NaN where their denominator is 0."""
    sums = np.asarray(sums, np.float64)
    rmse, rms = np.sqrt(sums[0] / count), np.sqrt(sums[1] / count)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(sums[0] > 0, rms / rmse, np.nan)
        skill = np.where(sums[3] > 0, 1.0 - sums[0] / sums[3], np.nan)
    return rmse, rms, ratio, sums[2] / count, np.sqrt(sums[3] / count), skill


@dataclass
class EnsembleRolloutResult:
    mean: Optional[np.ndarray]              # [norig, R s, N, C], physical units over the first len(std) variables
    spread: Optional[np.ndarray]            # [norig, R s, N, C], physical units (spread * std)
    members: Optional[np.ndarray]           # [E, norig, R s, N, C] with return_members
    is_gap: np.ndarray                      # [R s] bool: the rows no forecast covers (filled by the gap rule)
    rmse: Optional[np.ndarray]              # [R s, C] per absolute lead: of the ensemble mean
    rms_spread: Optional[np.ndarray]        # [R s, C]
    spread_skill: Optional[np.ndarray]      # [R s, C]: rms_spread / rmse
    crps: Optional[np.ndarray]              # [R s, C]: mean CRPS
    persistence_rmse: Optional[np.ndarray]  # [R s, C]
    skill: Optional[np.ndarray]             # [R s, C]: 1 - SSE(mean) / SSE_persistence
    n_origins: int
    n_members: int
    origins: np.ndarray
    cycles: int
    gap: str
    seed: int
    p_gcn: float
    p_lstm: float


def ensemble_rollout(model, features, edge_index, stats=None, origins=None, cycles: int = 3, members: int = 16,
                     p_gcn=None, p_lstm=None, seed=None, gap="midpoint", batch: int = 32, score: bool = True,
                     return_members: bool = False, ctx=None,
                     edge_weight=None, node_weights=None) -> EnsembleRolloutResult:
    """``rollout`` for an MC-dropout ensemble (``smaml_forecast_rollout_ensemble``): each of the ``members`` feeds
    its own forecast back in for ``cycles`` x ``(Hf + 1)`` steps, member ``e`` of cycle ``j`` under the library's
    masks of ``(seed, step 64 j + e)``. Defaults as ``ensemble_forecast`` (the model's own dropout rates,
    ``draw_dropout_seed()``) and ``rollout`` (``rollout_origins``; ``extend_stream`` with ``score=False`` to forecast
    past the last observation). Returns the ensemble mean and spread along the trajectory in physical units,
    optionally every member, and with ``score`` the metrics of ``ensemble_rollout_metrics`` per absolute lead and
    variable (count per lead: ``norig * N``, or ``norig * sum(v)`` with ``node_weights``, as in ``forecast``).

    Cost: with ``p_gcn == 0`` the observed rows' GCN features and projection are computed once per pass for all
    members and cycle 0 shares LSTM layer 0; ``p_gcn > 0`` recomputes every member's whole window each cycle on
    the per-layer kernels (correct, not tuned). Pass ``p_gcn=0.0`` for LSTM-only MC dropout."""
    import torch

    from . import _capi
    from .hybrid_model import draw_dropout_seed

    g = _gap_code(gap)
    R, E = int(cycles), int(members)
    c = _setup("ensemble_rollout", model, features, edge_index, edge_weight, stats, ctx, origins,
               lambda t_total, T, Hf: rollout_origins(t_total, T, Hf, R, score))
    p_gcn = float(model.base_stgcn.dropout.p) if p_gcn is None else float(p_gcn)
    p_lstm = float(model.dropout.p) if p_lstm is None else float(p_lstm)
    seed = draw_dropout_seed() if seed is None else int(seed) & 0xFFFFFFFF
    o, N, C, dev, s = c.entries, c.N, c.C, c.dev, c.Hf + 1
    is_gap = (np.arange(R * s) % s) == 0
    gname = "midpoint" if g else "persistence"
    tail = (int(o.size), E, o, R, gname, seed, p_gcn, p_lstm)
    if o.size == 0:
        return EnsembleRolloutResult(None, None, None, is_gap, None, None, None, None, None, None, *tail)
    mean = torch.empty(o.size, R, s, N, C, device=dev)
    spread = torch.empty(o.size, R, s, N, C, device=dev)
    mem = torch.empty(E, o.size, R, s, N, C, device=dev) if return_members else None
    sums = torch.empty(4, R * s, C, device=dev, dtype=torch.float64) if score else None
    with torch.no_grad(), _score_weights(c.ctx, node_weights if score else None, N):
        c.ctx.forecast_rollout_ensemble(_capi.stream_ptr(torch), c.theta, o, batch, R, E, p_gcn, p_lstm, seed, gap=g,
                                        scale=c.std if score else None, member_traj=mem, mean=mean, spread=spread,
                                        scores=sums)
        scale_t, shift_t = c.units()
        mean_o = (mean * scale_t + shift_t).view(o.size, R * s, N, C).cpu().numpy()
        spread_o = (spread * scale_t).view(o.size, R * s, N, C).cpu().numpy()
        mem_o = (mem * scale_t + shift_t).view(E, o.size, R * s, N, C).cpu().numpy() if mem is not None else None
    if not score:
        return EnsembleRolloutResult(mean_o, spread_o, mem_o, is_gap, None, None, None, None, None, None, *tail)
    rmse, rms, ratio, crps, prmse, skill = ensemble_rollout_metrics(sums.cpu().numpy(),
                                                                    score_count(o.size, N, node_weights))
    return EnsembleRolloutResult(mean_o, spread_o, mem_o, is_gap, rmse, rms, ratio, crps, prmse, skill, *tail)
