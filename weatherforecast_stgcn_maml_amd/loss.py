"""Weights of the training loss and of the forecast scores.

The library's loss is ``inv * sum W (pred - y)^2`` with ``inv = 1 / (B N Hf C)`` (``smaml_set_loss_weights``): it
does not normalise, so the helpers here scale a table to mean 1 and losses, clip thresholds and learning rates keep
their meaning. A table is ``[Hf*N, C]`` in the layout of the targets ``y`` (dataset.py:40-48): row ``h'*N + n'``,
column ``c`` -- the weight of target lead ``h'``, node ``n'``, variable ``c``. With the model's F4 pairing (flat
prediction row ``r = n*Hf + h`` meets target row ``r``) it is simply elementwise with ``pred`` and ``y`` as the
loss sees them. Weight 0 masks an element: its target may hold anything, NaN included.

``latitude_weights`` gives the node weights every published weather score uses (cosine of latitude); they go into
``make_loss_weights(node=...)`` for the loss and into ``forecast(..., node_weights=...)`` for the scores.
"""
from __future__ import annotations

import numpy as np


def latitude_weights(lats_deg) -> np.ndarray:
    """``cos(lat)`` per node, scaled to mean 1 (float64 ``[N]``). ``lats_deg``: the nodes' latitudes in degrees."""
    lat = np.asarray(lats_deg, np.float64).reshape(-1)
    if lat.size == 0 or not np.all(np.isfinite(lat)) or np.any(np.abs(lat) > 90.0):
        raise ValueError("latitudes must be finite degrees in [-90, 90]")
    w = np.clip(np.cos(np.deg2rad(lat)), 0.0, None)
    if not w.sum() > 0:
        raise ValueError("every node sits on a pole: no positive weight")
    return w / w.mean()


def _factor(x, n, name):
    if x is None:
        return np.ones(n)
    a = np.asarray(x.detach().cpu() if hasattr(x, "detach") else x, np.float64).reshape(-1)
    if a.size != n:
        raise ValueError(f"{name} has {a.size} entries, expected {n}")
    if not np.all(np.isfinite(a)) or np.any(a < 0):
        raise ValueError(f"{name} weights must be finite and >= 0")
    return a


def make_loss_weights(dims, node=None, variable=None, lead=None, normalize: bool = True) -> np.ndarray:
    """The separable table ``W[h'*N + n', c] = lead[h'] * node[n'] * variable[c]`` as float32 ``[Hf*N, C]`` (each
    factor defaults to ones), scaled to mean 1 unless ``normalize=False``."""
    Hf, N, C = dims.forecast_horizon, dims.num_nodes, dims.output_channels
    w = (_factor(lead, Hf, "lead")[:, None, None] * _factor(node, N, "node")[None, :, None] *
         _factor(variable, C, "variable")[None, None, :])
    if not w.sum() > 0:
        raise ValueError("loss weights have no positive entry")
    if normalize:
        w = w / w.mean()
    return np.ascontiguousarray(w.reshape(Hf * N, C), dtype=np.float32)


def normalize_loss_weights(W) -> np.ndarray:
    """Any table (or stack of tables ``[nsets, Hf*N, C]``, each on its own) scaled to mean 1, float32."""
    w = np.asarray(W, np.float64)
    m = w.mean(axis=(-2, -1), keepdims=True)
    if not np.all(m > 0):
        raise ValueError("loss weights have no positive entry")
    return np.ascontiguousarray(w / m, dtype=np.float32)


def weighted_mse_reference(pred, y, W):
    """``mean(W * (pred - y)**2)`` over all elements -- what the library computes with the table ``W`` -- for numpy
    arrays or torch tensors of one shape ``[..., Hf*N, C]`` (``W`` broadcasts over leading axes). Elements of weight
    0 count as exactly 0 whatever ``y`` holds there."""
    if hasattr(pred, "detach"):
        import torch

        Wt = torch.as_tensor(W, dtype=pred.dtype, device=pred.device)
        d = pred - torch.as_tensor(y, dtype=pred.dtype, device=pred.device)
        return torch.where(Wt > 0, Wt * d * d, torch.zeros((), dtype=pred.dtype, device=pred.device)).mean()
    p = np.asarray(pred)
    Wn = np.broadcast_to(np.asarray(W, p.dtype), p.shape)
    d = p - np.asarray(y, p.dtype)
    with np.errstate(invalid="ignore"):
        return np.where(Wn > 0, Wn * d * d, 0).mean(dtype=np.float64)
