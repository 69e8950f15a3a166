"""ctypes binding of ``libsmaml.so`` (C ABI declared in ``include/smaml.h``).

The product path has no CPU fallback: if the library is missing or no HIP device is
present, every compute entry point raises ``SmamlError``.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMAML_LIB") or os.path.join(HERE, "libsmaml.so")

# every function include/smaml.h declares (checked by tests/test_capi_cpu.py)
EXPORTS = (
    "smaml_last_error", "smaml_abi_version", "smaml_build_info", "smaml_param_layout", "smaml_graph_ell",
    "smaml_create", "smaml_destroy", "smaml_set_graph", "smaml_set_gcn_params", "smaml_reserve",
    "smaml_workspace_bytes", "smaml_so_kept_steps", "smaml_set_dropout", "smaml_set_task_ids", "smaml_gcn_conv", "smaml_forward", "smaml_set_tasks",
    "smaml_meta_step", "smaml_adamw_step", "smaml_adapt_steps", "smaml_timing", "smaml_timing_collect",
    "smaml_backward", "smaml_gcn_forward", "smaml_lstm_forward", "smaml_lstm_backward", "smaml_head_loss",
    "smaml_clip_sgd", "smaml_inner_loop", "smaml_alloc", "smaml_free", "smaml_comm_unique_id",
    "smaml_comm_init", "smaml_comm_allreduce", "smaml_comm_destroy", "smaml_variant_counts", "smaml_set_option",
    "smaml_dropout", "smaml_sync", "smaml_gcn_conv_ex", "smaml_gcn_conv_backward", "smaml_relu_mask",
    "smaml_adapt_prepare", "smaml_adapt_phases", "smaml_forecast", "smaml_forecast_bytes",
    "smaml_adapt_steps_multi", "smaml_adapt_prepare_multi", "smaml_forecast_ensemble", "smaml_backward_base",
    "smaml_adapt_steps_full", "smaml_adapt_full_stats", "smaml_forecast_rollout", "smaml_rollout_stats",
    "smaml_forecast_rollout_ensemble", "smaml_rollout_ensemble_stats", "smaml_graph_csr", "smaml_set_graph_weighted",
    "smaml_graph_stats", "smaml_loss_weights_check", "smaml_set_loss_weights", "smaml_set_score_weights",
    "smaml_loss_stats", "smaml_gcn_cache_invalidate", "smaml_meta_step_base", "smaml_meta_base_stats",
)
ABI_VERSION = 9
GCN_RELU, GCN_PLAIN = 1, 2  # smaml_gcn_conv_ex / _backward flags

# kernels.h enum Variant: launch counters per kernel tile configuration (smaml_variant_counts)
VARIANTS = ("fwd", "fwd_drop", "fwd_split", "fwd_img", "fwd_dual", "fwd_dual_kept", "fwd_dual_img", "bwd_big", "bwd_small", "bwd_split",
            "bwd_dual_big", "bwd_dual_big_kept", "bwd_dual_small", "bwd_dual_small_kept", "wgrad", "wgrad_wide", "wgrad_pair",
            "fwd_kw", "bwd_kw", "gcn_dedup", "xg_dedup", "wgrad_dedup", "f_compact", "gcn_cache", "gcn_cache_rows",
            "fwd_infer", "fwd_infer_drop")

# api.cpp enum Cat: one kernel per category (the bench's roofline kernel is one symbol)
TIMING_CATEGORIES = ("gcn_layer", "lstm_fwd_step", "lstm_fwd_dual", "head_loss", "head_dh", "lstm_bwd_step",
                     "lstm_bwd_dual", "wgrad", "wgrad_reduce", "misc", "xg_proj", "dg_rowsum",
                     "lstm_fwd_step_wall", "lstm_fwd_dual_wall", "lstm_bwd_step_wall", "lstm_bwd_dual_wall")

ERRORS = {1: "EINVAL", 2: "EHIP", 3: "ENOMEM", 4: "ESTATE", 5: "ENOTIMPL"}


class SmamlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"smaml error {ERRORS.get(code, code)}: {msg}")
        self.code = code


class Dims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "num_nodes", "window_size", "input_channels", "hidden_channels", "lstm_hidden_size",
        "lstm_num_layers", "forecast_horizon", "output_channels")]

    @classmethod
    def from_model(cls, d):
        return cls(d.num_nodes, d.window_size, d.input_channels, d.hidden_channels,
                   d.lstm_hidden_size, d.lstm_num_layers, d.forecast_horizon, d.output_channels)


_lock = threading.Lock()
_lib = None

P = ctypes.c_void_p
I32 = ctypes.c_int32
I64 = ctypes.c_int64
F32 = ctypes.c_float
PI64 = ctypes.POINTER(ctypes.c_int64)
PI32 = ctypes.POINTER(ctypes.c_int32)
PF32 = ctypes.POINTER(ctypes.c_float)
PDIMS = ctypes.POINTER(Dims)

_SIGS = {
    "smaml_last_error": ([], ctypes.c_char_p),
    "smaml_abi_version": ([], I32),
    "smaml_build_info": ([], ctypes.c_char_p),
    "smaml_param_layout": ([PDIMS, I32, PI64, PI64, I32, PI32, PI64], I32),
    "smaml_graph_ell": ([PI64, I64, I32, PI32, PF32], I32),
    "smaml_create": ([PDIMS, I32, ctypes.POINTER(P)], I32),
    "smaml_destroy": ([P], I32),
    "smaml_set_graph": ([P, PI64, I64], I32),
    "smaml_set_gcn_params": ([P, P], I32),
    "smaml_reserve": ([P, I32, I32], I32),
    "smaml_workspace_bytes": ([P], I64),
    "smaml_so_kept_steps": ([P], I32),
    "smaml_set_dropout": ([P, ctypes.c_float, ctypes.c_float, ctypes.c_uint32], I32),
    "smaml_set_task_ids": ([P, PI32, I32], I32),
    "smaml_gcn_conv": ([P, P, P, I32, I32, P, P, I32, P], I32),
    "smaml_forward": ([P, P, P, ctypes.POINTER(P), I32, P, P], I32),
    "smaml_set_tasks": ([P, I32, ctypes.POINTER(P), PI32], I32),
    "smaml_meta_step": ([P, P, P, I32, I32, I32, PI32, F32, F32, F32, P, P, P, P], I32),
    "smaml_adamw_step": ([P, P, P, P, P, P, I64, I32, F32, F32, F32, F32, F32, F32, P], I32),
    "smaml_adapt_steps": ([P, P, P, P, P, I32, I32, I32, PI32, P, F32, F32, F32, F32, F32, P], I32),
    "smaml_timing": ([P, I32], I32),
    "smaml_backward": ([P, P, P, P, P], I32),
    "smaml_backward_base": ([P, P, P, ctypes.POINTER(P), I32, P, P, P, ctypes.POINTER(P)], I32),
    "smaml_gcn_forward": ([P, P, ctypes.POINTER(P), I32, P], I32),
    "smaml_lstm_forward": ([P, P, P, P, I32, P], I32),
    "smaml_lstm_backward": ([P, P, P, P, P], I32),
    "smaml_head_loss": ([P, P, P, P, ctypes.POINTER(P), I32, P, P, P], I32),
    "smaml_clip_sgd": ([P, P, P, P, I32, F32, F32, P], I32),
    "smaml_inner_loop": ([P, P, P, I32, I32, PI32, F32, F32, P, P, P], I32),
    "smaml_alloc": ([P, I64, ctypes.POINTER(P)], I32),
    "smaml_free": ([P, P], I32),
    "smaml_comm_unique_id": ([ctypes.POINTER(ctypes.c_uint8)], I32),
    "smaml_comm_init": ([P, I32, I32, ctypes.POINTER(ctypes.c_uint8)], I32),
    "smaml_comm_allreduce": ([P, P, P, I64], I32),
    "smaml_comm_destroy": ([P], I32),
    "smaml_timing_collect": ([P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                              PI64, I32], I32),
    "smaml_variant_counts": ([P, PI64, I32, PI32, I32], I32),
    "smaml_set_option": ([P, ctypes.c_char_p, I64], I32),
    "smaml_gcn_cache_invalidate": ([P], I32),
    "smaml_dropout": ([P, P, P, I64, F32, ctypes.c_uint32, I32], I32),
    "smaml_sync": ([P, P], I32),
    "smaml_gcn_conv_ex": ([P, P, P, I32, I32, P, P, I32, I32, P], I32),
    "smaml_gcn_conv_backward": ([P, P, P, I32, I32, P, I32, P, I32, P, P], I32),
    "smaml_relu_mask": ([P, P, P, P, I64], I32),
    "smaml_adapt_prepare": ([P, P, I32], I32),
    "smaml_adapt_phases": ([P, ctypes.POINTER(ctypes.c_double), I32, PI32, PI64], I32),
    "smaml_forecast": ([P, P, P, I32, PI32, I32, I32, PF32, P, P], I32),
    "smaml_forecast_bytes": ([P], I64),
    "smaml_adapt_steps_multi": ([P, P, I32, PI32, P, P, P, I32, I32, I32, PI32, P, PF32, F32, F32, F32, F32, P], I32),
    "smaml_adapt_prepare_multi": ([P, P, I32, PI32, I32], I32),
    "smaml_forecast_ensemble": ([P, P, P, I32, PI32, I32, I32, I32, F32, F32, ctypes.c_uint32, PF32, P, P, P, P], I32),
}
_SIGS["smaml_adapt_steps_full"] = ([P, P, P, P, P, P, P, P, I32, I32, I32, PI32, P, F32, F32, F32, F32, F32, P, P], I32)
_SIGS["smaml_adapt_full_stats"] = ([P, PI64, I32, PI32], I32)
# smaml_adapt_full_stats order (launch counters of the last smaml_adapt_steps_full call)
ADAPT_FULL_STATS = ("steps", "gcn_keep_fused", "gcn_keep_layer", "gcn_dz_fused", "gcn_dz_composed", "gcn_recompute")
_SIGS["smaml_meta_step_base"] = ([P, P, P, I32, I32, I32, PI32, F32, F32, F32, P, P, P, P, P], I32)
_SIGS["smaml_meta_base_stats"] = ([P, PI64, I32, PI32], I32)
# smaml_meta_base_stats order (counters of the last smaml_meta_step_base call)
META_BASE_STATS = ("stages", "distinct", "per_sample", "tangent", "bytes", "rows")
_SIGS["smaml_forecast_rollout"] = ([P, P, P, I32, PI32, I32, I32, I32, I32, PF32, P, P], I32)
_SIGS["smaml_rollout_stats"] = ([P, PI64, I32, PI32], I32)
# smaml_rollout_stats order (host counters of the last smaml_forecast_rollout call; a row = one time step of one origin)
ROLLOUT_STATS = ("cycles", "gcn_rows", "graph_rows", "xg_rows", "append_launches")
ROLLOUT_GAPS = {"persistence": 0, "midpoint": 1}  # smaml_forecast_rollout's gap argument
_SIGS["smaml_forecast_rollout_ensemble"] = ([P, P, P, I32, PI32, I32, I32, I32, I32, I32, F32, F32, ctypes.c_uint32, PF32,
                                             P, P, P, P], I32)
_SIGS["smaml_rollout_ensemble_stats"] = ([P, PI64, I32, PI32], I32)
# smaml_rollout_ensemble_stats order (host counters of the last smaml_forecast_rollout_ensemble call; a row = one
# time step of one origin; member_rows / shared_rows went through the position-independent GCN)
ROLLOUT_ENSEMBLE_STATS = ("cycles", "member_rows", "shared_rows", "graph_rows", "xg_rows", "append_launches",
                          "member_groups")
ROLLOUT_ENSEMBLE_MAX_CYCLES = 1024  # the mask site's step 64 j + e has 16 bits
_SIGS["smaml_graph_csr"] = ([PI64, PF32, I64, I32, PI32, PI32, PF32, I64, PI64], I32)
_SIGS["smaml_set_graph_weighted"] = ([P, PI64, PF32, I64], I32)
_SIGS["smaml_graph_stats"] = ([P, PI64, I32, PI32], I32)
_SIGS["smaml_loss_weights_check"] = ([PDIMS, PF32, I32], I32)
_SIGS["smaml_set_loss_weights"] = ([P, PF32, I32], I32)
_SIGS["smaml_set_score_weights"] = ([P, PF32], I32)
_SIGS["smaml_loss_stats"] = ([P, PI64, I32, PI32], I32)
# smaml_loss_stats order (the tables held; weighted launches since the last set / clear of either table)
LOSS_STATS = ("loss_sets", "score_weights", "head_loss", "head_loss_small", "head_dual", "score_launches")
# smaml_graph_stats order (host counters of the live graph; form: 0 none, 1 ELL, 2 CSR)
GRAPH_STATS = ("form", "entries", "longest_row", "csr_layer_launches", "csr_gather_launches")
GRAPH_ELL, GRAPH_CSR = 1, 2
ELL_MAX_IN_DEGREE = 7  # kernels.h ELLW - 1
# smaml_adapt_phases order (api.cpp AdPhases)
ADAPT_PHASES = ("reserve_ms", "cache_alloc_ms", "cache_fill_ms", "steps_ms")


def lib():
    """Load libsmaml.so (raises SmamlError if it was not built)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise SmamlError(-1, f"{LIB_PATH} not built; run __graft_entry__.build()")
            L = ctypes.CDLL(LIB_PATH)
            L.smaml_abi_version.restype = I32
            if L.smaml_abi_version() != ABI_VERSION:
                raise SmamlError(-1, f"{LIB_PATH} has ABI {L.smaml_abi_version()}, expected {ABI_VERSION}; rebuild")
            for name, (args, res) in _SIGS.items():
                fn = getattr(L, name)
                fn.argtypes = args
                fn.restype = res
            _lib = L
    return _lib


def build_info() -> str:
    """The library's product form per GEMM family (smaml_build_info)."""
    return lib().smaml_build_info().decode()


def product_forms() -> dict:
    """{GEMM family: 0 = f32 MFMA, 1 = bf16x6 fragment split, 2 = bf16x6 staged split} (build_info())."""
    tail = build_info().split(":", 1)[1]
    return {k: int(v) for k, v in (kv.split("=") for kv in tail.split())}


def check(rc):
    if rc != 0:
        raise SmamlError(rc, lib().smaml_last_error().decode(errors="replace"))


def param_layout(dims, which: int):
    """[(offset, size)] of the flat trainable (which=0) or GCN (which=1) vector + total."""
    L = lib()
    d = Dims.from_model(dims)
    cap = 64
    offs = (ctypes.c_int64 * cap)()
    sizes = (ctypes.c_int64 * cap)()
    cnt = ctypes.c_int32()
    tot = ctypes.c_int64()
    check(L.smaml_param_layout(ctypes.byref(d), which, offs, sizes, cap, ctypes.byref(cnt),
                               ctypes.byref(tot)))
    return [(offs[i], sizes[i]) for i in range(cnt.value)], tot.value


def graph_ell(edge_index: np.ndarray, num_nodes: int):
    L = lib()
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    E = ei.shape[1]
    cols = np.zeros((num_nodes, 8), np.int32)
    vals = np.zeros((num_nodes, 8), np.float32)
    check(L.smaml_graph_ell(ei.ctypes.data_as(PI64), E, num_nodes, cols.ctypes.data_as(PI32),
                            vals.ctypes.data_as(PF32)))
    return cols, vals


def _edge_weight(edge_weight, E):
    if edge_weight is None:
        return None
    ew = np.ascontiguousarray(edge_weight, dtype=np.float32).reshape(-1)
    if ew.size != E:
        raise ValueError(f"edge_weight has {ew.size} entries for {E} edges")
    return ew


def graph_csr(edge_index: np.ndarray, num_nodes: int, edge_weight=None):
    """(rowptr [N + 1], cols [nnz], vals [nnz]) of the normalised adjacency in its general form
    (smaml_graph_csr: any in-degree, optional edge weights)."""
    L = lib()
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    E = ei.shape[1]
    ew = _edge_weight(edge_weight, E)
    cap = E + num_nodes
    rowptr = np.zeros(num_nodes + 1, np.int32)
    cols = np.zeros(cap, np.int32)
    vals = np.zeros(cap, np.float32)
    nnz = ctypes.c_int64()
    check(L.smaml_graph_csr(ei.ctypes.data_as(PI64), ew.ctypes.data_as(PF32) if ew is not None else None, E, num_nodes,
                            rowptr.ctypes.data_as(PI32), cols.ctypes.data_as(PI32), vals.ctypes.data_as(PF32), cap,
                            ctypes.byref(nnz)))
    return rowptr, cols[:nnz.value].copy(), vals[:nnz.value].copy()


def set_graph_auto(ctx, edge_index, edge_weight=None, skip_same=False):
    """Upload the graph to ``ctx`` in the form it needs: the ELL (``ctx.set_graph``) for an unweighted graph whose
    in-degree is at most 7 -- the path every such graph has always taken --, the CSR form
    (``ctx.set_graph_weighted``) for every other. ``skip_same``: do nothing if ``ctx.graph_key`` says that this
    graph, in this form, is the live one. Returns True if it uploaded."""
    ei = np.ascontiguousarray(edge_index, dtype=np.int64)
    ew = _edge_weight(edge_weight, ei.shape[1])
    ell = ew is None
    if ell and ei.size and ei.min() >= 0:  # (an index out of range: left to set_graph's own message)
        dst = ei[1][ei[0] != ei[1]]
        ell = dst.size == 0 or int(np.bincount(dst).max()) <= ELL_MAX_IN_DEGREE
    key = ei.tobytes() if ell else (b"csr", ei.tobytes(), None if ew is None else ew.tobytes())
    if skip_same and ctx.graph_key == key:
        return False
    if ell:
        ctx.set_graph(ei)
    else:
        ctx.set_graph_weighted(ei, ew)
    return True


def _loss_table(dims, w):
    """``w`` as the contiguous float32 [nsets][Hf*N][C] array smaml_set_loss_weights reads (one table: nsets = 1)."""
    rows, C = int(dims.forecast_horizon) * int(dims.num_nodes), int(dims.output_channels)
    if hasattr(w, "detach"):
        w = w.detach().cpu().numpy()
    if isinstance(w, (list, tuple)):
        w = np.stack([np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float32) for x in w])
    a = np.ascontiguousarray(w, dtype=np.float32)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[1:] != (rows, C) or a.shape[0] < 1:
        raise ValueError(f"loss weights must be [{rows}, {C}] or [nsets, {rows}, {C}], got {tuple(a.shape)}")
    return a


def loss_weights_check(dims, w):
    """smaml_loss_weights_check on the host: raises SmamlError naming the set and element of a bad weight."""
    d = dims if isinstance(dims, Dims) else Dims.from_model(dims)
    a = _loss_table(d, w)
    check(lib().smaml_loss_weights_check(ctypes.byref(d), a.ctypes.data_as(PF32), a.shape[0]))


def ptr(t) -> int:
    return t.data_ptr()


def _ptrs(ts):
    return (P * len(ts))(*[ptr(t) for t in ts])


def comm_unique_id() -> bytes:
    """128-byte RCCL unique id (rank 0), to ship to the other ranks."""
    buf = (ctypes.c_uint8 * 128)()
    check(lib().smaml_comm_unique_id(buf))
    return bytes(buf)


def stream_ptr(torch_mod):
    return torch_mod.cuda.current_stream().cuda_stream


class Context:
    """Owns one ``smaml_ctx`` (one GPU, one host thread)."""

    def __init__(self, dims, device: int = 0):
        self.dims = dims
        self._L = lib()
        self._h = P()
        self._d = Dims.from_model(dims)
        check(self._L.smaml_create(ctypes.byref(self._d), int(device), ctypes.byref(self._h)))
        self.device = device
        # A/B runs: SMAML_OPTIONS="key=value,key=value" applies smaml_set_option knobs to every context
        for kv in filter(None, os.environ.get("SMAML_OPTIONS", "").split(",")):
            k, _, v = kv.partition("=")
            self.set_option(k.strip(), int(v))
        self._keep = []
        self.graph_key = None

    def close(self):
        if self._h:
            self._L.smaml_destroy(self._h)
            self._h = P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- setup
    def set_graph(self, edge_index: np.ndarray):
        ei = np.ascontiguousarray(edge_index, dtype=np.int64)
        check(self._L.smaml_set_graph(self._h, ei.ctypes.data_as(PI64), ei.shape[1]))
        self.graph_key = ei.tobytes()

    def set_graph_weighted(self, edge_index: np.ndarray, edge_weight=None):
        """The graph in its general form (smaml_set_graph_weighted): any in-degree, ``edge_weight`` [E] or None."""
        ei = np.ascontiguousarray(edge_index, dtype=np.int64)
        ew = _edge_weight(edge_weight, ei.shape[1])
        check(self._L.smaml_set_graph_weighted(self._h, ei.ctypes.data_as(PI64),
                                               ew.ctypes.data_as(PF32) if ew is not None else None, ei.shape[1]))
        self.graph_key = (b"csr", ei.tobytes(), None if ew is None else ew.tobytes())

    def graph_stats(self):
        """{counter: value} of the live graph (smaml_graph_stats; host counters, no sync)."""
        n = len(GRAPH_STATS)
        buf = (ctypes.c_int64 * n)()
        cnt = ctypes.c_int32()
        check(self._L.smaml_graph_stats(self._h, buf, n, ctypes.byref(cnt)))
        assert cnt.value == n, (cnt.value, n)
        return {name: int(buf[i]) for i, name in enumerate(GRAPH_STATS)}

    def set_loss_weights(self, w):
        """Loss weights (smaml_set_loss_weights): one table [Hf*N, C], one per task [nsets, Hf*N, C] (array, tensor
        or a list of tables), or None to clear. Copied: the caller's array is free on return."""
        if w is None:
            check(self._L.smaml_set_loss_weights(self._h, None, 0))
            return
        a = _loss_table(self.dims, w)
        check(self._L.smaml_set_loss_weights(self._h, a.ctypes.data_as(PF32), a.shape[0]))

    def set_score_weights(self, v):
        """Node weights [N] of the forecast score sums (smaml_set_score_weights), or None to clear."""
        if v is None:
            check(self._L.smaml_set_score_weights(self._h, None))
            return
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        a = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
        if a.size != int(self.dims.num_nodes):
            raise ValueError(f"score weights must have {int(self.dims.num_nodes)} entries, got {a.size}")
        check(self._L.smaml_set_score_weights(self._h, a.ctypes.data_as(PF32)))

    def loss_stats(self):
        """{counter: value} of the weight tables and their launches (smaml_loss_stats; host counters, no sync)."""
        n = len(LOSS_STATS)
        buf = (ctypes.c_int64 * n)()
        cnt = ctypes.c_int32()
        check(self._L.smaml_loss_stats(self._h, buf, n, ctypes.byref(cnt)))
        assert cnt.value == n, (cnt.value, n)
        return {name: int(buf[i]) for i, name in enumerate(LOSS_STATS)}

    def set_gcn_params(self, flat):
        self._gcn = flat
        check(self._L.smaml_set_gcn_params(self._h, ptr(flat)))

    def reserve(self, tasks, batch):
        check(self._L.smaml_reserve(self._h, int(tasks), int(batch)))

    def workspace_bytes(self):
        return int(self._L.smaml_workspace_bytes(self._h))

    def so_kept_steps(self):
        return int(self._L.smaml_so_kept_steps(self._h))

    def set_dropout(self, p_gcn, p_lstm, seed):
        check(self._L.smaml_set_dropout(self._h, float(p_gcn), float(p_lstm), int(seed) & 0xFFFFFFFF))

    def set_task_ids(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        check(self._L.smaml_set_task_ids(self._h, a.ctypes.data_as(PI32), a.size))

    # --- compute
    def gcn_conv(self, stream, x, weight, bias, out):
        check(self._L.smaml_gcn_conv(self._h, stream, ptr(x), x.shape[0], x.shape[1], ptr(weight),
                                     ptr(bias), weight.shape[0], ptr(out)))

    def gcn_conv_ex(self, stream, x, weight, bias, out, flags=0):
        check(self._L.smaml_gcn_conv_ex(self._h, stream, ptr(x), x.shape[0], x.shape[1], ptr(weight), ptr(bias),
                                        weight.shape[0], int(flags), ptr(out)))

    def gcn_conv_backward(self, stream, x, weight, dz, dx=None, dwb=None, flags=0):
        check(self._L.smaml_gcn_conv_backward(self._h, stream, ptr(x), x.shape[0], x.shape[1], ptr(weight),
                                              weight.shape[0], ptr(dz), int(flags),
                                              ptr(dx) if dx is not None else None,
                                              ptr(dwb) if dwb is not None else None))

    def relu_mask(self, stream, g, h):
        check(self._L.smaml_relu_mask(self._h, stream, ptr(g), ptr(h), g.numel()))

    def forward(self, stream, theta, xs, pred, feats=None):
        arr = (P * len(xs))(*[ptr(x) for x in xs])
        check(self._L.smaml_forward(self._h, stream, ptr(theta), arr, len(xs), ptr(pred),
                                    ptr(feats) if feats is not None else None))

    def set_tasks(self, feats):
        arr = (P * len(feats))(*[ptr(f) for f in feats])
        tt = (ctypes.c_int32 * len(feats))(*[int(f.shape[0]) for f in feats])
        self._tasks = list(feats)
        # The per-stream GCN feature cache is keyed by stream address: a stream stays referenced here for as long
        # as the context may hold rows of it, so its memory cannot pass to another tensor in the meantime.
        pin = getattr(self, "_gc_pin", None)
        if pin is None or len(pin) > 256:
            if pin is not None:
                self.gcn_cache_invalidate()
            pin = self._gc_pin = {}
        for f in feats:
            pin[ptr(f)] = f
        check(self._L.smaml_set_tasks(self._h, len(feats), arr, tt))

    def gcn_cache_invalidate(self):
        """Forget the cached GCN features of every stream (smaml_gcn_cache_invalidate): after writing a registered
        stream's tensor in place."""
        check(self._L.smaml_gcn_cache_invalidate(self._h))

    def meta_step(self, stream, theta, order, steps, batch, windows: np.ndarray, inner_lr, max_norm,
                  query_scale, meta_grad=None, losses=None, norms=None, fast_out=None):
        w = np.ascontiguousarray(windows, dtype=np.int32)
        check(self._L.smaml_meta_step(
            self._h, stream, ptr(theta), int(order), int(steps), int(batch), w.ctypes.data_as(PI32),
            float(inner_lr), float(max_norm), float(query_scale),
            ptr(meta_grad) if meta_grad is not None else None,
            ptr(losses) if losses is not None else None,
            ptr(norms) if norms is not None else None,
            ptr(fast_out) if fast_out is not None else None))

    def meta_step_base(self, stream, theta, order, steps, batch, windows: np.ndarray, inner_lr, max_norm,
                       query_scale, meta_grad, gcn_meta_grad, losses=None, norms=None, fast_out=None):
        """``meta_step`` plus the GCN base's meta-gradient ``gcn_meta_grad`` [Pg] (smaml_meta_step_base; order 1
        or 2). The other outputs are bitwise ``meta_step``'s."""
        w = np.ascontiguousarray(windows, dtype=np.int32)
        check(self._L.smaml_meta_step_base(
            self._h, stream, ptr(theta), int(order), int(steps), int(batch), w.ctypes.data_as(PI32),
            float(inner_lr), float(max_norm), float(query_scale),
            ptr(meta_grad) if meta_grad is not None else None,
            ptr(gcn_meta_grad) if gcn_meta_grad is not None else None,
            ptr(losses) if losses is not None else None,
            ptr(norms) if norms is not None else None,
            ptr(fast_out) if fast_out is not None else None))

    def meta_base_stats(self):
        """{counter: value} of the last meta_step_base call (host counters, no sync)."""
        n = len(META_BASE_STATS)
        buf = (ctypes.c_int64 * n)()
        cnt = ctypes.c_int32()
        check(self._L.smaml_meta_base_stats(self._h, buf, n, ctypes.byref(cnt)))
        assert cnt.value == n, (cnt.value, n)
        return {name: int(buf[i]) for i, name in enumerate(META_BASE_STATS)}

    def adapt_steps(self, stream, theta, m, v, step0, windows: np.ndarray, lr_dev, betas, eps, wd, max_norm,
                    losses):
        w = np.ascontiguousarray(windows, dtype=np.int32)
        check(self._L.smaml_adapt_steps(self._h, stream, ptr(theta), ptr(m), ptr(v), int(step0), w.shape[0],
                                        w.shape[1], w.ctypes.data_as(PI32), ptr(lr_dev), float(betas[0]),
                                        float(betas[1]), float(eps), float(wd), float(max_norm), ptr(losses)))

    def adapt_steps_full(self, stream, theta, m, v, gcn, gcn_m, gcn_v, step0, windows: np.ndarray, lr_dev, betas, eps,
                         wd, max_norm, losses, norms=None):
        """``adapt_steps`` with the GCN base trained too (smaml_adapt_steps_full): ``gcn`` / ``gcn_m`` / ``gcn_v``
        [Pg] (layout which = 1) are updated in place like ``theta`` / ``m`` / ``v``, the clip is over both
        gradients jointly, and ``gcn`` becomes the context's GCN parameter vector. ``norms`` [nsteps]
        (device, optional): each step's joint gradient norm before clipping."""
        w = np.ascontiguousarray(windows, dtype=np.int32)
        self._gcn = gcn
        check(self._L.smaml_adapt_steps_full(self._h, stream, ptr(theta), ptr(m), ptr(v), ptr(gcn), ptr(gcn_m),
                                             ptr(gcn_v), int(step0), w.shape[0], w.shape[1], w.ctypes.data_as(PI32),
                                             ptr(lr_dev), float(betas[0]), float(betas[1]), float(eps), float(wd),
                                             float(max_norm), ptr(losses), ptr(norms) if norms is not None else None))

    def adapt_full_stats(self):
        """{counter: launches} of the last adapt_steps_full call (host counters, no sync)."""
        n = len(ADAPT_FULL_STATS)
        buf = (ctypes.c_int64 * n)()
        cnt = ctypes.c_int32()
        check(self._L.smaml_adapt_full_stats(self._h, buf, n, ctypes.byref(cnt)))
        assert cnt.value == n, (cnt.value, n)
        return {name: int(buf[i]) for i, name in enumerate(ADAPT_FULL_STATS)}

    def adapt_prepare(self, stream, batch=1):
        """Workspace + per-window feature cache for adapt_steps, allocated and touched now (no compute)."""
        check(self._L.smaml_adapt_prepare(self._h, stream, int(batch)))

    def adapt_steps_multi(self, stream, tasks, theta, m, v, step0, windows: np.ndarray, lr_dev, betas, eps, wds,
                          max_norm, losses):
        """Lockstep fine-tuning of the regions ``tasks`` (smaml_adapt_steps_multi): ``theta`` / ``m`` / ``v``
        [R, P], ``windows`` [nsteps, R, batch] (host), ``lr_dev`` and ``losses`` [nsteps, R] (device),
        ``wds`` [R] (host)."""
        t = np.ascontiguousarray(tasks, dtype=np.int32).reshape(-1)
        w = np.ascontiguousarray(windows, dtype=np.int32)
        wd = np.ascontiguousarray(wds, dtype=np.float32).reshape(-1)
        if w.ndim != 3 or w.shape[1] != t.size or wd.size != t.size:
            raise ValueError(f"windows {w.shape} / weight decays {wd.shape} do not match {t.size} regions")
        for name, a, shape in (("theta", theta, None), ("m", m, None), ("v", v, None),
                               ("lr_dev", lr_dev, (w.shape[0], t.size)), ("losses", losses, (w.shape[0], t.size))):
            if a.shape[0] != (shape or (t.size,))[0] or (shape and tuple(a.shape) != shape) or not a.is_contiguous():
                raise ValueError(f"{name} has shape {tuple(a.shape)} (contiguous: {a.is_contiguous()}) for "
                                 f"{t.size} regions x {w.shape[0]} steps")
        check(self._L.smaml_adapt_steps_multi(self._h, stream, t.size, t.ctypes.data_as(PI32), ptr(theta), ptr(m),
                                              ptr(v), int(step0), w.shape[0], w.shape[2], w.ctypes.data_as(PI32),
                                              ptr(lr_dev), wd.ctypes.data_as(PF32), float(betas[0]), float(betas[1]),
                                              float(eps), float(max_norm), ptr(losses)))

    def adapt_prepare_multi(self, stream, tasks, batch=1):
        """adapt_prepare for the regions of a lockstep call: the workspace and every region's feature cache."""
        t = np.ascontiguousarray(tasks, dtype=np.int32).reshape(-1)
        check(self._L.smaml_adapt_prepare_multi(self._h, stream, t.size, t.ctypes.data_as(PI32), int(batch)))

    def adapt_phases(self):
        """{phase: ms} of the last adapt_steps call (+ 'windows_filled_per_step')."""
        ms = (ctypes.c_double * len(ADAPT_PHASES))()
        n, filled = ctypes.c_int32(), ctypes.c_int64()
        check(self._L.smaml_adapt_phases(self._h, ms, len(ADAPT_PHASES), ctypes.byref(n), ctypes.byref(filled)))
        out = {k: ms[i] for i, k in enumerate(ADAPT_PHASES[:n.value])}
        out["windows_filled_per_step"] = filled.value
        return out

    def _list_and_scale(self, entries, scale):
        """The forecast calls' window or origin list as a flat int32 array and ``scale`` (or None) as float32 [C]."""
        e = np.ascontiguousarray(entries, dtype=np.int32).reshape(-1)
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
        if sc is not None and sc.size != self.dims.output_channels:
            raise ValueError(f"scale has {sc.size} entries, expected {self.dims.output_channels}")
        return e, sc

    def forecast(self, stream, theta, windows, batch, task=0, scale=None, pred=None, skill=None):
        """Rolling forecast of ``windows`` (starts into task ``task``'s stream) in passes of ``batch``:
        ``pred`` [nwin, N*Hf, C] float32 and / or ``skill`` [3, Hf, C] float64 device tensors
        (smaml_forecast; ``scale`` = per-variable factors of the skill sums, host, [C])."""
        w, sc = self._list_and_scale(windows, scale)
        check(self._L.smaml_forecast(self._h, stream, ptr(theta), int(task), w.ctypes.data_as(PI32), w.size, int(batch),
                                     sc.ctypes.data_as(PF32) if sc is not None else None,
                                     ptr(pred) if pred is not None else None,
                                     ptr(skill) if skill is not None else None))

    def forecast_ensemble(self, stream, theta, windows, batch, members, p_gcn, p_lstm, seed, task=0, scale=None,
                          mean=None, spread=None, member_pred=None, scores=None):
        """MC-dropout ensemble of ``members`` stochastic forwards per window (smaml_forecast_ensemble): member
        ``e`` under the masks of ``(seed, step e)``. Device tensors, each optional: ``mean`` / ``spread``
        [nwin, N*Hf, C], ``member_pred`` [members, nwin, N*Hf, C] float32, ``scores`` [4, Hf, C] float64
        (``forecast.ENSEMBLE_SUMS``; ``scale`` = their per-variable factors, host, [C])."""
        w, sc = self._list_and_scale(windows, scale)
        opt = lambda t: ptr(t) if t is not None else None  # noqa: E731
        check(self._L.smaml_forecast_ensemble(
            self._h, stream, ptr(theta), int(task), w.ctypes.data_as(PI32), w.size, int(batch), int(members),
            float(p_gcn), float(p_lstm), int(seed) & 0xFFFFFFFF, sc.ctypes.data_as(PF32) if sc is not None else None,
            opt(mean), opt(spread), opt(member_pred), opt(scores)))

    def forecast_rollout(self, stream, theta, origins, batch, cycles, gap=1, task=0, scale=None, traj=None,
                         skill=None):
        """Autoregressive rollout of ``cycles`` cycles from the ``origins`` (window starts into task ``task``'s
        stream) in passes of ``batch`` (smaml_forecast_rollout): ``traj`` [norig, cycles, Hf + 1, N, C] float32
        and / or ``skill`` [3, cycles * (Hf + 1), C] float64 device tensors; ``gap`` 1 = midpoint, 0 =
        persistence (``ROLLOUT_GAPS``); ``scale`` = per-variable factors of the skill sums, host, [C]."""
        o, sc = self._list_and_scale(origins, scale)
        check(self._L.smaml_forecast_rollout(self._h, stream, ptr(theta), int(task), o.ctypes.data_as(PI32), o.size,
                                             int(batch), int(cycles), int(gap),
                                             sc.ctypes.data_as(PF32) if sc is not None else None,
                                             ptr(traj) if traj is not None else None,
                                             ptr(skill) if skill is not None else None))

    def rollout_stats(self):
        """{counter: count} of the last forecast_rollout call (host counters, no sync)."""
        n = len(ROLLOUT_STATS)
        buf = (ctypes.c_int64 * n)()
        cnt = ctypes.c_int32()
        check(self._L.smaml_rollout_stats(self._h, buf, n, ctypes.byref(cnt)))
        assert cnt.value == n, (cnt.value, n)
        return {name: int(buf[i]) for i, name in enumerate(ROLLOUT_STATS)}

    def forecast_rollout_ensemble(self, stream, theta, origins, batch, cycles, members, p_gcn, p_lstm, seed, gap=1,
                                  task=0, scale=None, member_traj=None, mean=None, spread=None, scores=None):
        """Ensemble rollout (smaml_forecast_rollout_ensemble): ``members`` MC-dropout members, each fed its own
        forecast back in for ``cycles`` cycles; member ``e`` of cycle ``j`` under the masks of ``(seed, step 64 j +
        e)``. Device tensors, each optional: ``member_traj`` [members, norig, cycles, Hf + 1, N, C], ``mean`` /
        ``spread`` [norig, cycles, Hf + 1, N, C] float32, ``scores`` [4, cycles * (Hf + 1), C] float64
        (``forecast.ENSEMBLE_SUMS``; ``scale`` = their per-variable factors, host, [C]); ``gap`` as
        ``forecast_rollout``."""
        o, sc = self._list_and_scale(origins, scale)
        opt = lambda t: ptr(t) if t is not None else None  # noqa: E731
        check(self._L.smaml_forecast_rollout_ensemble(
            self._h, stream, ptr(theta), int(task), o.ctypes.data_as(PI32), o.size, int(batch), int(cycles), int(gap),
            int(members), float(p_gcn), float(p_lstm), int(seed) & 0xFFFFFFFF,
            sc.ctypes.data_as(PF32) if sc is not None else None, opt(member_traj), opt(mean), opt(spread), opt(scores)))

    def rollout_ensemble_stats(self):
        """{counter: count} of the last forecast_rollout_ensemble call (host counters, no sync)."""
        n = len(ROLLOUT_ENSEMBLE_STATS)
        buf = (ctypes.c_int64 * n)()
        cnt = ctypes.c_int32()
        check(self._L.smaml_rollout_ensemble_stats(self._h, buf, n, ctypes.byref(cnt)))
        assert cnt.value == n, (cnt.value, n)
        return {name: int(buf[i]) for i, name in enumerate(ROLLOUT_ENSEMBLE_STATS)}

    def forecast_bytes(self):
        return int(self._L.smaml_forecast_bytes(self._h))

    def backward(self, stream, theta, dpred, grad):
        check(self._L.smaml_backward(self._h, stream, ptr(theta), ptr(dpred), ptr(grad)))

    def backward_base(self, stream, theta, xs, dpred, grad, gcn_grad=None, dxs=None):
        """smaml_backward continued through the GCN base (smaml_backward_base) for the forward of the samples
        ``xs``: ``grad`` [P] as ``backward``; ``gcn_grad`` [Pg] (layout which=1, summed over the samples) and /
        or ``dxs`` (one [T*N, Cin] tensor per sample: d loss / d x), at least one of the two."""
        if dxs is not None and len(dxs) != len(xs):
            raise ValueError(f"{len(dxs)} dx tensors for {len(xs)} samples")
        check(self._L.smaml_backward_base(self._h, stream, ptr(theta), _ptrs(xs), len(xs), ptr(dpred), ptr(grad),
                                          ptr(gcn_grad) if gcn_grad is not None else None,
                                          _ptrs(dxs) if dxs is not None else None))

    def gcn_forward(self, stream, xs, feats):
        check(self._L.smaml_gcn_forward(self._h, stream, _ptrs(xs), len(xs), ptr(feats)))

    def lstm_forward(self, stream, theta, feats, hT):
        check(self._L.smaml_lstm_forward(self._h, stream, ptr(theta), ptr(feats), int(feats.shape[0]), ptr(hT)))

    def lstm_backward(self, stream, theta, dhT, grad):
        check(self._L.smaml_lstm_backward(self._h, stream, ptr(theta), ptr(dhT), ptr(grad)))

    def head_loss(self, stream, theta, hT, pred, ys=None, loss=None, dpred=None):
        check(self._L.smaml_head_loss(self._h, stream, ptr(theta), ptr(hT), _ptrs(ys) if ys is not None else None,
                                      int(hT.shape[0]), ptr(pred), ptr(loss) if loss is not None else None,
                                      ptr(dpred) if dpred is not None else None))

    def clip_sgd(self, stream, theta, grad, ntasks, lr, max_norm, norms=None):
        check(self._L.smaml_clip_sgd(self._h, stream, ptr(theta), ptr(grad), int(ntasks), float(lr),
                                     float(max_norm), ptr(norms) if norms is not None else None))

    def sync(self, stream):
        """Synchronise the stream; raises SmamlError if a grid-barrier kernel timed out."""
        check(self._L.smaml_sync(self._h, stream))

    def inner_loop(self, stream, theta, steps, batch, windows: np.ndarray, inner_lr, max_norm, fast_out,
                   losses=None, norms=None):
        w = np.ascontiguousarray(windows, dtype=np.int32)
        check(self._L.smaml_inner_loop(self._h, stream, ptr(theta), int(steps), int(batch), w.ctypes.data_as(PI32),
                                       float(inner_lr), float(max_norm), ptr(fast_out),
                                       ptr(losses) if losses is not None else None,
                                       ptr(norms) if norms is not None else None))

    def alloc(self, nbytes: int) -> int:
        out = P()
        check(self._L.smaml_alloc(self._h, int(nbytes), ctypes.byref(out)))
        return out.value

    def free(self, p: int):
        check(self._L.smaml_free(self._h, P(p)))

    def comm_init(self, rank: int, world: int, uid: bytes):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        check(self._L.smaml_comm_init(self._h, int(rank), int(world), buf))

    def comm_allreduce(self, stream, buf):
        check(self._L.smaml_comm_allreduce(self._h, stream, ptr(buf), buf.numel()))

    def comm_destroy(self):
        check(self._L.smaml_comm_destroy(self._h))

    def timing(self, enable: bool):
        check(self._L.smaml_timing(self._h, 1 if enable else 0))

    def timing_collect(self):
        n = len(TIMING_CATEGORIES)
        ms = (ctypes.c_double * n)()
        fl = (ctypes.c_double * n)()
        cnt = (ctypes.c_int64 * n)()
        check(self._L.smaml_timing_collect(self._h, ms, fl, cnt, n))
        return {name: {"ms": ms[i], "flops": fl[i], "launches": cnt[i]}
                for i, name in enumerate(TIMING_CATEGORIES)}

    def variant_counts(self, reset: bool = False):
        """{variant: launches} since the last reset (host counters, no sync)."""
        n = len(VARIANTS)
        buf = (ctypes.c_int64 * n)()
        cnt = ctypes.c_int32()
        check(self._L.smaml_variant_counts(self._h, buf, n, ctypes.byref(cnt), 1 if reset else 0))
        assert cnt.value == n, (cnt.value, n)
        return {name: int(buf[i]) for i, name in enumerate(VARIANTS)}

    def dropout(self, stream, x, p, seed, layer):
        check(self._L.smaml_dropout(self._h, stream, ptr(x), x.numel(), float(p), int(seed) & 0xFFFFFFFF, int(layer)))

    def set_option(self, key: str, value: int):
        check(self._L.smaml_set_option(self._h, key.encode(), int(value)))

    def adamw_step(self, stream, theta, grad, m, v, step, lr, betas, eps, wd, max_norm, norm_out=None):
        check(self._L.smaml_adamw_step(self._h, stream, ptr(theta), ptr(grad), ptr(m), ptr(v),
                                       theta.numel(), int(step), float(lr), float(betas[0]),
                                       float(betas[1]), float(eps), float(wd), float(max_norm),
                                       ptr(norm_out) if norm_out is not None else None))
