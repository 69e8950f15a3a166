"""smaml_meta_step_base without a device: the ABI's new names, the argument checks that need no device, and the
oracle of the base meta-gradient (tests/base_meta_oracle.py) checked against finite differences and for
discrimination -- the conditions that keep tests/test_gpu_base_meta.py from being vacuous.

Settings of the GPU cases (both at K = 3, two tasks, shapes P and Q of test_gpu_windows.py):
  unclipped  inner_lr 0.1, max_norm 10: every step's clip coefficient is exactly 1;
  clipped    inner_lr 0.5, max_norm 0.01: every step's coefficient is below 1.
At the default inner_lr 0.01 the second-order share of the base gradient is only about 1e-3 of it: too close to
the 1e-4 tolerance to tell the orders apart, so it is not used.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, synth
from weatherforecast_stgcn_maml_amd.config import ModelDims

import base_meta_oracle as bmo
import test_gpu_windows as gw

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {"unclipped": (0.1, 10.0), "clipped": (0.5, 0.01)}
GRAD_TOL = 1e-4
# the GPU cases' tables: every step consecutive, and C S C with query S (test_gpu_windows.TABLES["mixed_a"])
TABLES = {"consec": gw.TABLES["perm_base"], "mixed": gw.TABLES["mixed_a"]}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


_ORACLE = {}


def oracle(tag, table, order, setting, dtype=torch.float64):
    key = (tag, table, order, setting, dtype)
    if key not in _ORACLE:
        d, P, names, ei = gw.model(tag)
        PT = refcpu.to_torch(P)
        Pt, Pg = {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names}
        w = TABLES[table]
        tasks = [refcpu.TaskData(gw.stream(j), ei, d) for j in range(w.shape[1])]
        lr, mn = SETTINGS[setting]
        _ORACLE[key] = bmo.meta_step(Pt, Pg, tasks, w, lr, mn, order, dtype=dtype)
    return _ORACLE[key]


# ----------------------------------------------------------------------------- ABI
def test_header_exports_and_signatures_agree():
    hdr = open(os.path.join(REPO, "include", "smaml.h")).read()
    for name in ("smaml_meta_step_base", "smaml_meta_base_stats"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _capi.EXPORTS and name in _capi._SIGS
        assert hasattr(_capi.lib(), name)
    m = re.search(r"int\s+smaml_meta_step_base\s*\(([^;]*)\);", hdr)
    assert len(m.group(1).split(",")) == len(_capi._SIGS["smaml_meta_step_base"][0]) == 15
    m = re.search(r"int\s+smaml_meta_base_stats\s*\(([^;]*)\);", hdr)
    assert len(m.group(1).split(",")) == len(_capi._SIGS["smaml_meta_base_stats"][0]) == 4
    assert _capi.ABI_VERSION == 9 and _capi.lib().smaml_abi_version() == 9
    assert _capi.VARIANTS[-1] == "fwd_infer_drop"
    assert len(_capi.META_BASE_STATS) == 6


def _call(order, gcn_meta_grad):
    L = _capi.lib()
    w = (ctypes.c_int32 * 4)(0, 1, 2, 3)
    # pointers that are never dereferenced: the checks below fail before a context or a device is needed
    return L.smaml_meta_step_base(None, None, 256, order, 1, 2, w, 0.1, 1.0, 0.5, 512, gcn_meta_grad, None, None, None)


def test_argument_checks_need_no_device():
    L = _capi.lib()
    assert _call(0, 1024) == 1 and b"order" in L.smaml_last_error()  # SMAML_EINVAL
    assert _call(3, 1024) == 1 and b"order" in L.smaml_last_error()
    assert _call(2, None) == 1 and b"gcn_meta_grad" in L.smaml_last_error()
    assert _call(1, 1024 + 4) == 1 and b"gcn_meta_grad" in L.smaml_last_error()  # not 16-byte aligned
    assert _call(2, 1024) == 1 and b"ctx is NULL" in L.smaml_last_error()  # the next check in line
    cnt = ctypes.c_int32()
    assert L.smaml_meta_base_stats(None, None, 0, ctypes.byref(cnt)) == 1


def test_meta_learner_rejects_gcn_dropout_with_train_base():
    import inspect

    from weatherforecast_stgcn_maml_amd import train
    from weatherforecast_stgcn_maml_amd.maml import MetaLearner

    assert inspect.signature(MetaLearner.__init__).parameters["train_base"].default is False
    assert inspect.signature(train.meta_train).parameters["train_base"].default is False
    d, P, names, ei = gw.model("P")
    theta, gcn, _ = gw.split(P)
    with pytest.raises(ValueError, match="GCN dropout"):
        MetaLearner(d, gw.DEFAULT_CFG, gcn, theta, ei, device="cpu", dropout=(0.2, 0.0), train_base=True)


# ----------------------------------------------------------------------------- the oracle itself
def test_oracle_order2_passes_finite_differences():
    """Central differences of the float64 objective along two random directions in (theta, base) at a tiny shape,
    clipped (the clip's derivative is in the gradient) and unclipped, against the order-2 oracle's directional
    derivative. The first-order gradient must miss the same check: the mixed term is in the second-order one."""
    d = ModelDims(num_nodes=9, window_size=2, hidden_channels=8, lstm_hidden_size=8, lstm_num_layers=2)
    P = synth.init_params(91, d, gcn_bias_scale=0.1)
    PT = {k: v.double() for k, v in refcpu.to_torch(P).items()}
    names = refcpu.trainable_names(PT)
    Pt, Pg = {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names}
    ei = gw.grid_edges(d)
    tasks = [refcpu.TaskData(synth.make_features(9100 + j, 9, synth.t_total_for(12, 2, d.forecast_horizon)), ei, d)
             for j in range(2)]
    w = np.asarray([[[0, 1, 2], [3, 4, 5]], [[7, 2, 5], [1, 6, 0]], [[4, 5, 6], [8, 3, 1]]], np.int32)  # K = 2
    gnames = bmo.base_names(Pg)
    rng = np.random.default_rng(3)
    for lr, mn in ((0.5, 10.0), (0.5, 0.05)):
        r2 = bmo.meta_step(Pt, Pg, tasks, w, lr, mn, 2)
        r1 = bmo.meta_step(Pt, Pg, tasks, w, lr, mn, 1)
        coefs = [c for rec in r2["step_records"] for _, _, c in rec]
        assert all(c == 1.0 for c in coefs) if mn == 10.0 else all(c < 1.0 for c in coefs), coefs
        for _ in range(2):
            dt = {k: torch.from_numpy(rng.standard_normal(Pt[k].shape)) for k in names}
            dg = {k: torch.from_numpy(rng.standard_normal(Pg[k].shape)) for k in gnames}
            h = 1e-6
            f = lambda s: bmo.query_objective({k: Pt[k] + s * dt[k] for k in names},  # noqa: E731
                                              {k: Pg[k] + s * dg[k] if k in dg else Pg[k] for k in Pg}, tasks, w, lr, mn)
            fd = (f(h) - f(-h)) / (2 * h)
            ana = lambda r: float(sum((r["meta_grad"][k] * dt[k]).sum() for k in names) +  # noqa: E731
                                  sum((r["gcn_grad"][k] * dg[k]).sum() for k in gnames))
            # the base part alone, too: a wrong base gradient must not hide behind theta's
            fg = lambda s: bmo.query_objective(Pt, {k: Pg[k] + s * dg[k] if k in dg else Pg[k] for k in Pg},  # noqa: E731
                                               tasks, w, lr, mn)
            fdg = (fg(h) - fg(-h)) / (2 * h)
            anag = lambda r: float(sum((r["gcn_grad"][k] * dg[k]).sum() for k in gnames))  # noqa: E731
            print(f"lr {lr} max_norm {mn}: fd {fd:.10e} order2 {ana(r2):.10e} order1 {ana(r1):.10e}; "
                  f"base fd {fdg:.10e} order2 {anag(r2):.10e} order1 {anag(r1):.10e}")
            assert abs(ana(r2) - fd) <= 1e-6 * abs(fd), (ana(r2), fd)
            assert abs(anag(r2) - fdg) <= 1e-6 * abs(fdg), (anag(r2), fdg)
            assert abs(anag(r1) - fdg) > 1e-3 * abs(fdg), (anag(r1), fdg)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_gpu_cases_discriminate(tag, table, setting):
    """In every order-2 GPU case each base tensor's order-1-versus-order-2 difference is at least 10 times the
    gradient tolerance, and the clip engages at every step of the clipped setting and at none of the other."""
    r1, r2 = oracle(tag, table, 1, setting), oracle(tag, table, 2, setting)
    coefs = [c for rec in r2["step_records"] for _, _, c in rec]
    print(tag, table, setting, "coefs", [round(c, 4) for c in coefs])
    if setting == "clipped":
        assert all(c < 1.0 for c in coefs), coefs
    else:
        assert all(c == 1.0 for c in coefs), coefs
    for k in r2["gcn_grad"]:
        share = rel(r1["gcn_grad"][k].numpy(), r2["gcn_grad"][k].numpy())
        print(f"  {k}: order-1 vs order-2 {share:.3e}")
        assert share >= 10 * GRAD_TOL, (k, share)
        assert float(r2["gcn_grad"][k].abs().max()) > 0


def test_float32_oracle_is_close_to_float64():
    r64, r32 = oracle("P", "mixed", 2, "unclipped"), oracle("P", "mixed", 2, "unclipped", torch.float32)
    for k in r64["gcn_grad"]:
        e = rel(r32["gcn_grad"][k].numpy(), r64["gcn_grad"][k].numpy())
        print(k, f"{e:.2e}")
        assert e < 1e-5, (k, e)


def test_theta_part_is_refcpu_meta_step():
    """meta_grad, losses and adapted parameters of the oracle are refcpu.meta_step's (differentiating the base
    changes nothing about theta's gradient)."""
    d, P, names, ei = gw.model("P")
    for order in (1, 2):
        r = oracle("P", "mixed", order, "unclipped", torch.float32)
        ref = _refcpu("P", "mixed", order, "unclipped")
        for k in names:
            assert rel(r["meta_grad"][k].numpy(), ref["meta_grad"][k].numpy()) < 1e-5, (order, k)
        assert np.allclose(r["query_losses"], ref["query_losses"], rtol=1e-5)


def _refcpu(tag, table, order, setting):
    d, P, names, ei = gw.model(tag)
    PT = refcpu.to_torch(P)
    Pt, Pg = {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names}
    w = TABLES[table]
    tasks = [refcpu.TaskData(gw.stream(j), ei, d) for j in range(w.shape[1])]
    lr, mn = SETTINGS[setting]
    return refcpu.meta_step(Pt, Pg, tasks, None, w.shape[0] - 1, gw.B, None, lr, mn, order, windows=w)
