"""The ABI of ``smaml_adapt_steps_full`` / ``smaml_adapt_full_stats`` and the host logic of
``adapt.adapt(train_base=True)`` on a recording stub context: no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from weatherforecast_stgcn_maml_amd import _capi, params, synth
from weatherforecast_stgcn_maml_amd import adapt as A
from weatherforecast_stgcn_maml_amd.config import CONFIG1

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_bindings_agree():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("smaml_adapt_steps_full", 20), ("smaml_adapt_full_stats", 4)):
        m = re.search(name + r"\s*\((.*?)\);", txt, flags=re.S)
        assert m, f"include/smaml.h does not declare {name}"
        assert name in _capi.EXPORTS and name in _capi._SIGS
        assert hasattr(_capi.lib(), name)
        assert len(m.group(1).split(",")) == len(_capi._SIGS[name][0]) == nargs
    assert hasattr(_capi.Context, "adapt_steps_full") and hasattr(_capi.Context, "adapt_full_stats")
    assert len(_capi.ADAPT_FULL_STATS) == 6
    # two new symbols, the same ABI number and no new kernel-variant counter
    assert _capi.ABI_VERSION == 9 and _capi.lib().smaml_abi_version() == 9
    assert _capi.VARIANTS[-1] == "fwd_infer_drop"


def test_argument_errors_are_rejected_without_a_device():
    L = _capi.lib()
    P = ctypes.c_void_p
    fake = 256  # never dereferenced: every call below fails its argument checks first
    win = (ctypes.c_int32 * 1)(0)

    def call(ctx=None, vecs=(fake,) * 6, step0=0, nsteps=1, batch=1, windows=win, lr=fake, losses=fake, norms=None):
        return L.smaml_adapt_steps_full(ctx, None, *[P(x) if x else None for x in vecs], step0, nsteps, batch, windows,
                                        P(lr) if lr else None, 0.9, 0.999, 1e-8, 1e-4, 1.0,
                                        P(losses) if losses else None, norms)

    def msg():
        return L.smaml_last_error().decode()

    assert call() == 1 and "ctx is NULL" in msg()  # norms may be NULL; everything else is set
    for i in range(6):  # each of the six vectors: NULL, then misaligned
        vecs = [fake] * 6
        vecs[i] = 0
        assert call(vecs=vecs) == 1 and "NULL argument" in msg()
        vecs[i] = fake + 4
        assert call(vecs=vecs) == 1 and "16-byte aligned" in msg()
    assert call(windows=None) == 1 and "NULL argument" in msg()
    assert call(lr=0) == 1 and "NULL argument" in msg()
    assert call(losses=0) == 1 and "NULL argument" in msg()
    for kw in (dict(nsteps=0), dict(batch=0), dict(step0=-1), dict(nsteps=-3)):
        assert call(**kw) == 1 and "must be positive" in msg()
    cnt = ctypes.c_int32()
    assert L.smaml_adapt_full_stats(None, None, 0, ctypes.byref(cnt)) == 1


class StubContext:
    """Records what adapt() asks of the context; every step's loss in epoch e is LOSS[e]."""
    LOSS = [0.5, 1.5, 0.1, 0.1]

    def __init__(self, dims):
        self.dims = dims
        self.calls = []
        self.reserved = []

    def set_graph(self, ei):
        pass

    def set_gcn_params(self, flat):
        self.gcn_set = flat

    def set_tasks(self, feats):
        self.ntasks = len(feats)

    def set_task_ids(self, ids):
        self.task_ids = list(ids)

    def set_dropout(self, p_gcn, p_lstm, seed):
        self.dropout = (p_gcn, p_lstm, seed)

    def reserve(self, tasks, batch):
        self.reserved.append((tasks, batch))

    def adapt_prepare(self, stream, batch=1):
        raise AssertionError("adapt(train_base=True) must not build the frozen base's feature cache")

    def adapt_steps(self, *a, **k):
        raise AssertionError("adapt(train_base=True) must not run frozen-base steps")

    def adapt_steps_full(self, stream, theta, m, v, gcn, gcn_m, gcn_v, step0, windows, lr_dev, betas, eps, wd, max_norm,
                         losses, norms=None):
        assert theta.shape == m.shape == v.shape and gcn.shape == gcn_m.shape == gcn_v.shape
        assert windows.shape == (lr_dev.shape[0], 1) and windows.dtype == np.int32
        losses[:windows.shape[0]] = self.LOSS[len(self.calls)]
        theta += 1.0  # (adapted in place: the results must alias these vectors)
        gcn += 2.0
        gcn_m += 1.0  # (the moments must be carried from epoch to epoch)
        self.calls.append(dict(step0=step0, windows=np.array(windows), lr=lr_dev.clone().numpy(), wd=wd, betas=betas,
                               eps=eps, max_norm=max_norm, ids=(theta.data_ptr(), m.data_ptr(), v.data_ptr(),
                                                                gcn.data_ptr(), gcn_m.data_ptr(), gcn_v.data_ptr()),
                               gm0=float(gcn_m[0]), dropout=self.dropout))

    def meta_step(self, stream, theta, order, steps, batch, windows, inner_lr, max_norm, query_scale, losses=None, **kw):
        assert order == 0 and steps == 0
        losses.fill_(0.25)
        self.calls.append(dict(validate=np.array(windows).reshape(-1).tolist(), theta0=float(theta[0])))


def test_adapt_train_base_drives_the_full_entry_point(monkeypatch):
    monkeypatch.setattr(_capi, "stream_ptr", lambda torch_mod: 0)
    d = CONFIG1
    P = synth.init_params(1, d)
    tr = {k: v for k, v in P.items() if k.startswith(("lstm.", "output_layer."))}
    gcn = {k: v for k, v in P.items() if k.startswith("base_stgcn.conv")}
    feats = synth.make_features(0, d.num_nodes, synth.t_total_for(20))  # n_max 20 -> 16 training windows
    ctx = StubContext(d)
    torch.manual_seed(11)
    want_orders = [A.random_sampler_order(16).numpy() for _ in range(4)]
    torch.manual_seed(11)
    res = A.adapt(d, feats, np.array([[0, 1], [1, 0]]), gcn, tr, "Moscow", epochs=4, device="cpu", ctx=ctx,
                  dropout=(0.2, 0.1), dropout_seed=9, train_base=True)
    assert ctx.reserved == [(1, 1)] and ctx.ntasks == 1 and ctx.task_ids == [0]
    steps = [c for c in ctx.calls if "step0" in c]
    assert len(steps) == 4 and [c["step0"] for c in steps] == [0, 16, 32, 48]
    lr0, wd = A.climate_optimizer_config("Moscow")
    sched = A.ClimateAwareLRScheduler("Moscow", lr0)
    lrs = [lr0] + [sched.step(StubContext.LOSS[e]) for e in range(3)]
    for e, c in enumerate(steps):
        np.testing.assert_array_equal(c["windows"][:, 0], want_orders[e])
        assert np.all(c["lr"] == np.float32(lrs[e])) and c["lr"].shape == (16,)
        assert c["wd"] == wd and c["betas"] == (0.9, 0.999) and c["eps"] == 1e-8 and c["max_norm"] == 1.0
        assert c["ids"] == steps[0]["ids"] and len(set(c["ids"])) == 6  # one set of vectors for the whole run
        assert c["gm0"] == e + 1.0 and c["dropout"] == (0.2, 0.1, 9)
    assert res.lrs == lrs and res.epoch_losses == pytest.approx(StubContext.LOSS, rel=1e-6)
    # the results are the adapted vectors; the validation ran on them, in eval mode, after the last epoch
    th0 = float(params.pack(tr, d, which=0)[0])
    g0 = float(params.pack(gcn, d, which=1)[0])
    assert float(res.theta[0]) == pytest.approx(th0 + 4.0) and float(res.gcn[0]) == pytest.approx(g0 + 8.0)
    assert res.gcn is ctx.gcn_set and res.gcn.data_ptr() == steps[0]["ids"][3]
    assert set(params.unpack(res.gcn, d, 1)) == set(gcn)
    val = ctx.calls[-1]
    assert val["validate"] == [16, 17, 18, 19] and val["theta0"] == pytest.approx(th0 + 4.0)
    assert ctx.dropout == (0.0, 0.0, 0) and res.val_loss == pytest.approx(0.25)
    assert res.n_train == 16 and res.n_val == 4


def test_adapt_default_path_is_untouched(monkeypatch):
    """train_base defaults to False: the frozen-base calls, no GCN vector in the result."""
    monkeypatch.setattr(_capi, "stream_ptr", lambda torch_mod: 0)
    d = CONFIG1
    P = synth.init_params(1, d)
    tr = {k: v for k, v in P.items() if k.startswith(("lstm.", "output_layer."))}
    gcn = {k: v for k, v in P.items() if k.startswith("base_stgcn.conv")}
    feats = synth.make_features(0, d.num_nodes, synth.t_total_for(20))

    class Frozen(StubContext):
        def adapt_prepare(self, stream, batch=1):
            self.calls.append(dict(prepare=batch))

        def adapt_steps(self, stream, theta, m, v, step0, windows, lr_dev, betas, eps, wd, max_norm, losses):
            losses[:windows.shape[0]] = 0.5
            self.calls.append(dict(frozen=step0))

        def adapt_steps_full(self, *a, **k):
            raise AssertionError("the default path must not train the base")

    ctx = Frozen(d)
    res = A.adapt(d, feats, np.array([[0, 1], [1, 0]]), gcn, tr, "Delhi", epochs=2, device="cpu", ctx=ctx)
    assert [c for c in ctx.calls if "validate" not in c] == [dict(prepare=1), dict(frozen=0), dict(frozen=16)]
    assert ctx.reserved == [] and res.gcn is None
