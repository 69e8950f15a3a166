"""Host logic of the lockstep adaptation (``adapt.adapt_many``) on a stub context, and the ABI of its
entry points: no GPU."""
import os
import re

import numpy as np
import pytest
import torch

from weatherforecast_stgcn_maml_amd import _capi, synth
from weatherforecast_stgcn_maml_amd import adapt as A
from weatherforecast_stgcn_maml_amd.config import CONFIG1

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_9_declares_the_lockstep_entry_points():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = set(re.findall(r"\b(smaml_[a-z_0-9]+)\s*\(", txt))
    for name in ("smaml_adapt_steps_multi", "smaml_adapt_prepare_multi"):
        assert name in decl and name in _capi.EXPORTS and name in _capi._SIGS
        assert hasattr(_capi.lib(), name)
    assert _capi.ABI_VERSION == 9 and _capi.lib().smaml_abi_version() == 9
    # the declared parameter count is the binding's
    m = re.search(r"smaml_adapt_steps_multi\s*\((.*?)\);", txt, flags=re.S)
    assert len(m.group(1).split(",")) == len(_capi._SIGS["smaml_adapt_steps_multi"][0]) == 18
    m = re.search(r"smaml_adapt_prepare_multi\s*\((.*?)\);", txt, flags=re.S)
    assert len(m.group(1).split(",")) == len(_capi._SIGS["smaml_adapt_prepare_multi"][0]) == 5


def test_lockstep_groups_by_training_windows():
    assert A.lockstep_groups([16, 8, 16, 960, 8]) == [[0, 2], [1, 4], [3]]
    assert A.lockstep_groups([960] * 18) == [list(range(18))]
    assert A.lockstep_groups([]) == []


def test_check_orders_names_the_region():
    ok = [np.tile(np.arange(16), (3, 1)), np.tile(np.arange(8), (3, 1))]
    out = A.check_orders(ok, [16, 8], 3)
    assert [o.shape for o in out] == [(3, 16), (3, 8)] and all(o.dtype == np.int32 for o in out)
    assert [o.shape for o in A.check_orders(ok, [16, 8], 2)] == [(2, 16), (2, 8)]  # later epochs go unused
    with pytest.raises(ValueError, match=r"orders\[1\] has shape \(3, 8\), expected \(3, 16\)"):
        A.check_orders(ok, [16, 16], 3)
    with pytest.raises(ValueError, match=r"orders\[0\] has shape \(3, 16\), expected \(4, 16\)"):
        A.check_orders(ok, [16, 8], 4)  # too few epochs
    with pytest.raises(ValueError, match="orders has 2 entries for 3 regions"):
        A.check_orders(ok, [16, 8, 8], 3)
    with pytest.raises(ValueError, match=r"orders\[0\]"):
        A.check_orders([[np.arange(16), np.arange(15)], ok[1]], [16, 8], 2)  # ragged


class StubContext:
    """Records what adapt_many asks of the context; every step's loss of task t in epoch e is
    LOSS[t][e] (chosen to drive the schedulers' loss branches apart)."""
    LOSS = {0: [0.5, 0.5, 0.5, 1.5, 0.1], 1: [0.5, 0.5, 0.5, 0.1, 1.5], 2: [0.5, 0.5, 0.5, 0.5, 0.5]}

    def __init__(self, dims):
        self.dims = dims
        self.calls = []
        self.prepared = []
        self.task_ids = None
        self.ntasks = 0
        self.epoch_of = {}

    def set_graph(self, ei):
        pass

    def set_gcn_params(self, flat):
        pass

    def set_tasks(self, feats):
        self.ntasks = len(feats)

    def set_task_ids(self, ids):
        self.task_ids = list(ids)

    def set_dropout(self, p_gcn, p_lstm, seed):
        self.dropout = (p_gcn, p_lstm, seed)

    def adapt_prepare_multi(self, stream, tasks, batch=1):
        self.prepared.append((list(tasks), batch))

    def adapt_steps_multi(self, stream, tasks, theta, m, v, step0, windows, lr_dev, betas, eps, wds, max_norm, losses):
        assert theta.shape == m.shape == v.shape and theta.shape[0] == len(tasks) and theta.is_contiguous()
        assert lr_dev.shape == losses.shape == (windows.shape[0], len(tasks)) and windows.shape[2] == 1
        for i, t in enumerate(tasks):
            e = self.epoch_of.get(t, 0)
            losses[:, i] = self.LOSS[t][e]
            self.epoch_of[t] = e + 1
        theta += 1.0  # (adapted in place: the results must alias the group's rows)
        self.calls.append(dict(tasks=list(tasks), step0=step0, windows=np.array(windows), wds=list(wds),
                               lr=lr_dev.clone().numpy(), betas=betas, eps=eps, max_norm=max_norm))

    def forecast(self, stream, theta, windows, batch, task=0, scale=None, pred=None, skill=None):
        assert scale is None and pred is None
        skill.zero_()
        skill[0] = float(task + 1)  # every (lead, variable) sum
        self.calls.append(dict(forecast=task, windows=list(windows), theta0=float(theta[0])))


@pytest.fixture
def stubbed(monkeypatch):
    monkeypatch.setattr(_capi, "stream_ptr", lambda torch_mod: 0)
    d = CONFIG1
    P = synth.init_params(1, d)
    tr = {k: v for k, v in P.items() if k.startswith(("lstm.", "output_layer."))}
    gcn = {k: v for k, v in P.items() if k.startswith("base_stgcn.conv")}
    # n_max 20, 10, 20 -> 16, 8, 16 training windows
    streams = [synth.make_features(j, d.num_nodes, synth.t_total_for(n)) for j, n in enumerate((20, 10, 20))]
    ei = np.array([[0, 1], [1, 0]])
    return d, tr, gcn, streams, ei


NAMES = ("Thailand", "Moscow", "Delhi")


def test_adapt_many_groups_schedules_and_decays_per_region(stubbed):
    d, tr, gcn, streams, ei = stubbed
    ctx = StubContext(d)
    torch.manual_seed(11)
    want_orders = [[A.random_sampler_order(n).numpy() for _ in range(5)] for n in (16, 8, 16)]
    torch.manual_seed(11)
    res = A.adapt_many(d, streams, ei, gcn, tr, NAMES, epochs=5, device="cpu", ctx=ctx)
    assert ctx.ntasks == 3 and ctx.task_ids == [0, 0, 0]
    assert ctx.prepared == [([0, 2], 1), ([1], 1)]
    steps = [c for c in ctx.calls if "tasks" in c]
    # regions 0 and 2 (16 training windows) in lockstep for all their epochs, then region 1 alone
    assert [c["tasks"] for c in steps] == [[0, 2]] * 5 + [[1]] * 5
    assert [c["step0"] for c in steps] == [0, 16, 32, 48, 64] + [0, 8, 16, 24, 32]
    for e in range(5):
        # shuffle orders: the global RNG's draws region by region, each region's epochs in turn
        np.testing.assert_array_equal(steps[e]["windows"][:, 0, 0], want_orders[0][e])
        np.testing.assert_array_equal(steps[e]["windows"][:, 1, 0], want_orders[2][e])
        np.testing.assert_array_equal(steps[5 + e]["windows"][:, 0, 0], want_orders[1][e])
    # weight decay and learning rate by climate; one scheduler per region stepped on its own epoch mean
    assert steps[0]["wds"] == [1e-5, 1e-4] and steps[5]["wds"] == [5e-5]
    for r, name in enumerate(NAMES):
        lr0, _ = A.climate_optimizer_config(name)
        sched = A.ClimateAwareLRScheduler(name, lr0)
        lrs = [lr0]
        for e in range(4):
            lrs.append(sched.step(StubContext.LOSS[r][e]))
        assert res[r].lrs == lrs and res[r].epoch_losses == pytest.approx(StubContext.LOSS[r], rel=1e-6)
        col = [c for c in steps if r in c["tasks"]]
        for e in range(5):
            got = col[e]["lr"][:, col[e]["tasks"].index(r)]
            assert np.all(got == np.float32(lrs[e])), (r, e)
    # the loss branches really differ between the regions in lockstep (x 1.1 above 1.0, x 0.95 below 0.2)
    # (the climate multiplier enters twice, in the optimiser's lr and in the scheduler: adaptive_scheduler.py)
    assert res[0].lrs[4] / res[2].lrs[4] == pytest.approx(0.9 * 0.9 * 1.1, rel=1e-12)
    # validation: each region's held-out windows on its own task and adapted parameters
    fc = [c for c in ctx.calls if "forecast" in c]
    assert [c["forecast"] for c in fc] == [0, 2, 1]
    assert fc[0]["windows"] == [16, 17, 18, 19] and fc[2]["windows"] == [8, 9]
    per = d.num_nodes * d.forecast_horizon * d.output_channels
    for r, nval in enumerate((4, 2, 4)):
        assert res[r].n_val == nval and res[r].n_train == (16, 8, 16)[r]
        assert res[r].val_loss == pytest.approx((r + 1) * d.forecast_horizon * d.output_channels / (nval * per))
    # the results are the adapted rows (5 epochs of the stub's += 1), not the shared start
    th0 = float(A.params.pack(tr, d, which=0)[0])
    assert all(float(r.theta[0]) == pytest.approx(th0 + 5.0) for r in res)
    assert all(c["theta0"] == pytest.approx(th0 + 5.0) for c in fc)


def test_adapt_many_checks_orders_and_names(stubbed):
    d, tr, gcn, streams, ei = stubbed
    orders = [np.tile(np.arange(16), (2, 1)), np.tile(np.arange(16), (2, 1)), np.tile(np.arange(16), (2, 1))]
    with pytest.raises(ValueError, match=r"orders\[1\] has shape \(2, 16\), expected \(2, 8\)"):
        A.adapt_many(d, streams, ei, gcn, tr, NAMES, epochs=2, device="cpu", ctx=StubContext(d), orders=orders)
    with pytest.raises(ValueError, match="2 region names for 3 streams"):
        A.adapt_many(d, streams, ei, gcn, tr, NAMES[:2], epochs=2, device="cpu", ctx=StubContext(d))
    ctx = StubContext(d)
    orders[1] = np.tile(np.arange(8)[::-1], (2, 1))
    A.adapt_many(d, streams, ei, gcn, tr, NAMES, epochs=2, device="cpu", ctx=ctx, orders=orders)
    alone = [c for c in ctx.calls if c.get("tasks") == [1]]
    assert len(alone) == 2 and list(alone[0]["windows"][:, 0, 0]) == list(range(8))[::-1]
