"""Whole-model regional adaptation (``smaml_adapt_steps_full``, ``adapt(train_base=True)``): the GCN base trained
inside the adapt step, against the CPU oracle.

The oracle is composed here from unchanged ``oracle/refcpu.py`` functions, as test_gpu_base_grad.py does:
``stgcn_features`` OUTSIDE ``no_grad``, ``batched_forward``, ``mse``, ``refcpu.Dropout(seed, p, p, 0, step)``, then
``torch.nn.utils.clip_grad_norm_`` over ALL leaves and one ``torch.optim.Adam(all leaves, lr, weight_decay)``.

Tolerances, per tensor, relative L2: adapted parameters of both layouts, per-step losses and norms 1e-5 (the
project's); the UPDATE (adapted - initial) of every tensor 1e-3 -- 50 x the f32 / f64 sensitivity of this
composition measured on the CPU (<= 2e-5), where a wrong or missing conv gradient gives O(1). Every graph is the
5 x 5 grid (N = 25) except the config-4 case.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, params, synth
from weatherforecast_stgcn_maml_amd.adapt import adapt, climate_optimizer_config
from weatherforecast_stgcn_maml_amd.config import CONFIG1, CONFIG2, ModelDims

from test_gpu_parity import DEV, grid_edges, rel

pytestmark = pytest.mark.gpu

SEED = 4711
LR, WD = 6e-4, 1e-4
STEP0 = 5  # the Adam step and the dropout step of the call's first step: a later call of a run


def _dims(T, Cin, Hc, H, L, Hf=2, C=2, N=25):
    return ModelDims(num_nodes=N, window_size=T, input_channels=Cin, hidden_channels=Hc, lstm_hidden_size=H,
                     lstm_num_layers=L, forecast_horizon=Hf, output_channels=C)


# name -> (dims, batch, dropout p, steps, max_norm): each the smallest shape that reaches its edge
CASES = {
    "cfg1": (CONFIG1, 1, 0.0, 8, 1.0),
    # the fused keeping kernel: 50 rows t >= 1 = one workgroup, a partial wave and two empty waves
    "hc256_t3": (_dims(3, 8, 256, 32, 2), 1, 0.0, 8, 1.0),
    # two workgroups (128 + 22 rows per sample), sample indexing, masks stored into h[k]
    "hc256_t7_b2": (_dims(7, 8, 256, 32, 2), 2, 0.2, 8, 1.0),
    # 225 rows x Hc = 48: partial row and column tiles of k_gcn_dz, K = 48; per-layer keep
    "hc48_b3": (_dims(3, 8, 48, 32, 1), 3, 0.0, 12, 1.0),
    "hc48_b3_clip": (_dims(3, 8, 48, 32, 1), 3, 0.0, 12, 0.05),
    # T = 1: every row aggregates over the graph, k_gcn_dz's epilogue masks nothing
    "t1_hc16": (_dims(1, 4, 16, 64, 2, Hf=1, C=4), 2, 0.0, 8, 1.0),
    # config-4 shapes: the real grids (83 workgroups of the keeping kernel, 166 x 2 tiles of k_gcn_dz)
    "cfg4": (CONFIG2, 1, 0.0, 4, 1.0),
}
FUSED_KEEP = {"hc256_t3", "hc256_t7_b2", "cfg4"}
N_WINDOWS = 9  # distinct window starts of every case's stream


def split_names(P):
    tr = [k for k in P if k.startswith(("lstm.", "output_layer."))]
    gc = [k for k in P if k.startswith("base_stgcn.conv")]
    return tr, gc


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    d, B, p, steps, max_norm = CASES[name]
    P = synth.init_params(21, d, gcn_bias_scale=0.1)
    t_total = N_WINDOWS + d.window_size + d.forecast_horizon
    feats = np.ascontiguousarray(synth.make_features(3100, d.num_nodes, t_total)[:, :, :d.input_channels])
    rng = np.random.default_rng(5)
    windows = rng.integers(0, N_WINDOWS - 1, size=(steps, B)).astype(np.int32)  # repeated and scattered
    windows[1] = windows[0]
    lrs = (LR * (1.0 - 0.03 * np.arange(steps))).astype(np.float32)
    return d, B, p, steps, max_norm, P, feats, grid_edges(d), windows, lrs


def _adam_with_step0(leaves, lr, wd, step0):
    """Adam whose first step() is step step0 + 1 with zero moments (what the library computes for step0 > 0)."""
    opt = torch.optim.Adam(leaves, lr=lr, weight_decay=wd)
    for q in leaves:
        opt.state[q] = {"step": torch.tensor(float(step0)), "exp_avg": torch.zeros_like(q),
                        "exp_avg_sq": torch.zeros_like(q)}
    return opt


def oracle_steps(d, B, p, P, feats, ei, windows, lrs, max_norm, wd=WD, step0=STEP0):
    tr, gc = split_names(P)
    Pt = {k: v.clone() for k, v in refcpu.to_torch(P).items()}
    names = tr + gc
    for k in names:
        Pt[k].requires_grad_(True)
    leaves = [Pt[k] for k in names]
    task = refcpu.TaskData(feats, ei, d)
    opt = _adam_with_step0(leaves, float(lrs[0]), wd, step0)
    losses, norms, tnorms = [], [], []
    for k in range(len(windows)):
        for pg in opt.param_groups:
            pg["lr"] = float(lrs[k])
        opt.zero_grad()
        drop = refcpu.Dropout(SEED, p, p, 0, step0 + k) if p > 0 else None
        fs = [refcpu.stgcn_features(task.xy(int(i))[0], task.edge_index, Pt, drop, b, B)
              for b, i in enumerate(windows[k])]
        preds = refcpu.batched_forward(Pt, fs, d, drop)
        loss = torch.stack([refcpu.mse(q, task.xy(int(i))[1]) for q, i in zip(preds, windows[k])]).mean()
        loss.backward()
        tnorms.append(float(torch.stack([Pt[n].grad.norm(2) for n in tr]).norm(2)))
        norms.append(float(torch.nn.utils.clip_grad_norm_(leaves, max_norm)))
        opt.step()
        losses.append(float(loss.detach()))
    return {k: v.detach().numpy() for k, v in Pt.items()}, np.array(losses), np.array(norms), np.array(tnorms)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    d, B, p, steps, max_norm, P, feats, ei, windows, lrs = case_inputs(name)
    return oracle_steps(d, B, p, P, feats, ei, windows, lrs, max_norm)


class Run:
    """A context with the case's graph, stream and start vectors on the device."""

    def __init__(self, name, options=()):
        self.d, self.B, self.p, self.steps, self.max_norm, self.P, feats, ei, self.windows, lrs = case_inputs(name)
        d = self.d
        self.tr, self.gc = split_names(self.P)
        self.ctx = _capi.Context(d, 0)
        for k, v in options:
            self.ctx.set_option(k, v)
        self.ctx.set_graph(ei)
        self.stream_t = torch.from_numpy(feats).to(DEV)
        self.ctx.set_tasks([self.stream_t])
        self.ctx.set_task_ids([0])
        self.ctx.set_dropout(self.p, self.p, SEED)
        self.theta = params.pack({k: torch.from_numpy(self.P[k]) for k in self.tr}, d, device=DEV)
        self.gcn = params.pack({k: torch.from_numpy(self.P[k]) for k in self.gc}, d, which=1, device=DEV)
        self.m, self.v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
        self.gm, self.gv = torch.zeros_like(self.gcn), torch.zeros_like(self.gcn)
        self.lr_dev = torch.from_numpy(lrs).to(DEV)
        self.losses = torch.full((self.steps,), float("nan"), device=DEV)
        self.norms = torch.full((self.steps,), float("nan"), device=DEV)
        self.st = _capi.stream_ptr(torch)

    def full(self, windows=None, norms=True, step0=STEP0):
        w = self.windows if windows is None else windows
        self.ctx.adapt_steps_full(self.st, self.theta, self.m, self.v, self.gcn, self.gm, self.gv, step0, w,
                                  self.lr_dev, (0.9, 0.999), 1e-8, WD, self.max_norm, self.losses,
                                  self.norms if norms else None)
        torch.cuda.synchronize()
        return self

    def state(self):
        return [t.clone() for t in (self.theta, self.m, self.v, self.gcn, self.gm, self.gv, self.losses, self.norms)]

    def tensors(self):
        got = dict(params.unpack(self.theta, self.d, 0))
        got.update(params.unpack(self.gcn, self.d, 1))
        return {k: v.cpu().numpy() for k, v in got.items()}


def check_against_oracle(name, r, tag=""):
    ref, ref_losses, ref_norms, _ = case_oracle(name)
    e = rel(r.losses.cpu(), ref_losses)
    print(f"{name}{tag} losses rel {e:.3e}")
    assert e < 1e-5, e
    e = rel(r.norms.cpu(), ref_norms)
    print(f"{name}{tag} norms rel {e:.3e}")
    assert e < 1e-5, e
    got = r.tensors()
    assert set(got) == set(r.tr) | set(r.gc)
    for k, a in got.items():
        e = rel(a, ref[k])
        eu = rel(a.astype(np.float64) - r.P[k], ref[k].astype(np.float64) - r.P[k])
        print(f"{name}{tag} {k} rel {e:.3e} update rel {eu:.3e}")
        assert e < 1e-5, (k, e)
        assert eu < 1e-3, (k, eu)


def expected_stats(name, steps, keep=1, dz_fused=0):
    fused = name in FUSED_KEEP
    return {"steps": steps,
            "gcn_keep_fused": steps if keep and fused else 0,
            "gcn_keep_layer": 4 * steps if keep and not fused else 0,
            "gcn_dz_fused": 3 * steps if dz_fused else 0,
            "gcn_dz_composed": 0 if dz_fused else 9 * steps,
            "gcn_recompute": 0 if keep else 3 * steps}


def test_the_oracle_trains_the_base_and_clips_jointly():
    """Conditions on the oracle itself, so that the comparisons below cannot pass vacuously."""
    worst = 0.0
    for name in CASES:
        if name == "cfg4":
            continue
        d, B, p, steps, max_norm, P, *_ = case_inputs(name)
        ref, _, norms, tnorms = case_oracle(name)
        for k in split_names(P)[1]:
            moved = rel(ref[k], P[k])
            assert moved > 1e-3, (name, k, moved)
        worst = max(worst, float(np.max(np.abs(norms - tnorms) / norms)))
    print(f"largest joint vs trainable-only norm difference {worst:.3f}")
    assert worst > 0.01
    assert np.min(case_oracle("hc48_b3_clip")[2]) > CASES["hc48_b3_clip"][4]  # the clip case clips at every step


@pytest.mark.parametrize("name", list(CASES))
def test_adapt_steps_full_matches_oracle(name):
    r = Run(name).full()
    check_against_oracle(name, r)
    st = r.ctx.adapt_full_stats()
    assert st == expected_stats(name, r.steps), st
    # the pads of both layouts and of all moments are zero
    for which, vecs in ((0, (r.theta, r.m, r.v)), (1, (r.gcn, r.gm, r.gv))):
        used = torch.zeros_like(vecs[0], dtype=torch.bool)
        lay = params.gcn_layout(r.d)[0] if which else params.trainable_layout(r.d)[0]
        for _, shape, off in lay:
            used[off:off + int(np.prod(shape))] = True
        for t in vecs:
            assert float(t[~used].abs().sum()) == 0.0
    if name == "cfg1":  # the forecast after the call sees the adapted base
        ref, *_ = case_oracle(name)
        d = r.d
        Pt = {k: torch.from_numpy(v) for k, v in ref.items()}
        task = refcpu.TaskData(r.stream_t.cpu().numpy(), grid_edges(d), d)
        wins = [0, 3, 7]
        with torch.no_grad():
            fs = [refcpu.stgcn_features(task.xy(i)[0], task.edge_index, Pt) for i in wins]
            want = torch.stack(refcpu.batched_forward(Pt, fs, d)).numpy()
        r.ctx.set_dropout(0.0, 0.0, 0)
        pred = torch.empty(len(wins), d.num_nodes * d.forecast_horizon, d.output_channels, device=DEV)
        r.ctx.forecast(r.st, r.theta, wins, 2, pred=pred)
        torch.cuda.synchronize()
        e = rel(pred.cpu(), want)
        print(f"forecast after the call rel {e:.3e}")
        assert e < 1e-5


@pytest.mark.parametrize("name", ["hc256_t7_b2", "hc48_b3", "t1_hc16", "cfg4"])
def test_repeatable_and_dz_arms_bitwise(name):
    """Two runs from the same start agree bitwise; so does the fused layer-to-layer gradient (gcn_dz_fused = 1:
    k_gcn_dz, one GEMM with the mask in its epilogue plus the gather over the t = 0 rows) against the default's
    GEMM + gather + mask over all rows."""
    a = Run(name).full().state()
    b = Run(name).full().state()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    r = Run(name, (("gcn_dz_fused", 1),)).full()
    assert r.ctx.adapt_full_stats() == expected_stats(name, r.steps, dz_fused=1)
    assert all(torch.equal(x, y) for x, y in zip(a, r.state()))


@pytest.mark.parametrize("name", ["hc256_t7_b2", "hc48_b3"])
def test_recompute_arm_stays_within_tolerance(name):
    """gcn_keep = 0: the frozen-base forward plus smaml_backward_base's recompute of conv1..conv3."""
    r = Run(name, (("gcn_keep", 0),)).full()
    assert r.ctx.adapt_full_stats() == expected_stats(name, r.steps, keep=0)
    check_against_oracle(name, r, " gcn_keep=0")


@pytest.mark.parametrize("name", ["cfg1", "hc256_t3"])
def test_first_loss_is_the_frozen_step_s_and_the_cache_follows_the_base(name):
    """From equal starts the first step's loss is smaml_adapt_steps's, bitwise (the same forward kernels); after a
    full call smaml_adapt_steps recomputes its feature cache from the adapted base."""
    r = Run(name).full()
    f = Run(name)
    f.ctx.set_gcn_params(f.gcn)
    w1 = f.windows[:1]
    loss = torch.empty(1, device=DEV)
    f.ctx.adapt_steps(f.st, f.theta, f.m, f.v, STEP0, w1, f.lr_dev, (0.9, 0.999), 1e-8, WD, f.max_norm, loss)
    torch.cuda.synchronize()
    assert torch.equal(loss[0], r.losses[0])
    # fill the frozen path's cache at the start parameters, train the base, then a frozen step again
    g = Run(name)
    g.ctx.set_gcn_params(g.gcn)
    scratch = [g.theta.clone(), g.m.clone(), g.v.clone(), torch.empty(2, device=DEV)]
    g.ctx.adapt_steps(g.st, scratch[0], scratch[1], scratch[2], 0, g.windows[:2], g.lr_dev, (0.9, 0.999), 1e-8, WD,
                      g.max_norm, scratch[3])
    g.full()
    g.ctx.adapt_steps(g.st, g.theta, g.m, g.v, STEP0 + g.steps, w1, g.lr_dev, (0.9, 0.999), 1e-8, WD, g.max_norm, loss)
    torch.cuda.synchronize()
    ref, *_ = case_oracle(name)
    d = g.d
    Pt = {k: torch.from_numpy(v) for k, v in ref.items()}
    task = refcpu.TaskData(g.stream_t.cpu().numpy(), grid_edges(d), d)
    with torch.no_grad():
        i = int(w1[0, 0])
        want = float(refcpu.mse(refcpu.batched_forward(
            Pt, [refcpu.stgcn_features(task.xy(i)[0], task.edge_index, Pt)], d)[0], task.xy(i)[1]))
    assert abs(float(loss[0]) - want) < 1e-5 * want, (float(loss[0]), want)


@pytest.mark.parametrize("name", ["cfg1", "hc256_t3"])
def test_two_segment_update_is_bitwise_the_one_segment_update(name):
    """With max_norm = 1e30 the clip coefficient is exactly 1 whether the norm is the trainable vector's or the
    joint one, so one step from equal starts on the same window leaves theta, m and v bitwise equal: the R = 1,
    S = 2 clip + Adam launch (smaml_adapt_steps_full) against the R = 1, S = 1 launch (smaml_adapt_steps). The
    base itself has moved."""
    r, f = Run(name), Run(name)
    r.max_norm = 1e30
    r.full(windows=r.windows[:1])
    f.ctx.set_gcn_params(f.gcn)
    loss = torch.empty(1, device=DEV)
    f.ctx.adapt_steps(f.st, f.theta, f.m, f.v, STEP0, f.windows[:1], f.lr_dev, (0.9, 0.999), 1e-8, WD, 1e30, loss)
    torch.cuda.synchronize()
    assert torch.equal(loss[0], r.losses[0])
    for a, b in ((r.theta, f.theta), (r.m, f.m), (r.v, f.v)):
        assert torch.equal(a, b)
    assert float(r.m.abs().sum()) > 0.0  # the step did run
    assert not torch.equal(r.gcn, f.gcn)
    assert float(f.gm.abs().sum()) == 0.0 and float(r.gm.abs().sum()) > 0.0


def test_workspace_is_not_grown_and_errors_leave_the_vectors():
    name = "hc48_b3"
    r = Run(name)
    r.ctx.reserve(1, r.B)
    ws = r.ctx.workspace_bytes()
    r.full()
    assert r.ctx.workspace_bytes() == ws
    r.full(norms=False)  # norms may be NULL
    before = r.state()
    bad = r.windows.copy()
    bad[-1, -1] = N_WINDOWS  # the last start whose target rows run past the stream
    with pytest.raises(_capi.SmamlError, match="EINVAL"):
        r.full(windows=bad)
    with pytest.raises(_capi.SmamlError, match="EINVAL"):
        r.full(step0=-1)
    with pytest.raises(_capi.SmamlError, match="EINVAL"):  # a misaligned GCN vector
        r.ctx.adapt_steps_full(r.st, r.theta, r.m, r.v, r.gcn[1:], r.gm, r.gv, 0, r.windows, r.lr_dev, (0.9, 0.999),
                               1e-8, WD, 1.0, r.losses)
    no_tasks = _capi.Context(r.d, 0)
    no_tasks.set_graph(grid_edges(r.d))
    with pytest.raises(_capi.SmamlError, match="ESTATE"):
        no_tasks.adapt_steps_full(r.st, r.theta, r.m, r.v, r.gcn, r.gm, r.gv, 0, r.windows, r.lr_dev, (0.9, 0.999),
                                  1e-8, WD, 1.0, r.losses)
    odd = _capi.Context(_dims(3, 8, 40, 32, 1), 0)  # hidden_channels % 16: the LSTM path's dims check
    odd.set_graph(grid_edges(r.d))
    odd.set_tasks([r.stream_t])
    with pytest.raises(_capi.SmamlError, match="EINVAL"):
        odd.adapt_steps_full(r.st, r.theta, r.m, r.v, r.gcn, r.gm, r.gv, 0, r.windows, r.lr_dev, (0.9, 0.999),
                             1e-8, WD, 1.0, r.losses)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, r.state()))


def test_adapt_train_base_matches_the_oracle_loop():
    """adapt(train_base=True) over 2 epochs against the same oracle loop: learning rates, epoch losses, adapted
    parameters of both layouts, validation loss on the adapted base."""
    d = CONFIG1
    region = "Delhi"
    P = synth.init_params(21, d, gcn_bias_scale=0.1)
    tr, gc = split_names(P)
    ei = grid_edges(d)
    feats = synth.make_features(3100, d.num_nodes, synth.t_total_for(20))
    rng = np.random.default_rng(3)
    orders = [rng.permutation(16).astype(np.int32) for _ in range(2)]
    res = adapt(d, feats, ei, {k: P[k] for k in gc}, {k: P[k] for k in tr}, region, epochs=2, device=DEV,
                orders=orders, train_base=True)
    assert res.n_train == 16 and res.n_val == 4 and res.gcn is not None
    lr0, wd = climate_optimizer_config(region)
    lrs, epoch_losses = [lr0], []
    Pn = P
    # the oracle loop epoch by epoch: Adam's state carried by hand (moments and step count)
    Pt = {k: v.clone() for k, v in refcpu.to_torch(P).items()}
    names = tr + gc
    for k in names:
        Pt[k].requires_grad_(True)
    leaves = [Pt[k] for k in names]
    opt = torch.optim.Adam(leaves, lr=lr0, weight_decay=wd)
    task = refcpu.TaskData(feats, ei, d)
    for ep in range(2):
        for pg in opt.param_groups:
            pg["lr"] = lrs[ep]
        ls = []
        for i in orders[ep]:
            opt.zero_grad()
            f = refcpu.stgcn_features(task.xy(int(i))[0], task.edge_index, Pt)
            loss = refcpu.mse(refcpu.batched_forward(Pt, [f], d)[0], task.xy(int(i))[1])
            loss.backward()
            torch.nn.utils.clip_grad_norm_(leaves, 1.0)
            opt.step()
            ls.append(float(loss.detach()))
        epoch_losses.append(sum(ls) / len(ls))
        lrs.append(refcpu.climate_lr(region, ep + 1, lr0, epoch_losses[-1]))
    with torch.no_grad():
        vals = []
        for i in range(16, 20):
            f = refcpu.stgcn_features(task.xy(i)[0], task.edge_index, Pt)
            vals.append(float(refcpu.mse(refcpu.batched_forward(Pt, [f], d)[0], task.xy(i)[1])))
    ref_val = sum(vals) / len(vals)
    np.testing.assert_allclose(res.lrs, lrs[:2], rtol=1e-12)
    assert rel(res.epoch_losses, epoch_losses) < 1e-5
    got = dict(params.unpack(res.theta, d, 0))
    got.update(params.unpack(res.gcn, d, 1))
    for k in names:
        e = rel(got[k].cpu().numpy(), Pt[k].detach().numpy())
        assert e < 1e-5, (k, e)
        assert rel(got[k].cpu().numpy(), Pn[k]) > 1e-4, k  # it moved
    assert abs(res.val_loss - ref_val) < 1e-5 * ref_val, (res.val_loss, ref_val)
