"""GPU tests of the weighted training loss (``smaml_set_loss_weights``) and the node-weighted forecast scores
(``smaml_set_score_weights``) through every consumer, against the CPU oracle of tests/weighted_loss_oracle.py.

Shapes are the smallest that reach each kernel: P (N = 49, T = 3, Hc = 16, H = 32, L = 2; B = 6: 294 rows, the SIMT
head ``k_head_loss_small``), M (the same with L = 1 and B = 42: 2,058 rows, above SMAML_HEAD_SMALL_M = 2,048, so the
MFMA head ``k_head_loss`` with 17 row tiles, the last partial), A (N = 25, T = 3, H = 32, L = 2: the adapt paths) and
CONFIG1 (N = 25, H = 32: the four score calls). Tables are ``draw_tables``'s: per task one separable and one random
table from [0.25, 4] with about 10 % zeros, scaled to mean 1. Tolerances are the project's (test_gpu_parity.py):
per-step losses and adapted parameters 1e-5 rel-L2, query loss and meta-gradient 1e-4, predictions and score sums
1e-5. tests/test_weighted_loss_cpu.py shows the float32 oracle itself within a tenth of each.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast, params, synth
from weatherforecast_stgcn_maml_amd import adapt as A
from weatherforecast_stgcn_maml_amd.config import CONFIG1, MamlConfig, ModelDims
from weatherforecast_stgcn_maml_amd.maml import MetaLearner

import weighted_loss_oracle as wlo
from test_gpu_forecast import SCALE, case
from test_gpu_parity import DEV, build_hybrid, grid_edges, rel, split

pytestmark = pytest.mark.gpu

P_DIMS = ModelDims(num_nodes=49, window_size=3, hidden_channels=16, lstm_hidden_size=32, lstm_num_layers=2)
M_DIMS = ModelDims(num_nodes=49, window_size=3, hidden_channels=16, lstm_hidden_size=32, lstm_num_layers=1)
A_DIMS = ModelDims(num_nodes=25, window_size=3, hidden_channels=16, lstm_hidden_size=32, lstm_num_layers=2)
B, T, HF, C = 6, 3, P_DIMS.forecast_horizon, P_DIMS.output_channels
NWIN = 40  # windows per stream of shape P
LAST = NWIN - 1


def run6(w0):
    return list(range(w0, w0 + B))


# K = 2, 2 tasks: a consecutive step, a scattered one, and query batches that end at the last window / start at 0
P_TABLE = np.asarray([[run6(4), run6(20)], [[17, 3, 39, 8, 22, 11], [31, 5, 14, 26, 2, 19]],
                      [run6(LAST - B + 1), run6(0)]], np.int32)


@functools.lru_cache(maxsize=None)
def p_case():
    d = P_DIMS
    P = synth.init_params(301, d, gcn_bias_scale=0.1)
    feats = [synth.make_features(8300 + j, d.num_nodes, synth.t_total_for(NWIN, T, HF)) for j in range(2)]
    return d, P, grid_edges(d), feats, [wlo.draw_tables(d, 500)[0], wlo.draw_tables(d, 501)[1]]


def torch_params(P):
    PT = refcpu.to_torch(P)
    names = refcpu.trainable_names(PT)
    return {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names}, names


def learner(d, P, ei, feats, K, batch, order, tables=None, dropout=(0.0, 0.0), seed=0):
    theta, gcn, _ = split(P)
    ml = MetaLearner(d, MamlConfig(inner_steps=K, batch=batch, order=order), gcn, theta, ei, device=DEV, task_group=None,
                     dropout=dropout, dropout_seed=seed)
    ml.set_tasks(feats, loss_weights=tables)
    return ml


def outputs(ml, w):
    fast = torch.zeros(w.shape[1], ml.theta.numel(), device=DEV)
    res = ml.meta_step(windows=w, fast_out=fast)
    torch.cuda.synchronize()
    return (res.losses.cpu().numpy(), res.norms.cpu().numpy(), ml.meta_grad.cpu().numpy().copy(), fast.cpu().numpy())


def check_meta(label, out, ref, d, names, order):
    """The project's tolerances; prints each figure before it asserts."""
    losses, _, mg, fast = out
    K, Z = losses.shape[0] - 1, losses.shape[1]
    for a in out:
        assert np.isfinite(a).all(), label
    e_step = max(rel(losses[:K, j], [r[0] for r in ref["step_records"][j]]) for j in range(Z)) if K else 0.0
    e_query = max(abs(losses[-1, j] - ref["query_losses"][j]) / ref["query_losses"][j] for j in range(Z))
    e_ad = max(rel(params.unpack(torch.from_numpy(fast[j]), d, 0)[k].numpy(), ref["adapted"][j][k].numpy())
               for j in range(Z) for k in names)
    e_mg = 0.0
    if order >= 1:
        got = params.unpack(torch.from_numpy(mg), d, 0)
        e_mg = max(rel(got[k].numpy(), ref["meta_grad"][k].numpy()) for k in names)
    print(f"ERR {label}: step losses {e_step:.3g} (1e-5), adapted {e_ad:.3g} (1e-5), query {e_query:.3g} (1e-4), "
          f"meta-gradient {e_mg:.3g} (1e-4)")
    assert e_step < 1e-5 and e_ad < 1e-5 and e_query < 1e-4 and e_mg < 1e-4


# ----------------------------------------------------------------------------- 1. ones are bitwise
def test_all_ones_tables_are_bitwise_the_unweighted_meta_step():
    d, P, ei, feats, _ = p_case()
    ones = np.ones((HF * d.num_nodes, C), np.float32)
    outs = []
    for tables in (None, ones, [ones, ones]):
        ml = learner(d, P, ei, feats, 2, B, 2, tables)
        outs.append(outputs(ml, P_TABLE))
        st = ml.ctx.loss_stats()
        assert st["loss_sets"] == (0 if tables is None else 1 if tables is ones else 2)
        assert (st["head_loss_small"] > 0 and st["head_dual"] > 0) == (tables is not None), st
    for other in outs[1:]:
        for name, a, b in zip(("losses", "norms", "meta_grad", "fast_out"), outs[0], other):
            assert np.array_equal(a, b), name
    assert np.isfinite(outs[0][2]).all() and np.abs(outs[0][2]).max() > 0


def adapt_ctx(d, P, ei, streams):
    theta, gcn, _ = split(P)
    ctx = _capi.Context(d, 0)
    ctx.set_graph(ei)
    gflat = params.pack({k: torch.from_numpy(v) for k, v in gcn.items() if k.startswith("base_stgcn.conv")}, d, which=1,
                        device=DEV)
    ctx.set_gcn_params(gflat)
    ts = [torch.from_numpy(np.ascontiguousarray(f)).to(DEV) for f in streams]
    ctx.set_tasks(ts)
    ctx.set_task_ids([0] * len(ts))
    th = params.pack({k: torch.from_numpy(v) for k, v in theta.items()}, d, device=DEV)
    return ctx, th, gflat, ts


ADAPT_LRS = np.asarray([6e-4, 5e-4, 4e-4], np.float32)
WD = 1e-4


def run_adapt_steps(ctx, th0, windows, lrs=ADAPT_LRS):
    th = th0.clone()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    losses = torch.zeros(len(windows), device=DEV)
    ctx.adapt_steps(_capi.stream_ptr(torch), th, m, v, 0, np.asarray(windows, np.int32), torch.from_numpy(lrs).to(DEV),
                    (0.9, 0.999), 1e-8, WD, 1.0, losses)
    torch.cuda.synchronize()
    return th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), losses.cpu().numpy()


@functools.lru_cache(maxsize=None)
def a_case():
    d = A_DIMS
    P = synth.init_params(302, d, gcn_bias_scale=0.1)
    feats = [synth.make_features(8400 + j, d.num_nodes, synth.t_total_for(10, T, HF)) for j in range(2)]
    return d, P, grid_edges(d), feats, [wlo.draw_tables(d, 510)[0], wlo.draw_tables(d, 511)[1]]


def test_all_ones_table_is_bitwise_the_unweighted_adapt_steps():
    d, P, ei, feats, _ = a_case()
    ctx, th, _, _ = adapt_ctx(d, P, ei, feats[:1])
    windows = [[3], [0], [7]]
    plain = run_adapt_steps(ctx, th, windows)
    ctx.set_loss_weights(np.ones((HF * d.num_nodes, C), np.float32))
    ones = run_adapt_steps(ctx, th, windows)
    assert ctx.loss_stats()["head_loss_small"] == 3
    for a, b in zip(plain, ones):
        assert np.array_equal(a, b)
    assert not np.array_equal(plain[0], th.cpu().numpy())
    ctx.close()


# ----------------------------------------------------------------------------- 6. scores (and their ones)
SEVEN = list(range(7))  # inputs and y_last of every window / origin lie in rows 0 .. 29 of a T = 24 stream
NAN_ROW0 = 30
E_SEED = 20240611


@functools.lru_cache(maxsize=None)
def score_case():
    """CONFIG1's model of test_gpu_forecast.py on a stream whose weather channels are NaN from row 30 on at the nodes
    of weight 0: every one of the seven windows / origins has such targets, none reads them as inputs."""
    c = case(CONFIG1)
    d = c.d
    rng = np.random.default_rng(77)
    v = rng.uniform(0.25, 4.0, d.num_nodes)
    v[[2, 11, 24]] = 0.0
    v = (v / v.mean()).astype(np.float32)
    f = c.feats.copy()
    f[NAN_ROW0:, v == 0, :d.output_channels] = np.nan
    return c, v, f, torch.from_numpy(f).to(DEV)


def score_ctx(c, stream):
    ctx = c.context()
    ctx.set_tasks([stream])
    return ctx


def run_scores(c, ctx, kind, batch, scale=SCALE):
    """The four score calls on SEVEN: (predictions as the reference takes them, sums) as numpy."""
    d = c.d
    N, Hf, Cc, s = d.num_nodes, d.forecast_horizon, d.output_channels, d.forecast_horizon + 1
    st, n = _capi.stream_ptr(torch), len(SEVEN)
    if kind == "forecast":
        x = torch.zeros(n, N * Hf, Cc, device=DEV)
        q = torch.zeros(3, Hf, Cc, device=DEV, dtype=torch.float64)
        ctx.forecast(st, c.theta, SEVEN, batch, scale=scale, pred=x, skill=q)
    elif kind == "ensemble":
        x = torch.zeros(3, n, N * Hf, Cc, device=DEV)
        q = torch.zeros(4, Hf, Cc, device=DEV, dtype=torch.float64)
        ctx.forecast_ensemble(st, c.theta, SEVEN, batch, 3, 0.0, 0.2, E_SEED, scale=scale, member_pred=x, scores=q)
    elif kind == "rollout":
        x = torch.zeros(n, 2, s, N, Cc, device=DEV)
        q = torch.zeros(3, 2 * s, Cc, device=DEV, dtype=torch.float64)
        ctx.forecast_rollout(st, c.theta, SEVEN, batch, 2, 1, scale=scale, traj=x, skill=q)
    else:
        x = torch.zeros(2, n, 2, s, N, Cc, device=DEV)
        q = torch.zeros(4, 2 * s, Cc, device=DEV, dtype=torch.float64)
        ctx.forecast_rollout_ensemble(st, c.theta, SEVEN, batch, 2, 2, 0.0, 0.2, E_SEED, gap=1, scale=scale,
                                      member_traj=x, scores=q)
    torch.cuda.synchronize()
    return x.cpu().numpy(), q.cpu().numpy()


def reference_sums(kind, c, x, feats, v):
    if kind == "forecast":
        return forecast.skill_reference(x, feats, SEVEN, c.d, SCALE, node_weights=v)
    if kind == "ensemble":
        return forecast.ensemble_reference(x, feats, SEVEN, c.d, SCALE, node_weights=v)[2]
    if kind == "rollout":
        return forecast.rollout_skill_reference(x, feats, SEVEN, c.d, SCALE, node_weights=v)
    return forecast.ensemble_rollout_reference(x, feats, SEVEN, c.d, SCALE, node_weights=v)[2]


KINDS = ["forecast", "ensemble", "rollout", "rollout_ensemble"]


def relmax0(a, b):
    """Largest relative error per entry; an entry whose reference is exactly 0 (the variance of a gap row that
    every member shares) must be exactly 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(a[b == 0] == 0)
    return float(np.max(np.abs(a[b != 0] - b[b != 0]) / np.abs(b[b != 0])))


@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_node_weights_are_bitwise_the_unweighted_scores(kind):
    c = case(CONFIG1)
    ctx = c.context()
    x0, q0 = run_scores(c, ctx, kind, 7)
    ctx.set_score_weights(np.ones(c.d.num_nodes, np.float32))
    x1, q1 = run_scores(c, ctx, kind, 7)
    st = ctx.loss_stats()
    assert st["score_weights"] == 1 and st["score_launches"] > 0, st
    assert np.array_equal(x0, x1) and np.array_equal(q0, q1)
    assert np.isfinite(q0).all() and q0[0].min() > 0
    ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_weighted_scores_match_the_reference_and_mask_nan_targets(kind):
    c, v, feats, stream = score_case()
    ctx = score_ctx(c, stream)
    _, q_nan = run_scores(c, ctx, kind, 7)
    assert np.isnan(q_nan).any()  # control: unweighted, the NaN targets reach the sums
    ctx.set_score_weights(v)
    x, q = run_scores(c, ctx, kind, 7)
    assert np.isfinite(q).all() and np.isfinite(x).all()
    want = reference_sums(kind, c, x, feats, v)
    e = relmax0(q, want)
    _, q3 = run_scores(c, ctx, kind, 3)  # passes of 3, 3 and 1
    e3 = relmax0(q3, q)
    print(f"ERR {kind}: weighted sums against the reference {e:.3g} (1e-5), passes of 3 against one pass {e3:.3g} (1e-6)")
    assert e <= 1e-5 and e3 <= 1e-6
    # the weights matter: the unweighted reference on the clean stream is another number
    plain = reference_sums(kind, c, x, c.feats, None)
    assert relmax0(np.where(plain == 0, 0, q), plain) > 1e-2
    ctx.set_score_weights(None)
    assert ctx.loss_stats()["score_weights"] == 0
    ctx.close()


def test_python_wrappers_divide_by_the_weight_sum_and_clear_the_weights():
    c, v, feats, stream = score_case()
    d = c.d
    model = build_hybrid(d, c.P)
    ctx = score_ctx(c, stream)
    count = len(SEVEN) * float(np.asarray(v, np.float64).sum())
    r = forecast.forecast(model, stream, c.ei, windows=SEVEN, batch=7, ctx=ctx, node_weights=v)
    s = forecast.skill_reference(r.pred.reshape(len(SEVEN), -1, d.output_channels), feats, SEVEN, d, node_weights=v)
    assert relmax0(r.rmse, np.sqrt(s[0] / count)) <= 1e-5 and relmax0(r.mae, s[1] / count) <= 1e-5
    ro = forecast.rollout(model, stream, c.ei, origins=SEVEN, cycles=2, batch=7, ctx=ctx, node_weights=v)
    s = forecast.rollout_skill_reference(ro.traj, feats, SEVEN, d, node_weights=v)
    assert relmax0(ro.rmse, np.sqrt(s[0] / count)) <= 1e-5 and relmax0(ro.mae, s[1] / count) <= 1e-5
    en = forecast.ensemble_forecast(model, stream, c.ei, members=3, p_gcn=0.0, p_lstm=0.2, seed=E_SEED, windows=SEVEN,
                                    batch=7, return_members=True, ctx=ctx, node_weights=v)
    s = forecast.ensemble_reference(en.members.reshape(3, len(SEVEN), -1, d.output_channels), feats, SEVEN, d,
                                    node_weights=v)[2]
    assert relmax0(en.rmse, np.sqrt(s[0] / count)) <= 1e-5 and relmax0(en.crps, s[2] / count) <= 1e-5
    er = forecast.ensemble_rollout(model, stream, c.ei, origins=SEVEN, cycles=2, members=2, p_gcn=0.0, p_lstm=0.2,
                                   seed=E_SEED, batch=7, return_members=True, ctx=ctx, node_weights=v)
    s = forecast.ensemble_rollout_reference(er.members, feats, SEVEN, d, node_weights=v)[2]
    assert relmax0(er.rmse, np.sqrt(s[0] / count)) <= 1e-5 and relmax0(er.crps, s[2] / count) <= 1e-5
    assert ctx.loss_stats()["score_weights"] == 0  # every call cleared them again
    ctx.close()


# ----------------------------------------------------------------------------- 2. parity, small head
@functools.lru_cache(maxsize=None)
def p_oracle(order, drop_seed=None):
    d, P, ei, feats, tables = p_case()
    Pt, Pg, _ = torch_params(P)
    tasks = [refcpu.TaskData(f, ei, d) for f in feats]
    cfg = MamlConfig()
    dropout = None if drop_seed is None else (drop_seed, 0.2, 0.2)
    return wlo.meta_step(Pt, Pg, tasks, tables, P_TABLE, 2, B, cfg.inner_lr, cfg.max_norm, order, cfg.query_loss_scale,
                         dropout=dropout)


@pytest.mark.parametrize("order", [0, 1, 2])
def test_small_head_matches_the_weighted_oracle(order):
    d, P, ei, feats, tables = p_case()
    ml = learner(d, P, ei, feats, 2, B, order, tables)
    out = outputs(ml, P_TABLE)
    st = ml.ctx.loss_stats()
    print(f"order {order}: {st}")
    assert st["loss_sets"] == 2 and st["head_loss_small"] > 0 and st["head_loss"] == 0
    assert (st["head_dual"] > 0) == (order == 2)
    check_meta(f"P order {order}", out, p_oracle(order), d, torch_params(P)[2], order)
    # the tables matter, and which task reads which: the unweighted and the swapped oracles are elsewhere
    plain = refcpu.meta_step(*torch_params(P)[:2], [refcpu.TaskData(f, ei, d) for f in feats], None, 2, B, None, 0.01, 1.0,
                             0, windows=P_TABLE) if order == 0 else None
    if plain is not None:
        assert all(abs(out[0][-1, j] - plain["query_losses"][j]) > 1e-3 * plain["query_losses"][j] for j in range(2))


def test_small_head_with_dropout_matches_the_weighted_oracle():
    d, P, ei, feats, tables = p_case()
    ml = learner(d, P, ei, feats, 2, B, 1, tables, dropout=(0.2, 0.2), seed=5)
    out = outputs(ml, P_TABLE)
    seed = (5 * 1000003 + 1) & 0xFFFFFFFF  # MetaLearner's seed of its first meta-step
    check_meta("P order 1 dropout", out, p_oracle(1, seed), d, torch_params(P)[2], 1)


def test_task_groups_upload_each_group_s_tables():
    """task_group = 1: one smaml_meta_step per task, each after its own table's upload (set 0 of a one-set table is
    then the task's): the oracle's result, not that of the first task's table for both."""
    d, P, ei, feats, tables = p_case()
    theta, gcn, _ = split(P)
    ml = MetaLearner(d, MamlConfig(inner_steps=2, batch=B, order=1), gcn, theta, ei, device=DEV, task_group=1)
    ml.set_tasks(feats, loss_weights=tables)
    assert len(ml._groups) == 2
    out = outputs(ml, P_TABLE)
    assert ml.ctx.loss_stats()["loss_sets"] == 1
    check_meta("P order 1, task groups of 1", out, p_oracle(1), d, torch_params(P)[2], 1)


# ----------------------------------------------------------------------------- 3. parity, MFMA head
def test_mfma_head_matches_the_weighted_oracle():
    d = M_DIMS
    Bm = 42  # 42 x 49 = 2,058 rows: 17 row tiles of 128, the last one partial (10 rows)
    P = synth.init_params(303, d, gcn_bias_scale=0.1)
    ei = grid_edges(d)
    feats = [synth.make_features(8500, d.num_nodes, synth.t_total_for(2 * Bm, T, HF))]
    table = wlo.draw_tables(d, 520)[1]
    w = np.asarray([[list(range(Bm))], [list(range(Bm, 2 * Bm))]], np.int32)
    ml = learner(d, P, ei, feats, 1, Bm, 2, table)
    out = outputs(ml, w)
    st = ml.ctx.loss_stats()
    print(st)
    assert st["head_loss"] > 0 and st["head_dual"] > 0 and st["head_loss_small"] == 0
    Pt, Pg, names = torch_params(P)
    cfg = MamlConfig()
    ref = wlo.meta_step(Pt, Pg, [refcpu.TaskData(feats[0], ei, d)], [table], w, 1, Bm, cfg.inner_lr, cfg.max_norm, 2,
                        cfg.query_loss_scale)
    check_meta("M order 2", out, ref, d, names, 2)


# ----------------------------------------------------------------------------- 4. masked NaN targets
def test_zero_weights_mask_nan_targets():
    d, P, ei, feats, _ = p_case()
    tables = [wlo.draw_tables(d, 530)[0], wlo.draw_tables(d, 531)[0]]  # separable: whole nodes masked
    t_total = feats[0].shape[0]
    nan_feats, zero_feats = [], []
    for f, W in zip(feats, tables):
        masked = np.all(W.reshape(HF, d.num_nodes, C) == 0, axis=(0, 2))
        assert masked.sum() >= 1
        a, z = f.copy(), f.copy()
        a[t_total - HF:, masked, :C] = np.nan  # the last Hf rows: no window reads them as inputs (w + T <= t_total - Hf - 1)
        z[t_total - HF:, masked, :C] = 0.0
        nan_feats.append(a)
        zero_feats.append(z)
    assert P_TABLE.max() + T <= t_total - HF - 1 and P_TABLE.max() == LAST
    ml = learner(d, P, ei, nan_feats, 2, B, 2, tables)
    out = outputs(ml, P_TABLE)
    Pt, Pg, names = torch_params(P)
    cfg = MamlConfig()
    ref = wlo.meta_step(Pt, Pg, [refcpu.TaskData(f, ei, d) for f in zero_feats], tables, P_TABLE, 2, B, cfg.inner_lr,
                        cfg.max_norm, 2, cfg.query_loss_scale)
    check_meta("P order 2, NaN targets", out, ref, d, names, 2)
    # control: the same call without the tables reaches the NaNs (task 0's query batch ends at the last window)
    ml.set_tasks(nan_feats, loss_weights=None)
    assert ml.ctx.loss_stats()["loss_sets"] == 0
    assert np.isnan(outputs(ml, P_TABLE)[0][-1, 0])


def test_head_loss_masks_nan_targets():
    d, P, ei, _, _ = a_case()
    N, H = d.num_nodes, d.lstm_hidden_size
    W = wlo.draw_tables(d, 540)[1]
    ctx, th, _, _ = adapt_ctx(d, P, ei, [a_case()[3][0]])
    rng = np.random.default_rng(9)
    h = rng.standard_normal((3, N, H)).astype(np.float32)
    ys = rng.standard_normal((3, HF * N, C)).astype(np.float32)
    ys_nan = ys.copy()
    ys_nan[:, W == 0] = np.nan
    st = _capi.stream_ptr(torch)
    hT = torch.from_numpy(h).to(DEV)
    pred, dpred, loss = torch.zeros(3, N * HF, C, device=DEV), torch.zeros(3, N * HF, C, device=DEV), torch.zeros(1, device=DEV)
    ctx.set_loss_weights(W)
    ctx.head_loss(st, th, hT, pred, [torch.from_numpy(y).to(DEV) for y in ys_nan], loss, dpred)
    torch.cuda.synchronize()
    po = (h.astype(np.float64).reshape(3 * N, H) @ P["output_layer.weight"].astype(np.float64).T
          + P["output_layer.bias"].astype(np.float64)).reshape(3, N * HF, C)
    want = (W * (po - ys) ** 2).mean()
    e_l, e_d = abs(float(loss) - want) / want, rel(dpred.cpu(), 2.0 * W * (po - ys) / po.size)
    print(f"ERR head_loss: loss {e_l:.3g} (1e-5), dpred {e_d:.3g} (1e-5)")
    assert e_l < 1e-5 and e_d < 1e-5
    assert bool((dpred.cpu()[:, torch.from_numpy(W == 0)] == 0).all()) and ctx.loss_stats()["head_loss_small"] == 1
    ctx.set_loss_weights(None)
    ctx.head_loss(st, th, hT, pred, [torch.from_numpy(y).to(DEV) for y in ys_nan], loss, dpred)
    torch.cuda.synchronize()
    assert np.isnan(float(loss))  # control
    ctx.close()


# ----------------------------------------------------------------------------- 5. adapt paths
def check_adapt(label, got_theta, got_losses, ref, ref_losses, d, names):
    e_l = rel(got_losses, ref_losses)
    got = params.unpack(torch.from_numpy(np.asarray(got_theta)), d, 0)
    e_p = max(rel(got[k].numpy(), ref[k]) for k in names)
    print(f"ERR {label}: step losses {e_l:.3g} (1e-5), parameters {e_p:.3g} (1e-5)")
    assert e_l < 1e-5 and e_p < 1e-5


def test_adapt_steps_with_the_feature_cache_matches_the_weighted_oracle():
    d, P, ei, feats, tables = a_case()
    names = torch_params(P)[2]
    ctx, th, _, _ = adapt_ctx(d, P, ei, feats[:1])
    ctx.set_loss_weights(tables[1])
    windows = [[3], [0], [3]]  # window 3 twice: its second use reads the cache slot
    got = run_adapt_steps(ctx, th, windows)
    assert ctx.loss_stats()["head_loss_small"] == 3
    ref, ref_losses = wlo.adam_steps(d, P, feats[0], ei, windows, ADAPT_LRS, tables[1], WD)
    check_adapt("adapt_steps B = 1", got[0], got[3], ref, ref_losses, d, names)
    _, plain_losses = wlo.adam_steps(d, P, feats[0], ei, windows, ADAPT_LRS, None, WD)
    assert abs(got[3][0] - plain_losses[0]) > 1e-3 * plain_losses[0]  # the table matters
    ctx.close()


def test_adapt_steps_full_matches_the_weighted_oracle():
    d, P, ei, feats, tables = a_case()
    ctx, th, gflat, _ = adapt_ctx(d, P, ei, feats[:1])
    ctx.set_loss_weights(tables[0])
    windows = np.asarray([[3, 0], [1, 5], [3, 6]], np.int32)
    th, g = th.clone(), gflat.clone()
    m, v, gm, gv = torch.zeros_like(th), torch.zeros_like(th), torch.zeros_like(g), torch.zeros_like(g)
    losses = torch.zeros(3, device=DEV)
    ctx.adapt_steps_full(_capi.stream_ptr(torch), th, m, v, g, gm, gv, 0, windows, torch.from_numpy(ADAPT_LRS).to(DEV),
                         (0.9, 0.999), 1e-8, WD, 1.0, losses)
    torch.cuda.synchronize()
    ref, ref_losses = wlo.adam_steps(d, P, feats[0], ei, windows, ADAPT_LRS, tables[0], WD, train_base=True)
    names = torch_params(P)[2]
    check_adapt("adapt_steps_full B = 2", th.cpu().numpy(), losses.cpu().numpy(), ref, ref_losses, d, names)
    gg = params.unpack(g.cpu(), d, 1)
    e_g = max(rel(gg[k].numpy(), ref[k]) for k in gg)
    print(f"ERR adapt_steps_full: GCN parameters {e_g:.3g} (1e-5)")
    assert e_g < 1e-5
    ctx.close()


def test_adapt_steps_multi_reads_the_set_of_the_task_index():
    """Two registered tasks, regions [1, 0], two different tables: region 0 adapts task 1 under table 1."""
    d, P, ei, feats, tables = a_case()
    names = torch_params(P)[2]
    ctx, th0, _, _ = adapt_ctx(d, P, ei, feats)
    ctx.set_loss_weights(tables)
    tasks = [1, 0]
    windows = np.asarray([[[3], [2]], [[0], [6]], [[3], [1]]], np.int32)  # [steps][region][1]
    th = th0.unsqueeze(0).repeat(2, 1).contiguous()
    m, v = torch.zeros_like(th), torch.zeros_like(th)
    lr = torch.from_numpy(ADAPT_LRS).to(DEV).unsqueeze(1).repeat(1, 2).contiguous()
    losses = torch.zeros(3, 2, device=DEV)
    ctx.adapt_steps_multi(_capi.stream_ptr(torch), tasks, th, m, v, 0, windows, lr, (0.9, 0.999), 1e-8, [WD, WD], 1.0,
                          losses)
    torch.cuda.synchronize()
    for r, t in enumerate(tasks):
        ref, ref_losses = wlo.adam_steps(d, P, feats[t], ei, windows[:, r], ADAPT_LRS, tables[t], WD)
        check_adapt(f"adapt_steps_multi region {r} (task {t})", th[r].cpu().numpy(), losses[:, r].cpu().numpy(), ref,
                    ref_losses, d, names)
        wrong, wl = wlo.adam_steps(d, P, feats[t], ei, windows[:, r], ADAPT_LRS, tables[r], WD)
        assert rel(losses[:, r].cpu().numpy(), wl) > 1e-3  # the table of the region's POSITION is another result
    ctx.close()


def test_adapt_val_loss_is_the_weighted_validation_loss():
    d, P, ei, feats, tables = a_case()
    theta, gcn, _ = split(P)
    convs = {k: v for k, v in gcn.items() if k.startswith("base_stgcn.conv")}
    n = synth.num_samples(feats[0].shape[0], T, HF)
    res = A.adapt(d, feats[0], ei, convs, theta, "Delhi", epochs=0, device=DEV, loss_weights=tables[1])
    want = wlo.weighted_val_loss(d, P, feats[0], ei, range(int(0.8 * n), n), tables[1])
    plain = wlo.weighted_val_loss(d, P, feats[0], ei, range(int(0.8 * n), n), None)
    print(f"adapt val_loss {res.val_loss:.6g}, oracle {want:.6g} (unweighted {plain:.6g})")
    assert abs(res.val_loss - want) < 1e-5 * want and abs(want - plain) > 1e-3 * plain
    many = A.adapt_many(d, feats, ei, convs, theta, ["Delhi", "Moscow"], epochs=0, device=DEV, loss_weights=tables)
    for r in range(2):
        w = wlo.weighted_val_loss(d, P, feats[r], ei, range(int(0.8 * n), n), tables[r])
        assert abs(many[r].val_loss - w) < 1e-5 * w, r


# ----------------------------------------------------------------------------- 7. state
def test_state_rules():
    d, P, ei, feats, tables = p_case()
    ml = learner(d, P, ei, feats, 2, B, 1, None)
    base = outputs(ml, P_TABLE)
    ctx = ml.ctx
    # three sets for two tasks: SMAML_ESTATE naming both numbers, nothing launched
    ctx.set_loss_weights([tables[0], tables[1], tables[0]])
    before = ctx.loss_stats()
    with pytest.raises(_capi.SmamlError) as e:
        ml.meta_step(windows=P_TABLE)
    assert e.value.code == 4 and "3" in str(e.value) and "2" in str(e.value), str(e.value)
    assert ctx.loss_stats() == before and before["loss_sets"] == 3 and before["head_loss_small"] == 0
    # a failed set leaves the live table alone
    ctx.set_loss_weights(tables)
    bad = tables[0].copy()
    bad[5, 3] = -1.0
    with pytest.raises(_capi.SmamlError):
        ctx.set_loss_weights([bad, tables[1]])
    assert ctx.loss_stats()["loss_sets"] == 2
    # the table survives set_tasks, set_graph, set_gcn_params and reserve
    ml.step, ml.meta_steps = 0, 0
    ml.theta.copy_(params.pack(split(P)[0], d, which=0, device=DEV))
    ml.m.zero_(), ml.v.zero_()
    ctx.set_tasks(ml.tasks)
    ctx.set_graph(ei)
    ctx.set_gcn_params(ml.gcn)
    ctx.reserve(3, 8)
    weighted = outputs(ml, P_TABLE)
    assert ctx.loss_stats()["loss_sets"] == 2 and ctx.loss_stats()["head_loss_small"] > 0
    fresh = outputs(learner(d, P, ei, feats, 2, B, 1, tables), P_TABLE)
    for a, b in zip(weighted, fresh):
        assert np.array_equal(a, b)
    assert not np.array_equal(weighted[0], base[0])
    # clearing restores the unweighted bits
    ctx.set_loss_weights(None)
    ml.theta.copy_(params.pack(split(P)[0], d, which=0, device=DEV))
    ml.m.zero_(), ml.v.zero_()
    ml.step = 0
    again = outputs(ml, P_TABLE)
    for a, b in zip(again, base):
        assert np.array_equal(a, b)


def test_a_pending_forward_backward_pair_stays_valid_across_set_loss_weights():
    d, P, ei, feats, tables = a_case()
    ctx, th, _, ts = adapt_ctx(d, P, ei, feats[:1])
    N = d.num_nodes
    xs = [ts[0][w:w + T].reshape(T * N, -1) for w in (0, 4)]
    st = _capi.stream_ptr(torch)
    dp = torch.from_numpy(np.random.default_rng(3).standard_normal((2, N * HF, C)).astype(np.float32)).to(DEV)
    grads = []
    for between in (False, True):
        pred, grad = torch.zeros(2, N * HF, C, device=DEV), torch.zeros_like(th)
        ctx.forward(st, th, xs, pred)
        if between:
            ctx.set_loss_weights(tables[0])
            ctx.set_score_weights(np.ones(N, np.float32))
        ctx.backward(st, th, dp, grad)
        torch.cuda.synchronize()
        grads.append(grad.cpu().numpy())
    assert np.array_equal(grads[0], grads[1]) and np.abs(grads[0]).max() > 0
    ctx.close()
