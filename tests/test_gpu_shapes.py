"""Oracle parity over the shape space the C ABI accepts, and rejection of the rest.

``check_dims`` (api.cpp) accepts lstm_hidden_size 32 / 64 / 128 / 256, 1..8 layers, any window length and
any head width up to 128 columns; the other GPU test files run three shapes of that space (CONFIG1,
CONFIG2, CONFIG5). Here every entry point that launches the LSTM or the head runs against
``oracle/refcpu.py`` (f32) at the smallest shape that is the first to reach a code path:

====  =================================  ===============================================================
 id   dims                               the first to reach
====  =================================  ===============================================================
 A    N=49, Hc=32, H=256, L=2, T=4       ``HT = 256``: two 128-unit column tiles in the BPTT step and its
                                         tangent twin, ``grid.y = 2`` in ``k_gemm_nn``, 8 unit groups in the
                                         gate kernels, four 64-unit column tiles on ``CfgNNs``, the MFMA head
                                         ``k_head_loss`` at small M (the SIMT head stops at H = 128), the
                                         ``<256>`` kw kernels, 1024-row x 513-column wide weight gradients
 B    N=25, Hc=48, H=64, L=3, T=3        ``HT = 64`` against an oracle; Hc a multiple of 16 and of nothing
                                         larger (3 K tiles); 2H = 128 columns: weight gradients that are not
                                         ``wgrad_wide``; an odd layer count
 C    N=36, Hc=16, H=32, L=4, T=2        T < L: no diagonal holds all layers; Hc is exactly one K tile
 D    N=25, Hc=64, H=128, L=2, T=1       one time step: ``h_{t-1}`` never exists, a forecast ring of one step,
                                         consecutive windows that share no stream row (the fused GCN is off)
 E1   CONFIG1 with Hf=8, C=16            Hf*C = 128, the head's column limit
 E2   CONFIG1 with Hf=8, C=8             Hf*C = 64: the 64-thread SIMT head exactly full
 E3   CONFIG1 with Hf=17, C=4            Hf*C = 68: the 128-thread head mostly idle; the target pairing
                                         r = n Hf + h -> (r / N, r % N) with an Hf that divides nothing
 E4   CONFIG1 with Hf=5, C=3             rejected (below)
====  =================================  ===============================================================

The batch of A..D makes M = B N one full 256-row gate tile plus a partial one (A: 6 x 49 = 294, B and D:
11 x 25 = 275, C: 8 x 36 = 288), which is also two full 128-row BPTT tiles plus a partial one.

Which kernel a launch takes depends on its size, and at these sizes the defaults take the small-grid forms
(grouped weight gradients up to ``wgrad_group_max_rows`` = 2048 rows per launch set, the kw / split-K steps,
the 64 x 64 BPTT tiles). The meta-step tests therefore run two arms against one oracle: the defaults, and
``big``: ``wgrad_group_max_rows = 0``, ``bwd_big_min = bwdd_big_min = 0``, ``split_max = 1`` -- the kernels the
bench runs (128 x 128 BPTT tiles, per-problem weight gradients on the wide tiles where the shape allows them,
the layer-0 projection over distinct stream rows, compact features). ``variant_counts`` asserts which ran.
What no counter shows follows from the shape alone: at H = 256 ``ntn = ceil(H / CfgBwd::BN) = 2`` for every
big-tile BPTT launch and ``grid.y = ceil(H / CfgNN::BN) = 2`` for every ``k_gemm_nn``; ``head_small`` is false
for H > 128, so every head launch of A is ``k_head_loss`` and ``dh_fused`` is off.

Tolerances are the project's (test_gpu_parity.py): predictions, per-step losses, adapted parameters <= 1e-5
rel-L2; query MSE and meta-gradients <= 1e-4.

Rejected shapes. The tile loaders of the default path need every K segment to be a multiple of BK = 16
(loaders.h), so the LSTM / head entry points refuse hidden_channels % 16 != 0 (``check_lstm_dims``); the GCN
entry points keep working at any multiple of 4. Hf*C % 4 != 0 (E4) is refused too, settled by reading the
three readers of ``dpred`` / ``pred`` rows: ``k_head_wgrad_small`` reads scalars and would be correct, but
``k_gemm_nn`` (dh_T = dpred . Wo) reads ``dpred`` through ``RowMajorKC{dpred, M, HfC}``, whose 16-byte load at
the last K group of a row starts inside the row (k < K passes its check) and runs up to 3 floats into the
next row -- past the buffer at the last row -- and is 4-byte aligned only, since rows are HfC floats; the
split-K head weight gradient reads the same rows as float4 columns of its B operand. Not in bounds, so not
run: rejected.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast, params, synth
from weatherforecast_stgcn_maml_amd import adapt as adapt_mod
from weatherforecast_stgcn_maml_amd.config import CONFIG1, MamlConfig, ModelDims
from weatherforecast_stgcn_maml_amd.maml import MetaLearner, stream_len_for, window_table

import test_gpu_ensemble as ens
from test_gpu_api import oracle_grads
from test_gpu_forecast import case, relmax
from test_gpu_parity import DEV, _check_meta_step, _oracle_meta_step, build_hybrid, grid_edges, rel, split

pytestmark = pytest.mark.gpu

SHAPES = {
    "A": ModelDims(num_nodes=49, window_size=4, hidden_channels=32, lstm_hidden_size=256, lstm_num_layers=2),
    "B": ModelDims(num_nodes=25, window_size=3, hidden_channels=48, lstm_hidden_size=64, lstm_num_layers=3),
    "C": ModelDims(num_nodes=36, window_size=2, hidden_channels=16, lstm_hidden_size=32, lstm_num_layers=4),
    "D": ModelDims(num_nodes=25, window_size=1, hidden_channels=64, lstm_hidden_size=128, lstm_num_layers=2),
    "E1": dataclasses.replace(CONFIG1, forecast_horizon=8, output_channels=16),
    "E2": dataclasses.replace(CONFIG1, forecast_horizon=8, output_channels=8),
    "E3": dataclasses.replace(CONFIG1, forecast_horizon=17, output_channels=4),
}
BATCH = {"A": 6, "B": 11, "C": 8, "D": 11, "E1": 11, "E2": 11, "E3": 11}  # one full 256-row tile + a partial one
SEEDS = {k: 70 + i for i, k in enumerate(SHAPES)}
BIG = 1 << 30


def scale_for(d):
    return np.linspace(0.5, 3.0, d.output_channels)


def sample(d, feats, i):
    return synth.sample_xy(feats, i, d.window_size, d.forecast_horizon, d.output_channels)


def setup(tag, cfg, n_tasks, **kw):
    """(P, names, ei, feats, MetaLearner) of shape `tag`: seeds fixed per shape, all tasks in one pass."""
    d = SHAPES[tag]
    P = synth.init_params(SEEDS[tag], d, gcn_bias_scale=0.1)
    theta, gcn, names = split(P)
    ei = grid_edges(d)
    feats = [synth.make_features(100 * SEEDS[tag] + j, d.num_nodes, stream_len_for(cfg, d)) for j in range(n_tasks)]
    kw.setdefault("task_group", None)
    ml = MetaLearner(d, cfg, gcn, theta, ei, device=DEV, **kw)
    ml.set_tasks(feats)
    return P, names, ei, feats, ml


def check_adapted(fast, ref, d, names):
    for j in range(fast.shape[0]):
        ad = params.unpack(fast[j], d, 0)
        for k in names:
            assert rel(ad[k].cpu().numpy(), ref["adapted"][j][k].numpy()) < 1e-5, (j, k)


def relmax0(a, b):
    """relmax for sums that can be exactly 0 (the persistence error of a time-of-day channel, a target of
    E1's 16, over windows inside one day): a zero reference entry must be a zero, the rest as relmax."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.all(a[b == 0] == 0), a[b == 0]
    return float(np.max(np.abs(a[b != 0] - b[b != 0]) / np.abs(b[b != 0])))


def fwd_launches(vc):
    return vc["fwd"] + vc["fwd_split"] + vc["fwd_kw"] + vc["fwd_drop"]


def bwd_launches(vc):
    return vc["bwd_big"] + vc["bwd_small"] + vc["bwd_split"] + vc["bwd_kw"]


# ----------------------------------------------------------------------------- meta-step, orders 1 and 2
@pytest.mark.parametrize("arm", ["default", "big"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("tag", ["A", "B", "C", "D"])
def test_meta_step_matches_oracle(tag, order, arm):
    """K = 2 inner steps, 2 tasks, the shape's batch: per-step losses, adapted parameters, query MSE and the
    meta-gradient. `default`: the knobs as they are (small-grid forms at these sizes); `big`: the bench's
    kernels forced (module docstring).

    D is the regression test of two T = 1 defects: on the default knobs the
    per-layer GCN's row expansion was a launch of B (T - 1) = 0 blocks (SMAML_EHIP), and in the `big` arm the
    compact feature layout, (2B - 1) N rows in a slab of B N, was written past each task's slab and, at
    second order, past the kept-features buffer."""
    d = SHAPES[tag]
    cfg = MamlConfig(inner_steps=2, batch=BATCH[tag], order=order)
    P, names, ei, feats, ml = setup(tag, cfg, 2)
    if arm == "big":
        for k, v in (("wgrad_group_max_rows", 0), ("bwd_big_min", 0), ("bwdd_big_min", 0), ("split_max", 1)):
            ml.ctx.set_option(k, v)
    fast = torch.zeros(2, ml.theta.numel(), device=DEV)
    ml.ctx.variant_counts(reset=True)
    res = ml.meta_step(fast_out=fast)
    vc = ml.ctx.variant_counts()
    print(f"{tag} order {order} {arm}: {({k: v for k, v in vc.items() if v})}")
    K, diags = cfg.inner_steps, d.window_size + d.lstm_num_layers - 1
    assert fwd_launches(vc) == (K + 1) * diags and bwd_launches(vc) == (K + 1) * diags, vc
    if arm == "big":
        # every diagonal of every forward / backward on the big tiles: K inner steps + the query batch
        assert vc["fwd"] == (K + 1) * diags and vc["fwd_split"] == vc["fwd_kw"] == 0, vc
        assert vc["bwd_big"] == (K + 1) * diags and vc["bwd_small"] == vc["bwd_split"] == vc["bwd_kw"] == 0, vc
        if order == 2:
            assert vc["bwd_dual_big"] + vc["bwd_dual_big_kept"] == K * diags, vc
            assert vc["bwd_dual_small"] == vc["bwd_dual_small_kept"] == 0, vc
        # weight gradients per problem: 256 x 256 tiles wherever 4H and cin + H are multiples of 256
        wide = (4 * d.lstm_hidden_size) % 256 == 0 and (2 * d.lstm_hidden_size) % 256 == 0
        assert (vc["wgrad_wide"] > 0) == wide, vc
        if d.window_size > 1:  # consecutive windows share stream rows: layer 0's projection once per row
            assert vc["xg_dedup"] > 0 and vc["wgrad_dedup"] > 0, vc
        # ... and the features stored once per row; never for one-step windows, whose compact rows do not fit
        assert vc["f_compact"] == ((K + 1) if d.window_size > 1 else 0), vc
    else:
        # small grids: every BPTT diagonal on the kw kernel, forward diagonals on it where their K is long
        # enough to split, the LSTM weight gradients of a backward as one grouped launch (not counted)
        assert vc["bwd_kw"] == (K + 1) * diags and vc["fwd_split"] == vc["bwd_split"] == 0, vc
        if order == 2:
            assert vc["bwd_dual_small_kept"] == K * diags and vc["bwd_dual_big"] == vc["bwd_dual_big_kept"] == 0, vc
        else:
            # what `wgrad` counts here is the head's split-K weight gradient: once per backward at H = 256,
            # where the head is k_head_loss and its gradient the MFMA kernel's; never with the SIMT head
            assert vc["wgrad"] == ((K + 1) if d.lstm_hidden_size > 128 else 0) and vc["wgrad_wide"] == 0, vc
    ref = _oracle_meta_step(("shapes", tag, order), d, P, names, feats, ei, cfg, list(ml.default_windows()[-1, 0]))
    _check_meta_step(res, ml, ref, d, names, 2, K)
    check_adapted(fast, ref, d, names)


# ----------------------------------------------------------------------------- forced tile variants
@pytest.mark.parametrize("tiles", ["big", "small", "split", "kw"])
@pytest.mark.parametrize("keep", [-1, 0])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_second_order_tile_variants(tag, keep, tiles):
    """Every BPTT tile variant forced as test_second_order_tile_variants_task_groups forces them (B = 1,
    K = 2, 3 tasks in task groups of 2), at H = 256 and H = 64."""
    d = SHAPES[tag]
    cfg = MamlConfig(inner_steps=2, batch=1, order=2)
    P, names, ei, feats, ml = setup(tag, cfg, 3, task_group=2)
    assert len(ml._groups) == 2
    big = 0 if tiles == "big" else BIG
    ml.ctx.set_option("bwd_big_min", big)
    ml.ctx.set_option("bwdd_big_min", big)
    ml.ctx.set_option("split_max", 4 if tiles in ("split", "kw") else 1)
    ml.ctx.set_option("small_kw", 1 if tiles == "kw" else 0)
    ml.ctx.set_option("keep", keep)
    ml.ctx.variant_counts(reset=True)
    res = ml.meta_step()
    vc = ml.ctx.variant_counts()
    print(f"{tag} keep {keep} {tiles}: {({k: v for k, v in vc.items() if v})}")
    dual = ("bwd_dual_big" if tiles == "big" else "bwd_dual_small") + ("_kept" if keep else "")
    assert vc[dual] > 0, vc
    if tiles == "big":
        assert vc["bwd_big"] > 0 and vc["bwd_small"] == vc["bwd_split"] == 0, vc
    elif tiles == "small":
        assert vc["bwd_small"] > 0 and vc["bwd_big"] == vc["bwd_split"] == 0 and vc["fwd_split"] == 0, vc
    elif tiles == "split":
        assert vc["bwd_split"] > 0 and vc["fwd_split"] > 0 and vc["bwd_big"] == 0, vc
    else:
        assert vc["bwd_kw"] > 0 and vc["fwd_kw"] > 0 and vc["bwd_split"] == vc["bwd_big"] == 0, vc
    ref = _oracle_meta_step(("shapes-groups", tag), d, P, names, feats, ei, cfg, list(ml.default_windows()[-1, 0]))
    _check_meta_step(res, ml, ref, d, names, 3, cfg.inner_steps)


# ----------------------------------------------------------------------------- dropout
_DROP_ORACLE = {}


@pytest.mark.parametrize("tiles", ["big", "small"])
@pytest.mark.parametrize("tag", ["A", "B"])
def test_meta_step_dropout_matches_oracle(tag, tiles):
    """Train-mode dropout (0.2 / 0.2), second order, K = 1, as test_second_order_bench_tiles_b32_dropout: the
    element loaders (any multiple of 4) and the `_drop` kernels of HT = 256 and HT = 64, on the 128 x 128 and
    on the 64 x 64 BPTT tiles, against the oracle's restated masks."""
    d = SHAPES[tag]
    cfg = MamlConfig(inner_steps=1, batch=BATCH[tag], order=2)
    P, names, ei, feats, ml = setup(tag, cfg, 1, dropout=(0.2, 0.2), dropout_seed=9)
    ml.set_tasks(feats, task_ids=[4])
    big = 0 if tiles == "big" else BIG
    ml.ctx.set_option("bwd_big_min", big)
    ml.ctx.set_option("bwdd_big_min", big)
    ml.ctx.variant_counts(reset=True)
    res = ml.meta_step()
    vc = ml.ctx.variant_counts()
    print(f"{tag} dropout {tiles}: {({k: v for k, v in vc.items() if v})}")
    assert vc["fwd_drop"] > 0 and vc["fwd"] == vc["fwd_kw"] == vc["fwd_split"] == 0, vc
    if tiles == "big":
        assert vc["bwd_big"] > 0 and vc["bwd_small"] == 0, vc
        assert vc["bwd_dual_big"] + vc["bwd_dual_big_kept"] > 0, vc
    else:
        assert vc["bwd_small"] > 0 and vc["bwd_big"] == vc["bwd_kw"] == vc["bwd_split"] == 0, vc
        assert vc["bwd_dual_small"] + vc["bwd_dual_small_kept"] > 0, vc
    if tag not in _DROP_ORACLE:
        seed = (9 * 1000003 + 1) & 0xFFFFFFFF  # MetaLearner's seed of its first meta-step
        PT = refcpu.to_torch(P)
        _DROP_ORACLE[tag] = refcpu.meta_step(
            {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names},
            [refcpu.TaskData(f, ei, d) for f in feats], list(ml.default_windows()[-1, 0]), cfg.inner_steps, cfg.batch,
            cfg.inner_steps * cfg.batch, cfg.inner_lr, cfg.max_norm, cfg.order, dropout=(seed, 0.2, 0.2), task_ids=[4])
    _check_meta_step(res, ml, _DROP_ORACLE[tag], d, names, 1, cfg.inner_steps)


# ----------------------------------------------------------------------------- head widths
@pytest.mark.parametrize("tag", ["E1", "E2", "E3"])
def test_meta_step_head_widths(tag):
    """First order, K = 1, B = 2, 2 tasks on 24-channel streams with C != 12 targets: the SIMT head with 64
    and 128 threads (full, and mostly idle) and the F4 pairing with Hf = 17."""
    d = SHAPES[tag]
    cfg = MamlConfig(inner_steps=1, batch=2, order=1)
    P, names, ei, feats, ml = setup(tag, cfg, 2)
    fast = torch.zeros(2, ml.theta.numel(), device=DEV)
    res = ml.meta_step(fast_out=fast)
    ref = _oracle_meta_step(("shapes", tag, 1), d, P, names, feats, ei, cfg, list(ml.default_windows()[-1, 0]))
    _check_meta_step(res, ml, ref, d, names, 2, cfg.inner_steps)
    check_adapted(fast, ref, d, names)


# ----------------------------------------------------------------------------- operators
def operator_context(d, P):
    Ptr, Pg, names = split(P)
    ctx = _capi.Context(d, 0)
    ctx.set_graph(grid_edges(d))
    ctx.set_gcn_params(params.pack({k: torch.from_numpy(v) for k, v in Pg.items()}, d, which=1, device=DEV))
    theta = params.pack({k: torch.from_numpy(v) for k, v in Ptr.items()}, d, device=DEV)
    return ctx, theta, names


@pytest.mark.parametrize("tag", ["A", "B", "C", "D"])
def test_lstm_and_head_operators(tag):
    """smaml_gcn_forward, smaml_lstm_forward, smaml_head_loss, smaml_lstm_backward on the shape's batch, as
    test_lstm_and_head_operators_match_oracle."""
    d = SHAPES[tag]
    B, N, T, H = BATCH[tag], d.num_nodes, d.window_size, d.lstm_hidden_size
    P = synth.init_params(SEEDS[tag] + 1, d, gcn_bias_scale=0.1)
    ei = grid_edges(d)
    feats = synth.make_features(synth.task_seed(1), N, synth.t_total_for(B, T, d.forecast_horizon))
    xs, ys = zip(*[sample(d, feats, i) for i in range(B)])
    ctx, theta, names = operator_context(d, P)
    st = _capi.stream_ptr(torch)
    xg = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in xs]
    yg = [torch.from_numpy(np.ascontiguousarray(y)).to(DEV) for y in ys]
    F = torch.empty(B, T * N, d.hidden_channels, device=DEV)
    ctx.gcn_forward(st, xg, F)
    hT = torch.empty(B, N, H, device=DEV)
    ctx.lstm_forward(st, theta, F, hT)
    pred = torch.empty(B, N * d.forecast_horizon, d.output_channels, device=DEV)
    loss = torch.empty(1, device=DEV)
    dpred = torch.empty_like(pred)
    ctx.head_loss(st, theta, hT, pred, yg, loss, dpred)
    Wo = params.unpack(theta, d)["output_layer.weight"]
    dhT = (dpred.view(B * N, -1) @ Wo).view(B, N, H).contiguous()
    grad = torch.empty_like(theta)
    ctx.lstm_backward(st, theta, dhT, grad)
    torch.cuda.synchronize()

    Pt = {k: torch.from_numpy(v).clone().requires_grad_(k in names) for k, v in P.items()}
    eic = torch.from_numpy(ei).long()
    Fo = [refcpu.stgcn_features(torch.from_numpy(x), eic, Pt).detach() for x in xs]
    seq = torch.cat([f.view(T, N, -1).permute(1, 0, 2) for f in Fo])
    hTo = refcpu.lstm_stack(seq, Pt, d.lstm_num_layers)
    predo = (hTo @ Pt["output_layer.weight"].t() + Pt["output_layer.bias"]).view(B, N * d.forecast_horizon, -1)
    losso = torch.stack([refcpu.mse(predo[b], torch.from_numpy(ys[b])) for b in range(B)]).mean()
    losso.backward()
    assert rel(F.cpu(), torch.stack(Fo)) < 1e-5
    assert rel(hT.cpu(), hTo.detach().view(B, N, H)) < 1e-5
    assert rel(pred.cpu(), predo.detach()) < 1e-5
    assert abs(float(loss) - float(losso)) < 1e-5 * float(losso)
    g = params.unpack(grad, d)
    for k in names:
        if k.startswith("lstm."):
            assert rel(g[k].cpu(), Pt[k].grad) < 1e-4, k
        else:
            assert float(g[k].abs().max()) == 0.0, k  # lstm_backward leaves the head to the caller
    pred2 = torch.empty_like(pred)
    ctx.head_loss(st, theta, hT, pred2)
    torch.cuda.synchronize()
    assert torch.equal(pred2, pred)
    ctx.close()


@pytest.mark.parametrize("tag", ["E1", "E2", "E3"])
def test_head_loss_operator_widths(tag):
    """smaml_head_loss alone on given h_T rows (11 samples: 275 rows) at the three head widths: predictions,
    the loss with the F4 pairing of the targets, and dpred = 2 (pred - y) / count."""
    d = SHAPES[tag]
    B, N, H, Hf, C = BATCH[tag], d.num_nodes, d.lstm_hidden_size, d.forecast_horizon, d.output_channels
    P = synth.init_params(SEEDS[tag] + 1, d, gcn_bias_scale=0.1)
    feats = synth.make_features(synth.task_seed(1), N, synth.t_total_for(B, d.window_size, Hf))
    ys = [sample(d, feats, i)[1] for i in range(B)]
    ctx, theta, _ = operator_context(d, P)
    st = _capi.stream_ptr(torch)
    h = np.random.default_rng(SEEDS[tag]).standard_normal((B, N, H)).astype(np.float32)
    hT = torch.from_numpy(h).to(DEV)
    yg = [torch.from_numpy(np.ascontiguousarray(y)).to(DEV) for y in ys]
    pred = torch.empty(B, N * Hf, C, device=DEV)
    loss = torch.empty(1, device=DEV)
    dpred = torch.empty_like(pred)
    ctx.head_loss(st, theta, hT, pred, yg, loss, dpred)
    torch.cuda.synchronize()
    po = (h.astype(np.float64).reshape(B * N, H) @ P["output_layer.weight"].astype(np.float64).T
          + P["output_layer.bias"].astype(np.float64)).reshape(B, N * Hf, C)
    yo = np.stack(ys).astype(np.float64)
    assert rel(pred.cpu(), po) < 1e-5
    assert abs(float(loss) - ((po - yo) ** 2).mean()) < 1e-5 * ((po - yo) ** 2).mean()
    assert rel(dpred.cpu(), 2.0 * (po - yo) / po.size) < 1e-5
    ctx.close()


def test_autograd_shim_h256():
    """smaml_forward + smaml_backward through the torch.autograd shim at A (one sample: M = 49 rows)."""
    d = SHAPES["A"]
    P = synth.init_params(SEEDS["A"] + 2, d, gcn_bias_scale=0.1)
    ei = grid_edges(d)
    feats = synth.make_features(synth.task_seed(3), d.num_nodes, synth.t_total_for(4, d.window_size, d.forecast_horizon))
    x, y = sample(d, feats, 2)
    loss_o, pred_o, g_o = oracle_grads(P, x, y, ei, d)
    m = build_hybrid(d, P).train()
    pred = m(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), torch.from_numpy(ei).to(DEV))
    loss = torch.nn.functional.mse_loss(pred, torch.from_numpy(y).to(DEV))
    loss.backward()
    assert rel(pred.detach().cpu(), pred_o) < 1e-5
    assert abs(float(loss) - loss_o) < 1e-5 * loss_o
    sd = dict(m.named_parameters())
    for k, g in g_o.items():
        assert sd[k].grad is not None, k
        assert rel(sd[k].grad.cpu(), g) < 1e-4, (k, rel(sd[k].grad.cpu(), g))


# ----------------------------------------------------------------------------- adaptation
_ADAPT = {}


def adapt_case(tag):
    """Model, 3 streams of 8 windows (6 training + 2 validation), recorded shuffle orders of 2 epochs and the
    oracle's adaptation of each stream (computed on demand, once)."""
    if tag not in _ADAPT:
        d = SHAPES[tag]
        P = synth.init_params(SEEDS[tag] + 3, d, gcn_bias_scale=0.1)
        tr, gcn, _ = split(P)
        rng = np.random.default_rng(SEEDS[tag])
        _ADAPT[tag] = dict(
            d=d, P=P, tr=tr, convs={k: v for k, v in gcn.items() if k.startswith("base_stgcn.conv")}, ei=grid_edges(d),
            feats=[synth.make_features(3100 + 10 * SEEDS[tag] + j, d.num_nodes,
                                       synth.t_total_for(8, d.window_size, d.forecast_horizon)) for j in range(3)],
            orders=[np.stack([rng.permutation(6) for _ in range(2)]).astype(np.int32) for _ in range(3)], ref={})
    return _ADAPT[tag]


def adapt_oracle(a, j, region):
    if (j, region) not in a["ref"]:
        PT = refcpu.to_torch(a["P"])
        tr_t, gcn_t, _ = split(PT)
        a["ref"][(j, region)] = refcpu.adapt_reference(tr_t, gcn_t, refcpu.TaskData(a["feats"][j], a["ei"], a["d"]),
                                                       region, 2, orders=a["orders"][j])
    return a["ref"][(j, region)]


def check_adapt(a, res, ref):
    ref_p, ref_losses, ref_lrs, ref_val, _ = ref
    assert res.n_train == 6 and res.n_val == 2
    np.testing.assert_allclose(res.lrs, ref_lrs, rtol=1e-12)
    assert rel(res.epoch_losses, ref_losses) < 1e-5, (res.epoch_losses, ref_losses)
    got = params.unpack(res.theta, a["d"], 0)
    for k in a["tr"]:
        assert rel(got[k].cpu().numpy(), ref_p[k].numpy()) < 1e-5, k
    assert abs(res.val_loss - ref_val) < 1e-5 * ref_val, (res.val_loss, ref_val)


@pytest.mark.parametrize("small_kw", [0, 1, 2], ids=["split-k", "kw", "kw-bwd-img"])
@pytest.mark.parametrize("tag", ["A", "B", "D"])
def test_adaptation_matches_oracle(tag, small_kw):
    """Batch-1 fine-tuning, 2 epochs of 6 windows + the 2-window validation, as
    test_adaptation_n441_matches_oracle: the small-grid steps of HT = 256 / 64 / 128 (the last with T = 1)."""
    a = adapt_case(tag)
    ctx = _capi.Context(a["d"], 0)
    ctx.set_option("small_kw", small_kw)
    ctx.variant_counts(reset=True)
    res = adapt_mod.adapt(a["d"], a["feats"][0], a["ei"], a["convs"], a["tr"], "Moscow", epochs=2, device=DEV, ctx=ctx,
                          orders=a["orders"][0])
    vc = ctx.variant_counts()
    print(f"{tag} small_kw {small_kw}: {({k: v for k, v in vc.items() if v})}")
    if small_kw:
        assert vc["fwd_kw"] > 0 and vc["bwd_kw"] > 0 and vc["bwd_split"] == 0, vc
    else:
        assert vc["fwd_kw"] == 0 and vc["bwd_kw"] == 0 and vc["bwd_split"] > 0, vc
    check_adapt(a, res, adapt_oracle(a, 0, "Moscow"))
    ctx.close()


def test_lockstep_adaptation_h256():
    """smaml_adapt_steps_multi with 3 regions (three climates) at A, each region against the oracle run on
    that region alone."""
    a = adapt_case("A")
    regions = ("Thailand", "Moscow", "Delhi")
    ctx = _capi.Context(a["d"], 0)
    ctx.set_option("adapt_group", 0)  # the three regions as one launch set
    res = adapt_mod.adapt_many(a["d"], a["feats"], a["ei"], a["convs"], a["tr"], regions, epochs=2, device=DEV,
                               orders=a["orders"], ctx=ctx)
    for r in range(3):
        check_adapt(a, res[r], adapt_oracle(a, r, regions[r]))
    ctx.close()


# ----------------------------------------------------------------------------- forecast
@pytest.mark.parametrize("tag", ["A", "B", "C", "D", "E1", "E2", "E3"])
def test_forecast_matches_oracle(tag):
    """One pass of consecutive windows (one full 256-row tile and a masked one; the GCN and layer 0's
    projection once per distinct stream row, as test_gpu_forecast.py asserts at CONFIG1) and one of scattered
    windows: predictions and the skill sums."""
    d = SHAPES[tag]
    c = case(d)
    ctx = c.context()
    scale = scale_for(d)
    for windows, batch, consecutive in ((list(range(BATCH[tag])), BATCH[tag], True), ([9, 2, 30, 3], 4, False)):
        ctx.variant_counts(reset=True)
        pred, skill = c.run(ctx, windows, batch, scale=scale)
        vc = ctx.variant_counts()
        print(f"{tag} windows {windows}: {({k: v for k, v in vc.items() if v})}")
        assert vc["fwd_infer"] == d.window_size + d.lstm_num_layers - 1, vc
        assert vc["fwd"] == 0 and vc["fwd_split"] == 0 and vc["fwd_kw"] == 0, vc
        if consecutive:
            assert vc["gcn_dedup"] == 1 and vc["xg_dedup"] == 1 and vc["f_compact"] == 1, vc
        else:
            assert vc["gcn_dedup"] == 0 and vc["xg_dedup"] == 0, vc
        po = c.oracle(windows)
        r = rel(pred, po)
        rs = relmax0(skill, forecast.skill_reference(po, c.feats, windows, d, scale))
        print(f"{tag} windows {windows}: pred rel-L2 {r:.3g}, skill sums max rel {rs:.3g}")
        assert r <= 1e-5
        assert rs <= 1e-5
    assert ctx.workspace_bytes() == 0 and ctx.forecast_bytes() > 0
    ctx.close()


# ----------------------------------------------------------------------------- ensemble
@pytest.mark.parametrize("p_gcn", [0.0, 0.2])
@pytest.mark.parametrize("tag", ["A", "B", "D"])
def test_ensemble_matches_oracle(tag, p_gcn):
    """4 MC-dropout members, p_lstm = 0.2, with and without GCN dropout (per-member features / the shared
    layer 0): members against refcpu.batch_loss under Dropout(seed, p_gcn, p_lstm, 0, e), the statistics
    against forecast.ensemble_reference (test_gpu_ensemble.py's reference)."""
    d = SHAPES[tag]
    c = case(d)
    ctx = c.context()
    windows = list(range(BATCH[tag]))
    ctx.variant_counts(reset=True)
    mean, spread, mem, scores = ens.run(c, ctx, windows, BATCH[tag], 4, p_gcn, 0.2)
    vc = ctx.variant_counts()
    print(f"{tag} p_gcn {p_gcn}: {({k: v for k, v in vc.items() if v})}")
    assert vc["fwd_infer_drop"] > 0 and vc["fwd_infer"] == 0 and vc["fwd"] == 0 and vc["fwd_drop"] == 0, vc
    assert vc["gcn_dedup"] == vc["xg_dedup"] == (0 if p_gcn else 1), vc
    ens.check_members(mem, ens.oracle(c, windows, p_gcn, 0.2, 4), f"{tag} p_gcn {p_gcn}")
    m_ref, s_ref, sc_ref = forecast.ensemble_reference(mem, c.feats, windows, d, ens.SCALE)
    assert relmax(mean, m_ref) <= 1e-5 and relmax(spread, s_ref) <= 1e-5 and relmax(scores, sc_ref) <= 1e-5
    ctx.close()


# ----------------------------------------------------------------------------- order-only knobs at H = 256
@pytest.mark.parametrize("knob", ["gate_img", "bptt_streams", "xg_dedup"])
def test_order_only_knobs_h256(knob):
    """gate_img 0 / 1 and bptt_streams 1 / 2 leave every row's arithmetic unchanged (bitwise, as
    test_gate_images_bitwise and test_order_only_knobs_bitwise assert at H = 128); xg_dedup / wgrad_dedup off
    sums the same products in another order (1e-6 on losses and norms, 1e-5 on the meta-gradient, as
    test_xg_dedup_against_oracle_and_off). Second order, K = 2, 2 tasks x B = 6, the big tiles forced and the
    grouped small-grid launches off, so that the knob's kernels are the ones that run."""
    cfg = MamlConfig(inner_steps=2, batch=BATCH["A"], order=2)
    out = []
    for on in (1, 0):
        _, _, _, _, ml = setup("A", cfg, 2)
        for k, v in (("wgrad_group_max_rows", 0), ("bwd_big_min", 0), ("bwdd_big_min", 0), ("split_max", 1)):
            ml.ctx.set_option(k, v)
        if knob == "bptt_streams":
            ml.ctx.set_option(knob, 2 if on else 1)
        else:
            ml.ctx.set_option(knob, on)
            if knob == "xg_dedup":
                ml.ctx.set_option("wgrad_dedup", on)
        ml.ctx.variant_counts(reset=True)
        res = ml.meta_step()
        vc = ml.ctx.variant_counts()
        print(f"{knob} {on}: {({k: v for k, v in vc.items() if v})}")
        assert vc["bwd_big"] > 0 and vc["bwd_dual_big_kept"] > 0, vc
        if knob == "gate_img":
            assert (vc["fwd_img"] > 0) == bool(on), vc
        if knob == "xg_dedup":
            assert (vc["xg_dedup"] > 0) == bool(on) and (vc["wgrad_dedup"] > 0) == bool(on), vc
        out.append((res.losses.cpu(), res.norms.cpu(), ml.meta_grad.cpu().clone()))
        del ml
    if knob == "xg_dedup":
        assert rel(out[0][0].numpy(), out[1][0].numpy()) < 1e-6
        assert rel(out[0][1].numpy(), out[1][1].numpy()) < 1e-6
        assert rel(out[0][2].numpy(), out[1][2].numpy()) < 1e-5
    else:
        for a, b in zip(out[0], out[1]):
            assert torch.equal(a, b)


def test_ens_share_bitwise_h256():
    """ens_share 0 / 1 at A: the shared layer 0 (p_gcn = 0) gives every member bitwise what its own layer 0
    gives (test_gpu_ensemble.py asserts it at H = 32)."""
    d = SHAPES["A"]
    c = case(d)
    ctx = c.context()
    windows = list(range(BATCH["A"]))
    shared = ens.run(c, ctx, windows, BATCH["A"], 3, 0.0, 0.2)
    ctx.set_option("ens_share", 0)
    own = ens.run(c, ctx, windows, BATCH["A"], 3, 0.0, 0.2)
    for a, b in zip(shared, own):
        assert np.array_equal(a, b)
    assert rel(shared[2][0], shared[2][1]) > 1e-2  # the members do differ
    ctx.close()


# ----------------------------------------------------------------------------- rejected shapes
REJECTED = {
    "Hc=40": (ModelDims(num_nodes=25, window_size=2, hidden_channels=40, lstm_hidden_size=32, lstm_num_layers=1),
              "hidden_channels"),
    "Hc=36": (ModelDims(num_nodes=25, window_size=2, hidden_channels=36, lstm_hidden_size=32, lstm_num_layers=1),
              "hidden_channels"),
    "E4": (dataclasses.replace(CONFIG1, forecast_horizon=5, output_channels=3), "forecast_horizon\\*output_channels"),
}


@pytest.mark.parametrize("name", list(REJECTED))
def test_unsupported_shapes_are_rejected_before_any_launch(name):
    """A context of such a shape is created (the GCN entry points serve it); every entry point that plans a
    gate-GEMM, BPTT or head launch returns SMAML_EINVAL naming the dimension, launches nothing (all launch
    counters stay 0) and allocates nothing (workspace and forecast bytes unchanged). The context's GCN stack
    still matches the oracle."""
    d, word = REJECTED[name]
    N, T, H, Hf, C = d.num_nodes, d.window_size, d.lstm_hidden_size, d.forecast_horizon, d.output_channels
    P = synth.init_params(91, d, gcn_bias_scale=0.1)
    ctx, theta, _ = operator_context(d, P)
    feats = synth.make_features(9100, N, synth.t_total_for(6, T, Hf))
    stream = torch.from_numpy(feats).to(DEV)
    ctx.set_tasks([stream, stream])
    st = _capi.stream_ptr(torch)
    x = stream[:T].reshape(T * N, -1).contiguous()
    F = torch.zeros(1, T * N, d.hidden_channels, device=DEV)
    hT = torch.zeros(1, N, H, device=DEV)
    pred = torch.zeros(1, N * Hf, C, device=DEV)
    grad, fast = torch.zeros_like(theta), torch.zeros(1, theta.numel(), device=DEV)
    th2 = theta.unsqueeze(0).repeat(2, 1).contiguous()
    m2, v2 = torch.zeros_like(th2), torch.zeros_like(th2)
    w1 = window_table(MamlConfig(inner_steps=1, batch=1), 2)
    lr1, lr2 = torch.full((1,), 1e-3, device=DEV), torch.full((1, 2), 1e-3, device=DEV)
    l1, l2 = torch.zeros(1, device=DEV), torch.zeros(1, 2, device=DEV)
    skill = torch.zeros(3, Hf, C, device=DEV, dtype=torch.float64)
    zero = np.zeros((1, 1), np.int32)
    calls = {
        "smaml_forward": lambda: ctx.forward(st, theta, [x], pred),
        "smaml_backward": lambda: ctx.backward(st, theta, pred, grad),
        "smaml_lstm_forward": lambda: ctx.lstm_forward(st, theta, F, hT),
        "smaml_lstm_backward": lambda: ctx.lstm_backward(st, theta, hT, grad),
        "smaml_head_loss": lambda: ctx.head_loss(st, theta, hT, pred),
        "smaml_meta_step": lambda: ctx.meta_step(st, theta, 1, 1, 1, w1, 0.01, 1.0, 0.5, meta_grad=grad),
        "smaml_inner_loop": lambda: ctx.inner_loop(st, theta, 1, 1, w1, 0.01, 1.0, torch.zeros_like(th2)),
        "smaml_adapt_prepare": lambda: ctx.adapt_prepare(st, 1),
        "smaml_adapt_steps": lambda: ctx.adapt_steps(st, fast[0], torch.zeros_like(theta), torch.zeros_like(theta), 0,
                                                     zero, lr1, (0.9, 0.999), 1e-8, 0.0, 1.0, l1),
        "smaml_adapt_prepare_multi": lambda: ctx.adapt_prepare_multi(st, [0, 1], 1),
        "smaml_adapt_steps_multi": lambda: ctx.adapt_steps_multi(st, [0, 1], th2, m2, v2, 0, np.zeros((1, 2, 1), np.int32),
                                                                 lr2, (0.9, 0.999), 1e-8, [0.0, 0.0], 1.0, l2),
        "smaml_forecast": lambda: ctx.forecast(st, theta, [0], 1, pred=pred, skill=skill),
        "smaml_forecast_ensemble": lambda: ctx.forecast_ensemble(st, theta, [0], 1, 2, 0.0, 0.2, 1, mean=pred),
    }
    ws, fb = ctx.workspace_bytes(), ctx.forecast_bytes()
    ctx.variant_counts(reset=True)
    for entry, call in calls.items():
        with pytest.raises(_capi.SmamlError, match=f"EINVAL.*{word}") as e:
            call()
        assert "must be a multiple of" in str(e.value), (entry, str(e.value))
    torch.cuda.synchronize()
    assert not any(ctx.variant_counts().values()), ctx.variant_counts()
    assert ctx.workspace_bytes() == ws and ctx.forecast_bytes() == fb
    # the GCN stack of the same context (K tails handled by its loaders)
    Fg = torch.empty(1, T * N, d.hidden_channels, device=DEV)
    ctx.gcn_forward(st, [x], Fg)
    torch.cuda.synchronize()
    PT = refcpu.to_torch(P)
    ref = refcpu.stgcn_features(x.cpu(), torch.from_numpy(grid_edges(d)).long(),
                                {k: v for k, v in PT.items() if k.startswith("base_stgcn")})
    assert rel(Fg[0].cpu(), ref) < 1e-5
    ctx.close()


def test_gcn_dropin_at_widths_the_lstm_rejects():
    """GCNConv(8, 40) (forward and backward) and STGCN with hidden_channels = 40 on the drop-in path against
    refcpu.gcn_conv / refcpu.stgcn_forward: the GCN loaders handle K tails, and the drop-in's contexts are
    GCN-only, so the LSTM shape rules do not touch them."""
    from weatherforecast_stgcn_maml_amd.model import STGCN, GCNConv

    torch.manual_seed(0)
    d = ModelDims(num_nodes=25, window_size=2, hidden_channels=40, lstm_hidden_size=32, lstm_num_layers=1)
    ei = grid_edges(d)
    conv = GCNConv(8, 40)
    with torch.no_grad():
        conv.bias.uniform_(-0.1, 0.1)
    rows = 3 * d.num_nodes + 7
    x = torch.randn(rows, 8)
    W = conv.lin.weight.detach().clone().requires_grad_(True)
    b = conv.bias.detach().clone().requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    ref = refcpu.gcn_conv(xr, torch.from_numpy(ei), W, b)
    R = torch.randn(rows, 40)
    (ref * R).sum().backward()
    conv = conv.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = conv(xg, torch.from_numpy(ei).to(DEV))
    assert rel(out.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    (out * R.to(DEV)).sum().backward()
    assert rel(conv.lin.weight.grad.cpu(), W.grad) < 1e-5
    assert rel(conv.bias.grad.cpu(), b.grad) < 1e-5
    assert rel(xg.grad.cpu(), xr.grad) < 1e-5

    P = synth.init_params(92, d, gcn_bias_scale=0.1)
    base = STGCN(d.input_channels, d.hidden_channels, d.output_channels, d.window_size, d.forecast_horizon,
                 dropout_rate=0.0)
    base.load_state_dict({k[len("base_stgcn."):]: torch.from_numpy(v) for k, v in P.items()
                          if k.startswith("base_stgcn.")})
    base = base.to(DEV).eval()
    xs, _ = sample(d, synth.make_features(9200, d.num_nodes, synth.t_total_for(1, d.window_size, d.forecast_horizon)), 0)
    with torch.no_grad():
        got = base(torch.from_numpy(np.ascontiguousarray(xs)).to(DEV), torch.from_numpy(ei).to(DEV)).cpu().numpy()
    want = refcpu.stgcn_forward(torch.from_numpy(np.ascontiguousarray(xs)), torch.from_numpy(ei).long(),
                                refcpu.to_torch(P), d, None)
    assert rel(got, want.numpy()) < 1e-5
