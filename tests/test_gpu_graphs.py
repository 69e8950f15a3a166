"""Every graph consumer on irregular graphs (``oracle/graphs.py``), against the CPU oracle on the same graph.

Every other GPU test builds its graph with ``build_spatial_graph`` on a square grid (in-degree 3..6, nothing
isolated, no duplicate, no self loop, A_hat almost symmetric, N a perfect square). The fixtures here: ``mixed37``
(a full ELL row of 7 in-edges with the self loop in the eighth slot, two isolated nodes -- one of them the last,
so ``edge_index.max() + 1 < N`` -- a duplicate edge, self loops in the input, shuffled columns), ``chain37``
(A_hat differs from A_hat^T at every node), ``fan150`` (a 101-entry row of the CSR of A_hat^T; a full ELL row
whose sources lie past the 128-row tile of ``k_gcn_layer``; N not a square, more than one tile), ``empty37``
(A_hat = I) and ``over`` (in-degree 8: rejected).

Which consumer each entry point reaches:

=============================  ===========================================================================
 entry point                    graph consumer
=============================  ===========================================================================
 gcn_conv, gcn_conv_ex          ``GcnA`` (the ELL gather in k_gcn_layer's A-operand prologue)
 gcn_conv_backward              ``k_gather_rows`` with the ELL (A_hat x for dW) and with the CSR (A_hat^T dz)
 GCNConv / STGCN modules        the three above, context sized by ``edge_index.max() + 1``
 forward, forecast[_ensemble],  ``GcnA`` on the t = 0 rows of every sample / distinct stream row, four layers
 forecast_rollout, meta_step,
 adapt_steps (cache fill)
 backward_base                  ``k_gather_rows`` (CSR and ELL) over all samples (``rps`` = T N)
 adapt_steps_full               ``k_gather_rows`` (gcn_dz_fused 0) or ``k_gcn_dz`` + ``k_gcn_dz_top`` (1)
=============================  ===========================================================================

The hybrid model is the smallest the LSTM entry points accept: T = 3, B = 2, Hc = 32, H = 32, two layers (one on
``chain37``). Tolerances are those of the grid-graph test of the same entry point, named at each comparison.
Guard bands as in test_gpu_windows.py: every input a kernel reads through the graph (operator inputs, samples,
streams) is the middle slice of a device tensor whose 16 rows on either side are NaN, outputs are pre-filled
with NaN, and every case asserts finite outputs first. tests/test_graphs_cpu.py checks the fixtures, the
builders and that the oracle tells each graph from its reverse, from its de-duplicated form and from an ELL
without the eighth slot by at least 100 x these tolerances.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import graphs, refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast, params, synth
from weatherforecast_stgcn_maml_amd import adapt as adapt_mod
from weatherforecast_stgcn_maml_amd.config import MamlConfig, ModelDims
from weatherforecast_stgcn_maml_amd.maml import MetaLearner, stream_len_for

import test_gpu_adapt_full as taf
import test_gpu_base_grad as tbg
import test_gpu_ensemble as ens
import test_gpu_rollout as tro
from test_gpu_forecast import SCALE, Case, relmax
from test_gpu_parity import DEV, _check_meta_step, rel, split
from test_gpu_shapes import check_adapted
from test_gpu_windows import BIG_ARM

pytestmark = pytest.mark.gpu

PAD = 16
NAN = float("nan")
OP_SHAPES = [(8, 40), (24, 64)]
HYB_B = 2


def guarded(a):
    """`a` ([rows, ...] float32, host) as the middle slice of a device tensor with PAD NaN rows on either side."""
    a = np.ascontiguousarray(a, np.float32)
    rows = a.shape[0]
    big = torch.full((PAD + rows + PAD,) + a.shape[1:], NAN, device=DEV)
    big[PAD:PAD + rows] = torch.from_numpy(a)
    view = big[PAD:PAD + rows]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    assert bool(torch.isnan(big[:PAD]).all()) and bool(torch.isnan(big[PAD + rows:]).all())
    return view


def finite(what, *tensors):
    for t in tensors:
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        assert np.isfinite(a).all(), f"{what}: not finite (unwritten, or a read outside the input reached it)"


def edges(name, edge_fn=None):
    ei, n = graphs.get(name)
    return (edge_fn(ei) if edge_fn else ei), n


def hybrid_dims(name):
    return ModelDims(num_nodes=graphs.NUM_NODES[name], window_size=3, hidden_channels=32, lstm_hidden_size=32,
                     lstm_num_layers=1 if name == "chain37" else 2)


def nseed(name):
    return 600 + 10 * list(graphs.ACCEPTED).index(name)


# ----------------------------------------------------------------------------- operators
@functools.lru_cache(maxsize=None)
def operator_inputs(name, cin, cout):
    """x [3 N + 7, cin], W [cout, cin], b [cout], R [3 N + 7, cout] (the loss is sum(out * R))."""
    n = graphs.NUM_NODES[name]
    rows = 3 * n + 7
    rng = np.random.default_rng(nseed(name) + cin)
    a = np.sqrt(6.0 / (cin + cout))
    return (rng.standard_normal((rows, cin)).astype(np.float32), rng.uniform(-a, a, (cout, cin)).astype(np.float32),
            rng.uniform(-0.1, 0.1, cout).astype(np.float32), rng.standard_normal((rows, cout)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def operator_oracle(name, cin, cout, edge_fn=None):
    """refcpu.gcn_conv (f32) and torch autograd of sum(out * R) on the fixture (or on edge_fn of it)."""
    ei, _ = edges(name, edge_fn)
    x, w, b, R = (torch.from_numpy(a).clone() for a in operator_inputs(name, cin, cout))
    for t in (x, w, b):
        t.requires_grad_(True)
    out = refcpu.gcn_conv(x, torch.from_numpy(ei), w, b)
    (out * R).sum().backward()
    o = out.detach().numpy()
    return {"out": o, "relu": np.maximum(o, 0.0), "dx": x.grad.numpy(), "dW": w.grad.numpy(), "db": b.grad.numpy()}


def operator_context(name, cin, cout):
    ei, n = graphs.get(name)
    ctx = _capi.Context(ModelDims(num_nodes=n, window_size=1, input_channels=cin, hidden_channels=cout,
                                  lstm_hidden_size=32, lstm_num_layers=1, forecast_horizon=1, output_channels=1), 0)
    ctx.set_graph(ei)
    return ctx


@pytest.mark.parametrize("cin,cout", OP_SHAPES)
@pytest.mark.parametrize("name", graphs.ACCEPTED)
def test_operators_match_oracle(name, cin, cout):
    """smaml_gcn_conv, smaml_gcn_conv_ex with ReLU and smaml_gcn_conv_backward (dx, dW, db) at rows = 3 N + 7:
    1e-5 rel-L2 each, the bound of test_gcnconv_dropin_matches_oracle for the same four quantities."""
    x, w, b, R = operator_inputs(name, cin, cout)
    ref = operator_oracle(name, cin, cout)
    rows = x.shape[0]
    ctx = operator_context(name, cin, cout)
    st = _capi.stream_ptr(torch)
    xg, dzg = guarded(x), guarded(R)
    wg, bg = torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
    out, relu = torch.full((rows, cout), NAN, device=DEV), torch.full((rows, cout), NAN, device=DEV)
    dx, dwb = torch.full((rows, cin), NAN, device=DEV), torch.full((cout * cin + cout,), NAN, device=DEV)
    ctx.gcn_conv(st, xg, wg, bg, out)
    ctx.gcn_conv_ex(st, xg, wg, bg, relu, flags=_capi.GCN_RELU)
    ctx.gcn_conv_backward(st, xg, wg, dzg, dx=dx, dwb=dwb)
    torch.cuda.synchronize()
    finite(f"{name} {cin}->{cout}", out, relu, dx, dwb)
    got = {"out": out, "relu": relu, "dx": dx, "dW": dwb[:cout * cin].view(cout, cin), "db": dwb[cout * cin:]}
    errs = {k: rel(v.cpu(), ref[k]) for k, v in got.items()}
    print(f"ERR operators {name} {cin}->{cout}: " + ", ".join(f"{k} {e:.3g}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < 1e-5, (k, e)
    # dx alone and dW alone are the same launches' results
    dx2, dwb2 = torch.full_like(dx, NAN), torch.full_like(dwb, NAN)
    ctx.gcn_conv_backward(st, xg, wg, dzg, dx=dx2)
    ctx.gcn_conv_backward(st, xg, wg, dzg, dwb=dwb2)
    torch.cuda.synchronize()
    assert torch.equal(dx2, dx) and torch.equal(dwb2, dwb)
    ctx.close()


def test_short_inputs_are_rejected_before_any_launch():
    """rows < num_nodes without SMAML_GCN_PLAIN: row q < N gathers any of rows 0 .. N - 1 of x, so the three
    entry points return SMAML_EINVAL naming the rule and launch nothing (the outputs keep their fill);
    GCNConv.forward raises the same error for x.shape[0] < edge_index.max() + 1."""
    from weatherforecast_stgcn_maml_amd.model import GCNConv

    cin, cout = OP_SHAPES[0]
    x, w, b, R = operator_inputs("mixed37", cin, cout)
    ctx = operator_context("mixed37", cin, cout)
    st = _capi.stream_ptr(torch)
    rows = 36  # one short of the graph's 37 nodes
    xg, dzg = torch.from_numpy(x).to(DEV), torch.from_numpy(R).to(DEV)  # (3 N + 7 rows allocated: nothing can fault)
    wg, bg = torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)
    out = torch.full((rows, cout), -7.0, device=DEV)
    dx, dwb = torch.full((rows, cin), -7.0, device=DEV), torch.full((cout * cin + cout,), -7.0, device=DEV)
    ws = ctx.workspace_bytes()
    calls = {
        "smaml_gcn_conv": lambda: ctx.gcn_conv(st, xg[:rows], wg, bg, out),
        "smaml_gcn_conv_ex": lambda: ctx.gcn_conv_ex(st, xg[:rows], wg, bg, out, flags=_capi.GCN_RELU),
        "smaml_gcn_conv_backward": lambda: ctx.gcn_conv_backward(st, xg[:rows], wg, dzg[:rows], dx=dx, dwb=dwb),
    }
    for entry, call in calls.items():
        with pytest.raises(_capi.SmamlError, match=r"EINVAL.*rows \(36\) must be at least num_nodes \(37\)") as e:
            call()
        assert entry in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert ctx.workspace_bytes() == ws
    for t in (out, dx, dwb):
        assert bool((t == -7.0).all())
    ctx.close()
    ei, _ = graphs.get("mixed37")
    n_graph = int(ei.max()) + 1
    conv = GCNConv(cin, cout).to(DEV)
    eig = torch.from_numpy(ei).to(DEV)
    for grad in (False, True):
        xs = xg[:n_graph - 1].clone().requires_grad_(grad)
        with pytest.raises(_capi.SmamlError, match=f"EINVAL.*rows \\({n_graph - 1}\\) must be at least num_nodes"):
            conv(xs, eig)


# ----------------------------------------------------------------------------- module API
@pytest.mark.parametrize("cin,cout", OP_SHAPES)
@pytest.mark.parametrize("name", ["mixed37", "fan150"])
def test_gcnconv_module_matches_oracle(name, cin, cout):
    """GCNConv forward and autograd, as test_gcnconv_dropin_matches_oracle (1e-5 on the output and on the three
    gradients). On mixed37 the module sizes its context from edge_index.max() + 1 = 36 < N = 37."""
    from weatherforecast_stgcn_maml_amd.model import GCNConv

    x, w, b, R = operator_inputs(name, cin, cout)
    ref = operator_oracle(name, cin, cout)
    ei, n = graphs.get(name)
    assert (int(ei.max()) + 1 < n) == (name == "mixed37")
    conv = GCNConv(cin, cout)
    with torch.no_grad():
        conv.lin.weight.copy_(torch.from_numpy(w))
        conv.bias.copy_(torch.from_numpy(b))
    conv = conv.to(DEV)
    eig = torch.from_numpy(ei).to(DEV)
    xg = guarded(x).requires_grad_(True)
    with torch.no_grad():
        plain = conv(xg, eig)
    out = conv(xg, eig)
    (out * torch.from_numpy(R).to(DEV)).sum().backward()
    finite(f"GCNConv {name}", plain, out, conv.lin.weight.grad, conv.bias.grad, xg.grad)
    assert torch.equal(plain, out.detach())
    errs = {"out": rel(out.detach().cpu(), ref["out"]), "dx": rel(xg.grad.cpu(), ref["dx"]),
            "dW": rel(conv.lin.weight.grad.cpu(), ref["dW"]), "db": rel(conv.bias.grad.cpu(), ref["db"])}
    print(f"ERR GCNConv {name} {cin}->{cout}: " + ", ".join(f"{k} {e:.3g}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e < 1e-5, (k, e)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("name", ["mixed37", "fan150"])
def test_stgcn_module_matches_oracle(name, p):
    """STGCN forward and autograd in train mode, as test_stgcn_autograd_matches_oracle: output 1e-5, the
    gradient of every parameter and of x 1e-4, with the oracle under the module's own masks."""
    from weatherforecast_stgcn_maml_amd.hybrid_model import draw_dropout_seed
    from weatherforecast_stgcn_maml_amd.model import STGCN

    d = hybrid_dims(name)
    ei, n = graphs.get(name)
    P = synth.init_params(nseed(name) + 1, d, gcn_bias_scale=0.1)
    base = STGCN(d.input_channels, d.hidden_channels, d.output_channels, d.window_size, d.forecast_horizon,
                 dropout_rate=p)
    base.load_state_dict({k[len("base_stgcn."):]: torch.from_numpy(v) for k, v in P.items()
                          if k.startswith("base_stgcn.")})
    base = base.to(DEV).train()
    rng = np.random.default_rng(nseed(name) + 2)
    x = rng.standard_normal((d.window_size * n, d.input_channels)).astype(np.float32)
    R = rng.standard_normal((n * d.forecast_horizon, d.output_channels)).astype(np.float32)
    xg = guarded(x).requires_grad_(True)
    torch.manual_seed(11)
    out = base(xg, torch.from_numpy(ei).to(DEV))
    (out * torch.from_numpy(R).to(DEV)).sum().backward()
    torch.manual_seed(11)
    drop = refcpu.Dropout(draw_dropout_seed(), p, 0.0, 0, 0) if p > 0.0 else None
    Pt = {k: v.clone().requires_grad_(True) for k, v in refcpu.to_torch(P).items() if k.startswith("base_stgcn.")}
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    ref = refcpu.stgcn_forward(xt, torch.from_numpy(ei).long(), Pt, d, drop)
    (ref * torch.from_numpy(R)).sum().backward()
    sd = dict(base.named_parameters())
    finite(f"STGCN {name} p {p}", out, xg.grad, *[q.grad for q in sd.values()])
    e_out = rel(out.detach().cpu(), ref.detach())
    e_par = {k: rel(sd[k[len("base_stgcn."):]].grad.cpu(), v.grad) for k, v in Pt.items()}
    e_x = rel(xg.grad.cpu(), xt.grad)
    print(f"ERR STGCN {name} p {p}: out {e_out:.3g} (1e-5), parameters {max(e_par.values()):.3g} (1e-4), x {e_x:.3g} (1e-4)")
    assert e_out < 1e-5
    for k, e in e_par.items():
        assert e < 1e-4, (k, e)
    assert e_x < 1e-4


# ----------------------------------------------------------------------------- forward + backward_base
@functools.lru_cache(maxsize=None)
def hybrid_inputs(name):
    d = hybrid_dims(name)
    P = synth.init_params(nseed(name) + 3, d, gcn_bias_scale=0.1)
    rng = np.random.default_rng(nseed(name) + 4)
    xs = [rng.standard_normal((d.window_size * d.num_nodes, d.input_channels)).astype(np.float32) for _ in range(HYB_B)]
    R = rng.standard_normal((HYB_B, d.num_nodes * d.forecast_horizon, d.output_channels)).astype(np.float32)
    return d, P, xs, R


@functools.lru_cache(maxsize=None)
def hybrid_oracle(name, p, edge_fn=None):
    """(preds, {name: grad}, [dx]) of loss = sum(pred * R) with the GCN differentiable (test_gpu_base_grad.py's
    composition of refcpu functions), masks of Dropout(SEED, p, p, 0, 0) when p > 0."""
    d, P, xs, R = hybrid_inputs(name)
    ei, _ = edges(name, edge_fn)
    drop = refcpu.Dropout(tbg.SEED, p, p, 0, 0) if p > 0 else None
    return tbg.oracle_backward(P, xs, ei, d, lambda preds: sum((q * torch.from_numpy(R[b])).sum()
                                                               for b, q in enumerate(preds)), drop)


@pytest.mark.parametrize("fused", [1, 0], ids=["dx0_fused", "dx0_composed"])
@pytest.mark.parametrize("p", [0.0, 0.2], ids=["p0", "dropout"])
@pytest.mark.parametrize("name", ["mixed37", "chain37", "fan150"])
def test_forward_and_backward_base_match_oracle(name, p, fused):
    """smaml_forward + smaml_backward_base as test_backward_base_matches_oracle: predictions 1e-5, every
    gradient tensor of both layouts and every dx 1e-4."""
    d, P, xs, R = hybrid_inputs(name)
    preds_o, g_o, dx_o = hybrid_oracle(name, p)
    Ptr, Pg, _ = split(P)
    Pg = {k: v for k, v in Pg.items() if k.startswith("base_stgcn.conv")}
    ctx = _capi.Context(d, 0)
    ctx.set_option("dx0_fused", fused)
    ctx.set_graph(graphs.get(name)[0])
    gflat = params.pack({k: torch.from_numpy(v) for k, v in Pg.items()}, d, which=1, device=DEV)
    ctx.set_gcn_params(gflat)
    theta = params.pack({k: torch.from_numpy(v) for k, v in Ptr.items()}, d, device=DEV)
    xg = [guarded(x) for x in xs]
    Rg = torch.from_numpy(R).to(DEV)
    st = _capi.stream_ptr(torch)
    if p > 0:
        ctx.set_task_ids([0])
        ctx.set_dropout(p, p, tbg.SEED)
    pred = torch.full_like(Rg, NAN)
    ctx.forward(st, theta, xg, pred)
    grad, gg = torch.full_like(theta, NAN), torch.full_like(gflat, NAN)
    dxs = [torch.full_like(x, NAN) for x in xg]
    ctx.backward_base(st, theta, xg, Rg, grad, gg, dxs)
    torch.cuda.synchronize()
    finite(f"backward_base {name} p {p}", pred, grad, gg, *dxs)
    e_pred = max(rel(pred[b].cpu(), preds_o[b]) for b in range(HYB_B))
    got = dict(params.unpack(grad, d))
    got.update(params.unpack(gg, d, 1))
    assert len(got) == 4 * d.lstm_num_layers + 2 + 8
    e_g = {k: rel(v.cpu(), g_o[k]) for k, v in got.items()}
    e_dx = max(rel(dxs[b].cpu(), dx_o[b]) for b in range(HYB_B))
    e_gcn = max(e for k, e in e_g.items() if k.startswith("base_stgcn"))
    print(f"ERR backward_base {name} p {p} dx0_fused {fused}: pred {e_pred:.3g} (1e-5), gcn gradient {e_gcn:.3g} (1e-4), "
          f"every gradient {max(e_g.values()):.3g} (1e-4), dxs {e_dx:.3g} (1e-4)")
    assert e_pred < 1e-5
    for k, e in e_g.items():
        assert e < 1e-4, (k, e)
    assert e_dx < 1e-4
    ctx.close()


# ----------------------------------------------------------------------------- adapt_steps_full
AF_STEPS, AF_WINDOWS = 4, 6


@functools.lru_cache(maxsize=None)
def af_inputs(name):
    d = hybrid_dims(name)
    P = synth.init_params(nseed(name) + 5, d, gcn_bias_scale=0.1)
    feats = synth.make_features(nseed(name) + 6, d.num_nodes, AF_WINDOWS + d.window_size + d.forecast_horizon)
    rng = np.random.default_rng(nseed(name) + 7)
    windows = rng.integers(0, AF_WINDOWS - 1, size=(AF_STEPS, HYB_B)).astype(np.int32)
    windows[1] = windows[0]
    lrs = (taf.LR * (1.0 - 0.03 * np.arange(AF_STEPS))).astype(np.float32)
    return d, P, feats, windows, lrs


@functools.lru_cache(maxsize=None)
def af_oracle(name):
    d, P, feats, windows, lrs = af_inputs(name)
    return taf.oracle_steps(d, HYB_B, 0.0, P, feats, graphs.get(name)[0], windows, lrs, 1.0)


def af_run(name, options):
    d, P, feats, windows, lrs = af_inputs(name)
    tr, gc = taf.split_names(P)
    ctx = _capi.Context(d, 0)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.set_graph(graphs.get(name)[0])
    stream_t = guarded(feats)
    ctx.set_tasks([stream_t])
    ctx.set_task_ids([0])
    ctx.set_dropout(0.0, 0.0, taf.SEED)
    theta = params.pack({k: torch.from_numpy(P[k]) for k in tr}, d, device=DEV)
    gcn = params.pack({k: torch.from_numpy(P[k]) for k in gc}, d, which=1, device=DEV)
    m, v, gm, gv = (torch.zeros_like(t) for t in (theta, theta, gcn, gcn))
    losses, norms = torch.full((AF_STEPS,), NAN, device=DEV), torch.full((AF_STEPS,), NAN, device=DEV)
    ctx.adapt_steps_full(_capi.stream_ptr(torch), theta, m, v, gcn, gm, gv, taf.STEP0, windows,
                         torch.from_numpy(lrs).to(DEV), (0.9, 0.999), 1e-8, taf.WD, 1.0, losses, norms)
    torch.cuda.synchronize()
    stats = ctx.adapt_full_stats()
    ctx.close()
    return [theta, m, v, gcn, gm, gv, losses, norms], stats, stream_t


def af_check(name, label, state):
    """test_gpu_adapt_full.py's check_against_oracle: losses, norms and every adapted tensor 1e-5, every tensor's
    update (adapted - initial) 1e-3."""
    d, P, *_ = af_inputs(name)
    ref, ref_losses, ref_norms, _ = af_oracle(name)
    theta, _, _, gcn, _, _, losses, norms = state
    finite(f"adapt_steps_full {name} {label}", *state)
    got = dict(params.unpack(theta, d, 0))
    got.update(params.unpack(gcn, d, 1))
    e_l, e_n = rel(losses.cpu(), ref_losses), rel(norms.cpu(), ref_norms)
    e_p = {k: rel(v.cpu().numpy(), ref[k]) for k, v in got.items()}
    e_u = {k: rel(v.cpu().numpy().astype(np.float64) - P[k], ref[k].astype(np.float64) - P[k]) for k, v in got.items()}
    print(f"ERR adapt_steps_full {name} {label}: losses {e_l:.3g} (1e-5), norms {e_n:.3g} (1e-5), parameters "
          f"{max(e_p.values()):.3g} (1e-5), updates {max(e_u.values()):.3g} (1e-3)")
    assert e_l < 1e-5 and e_n < 1e-5
    assert len(got) == 4 * d.lstm_num_layers + 2 + 8
    for k in got:
        assert e_p[k] < 1e-5, (k, e_p[k])
        assert e_u[k] < 1e-3, (k, e_u[k])


@pytest.mark.parametrize("name", ["mixed37", "chain37", "fan150"])
def test_adapt_steps_full_matches_oracle_on_every_arm(name):
    """4 steps, B = 2. gcn_dz_fused 0 (GEMM + k_gather_rows + mask) and 1 (k_gcn_dz + k_gcn_dz_top) are bitwise
    equal and both inside the oracle's tolerance; gcn_keep 0 (the recompute arm) is inside it too."""
    d, P, *_ = af_inputs(name)
    ref, *_ = af_oracle(name)
    for k in taf.split_names(P)[1]:  # the oracle does train the base
        assert rel(ref[k], P[k]) > 1e-3, k
    composed, st0, _ = af_run(name, ())
    assert st0 == taf.expected_stats(name, AF_STEPS), st0
    af_check(name, "gcn_dz_fused 0", composed)
    fused, st1, _ = af_run(name, (("gcn_dz_fused", 1),))
    assert st1 == taf.expected_stats(name, AF_STEPS, dz_fused=1), st1
    af_check(name, "gcn_dz_fused 1", fused)
    assert all(torch.equal(a, b) for a, b in zip(composed, fused))
    recompute, st2, _ = af_run(name, (("gcn_keep", 0),))
    assert st2 == taf.expected_stats(name, AF_STEPS, keep=0), st2
    af_check(name, "gcn_keep 0", recompute)
    both, st3, _ = af_run(name, (("gcn_keep", 0), ("gcn_dz_fused", 1)))
    assert st3 == taf.expected_stats(name, AF_STEPS, keep=0, dz_fused=1), st3
    assert all(torch.equal(a, b) for a, b in zip(recompute, both))


# ----------------------------------------------------------------------------- adapt_steps, batched cache fill
def test_adaptation_with_batched_cache_fill_matches_oracle():
    """adapt() on mixed37: 2 epochs over 6 shuffled windows + the 2-window validation with the feature cache
    filled up front in runs of up to 3 consecutive windows (adapt_gcn_batch = 3: GCN passes over several
    single-window tasks), against refcpu.adapt_reference; test_gpu_shapes.py's check_adapt bounds (learning
    rates 1e-12, epoch losses, adapted parameters and validation loss 1e-5)."""
    name = "mixed37"
    d = hybrid_dims(name)
    ei, _ = graphs.get(name)
    P = synth.init_params(nseed(name) + 8, d, gcn_bias_scale=0.1)
    tr, gcn, _ = split(P)
    convs = {k: v for k, v in gcn.items() if k.startswith("base_stgcn.conv")}
    feats = synth.make_features(nseed(name) + 9, d.num_nodes, synth.t_total_for(8, d.window_size, d.forecast_horizon))
    rng = np.random.default_rng(nseed(name))
    orders = np.stack([rng.permutation(6) for _ in range(2)]).astype(np.int32)
    ctx = _capi.Context(d, 0)
    ctx.set_option("adapt_gcn_batch", 3)
    res = adapt_mod.adapt(d, guarded(feats), ei, convs, tr, "Moscow", epochs=2, device=DEV, ctx=ctx, orders=orders)
    assert ctx.adapt_phases()["windows_filled_per_step"] == 0  # nothing was left to the per-step fill
    PT = refcpu.to_torch(P)
    tr_t, gcn_t, _ = split(PT)
    ref_p, ref_losses, ref_lrs, ref_val, _ = refcpu.adapt_reference(tr_t, gcn_t, refcpu.TaskData(feats, ei, d), "Moscow",
                                                                    2, orders=orders)
    finite("adapt", res.theta, res.epoch_losses, res.val_loss)
    assert res.n_train == 6 and res.n_val == 2
    np.testing.assert_allclose(res.lrs, ref_lrs, rtol=1e-12)
    got = params.unpack(res.theta, d, 0)
    e_p = {k: rel(got[k].cpu().numpy(), ref_p[k].numpy()) for k in tr}
    e_l, e_v = rel(res.epoch_losses, ref_losses), abs(res.val_loss - ref_val) / ref_val
    print(f"ERR adapt_steps {name}: epoch losses {e_l:.3g}, parameters {max(e_p.values()):.3g}, validation {e_v:.3g} (1e-5)")
    assert e_l < 1e-5 and e_v < 1e-5
    for k, e in e_p.items():
        assert e < 1e-5, (k, e)
    ctx.close()


# ----------------------------------------------------------------------------- meta_step
MS_K = 2
_MS_ORACLE = {}


@functools.lru_cache(maxsize=None)
def ms_inputs(name):
    d = hybrid_dims(name)
    cfg = MamlConfig(inner_steps=MS_K, batch=HYB_B)
    P = synth.init_params(nseed(name) + 10, d, gcn_bias_scale=0.1)
    feats = [synth.make_features(nseed(name) + 11 + j, d.num_nodes, stream_len_for(cfg, d)) for j in range(2)]
    return d, P, feats


@pytest.mark.parametrize("arm", ["default", "big"])
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", ["mixed37", "fan150"])
def test_meta_step_matches_oracle(name, order, arm):
    """K = 2, 2 tasks, B = 2 on the default (all consecutive) window table; the default knobs and the `big` arm of
    test_gpu_shapes.py, in which the GCN must run once per distinct stream row (gcn_dedup once per forward).
    _check_meta_step's bounds: per-step losses 1e-5, query MSE and meta-gradient 1e-4; adapted parameters 1e-5."""
    d, P, feats = ms_inputs(name)
    theta, gcn, names = split(P)
    ei, _ = graphs.get(name)
    cfg = MamlConfig(inner_steps=MS_K, batch=HYB_B, order=order)
    ml = MetaLearner(d, cfg, gcn, theta, ei, device=DEV, task_group=None)
    ml.set_tasks([guarded(f) for f in feats])
    if arm == "big":
        for k, v in BIG_ARM:
            ml.ctx.set_option(k, v)
    fast = torch.zeros(2, ml.theta.numel(), device=DEV)
    ml.ctx.variant_counts(reset=True)
    res = ml.meta_step(fast_out=fast)
    vc = ml.ctx.variant_counts()
    print(f"{name} order {order} {arm}: {({k: v for k, v in vc.items() if v})}")
    if arm == "big":
        assert vc["gcn_dedup"] == MS_K + 1 and vc["f_compact"] == MS_K + 1 and vc["xg_dedup"] > 0, vc
    finite(f"meta_step {name} order {order} {arm}", res.losses, res.norms, ml.meta_grad, fast)
    qidx = list(ml.default_windows()[-1, 0])
    if (name, order) not in _MS_ORACLE:
        PT = refcpu.to_torch(P)
        _MS_ORACLE[(name, order)] = refcpu.meta_step(
            {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names},
            [refcpu.TaskData(f, ei, d) for f in feats], qidx, MS_K, HYB_B, MS_K * HYB_B, cfg.inner_lr, cfg.max_norm, order)
    ref = _MS_ORACLE[(name, order)]
    losses = res.losses.cpu().numpy()
    mg = params.unpack(ml.meta_grad, d, 0)
    e_step = max(rel(losses[:MS_K, j], [r[0] for r in ref["step_records"][j]]) for j in range(2))
    e_q = max(abs(losses[-1, j] - ref["query_losses"][j]) / ref["query_losses"][j] for j in range(2))
    e_mg = max(rel(mg[k].cpu().numpy(), ref["meta_grad"][k].numpy()) for k in names)
    e_ad = max(rel(params.unpack(fast[j], d, 0)[k].cpu().numpy(), ref["adapted"][j][k].numpy())
               for j in range(2) for k in names)
    print(f"ERR meta_step {name} order {order} {arm}: step losses {e_step:.3g} (1e-5), adapted {e_ad:.3g} (1e-5), "
          f"query MSE {e_q:.3g} (1e-4), meta-gradient {e_mg:.3g} (1e-4)")
    _check_meta_step(res, ml, ref, d, names, 2, MS_K)
    check_adapted(fast, ref, d, names)


# ----------------------------------------------------------------------------- forecast, ensemble, rollout
N_SCORE = 24  # scoreable windows of the stream: room for 2 rollout cycles from origins 0..4


class GraphCase(Case):
    """test_gpu_forecast.py's Case on a fixture graph, its stream between guard bands."""

    def __init__(self, name):
        d = hybrid_dims(name)
        self.d = d
        self.P = synth.init_params(nseed(name) + 13, d, gcn_bias_scale=0.1)
        Ptr, Pg, _ = split(self.P)
        self.ei = graphs.get(name)[0]
        self.feats = synth.make_features(nseed(name) + 14, d.num_nodes,
                                         synth.t_total_for(N_SCORE, d.window_size, d.forecast_horizon))
        self.gcn = params.pack({k: torch.from_numpy(v) for k, v in Pg.items()}, d, which=1, device=DEV)
        self.theta = params.pack({k: torch.from_numpy(v) for k, v in Ptr.items()}, d, device=DEV)
        self.stream = guarded(self.feats)
        self._oracle = {}


_GCASES = {}


def gcase(name):
    if name not in _GCASES:
        _GCASES[name] = GraphCase(name)
    return _GCASES[name]


def test_forecast_matches_oracle():
    """smaml_forecast on mixed37, one pass of consecutive windows (the GCN once per distinct stream row) and
    one of scattered windows: predictions and skill sums 1e-5 (test_gpu_forecast.py's check_against_oracle)."""
    c = gcase("mixed37")
    ctx = c.context()
    for windows, batch, consecutive in ((list(range(5)), 5, True), ([9, 2, 20, 3], 4, False)):
        ctx.variant_counts(reset=True)
        pred, skill = c.run(ctx, windows, batch)
        vc = ctx.variant_counts()
        assert vc["gcn_dedup"] == (1 if consecutive else 0) and vc["fwd_infer"] > 0, vc
        finite(f"forecast {windows}", pred, skill)
        po = c.oracle(windows)
        r, rs = rel(pred, po), relmax(skill, forecast.skill_reference(po, c.feats, windows, c.d, SCALE))
        print(f"ERR forecast mixed37 windows {windows}: pred {r:.3g} (1e-5), skill sums {rs:.3g} (1e-5)")
        assert r <= 1e-5
        assert rs <= 1e-5
    ctx.close()


def test_forecast_ensemble_matches_oracle():
    """smaml_forecast_ensemble on mixed37, 3 members, p_gcn = p_lstm = 0.2 (every member its own GCN features):
    members 1e-5 against refcpu.batch_loss under Dropout(seed, 0.2, 0.2, 0, e), statistics 1e-5 against
    forecast.ensemble_reference (test_gpu_ensemble.py's bounds)."""
    c = gcase("mixed37")
    ctx = c.context()
    windows, members = list(range(5)), 3
    mean, spread, mem, scores = ens.run(c, ctx, windows, 5, members, 0.2, 0.2)
    finite("ensemble", mean, spread, mem, scores)
    Pt, Pg, _ = split(refcpu.to_torch(c.P))
    task = refcpu.TaskData(c.feats, c.ei, c.d)
    want = []
    for e in range(members):
        with torch.no_grad():
            _, preds = refcpu.batch_loss(Pt, Pg, task, windows, refcpu.Dropout(ens.SEED, 0.2, 0.2, 0, e))
        want.append(np.stack([q.numpy() for q in preds]))
    ens.check_members(mem, np.stack(want), "mixed37 p_gcn 0.2")
    m_ref, s_ref, sc_ref = forecast.ensemble_reference(mem, c.feats, windows, c.d, SCALE)
    e = (relmax(mean, m_ref), relmax(spread, s_ref), relmax(scores, sc_ref))
    print(f"ERR ensemble mixed37: mean {e[0]:.3g}, spread {e[1]:.3g}, scores {e[2]:.3g} (1e-5)")
    assert max(e) <= 1e-5
    assert rel(mem[0], mem[1]) > 1e-2  # the members do differ
    ctx.close()


def test_forecast_rollout_matches_oracle_and_reuse_is_bitwise():
    """smaml_forecast_rollout on mixed37, 2 cycles from origins 0..4: roll_reuse 1 and 0 bitwise equal; every
    cycle's predictions 1e-5 against the oracle on the window rebuilt from the GPU's own earlier rows, gap rows
    bitwise (test_gpu_rollout.py's check_teacher_forced); skill sums 1e-5."""
    c = gcase("mixed37")
    ctx = c.context()
    origins, R = list(range(5)), 2
    t1, k1 = tro.run(c, ctx, origins, 5, R, 1)
    ctx.set_option("roll_reuse", 0)
    t0, k0 = tro.run(c, ctx, origins, 5, R, 1)
    finite("rollout", t1, k1, t0, k0)
    assert not np.any(t1 == tro.SENT) and not np.any(k1 == tro.SENT)
    assert np.array_equal(t0, t1) and np.array_equal(k0, k1)
    worst = tro.check_teacher_forced(c, c.feats, t1, origins, R, 1, tro.oracle_forward(c))
    rs = relmax(k1, forecast.rollout_skill_reference(t1, c.feats, origins, c.d, SCALE))
    print(f"ERR rollout mixed37: teacher-forced pred {worst:.3g} (1e-5), skill sums {rs:.3g} (1e-5)")
    assert rs <= 1e-5
    ctx.close()


# ----------------------------------------------------------------------------- the graph of a live context
def test_set_graph_on_a_live_context():
    """forward, forecast and adapt_steps (after adapt_prepare) on mixed37, then smaml_set_graph(chain37) on the
    same context and the three again: bitwise what a fresh context that only ever saw chain37 computes (the five
    graph buffers re-uploaded, the adaptation feature cache invalidated). Then smaml_set_graph(over): SMAML_EINVAL,
    and the next run is bitwise the run before it -- the old graph stays in force, cache included."""
    c = gcase("mixed37")  # N = 37, two layers: the model and the stream; the graph is what changes
    d = c.d
    st = _capi.stream_ptr(torch)
    T, N = d.window_size, d.num_nodes
    xs = [c.stream[w:w + T].reshape(T * N, -1) for w in (1, 4)]
    steps = np.asarray([[0], [3], [1], [0]], np.int32)

    def run_all(ctx):
        pred = torch.full((2, N * d.forecast_horizon, d.output_channels), NAN, device=DEV)
        ctx.forward(st, c.theta, xs, pred)
        fc, _ = c.run(ctx, [0, 1, 2, 6], 4, skill=False)
        ctx.adapt_prepare(st, 1)
        th, m, v = c.theta.clone(), torch.zeros_like(c.theta), torch.zeros_like(c.theta)
        losses = torch.full((len(steps),), NAN, device=DEV)
        ctx.adapt_steps(st, th, m, v, 0, steps, torch.full((len(steps),), 1e-3, device=DEV), (0.9, 0.999), 1e-8, 0.0,
                        1.0, losses)
        torch.cuda.synchronize()
        out = (pred.cpu().numpy(), fc, th.cpu().numpy(), losses.cpu().numpy())
        finite("set_graph", *out)
        return out

    mixed, chain = graphs.get("mixed37")[0], graphs.get("chain37")[0]
    live = c.context()
    assert live.graph_key == mixed.tobytes()
    on_mixed = run_all(live)
    live.set_graph(chain)
    on_chain = run_all(live)
    fresh = c.context()
    fresh.set_graph(chain)  # (before any launch: this context never computes with another graph)
    want = run_all(fresh)
    fresh.close()
    for a, b, m in zip(on_chain, want, on_mixed):
        assert np.array_equal(a, b)
        assert not np.array_equal(a, m)
    assert rel(on_chain[0], on_mixed[0]) > 1e-2  # the two graphs do give different predictions
    with pytest.raises(_capi.SmamlError, match="EINVAL.*in-degree exceeds the ELL width"):
        live.set_graph(graphs.over())
    again = run_all(live)
    for a, b in zip(again, on_chain):
        assert np.array_equal(a, b)
    live.close()
