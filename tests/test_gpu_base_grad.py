"""Gradients through the GCN base of the hybrid model: ``smaml_backward_base`` (C ABI) and the module API's
``base_grad`` switch against torch autograd through the CPU oracle.

The oracle is composed from ``oracle/refcpu.py``: ``stgcn_features`` called OUTSIDE ``no_grad`` (so it is
differentiable), ``batched_forward``, a loss, ``torch.autograd`` with ``requires_grad`` on the conv tensors, on
``x`` and on the trainable tensors. Tolerances are the project's for module gradients
(test_autograd_shim_grads_match_oracle, test_stgcn_autograd_matches_oracle): predictions 1e-5, every gradient
tensor 1e-4, both relative L2 per tensor. Every graph is the 5 x 5 grid (N = 25).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, params, synth
from weatherforecast_stgcn_maml_amd.config import CONFIG1, ModelDims

from test_gpu_parity import DEV, grid_edges, rel, split

pytestmark = pytest.mark.gpu

# name -> (dims, samples, dropout p or 0): each the smallest shape that reaches an edge of k_lstm_dx0 (64 x 128
# tiles over T*M rows x Hc columns, K = 4H) or of the chain behind it
CASES = {
    "cfg1": (CONFIG1, 1, 0.0),
    # 225 rows: a partial last row tile; Hc = 48: a partial column tile; K = 128; L = 1: dG0 is the only slab
    "t3_hc48": (ModelDims(num_nodes=25, window_size=3, input_channels=8, hidden_channels=48, lstm_hidden_size=32,
                          lstm_num_layers=1, forecast_horizon=2, output_channels=2), 3, 0.0),
    # T = 1: every row aggregates over the graph; one narrow column tile; K = 1024
    "t1_hc16": (ModelDims(num_nodes=25, window_size=1, input_channels=4, hidden_channels=16, lstm_hidden_size=256,
                          lstm_num_layers=2, forecast_horizon=1, output_channels=4), 2, 0.0),
    # dropout at every site: the recompute and the gradient take the forward's masks
    "drop": (ModelDims(num_nodes=25, window_size=2, input_channels=8, hidden_channels=64, lstm_hidden_size=64,
                       lstm_num_layers=3, forecast_horizon=2, output_channels=2), 2, 0.2),
}
SEED = 90210


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    d, B, p = CASES[name]
    P = synth.init_params(61, d, gcn_bias_scale=0.1)
    rng = np.random.default_rng(17)
    xs = [rng.standard_normal((d.window_size * d.num_nodes, d.input_channels)).astype(np.float32) for _ in range(B)]
    R = rng.standard_normal((B, d.num_nodes * d.forecast_horizon, d.output_channels)).astype(np.float32)
    return d, B, p, P, xs, R, grid_edges(d)


def oracle_backward(P, xs, ei, d, loss_fn, drop=None):
    """(preds, {name: grad}, [dx]) of loss_fn(preds) with the GCN differentiable (CPU autograd)."""
    Pt = {k: v.clone().requires_grad_(True) for k, v in refcpu.to_torch(P).items()}
    xt = [torch.from_numpy(x).clone().requires_grad_(True) for x in xs]
    eic = torch.from_numpy(ei).long()
    feats = [refcpu.stgcn_features(x, eic, Pt, drop, b, len(xt)) for b, x in enumerate(xt)]
    preds = refcpu.batched_forward(Pt, feats, d, drop)
    loss_fn(preds).backward()
    grads = {k: v.grad.numpy() for k, v in Pt.items() if v.grad is not None}
    return [p.detach().numpy() for p in preds], grads, [x.grad.numpy() for x in xt]


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    d, B, p, P, xs, R, ei = case_inputs(name)
    drop = refcpu.Dropout(SEED, p, p, 0, 0) if p > 0 else None
    return oracle_backward(P, xs, ei, d, lambda preds: sum((q * torch.from_numpy(R[b])).sum()
                                                           for b, q in enumerate(preds)), drop)


class Run:
    """A context with the case's graph, parameters and samples on the device."""

    def __init__(self, name):
        self.d, self.B, self.p, P, xs, R, ei = case_inputs(name)
        d = self.d
        Ptr, Pg, _ = split(P)
        Pg = {k: v for k, v in Pg.items() if k.startswith("base_stgcn.conv")}
        self.ctx = _capi.Context(d, 0)
        self.ctx.set_graph(ei)
        self.gflat = params.pack({k: torch.from_numpy(v) for k, v in Pg.items()}, d, which=1, device=DEV)
        self.ctx.set_gcn_params(self.gflat)
        self.theta = params.pack({k: torch.from_numpy(v) for k, v in Ptr.items()}, d, device=DEV)
        self.xs = [torch.from_numpy(x).to(DEV) for x in xs]
        self.R = torch.from_numpy(R).to(DEV)
        self.st = _capi.stream_ptr(torch)

    def forward(self):
        pred = torch.empty_like(self.R)
        if self.p > 0:
            self.ctx.set_task_ids([0])
            self.ctx.set_dropout(self.p, self.p, SEED)
        self.ctx.forward(self.st, self.theta, self.xs, pred)
        return pred

    def backward_base(self, want_gcn=True, want_dx=True, xs=None):
        grad = torch.full_like(self.theta, float("nan"))
        gg = torch.full_like(self.gflat, float("nan")) if want_gcn else None
        dxs = [torch.full_like(x, float("nan")) for x in self.xs] if want_dx else None
        self.ctx.backward_base(self.st, self.theta, self.xs if xs is None else xs, self.R, grad, gg, dxs)
        torch.cuda.synchronize()
        return grad, gg, dxs


@pytest.mark.parametrize("name", list(CASES))
def test_backward_base_matches_oracle(name):
    """Context.forward + Context.backward_base, loss = sum(pred * R): gcn_grad per tensor (layout which = 1),
    every dx[s] and grad against the oracle."""
    preds_o, g_o, dx_o = case_oracle(name)
    r = Run(name)
    d = r.d
    pred = r.forward()
    grad, gg, dxs = r.backward_base()
    for b in range(r.B):
        e = rel(pred[b].cpu(), preds_o[b])
        print(f"{name} pred[{b}] rel {e:.3e}")
        assert e < 1e-5, (b, e)
    got = dict(params.unpack(grad, d))
    got.update(params.unpack(gg, d, 1))
    assert len(got) == 4 * d.lstm_num_layers + 2 + 8
    for k, v in got.items():
        e = rel(v.cpu(), g_o[k])
        print(f"{name} {k} rel {e:.3e}")
        assert e < 1e-4, (k, e)
    for b in range(r.B):
        e = rel(dxs[b].cpu(), dx_o[b])
        print(f"{name} dx[{b}] rel {e:.3e}")
        assert e < 1e-4, (b, e)
    # the pads of gcn_grad are zero
    used = torch.zeros_like(gg, dtype=torch.bool)
    for _, shape, off in params.gcn_layout(d)[0]:
        used[off:off + int(np.prod(shape))] = True
    assert float(gg[~used].abs().sum()) == 0.0


@pytest.mark.parametrize("name", ["t3_hc48", "drop"])
def test_same_backward_and_repeatable(name):
    """grad of backward_base is smaml_backward's, bitwise; two backward_base runs agree bitwise; so does the
    composed form of the layer-0 input gradient (option dx0_fused = 0: GEMM + relu_mask + copies)."""
    r = Run(name)
    r.forward()
    grad0 = torch.empty_like(r.theta)
    r.ctx.backward(r.st, r.theta, r.R, grad0)
    torch.cuda.synchronize()
    r.forward()
    grad1, gg1, dx1 = r.backward_base()
    assert torch.equal(grad0, grad1)
    r.forward()
    grad2, gg2, dx2 = r.backward_base()
    assert torch.equal(grad1, grad2) and torch.equal(gg1, gg2)
    assert all(torch.equal(a, b) for a, b in zip(dx1, dx2))
    r.ctx.set_option("dx0_fused", 0)
    r.forward()
    grad3, gg3, dx3 = r.backward_base()
    assert torch.equal(grad1, grad3) and torch.equal(gg1, gg3)
    assert all(torch.equal(a, b) for a, b in zip(dx1, dx3))


def test_partial_requests_and_states():
    r = Run("t3_hc48")
    r.forward()
    _, gg, dxs = r.backward_base()
    r.forward()
    _, gg_only, none = r.backward_base(want_dx=False)
    assert none is None and torch.equal(gg, gg_only)
    r.forward()
    _, none, dx_only = r.backward_base(want_gcn=False)
    assert none is None and all(torch.equal(a, b) for a, b in zip(dxs, dx_only))
    # both outputs NULL: EINVAL, and the activations stay
    r.forward()
    with pytest.raises(_capi.SmamlError, match="EINVAL"):
        r.backward_base(want_gcn=False, want_dx=False)
    # another number of samples than the forward's: ESTATE, and the activations stay
    with pytest.raises(_capi.SmamlError, match="ESTATE"):
        r.ctx.backward_base(r.st, r.theta, r.xs[:2], r.R, torch.empty_like(r.theta), torch.empty_like(r.gflat))
    _, gg_again, _ = r.backward_base()
    assert torch.equal(gg, gg_again)
    # consumed: a second call without a forward
    with pytest.raises(_capi.SmamlError, match="ESTATE"):
        r.backward_base()


# ----------------------------------------------------------------------------- module API
def _module(d, P, p):
    from weatherforecast_stgcn_maml_amd.hybrid_model import HybridSTGCN_LSTM
    from weatherforecast_stgcn_maml_amd.model import STGCN

    base = STGCN(d.input_channels, d.hidden_channels, d.output_channels, d.window_size, d.forecast_horizon,
                 dropout_rate=p)
    m = HybridSTGCN_LSTM(base, d.lstm_hidden_size, d.lstm_num_layers, p, d.output_channels, d.forecast_horizon,
                         freeze_base=False, base_grad=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    return m.to(DEV)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_module_base_grad_matches_oracle(train):
    from weatherforecast_stgcn_maml_amd.hybrid_model import draw_dropout_seed

    d = CONFIG1
    P = synth.init_params(67, d, gcn_bias_scale=0.1)
    ei = grid_edges(d)
    x, y = synth.sample_xy(synth.make_features(6700, d.num_nodes, synth.t_total_for(1)), 0)
    m = _module(d, P, 0.2)
    m = m.train() if train else m.eval()
    assert m.base_grad
    eig = torch.from_numpy(ei).to(DEV)
    xg = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).requires_grad_()
    yg = torch.from_numpy(np.ascontiguousarray(y)).to(DEV)
    torch.manual_seed(23)
    pred = m(xg, eig)
    assert pred.grad_fn is not None
    torch.nn.functional.mse_loss(pred, yg).backward()
    torch.manual_seed(23)
    drop = refcpu.Dropout(draw_dropout_seed(), 0.2, 0.2, 0, 0) if train else None
    preds_o, g_o, dx_o = oracle_backward(P, [np.ascontiguousarray(x)], ei, d,
                                         lambda preds: refcpu.mse(preds[0], torch.from_numpy(y)), drop)
    assert rel(pred.detach().cpu(), preds_o[0]) < 1e-5
    sd = dict(m.named_parameters())
    assert len(g_o) == len(sd) - 2
    for k, g in g_o.items():  # every conv tensor and every trainable tensor
        assert sd[k].grad is not None, k
        e = rel(sd[k].grad.cpu(), g)
        print(f"{k} rel {e:.3e}")
        assert e < 1e-4, (k, e)
    e = rel(xg.grad.cpu(), dx_o[0])
    print(f"x rel {e:.3e}")
    assert e < 1e-4
    assert sd["base_stgcn.output_layer.weight"].grad is None and sd["base_stgcn.output_layer.bias"].grad is None
    # a frozen base gets no gradients; x still does
    m.freeze_base_model()
    m.zero_grad(set_to_none=True)
    xg.grad = None
    torch.nn.functional.mse_loss(m(xg, eig), yg).backward()
    assert all(p.grad is None for k, p in sd.items() if k.startswith("base_stgcn."))
    assert sd["lstm.weight_ih_l0"].grad is not None
    assert xg.grad is not None and float(xg.grad.abs().max()) > 0.0
    if not train:
        assert rel(xg.grad.cpu(), dx_o[0]) < 1e-4


def test_end_to_end_sgd_loop_trains_the_base():
    """test_unmodified_sgd_loop_matches_oracle with the whole hybrid trained: six steps of SGD with
    clip_grad_norm_ over ALL parameters, on the module with base_grad=True and on the oracle."""
    d = CONFIG1
    P = synth.init_params(71, d, gcn_bias_scale=0.1)
    ei = grid_edges(d)
    feats = synth.make_features(synth.task_seed(0), d.num_nodes, synth.t_total_for(6))

    def run(model_params, forward, steps=6):
        opt = torch.optim.SGD(model_params, lr=0.01)
        losses = []
        for i in range(steps):
            x, y = synth.sample_xy(feats, i)
            pred, yt = forward(x, y)
            loss = torch.nn.functional.mse_loss(pred, yt)
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model_params, 1.0)
            opt.step()
            losses.append(float(loss.detach()))
        return losses

    m = _module(d, P, 0.0).train()
    eig = torch.from_numpy(ei).to(DEV)
    hip_losses = run(list(m.parameters()),
                     lambda x, y: (m(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), eig),
                                   torch.from_numpy(y).to(DEV)))
    Pt = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in P.items()}
    eic = torch.from_numpy(ei).long()

    def oracle_forward(x, y):
        f = refcpu.stgcn_features(torch.from_numpy(np.ascontiguousarray(x)), eic, Pt)
        return refcpu.batched_forward(Pt, [f], d)[0], torch.from_numpy(y)

    ora_losses = run(list(Pt.values()), oracle_forward)
    print("losses", hip_losses, ora_losses)
    assert np.allclose(hip_losses, ora_losses, rtol=1e-5, atol=0)
    sd = dict(m.named_parameters())
    for k in range(1, 5):
        w = sd[f"base_stgcn.conv{k}.lin.weight"].detach().cpu().numpy()
        assert not np.array_equal(w, P[f"base_stgcn.conv{k}.lin.weight"]), k
        assert rel(w, Pt[f"base_stgcn.conv{k}.lin.weight"].detach()) < 1e-5, k
