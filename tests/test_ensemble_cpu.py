"""CPU statement of the ensemble statistics (``forecast.ensemble_reference`` / ``ensemble_metrics``), the
binding of ``smaml_forecast_ensemble`` and the host logic of ``forecast.ensemble_forecast`` on a stub context."""
import os
import re

import numpy as np
import pytest
import torch

from weatherforecast_stgcn_maml_amd import _capi, forecast, synth
from weatherforecast_stgcn_maml_amd.config import CONFIG1
from weatherforecast_stgcn_maml_amd.hybrid_model import HybridSTGCN_LSTM
from weatherforecast_stgcn_maml_amd.model import STGCN

from test_forecast_cpu import D, hand_case

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 9.0 / 8.0  # member offsets (-DELTA, 0, +DELTA)


def hand_members():
    """Three members around test_forecast_cpu.hand_case: the target of the F4 pairing plus twice that case's
    error -- +2 (r + 1) for variable 0, -2 (r + 1) for variable 1 at flat row r -- plus (-9/8, 0, +9/8).
    Per element: the mean's error is +-2 (r + 1) (>= 2 > 9/8, so every member errs on the same side), the
    unbiased variance is ((9/8)^2 + 0 + (9/8)^2) / 2 = 81/64, and
    CRPS = (1/3) 3 |2 (r + 1)| - (1/18) 2 (9/8 + 18/8 + 9/8) = 2 (r + 1) - 1/2. Everything is dyadic: exact."""
    feats, windows, pred = hand_case()
    T, Hf, N, C = D.window_size, D.forecast_horizon, D.num_nodes, D.output_channels
    y = np.stack([feats[w + T + 1:w + T + 1 + Hf, :, :C].reshape(Hf * N, C) for w in windows])  # F4: row r = h' N + n'
    base = y + 2.0 * (pred - y)
    members = np.stack([base - DELTA, base, base + DELTA]).astype(np.float32)
    return feats, windows, members, base


def test_ensemble_reference_hand_case():
    feats, windows, members, base = hand_members()
    scale = np.array([2.0, 0.5])
    mean, spread, s = forecast.ensemble_reference(members, feats, windows, D, scale)
    assert mean.dtype == spread.dtype == s.dtype == np.float64
    assert mean.shape == spread.shape == (2, 6, 2) and s.shape == (4, 2, 2)
    np.testing.assert_array_equal(mean, base.astype(np.float64))
    np.testing.assert_array_equal(spread, np.full((2, 6, 2), DELTA))
    s2 = scale ** 2
    # errors of the mean: 2, 4, 6 at lead 0 (rows 0..2), 8, 10, 12 at lead 1 (rows 3..5), in both windows
    np.testing.assert_array_equal(s[0], np.array([2 * (4 + 16 + 36) * s2, 2 * (64 + 100 + 144) * s2]))
    # variance 81/64 at each of 2 windows x 3 nodes
    np.testing.assert_array_equal(s[1], np.array([6 * 81 / 64 * s2, 6 * 81 / 64 * s2]))
    # CRPS = |error of the mean| - 1/2
    np.testing.assert_array_equal(s[2], np.array([2 * (2 + 4 + 6 - 1.5) * scale, 2 * (8 + 10 + 12 - 1.5) * scale]))
    # persistence as test_forecast_cpu: y_last - y = -10 (2 + h') at every node
    np.testing.assert_array_equal(s[3], np.array([6 * (20 * scale) ** 2, 6 * (30 * scale) ** 2]))
    assert forecast.ENSEMBLE_SUMS == ("mean_sse", "variance", "crps", "persistence_sse")
    # persistence and (for E = 1, below) the absolute error are skill_reference's own sums
    np.testing.assert_array_equal(s[3], forecast.skill_reference(members[0], feats, windows, D, scale)[2])
    # without a scale the factors are 1
    s1 = forecast.ensemble_reference(members, feats, windows, D)[2]
    np.testing.assert_array_equal(s1[0], s[0] / s2)
    np.testing.assert_array_equal(s1[2], s[2] / scale)


def test_ensemble_reference_is_the_f4_pairing_not_the_model_order():
    feats, windows, members, base = hand_members()
    T, Hf, N = D.window_size, D.forecast_horizon, D.num_nodes
    model_order = 0.0
    for i, w in enumerate(windows):
        for n in range(N):
            for h in range(Hf):
                model_order += float(base[i, n * Hf + h, 0] - feats[w + T + 1 + h, n, 0]) ** 2
    assert model_order != forecast.ensemble_reference(members, feats, windows, D)[2][0, :, 0].sum()
    with pytest.raises(ValueError):
        forecast.ensemble_reference(members[:, :1], feats, [feats.shape[0]], D)


def test_ensemble_reference_properties():
    feats, windows, _, base = hand_members()
    rng = np.random.default_rng(0)
    scale = np.array([1.5, 0.25])
    one = (base + rng.standard_normal(base.shape)).astype(np.float32)[None]
    sae = forecast.skill_reference(one[0], feats, windows, D, scale)[1]
    for members in (one, np.repeat(one, 3, axis=0)):  # E = 1, and identical members
        mean, spread, s = forecast.ensemble_reference(members, feats, windows, D, scale)
        np.testing.assert_allclose(mean, one[0].astype(np.float64), rtol=1e-15)
        assert np.all(spread <= 1e-7) and np.all(s[1] <= 1e-12)
        np.testing.assert_allclose(s[2], sae, rtol=1e-12)  # CRPS = |x - y|
    assert np.all(forecast.ensemble_reference(one, feats, windows, D)[1] == 0)  # E = 1: exactly 0
    # 0 <= CRPS <= the mean member absolute error
    members = (base + rng.standard_normal((5,) + base.shape)).astype(np.float32)
    s = forecast.ensemble_reference(members, feats, windows, D, scale)[2]
    mae = np.mean([forecast.skill_reference(m, feats, windows, D, scale)[1] for m in members], axis=0)
    assert np.all(s[2] >= 0) and np.all(s[2] <= mae)
    # element-wise too: a one-window, one-element view through a unit scale
    x = members[:, 0, 0, 0].astype(np.float64)
    y = float(feats[windows[0] + D.window_size + 1, 0, 0])
    crps = np.abs(x - y).mean() - np.abs(x[:, None] - x[None]).sum() / (2 * x.size ** 2)
    assert 0 <= crps <= np.abs(x - y).mean()


def test_ensemble_metrics():
    sums = np.array([[[8.0, 0.0]], [[2.0, 2.0]], [[3.0, 1.0]], [[32.0, 0.0]]])  # [4, Hf = 1, C = 2], 2 pairs each
    rmse, rms, ratio, crps, prmse = forecast.ensemble_metrics(sums, 2, members=4)
    want = (np.sqrt(sums[0] / 2), np.sqrt(sums[1] / 2), sums[2] / 2, np.sqrt(sums[3] / 2))
    for got, ref in zip((rmse, rms, crps, prmse), want):
        np.testing.assert_array_equal(got, ref)
    assert ratio[0, 0] == np.sqrt(5 / 4 * 2.0 / 8.0) and np.isnan(ratio[0, 1])
    assert forecast.ensemble_metrics(sums, 2, 1)[2][0, 0] == np.sqrt(2 * 2.0 / 8.0)
    with pytest.raises(TypeError):  # E is required: the finite-size factor needs it
        forecast.ensemble_metrics(sums, 2)
    with pytest.raises(ValueError):
        forecast.ensemble_metrics(sums, 2, 0)


def test_binding_of_smaml_forecast_ensemble():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+smaml_forecast_ensemble\s*\(([^)]*)\)\s*;", code)
    assert m, "include/smaml.h does not declare smaml_forecast_ensemble"
    assert len(m.group(1).split(",")) == 16
    assert "smaml_forecast_ensemble" in _capi.EXPORTS
    args, res = _capi._SIGS["smaml_forecast_ensemble"]
    assert len(args) == 16 and res is _capi.I32
    assert _capi.VARIANTS[-1] == "fwd_infer_drop"
    L = _capi.lib()
    assert hasattr(L, "smaml_forecast_ensemble")
    assert L.smaml_abi_version() == _capi.ABI_VERSION


class StubContext:
    """Records what ensemble_forecast asks of the context and answers with known numbers."""

    def __init__(self):
        self.graph_key = None
        self.calls = []

    def set_graph(self, ei):
        self.graph_key = np.ascontiguousarray(ei).tobytes()

    def set_gcn_params(self, flat):
        self.gcn = flat

    def set_tasks(self, feats):
        self.t_total = int(feats[0].shape[0])

    def forecast_ensemble(self, stream, theta, windows, batch, members, p_gcn, p_lstm, seed, task=0, scale=None,
                          mean=None, spread=None, member_pred=None, scores=None):
        self.calls.append(dict(windows=list(windows), batch=batch, members=members, p_gcn=p_gcn, p_lstm=p_lstm,
                               seed=seed, scale=None if scale is None else np.array(scale), scored=scores is not None,
                               with_members=member_pred is not None))
        mean.fill_(2.0)
        spread.fill_(0.5)
        if member_pred is not None:
            for e in range(members):
                member_pred[e] = float(e)
        if scores is not None:
            scores.zero_()
            scores[0], scores[1], scores[2], scores[3] = 16.0, 4.0, 3.0, 64.0


@pytest.fixture
def stubbed(monkeypatch):
    monkeypatch.setattr(_capi, "stream_ptr", lambda torch_mod: 0)
    d = CONFIG1
    base = STGCN(d.input_channels, d.hidden_channels, d.output_channels, d.window_size, d.forecast_horizon,
                 dropout_rate=0.3)
    m = HybridSTGCN_LSTM(base, d.lstm_hidden_size, d.lstm_num_layers, 0.2, d.output_channels, d.forecast_horizon)
    n_score = 5
    feats = synth.make_features(3, d.num_nodes, synth.t_total_for(n_score))
    ei = torch.tensor([[0, 1], [1, 0]])
    return d, m.eval(), feats, ei, n_score


def test_ensemble_forecast_host_logic_on_a_stub_context(stubbed):
    d, m, feats, ei, n_score = stubbed
    N, Hf, C = d.num_nodes, d.forecast_horizon, d.output_channels
    stats = {"mean": np.arange(1.0, 7.0), "std": np.full(6, 2.0)}  # six variables, as the checkpoints'
    ctx = StubContext()
    torch.manual_seed(5)
    res = forecast.ensemble_forecast(m, feats, ei, stats=stats, ctx=ctx)
    call = ctx.calls[-1]
    # defaults: the model's own rates, 16 members, passes of 32, a drawn seed, every scoreable window
    assert (call["p_gcn"], call["p_lstm"]) == (0.3, pytest.approx(0.2)) and (res.p_gcn, res.p_lstm) == (0.3, 0.2)
    assert call["members"] == 16 and call["batch"] == 32 and res.n_members == 16
    assert call["windows"] == list(range(n_score)) and res.n_windows == n_score
    assert 0 <= call["seed"] <= 0xFFFFFFFF and res.seed == call["seed"]
    torch.manual_seed(5)
    from weatherforecast_stgcn_maml_amd.hybrid_model import draw_dropout_seed
    assert call["seed"] == draw_dropout_seed()
    assert call["scored"] and not call["with_members"] and res.members is None
    std, mean = np.ones(C), np.zeros(C)
    std[:6], mean[:6] = 2.0, np.arange(1.0, 7.0)
    np.testing.assert_array_equal(call["scale"], std.astype(np.float32))
    # physical units: mean * std + mean, spread * std
    assert res.mean.shape == res.spread.shape == (n_score, Hf, N, C)
    np.testing.assert_array_equal(res.mean[0, 0, 0], (2.0 * std + mean).astype(np.float32))
    np.testing.assert_array_equal(res.spread[0, 0, 0], (0.5 * std).astype(np.float32))
    cnt = n_score * N
    for got, ref in ((res.rmse, np.sqrt(16.0 / cnt)), (res.rms_spread, np.sqrt(4.0 / cnt)), (res.crps, 3.0 / cnt),
                     (res.persistence_rmse, np.sqrt(64.0 / cnt)), (res.spread_skill, np.sqrt(17 / 16 * 4.0 / 16.0))):
        assert got.shape == (Hf, C) and np.all(got == ref)

    # explicit arguments; forecasting past the end of the stream without scores; the members
    res = forecast.ensemble_forecast(m, feats, ei, stats=stats, members=3, p_gcn=0.0, p_lstm=0.1, seed=2 ** 32 + 7,
                                     batch=4, score=False, return_members=True, ctx=ctx)
    call = ctx.calls[-1]
    assert (call["members"], call["p_gcn"], call["p_lstm"], call["seed"], call["batch"]) == (3, 0.0, 0.1, 7, 4)
    assert call["windows"] == list(range(n_score + Hf + 1)) and not call["scored"] and call["scale"] is None
    assert res.rmse is None and res.crps is None and res.spread_skill is None
    assert res.members.shape == (3, n_score + Hf + 1, Hf, N, C)
    np.testing.assert_array_equal(res.members[2, 0, 0, 0], (2.0 * std + mean).astype(np.float32))
    res = forecast.ensemble_forecast(m, feats, ei, windows=[4, 1], members=2, seed=1, ctx=ctx)
    assert ctx.calls[-1]["windows"] == [4, 1] and list(res.windows) == [4, 1]

    # the empty-window result: nothing is asked of the context
    ncalls = len(ctx.calls)
    res = forecast.ensemble_forecast(m, feats[:d.window_size + Hf], ei, members=4, seed=9, ctx=ctx)
    assert res.n_windows == 0 and res.mean is None and res.spread is None and res.rmse is None
    assert res.n_members == 4 and res.seed == 9 and len(ctx.calls) == ncalls
    # without a context a CPU model has nowhere to run (the model of this test lives on the CPU)
    with pytest.raises(_capi.SmamlError, match="HIP device"):
        forecast.ensemble_forecast(m, feats, ei)
