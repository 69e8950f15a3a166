"""GPU parity of ``smaml_forecast_ensemble`` (the MC-dropout inference step over the member axis, the shared
layer 0, the member groups, the statistics kernel) against the CPU oracle: member ``e`` of a window list is
``refcpu.batch_loss(Pt, Pg, task, windows, refcpu.Dropout(seed, p_gcn, p_lstm, 0, e))`` -- one training batch
holding the whole list -- and the statistics are ``forecast.ensemble_reference``.

Tolerances: members <= 1e-5 rel-L2 (the project's tolerance for train-mode dropout predictions,
test_gpu_api.py); statistics <= 1e-5 relative per entry; the same windows in other passes <= 1e-6 (f32 block
partials in another grouping, combined in double); other sharing / grouping options: bitwise.
"""
import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast
from weatherforecast_stgcn_maml_amd.config import CONFIG1, CONFIG2, ModelDims

from test_gpu_forecast import N_SCORE, SCALE, case, relmax
from test_gpu_parity import DEV, build_hybrid, rel, split

pytestmark = pytest.mark.gpu

SEED = 20240607
ELEVEN = list(range(11))  # 11 x 25 = 275 rows: one full 256-row gate tile and a masked one
_ORACLE = {}
_RUNS = {}


def oracle(c, windows, p_gcn, p_lstm, members, seed=SEED):
    """[E, nwin, N*Hf, C]: the members of `windows` as one training batch (computed once per argument set)."""
    out = []
    for e in range(members):
        key = (c.d, tuple(windows), p_gcn, p_lstm, seed, e)
        if key not in _ORACLE:
            Pt, Pg, _ = split(refcpu.to_torch(c.P))
            task = refcpu.TaskData(c.feats, c.ei, c.d)
            with torch.no_grad():
                _, preds = refcpu.batch_loss(Pt, Pg, task, list(windows), refcpu.Dropout(seed, p_gcn, p_lstm, 0, e))
            _ORACLE[key] = np.stack([p.numpy() for p in preds])
        out.append(_ORACLE[key])
    return np.stack(out)


def run(c, ctx, windows, batch, members, p_gcn, p_lstm, seed=SEED, scores=True, scale=SCALE, outputs="msep"):
    """(mean, spread, member_pred, scores) as numpy (None where not asked for: `outputs` letters m, s, e, p)."""
    d = c.d
    rows, C = d.num_nodes * d.forecast_horizon, d.output_channels
    mean = torch.zeros(len(windows), rows, C, device=DEV) if "m" in outputs else None
    spread = torch.zeros(len(windows), rows, C, device=DEV) if "s" in outputs else None
    mem = torch.zeros(members, len(windows), rows, C, device=DEV) if "e" in outputs else None
    sc = torch.zeros(4, d.forecast_horizon, C, device=DEV, dtype=torch.float64) if scores and "p" in outputs else None
    ctx.forecast_ensemble(_capi.stream_ptr(torch), c.theta, windows, batch, members, p_gcn, p_lstm, seed, scale=scale,
                          mean=mean, spread=spread, member_pred=mem, scores=sc)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (mean, spread, mem, sc))


def all_sites():
    """The all-sites case (tests 1 and 3 share its GPU run): CONFIG1, windows 0..10, E = 3, p = 0.2 / 0.2."""
    if "all" not in _RUNS:
        c = case(CONFIG1)
        ctx = c.context()
        ctx.variant_counts(reset=True)
        out = run(c, ctx, ELEVEN, 11, 3, 0.2, 0.2)
        _RUNS["all"] = (out, ctx.variant_counts(), ctx.workspace_bytes(), ctx.forecast_bytes())
    return _RUNS["all"]


def check_members(got, want, what):
    assert got.shape == want.shape
    for e in range(got.shape[0]):
        r = rel(got[e], want[e])
        print(f"{what}: member {e} rel-L2 {r:.3g}")
        assert r <= 1e-5


# 1 ---------------------------------------------------------------------------------------------------
def test_oracle_parity_all_sites_on():
    c = case(CONFIG1)
    (mean, spread, mem, scores), vc, wb, fb = all_sites()
    want = oracle(c, ELEVEN, 0.2, 0.2, 3)
    check_members(mem, want, "all sites")
    assert vc["fwd_infer_drop"] > 0 and vc["fwd_infer"] == 0 and vc["fwd"] == 0 and vc["fwd_drop"] == 0
    assert vc["gcn_dedup"] == 0 and vc["xg_dedup"] == 0  # GCN dropout: every member its own features
    assert wb == 0 and fb > 0
    # the members are different draws, and none is the eval forecast
    ev = c.oracle(ELEVEN)
    for a, b in ((mem[0], mem[1]), (mem[0], mem[2]), (mem[1], mem[2]), (mem[0], ev), (mem[1], ev), (mem[2], ev)):
        assert rel(a, b) > 1e-2


# 2 ---------------------------------------------------------------------------------------------------
def test_shared_path_counts_sharing_and_grouping():
    c = case(CONFIG1)
    ctx = c.context()
    got = {}
    for members in (3, 2):
        ctx.variant_counts(reset=True)
        got[members] = run(c, ctx, ELEVEN, 11, members, 0.0, 0.2)
        vc = ctx.variant_counts()
        # one pass: the GCN and layer 0's projection once, whatever E is
        assert vc["gcn_dedup"] == 1 and vc["xg_dedup"] == 1 and vc["f_compact"] == 1
        assert vc["fwd_infer_drop"] == c.d.window_size + c.d.lstm_num_layers - 1
    check_members(got[3][2], oracle(c, ELEVEN, 0.0, 0.2, 3), "shared")
    assert np.array_equal(got[2][2], got[3][2][:2])  # a member does not depend on how many there are
    ctx.set_option("ens_share", 0)
    unshared = run(c, ctx, ELEVEN, 11, 3, 0.0, 0.2)
    ctx.set_option("ens_share", 1)
    ctx.set_option("ens_group", 1)
    ctx.variant_counts(reset=True)
    one = run(c, ctx, ELEVEN, 11, 3, 0.0, 0.2)
    assert ctx.variant_counts()["fwd_infer_drop"] == 3 * (c.d.window_size + c.d.lstm_num_layers - 1)
    ctx.set_option("ens_group", 2)  # a full group and a partial one
    two = run(c, ctx, ELEVEN, 11, 3, 0.0, 0.2)
    ctx.set_option("ens_group", 0)
    allm = run(c, ctx, ELEVEN, 11, 3, 0.0, 0.2)
    for other in (unshared, one, two, allm):
        for a, b in zip(other, got[3]):
            assert np.array_equal(a, b)
    # grouping with GCN dropout too (per-member features)
    ref = all_sites()[0]
    ctx.set_option("ens_group", 2)
    for a, b in zip(run(c, ctx, ELEVEN, 11, 3, 0.2, 0.2), ref):
        assert np.array_equal(a, b)


# 3 ---------------------------------------------------------------------------------------------------
def test_statistics_against_the_reference():
    c = case(CONFIG1)
    (mean, spread, mem, scores), _, _, _ = all_sites()
    m_ref, s_ref, sc_ref = forecast.ensemble_reference(mem, c.feats, ELEVEN, c.d, SCALE)
    r_mean, r_spread, r_sc = relmax(mean, m_ref), relmax(spread, s_ref), relmax(scores, sc_ref)
    print(f"against the GPU's own members: mean {r_mean:.3g}, spread {r_spread:.3g}, scores {r_sc:.3g} (max rel)")
    assert r_mean <= 1e-5 and r_spread <= 1e-5 and r_sc <= 1e-5
    _, _, sc_or = forecast.ensemble_reference(oracle(c, ELEVEN, 0.2, 0.2, 3), c.feats, ELEVEN, c.d, SCALE)
    for k in (0, 2, 3):
        r = relmax(scores[k], sc_or[k])
        print(f"scores[{k}] against the oracle's members: max rel {r:.3g}")
        assert r <= 1e-5
    # The variance rests on differences of members, so it amplifies the members' 1e-5 tolerance. Probe (CPU):
    # the oracle's members with noise of 1e-5 rel-L2 per member move scores[1] by VAR_PROBE = 6e-6 relative
    # (the figure this test was specified with; repeating the probe on this very case with Gaussian noise, 20
    # draws, gave a median of 1.0e-5 and a maximum of 1.3e-5 per entry -- the smaller figure is kept). The
    # bound is 10 x the probe.
    VAR_PROBE = 6e-6
    r = relmax(scores[1], sc_or[1])
    print(f"scores[1] (variance) against the oracle's members: max rel {r:.3g} (bound {10 * VAR_PROBE:.3g})")
    assert r <= 10 * VAR_PROBE


# 4 ---------------------------------------------------------------------------------------------------
def test_pass_independence():
    c = case(CONFIG1)
    ctx = c.context()
    seven = list(range(7))
    want = oracle(c, seven, 0.2, 0.2, 2)
    ctx.variant_counts(reset=True)
    o3 = run(c, ctx, seven, 3, 2, 0.2, 0.2)  # passes of 3, 3 and 1
    o7 = run(c, ctx, seven, 7, 2, 0.2, 0.2)
    check_members(o3[2], want, "7 windows at batch 3")  # wrong mask offsets would differ at O(1)
    check_members(o7[2], want, "7 windows at batch 7")
    r = relmax(o3[3], o7[3])
    print(f"scores, 7 windows at batch 3 vs batch 7: max rel {r:.3g}")
    assert r <= 1e-6
    # the shared path cut into passes (consecutive passes of 3, 3, then one window without dedup)
    s3 = run(c, ctx, seven, 3, 2, 0.0, 0.2)
    check_members(s3[2], oracle(c, seven, 0.0, 0.2, 2), "shared, 7 windows at batch 3")
    odd = [9, 2, 30, 3]
    ctx.variant_counts(reset=True)
    for p_gcn in (0.2, 0.0):
        got = run(c, ctx, odd, 4, 2, p_gcn, 0.2)
        check_members(got[2], oracle(c, odd, p_gcn, 0.2, 2), f"non-consecutive, p_gcn {p_gcn}")
    vc = ctx.variant_counts()
    assert vc["gcn_dedup"] == 0 and vc["xg_dedup"] == 0 and vc["fwd_infer_drop"] > 0


# 5 ---------------------------------------------------------------------------------------------------
def test_zero_probabilities_are_the_deterministic_forecast():
    c = case(CONFIG1)
    ctx = c.context()
    pred, skill = c.run(ctx, ELEVEN, 4)
    mean, spread, mem, scores = run(c, ctx, ELEVEN, 4, 2, 0.0, 0.0)
    assert np.array_equal(mem[0], pred) and np.array_equal(mem[1], pred)
    assert np.array_equal(mean, pred)
    assert np.all(spread == 0) and np.all(scores[1] == 0)
    assert relmax(scores[0], skill[0]) <= 1e-6 and relmax(scores[3], skill[2]) <= 1e-6
    assert relmax(scores[2], skill[1]) <= 1e-6  # CRPS of identical members = the absolute error


# 6 ---------------------------------------------------------------------------------------------------
def test_hidden_128_dispatch():
    """CONFIG2 x 2 windows = 882 rows: four 256-row tiles (the last masked) x four 32-unit groups."""
    c = case(CONFIG2)
    ctx = c.context()
    got = run(c, ctx, [0, 1], 2, 2, 0.0, 0.2, outputs="e")
    check_members(got[2], oracle(c, [0, 1], 0.0, 0.2, 2), "CONFIG2")


# 6b --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 2])
def test_layer_counts(layers):
    """One layer: layer 0 is the top layer, whose h_T every member masks (kind 3) and hands to the head, so
    there is no layer above to share it with (ens_share must not leave members 1.. unwritten); no kind-2 site
    exists. Two layers: the smallest stack with a shared layer 0, and an even ring depth."""
    d = ModelDims(num_nodes=25, hidden_channels=32, lstm_hidden_size=32, lstm_num_layers=layers)
    c = case(d)
    ctx = c.context()
    # poison the rings first: a larger pass with other masks leaves every slot of every member written
    run(c, ctx, list(range(12, 23)), 11, 3, 0.0, 0.5, seed=SEED + 1, outputs="e")
    got = run(c, ctx, ELEVEN, 11, 3, 0.0, 0.2)
    check_members(got[2], oracle(c, ELEVEN, 0.0, 0.2, 3), f"{layers} layer(s), shared path")
    assert rel(got[2][0], got[2][1]) > 1e-2 and rel(got[2][1], got[2][2]) > 1e-2  # the head-input masks differ
    ctx.set_option("ens_share", 0)
    for a, b in zip(run(c, ctx, ELEVEN, 11, 3, 0.0, 0.2), got):
        assert np.array_equal(a, b)
    ctx.set_option("ens_share", 1)
    fresh = c.context()  # never-written rings
    for a, b in zip(run(c, fresh, ELEVEN, 11, 3, 0.0, 0.2), got):
        assert np.array_equal(a, b)
    odd = [5, 1, 20]
    both = run(c, ctx, odd, 2, 2, 0.2, 0.2)
    check_members(both[2], oracle(c, odd, 0.2, 0.2, 2), f"{layers} layer(s), all sites, passes of 2 and 1")


# 7 ---------------------------------------------------------------------------------------------------
def test_repeatable_state_isolation_and_errors():
    c = case(CONFIG1)
    d = c.d
    st = _capi.stream_ptr(torch)
    windows = list(range(9))
    ctx = c.context()
    a = run(c, ctx, windows, 4, 3, 0.2, 0.2)
    b = run(c, ctx, windows, 4, 3, 0.2, 0.2)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert ctx.workspace_bytes() == 0

    # a pending smaml_forward / smaml_backward pair stays valid across an ensemble call, the workspace
    # keeps its size, and a following smaml_forecast is unchanged
    T, N = d.window_size, d.num_nodes
    xs = [c.stream[w:w + T].reshape(T * N, -1) for w in (3, 8)]
    dpred = torch.from_numpy(np.random.default_rng(0).standard_normal((2, N * d.forecast_horizon, d.output_channels))
                             .astype(np.float32)).to(DEV)

    def pair(cx, between):
        pred, grad = torch.zeros_like(dpred), torch.zeros_like(c.theta)
        cx.forward(st, c.theta, xs, pred)
        ws = cx.workspace_bytes()
        if between:
            run(c, cx, windows, 4, 3, 0.2, 0.2)
            run(c, cx, windows, 4, 3, 0.0, 0.2)
        assert cx.workspace_bytes() == ws
        cx.backward(st, c.theta, dpred, grad)
        torch.cuda.synchronize()
        assert bool(grad.abs().sum() > 0)
        return pred.cpu(), grad.cpu()

    cx = c.context()
    want_fc = c.run(cx, windows, 4)
    want_pred, want_grad = pair(cx, False)
    got_pred, got_grad = pair(cx, True)
    assert torch.equal(got_pred, want_pred) and torch.equal(got_grad, want_grad)
    got_fc = c.run(cx, windows, 4)
    assert np.array_equal(got_fc[0], want_fc[0]) and np.array_equal(got_fc[1], want_fc[1])

    # 64 members (the statistics kernel's largest LDS footprint) against the reference
    mean, spread, mem, scores = run(c, ctx, [0, 1], 2, 64, 0.0, 0.2)
    m_ref, s_ref, sc_ref = forecast.ensemble_reference(mem, c.feats, [0, 1], d, SCALE)
    assert relmax(mean, m_ref) <= 1e-5 and relmax(spread, s_ref) <= 1e-5 and relmax(scores, sc_ref) <= 1e-5

    # every EINVAL case of the header
    t_total = c.feats.shape[0]
    last = t_total - T
    one = torch.zeros(1, N * d.forecast_horizon, d.output_channels, device=DEV)
    for members in (0, 65, -1):
        with pytest.raises(_capi.SmamlError, match="members"):
            ctx.forecast_ensemble(st, c.theta, [0], 4, members, 0.0, 0.2, SEED, mean=one)
    for p_gcn, p_lstm in ((1.0, 0.2), (0.2, 1.0), (-0.1, 0.2), (0.2, -0.1), (float("nan"), 0.2)):
        with pytest.raises(_capi.SmamlError, match="probabilities"):
            run(c, ctx, [0], 4, 2, p_gcn, p_lstm)
    with pytest.raises(_capi.SmamlError, match="all NULL"):
        run(c, ctx, [0], 4, 2, 0.0, 0.2, outputs="")
    with pytest.raises(_capi.SmamlError, match="window 0"):
        run(c, ctx, [last], 4, 2, 0.0, 0.2)  # scores need the targets
    with pytest.raises(_capi.SmamlError, match="window 1"):
        run(c, ctx, [0, N_SCORE], 4, 2, 0.0, 0.2)
    with pytest.raises(_capi.SmamlError, match="window 0"):
        run(c, ctx, [last + 1], 4, 2, 0.0, 0.2, scores=False)
    with pytest.raises(_capi.SmamlError):
        run(c, ctx, [-1], 4, 2, 0.0, 0.2, scores=False)
    with pytest.raises(_capi.SmamlError, match="aligned"):
        ctx.forecast_ensemble(st, c.theta[1:], [0], 4, 2, 0.0, 0.2, SEED, mean=one)
    # ... and a window past the end is fine without scores
    mean, spread, _, _ = run(c, ctx, [last], 4, 2, 0.0, 0.2, scores=False, outputs="ms")
    assert np.all(np.isfinite(mean)) and bool(spread.max() > 0)


# the Python entry ------------------------------------------------------------------------------------
def test_ensemble_forecast_function_physical_units_and_metrics():
    c = case(CONFIG1)
    d = c.d
    m = build_hybrid(d, c.P)
    ei = torch.from_numpy(c.ei).to(DEV)
    rng = np.random.default_rng(1)
    stats = {"mean": rng.standard_normal(6), "std": rng.uniform(0.5, 2.0, 6)}  # six variables, as the checkpoints'
    E, windows = 3, list(range(N_SCORE))
    res = forecast.ensemble_forecast(m, c.stream, ei, stats=stats, members=E, p_gcn=0.0, p_lstm=0.2, seed=SEED,
                                     batch=16, return_members=True)
    assert res.n_windows == N_SCORE and list(res.windows) == windows and res.n_members == E
    std, mean = np.ones(12), np.zeros(12)
    std[:6], mean[:6] = stats["std"], stats["mean"]
    mo = oracle(c, windows, 0.0, 0.2, E)
    shape = (N_SCORE, d.forecast_horizon, d.num_nodes, d.output_channels)
    assert res.members.shape == (E,) + shape and res.mean.shape == res.spread.shape == shape
    assert rel(res.members, (mo * std + mean).reshape((E,) + shape)) <= 1e-5
    m_ref, s_ref, sums = forecast.ensemble_reference(mo, c.feats, windows, d, std)
    assert rel(res.mean, (m_ref * std + mean).reshape(shape)) <= 1e-5
    # the spread in physical units is the normalised members' spread times std (no shift)
    own = forecast.ensemble_reference((res.members - mean) / std, c.feats, windows, d, std)[1].reshape(shape) * std
    assert rel(res.spread, own) <= 1e-4  # (members rounded to f32 in physical units and back)
    rmse, rms, ratio, crps, prmse = forecast.ensemble_metrics(sums, N_SCORE * d.num_nodes, E)
    for got, ref in ((res.rmse, rmse), (res.crps, crps), (res.persistence_rmse, prmse)):
        assert got.shape == (d.forecast_horizon, d.output_channels) and relmax(got, ref) <= 1e-5
    assert res.rms_spread.shape == res.spread_skill.shape == (d.forecast_horizon, d.output_channels)
    assert np.all(res.rms_spread > 0) and np.all(np.isfinite(res.spread_skill))
    # the model's own rates are the default (this model was built with none: the deterministic forecast)
    res0 = forecast.ensemble_forecast(m, c.stream, ei, stats=stats, members=2, batch=16)
    assert (res0.p_gcn, res0.p_lstm) == (0.0, 0.0) and np.all(res0.spread == 0)
    det = forecast.forecast(m, c.stream, ei, stats=stats, batch=16)
    assert np.array_equal(res0.mean, det.pred)
    # forecast only, to the end of the stream
    res2 = forecast.ensemble_forecast(m, c.stream, ei, stats=stats, members=2, p_gcn=0.0, p_lstm=0.2, seed=SEED,
                                      batch=16, score=False)
    assert res2.n_windows == N_SCORE + d.forecast_horizon + 1 and res2.rmse is None and res2.crps is None
    assert res2.mean.shape[0] == res2.n_windows and np.all(np.isfinite(res2.mean)) and bool(res2.spread.max() > 0)
