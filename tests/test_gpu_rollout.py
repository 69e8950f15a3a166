"""GPU tests of ``smaml_forecast_rollout`` (the forecast fed back in, cycle by cycle) against the CPU oracle.

The oracle is fed the GPU's own inputs ("teacher-forced"): for cycle ``j`` the window is rebuilt from the stream
and the GPU's ``traj`` of the cycles before it, and ``oracle.refcpu.hybrid_forward`` runs on that window, so the
prediction bound stays the project's 1e-5 rel-L2 with no allowance for feedback amplification. The rows the
definition fixes exactly -- the gap rows, and through them the fed-back rows a next window holds (the gap row of
cycle ``j + 1`` is formed from private row ``rho0 - 1``, the last row cycle ``j`` fed back) -- are compared
bitwise, the midpoint in numpy float32. Skill sums: 1e-5 relative per entry to ``rollout_skill_reference`` on
the GPU's ``traj``; regrouped passes 1e-6 (f32 block partials in another grouping, combined in double).
"""
import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast
from weatherforecast_stgcn_maml_amd.config import CONFIG1, CONFIG2, ModelDims

from test_gpu_forecast import SCALE, case, relmax
from test_gpu_parity import DEV, build_hybrid, rel

pytestmark = pytest.mark.gpu

SENT = -777.0  # pre-fill of every output buffer


def oracle_forward(c):
    Pt = {k: torch.from_numpy(v) for k, v in c.P.items()}
    eic = torch.from_numpy(c.ei).long()

    def fwd(x):
        with torch.no_grad():
            return refcpu.hybrid_forward(Pt, torch.from_numpy(np.ascontiguousarray(x, np.float32)), eic, c.d).numpy()

    return fwd


def run(c, ctx, origins, batch, R, gap, traj=True, skill=True, scale=SCALE):
    d = c.d
    s = d.forecast_horizon + 1
    t = torch.full((len(origins), R, s, d.num_nodes, d.output_channels), SENT, device=DEV) if traj else None
    k = torch.full((3, R * s, d.output_channels), SENT, device=DEV, dtype=torch.float64) if skill else None
    try:
        ctx.forecast_rollout(_capi.stream_ptr(torch), c.theta, origins, batch, R, gap, scale=scale, traj=t, skill=k)
    finally:
        torch.cuda.synchronize()
    return (t.cpu().numpy() if traj else None), (k.cpu().numpy() if skill else None)


def check_teacher_forced(c, feats, traj, origins, R, gap, fwd):
    """Every cycle's prediction rows against the oracle on the window rebuilt from the GPU's own earlier rows;
    the gap rows bitwise. ``feats`` may carry NaN weather past a window: only channels >= C are taken there."""
    d = c.d
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    s = Hf + 1
    worst = 0.0
    for j in range(R):
        got, want = [], []
        for i, o in enumerate(origins):
            X = np.zeros((T + R * s, N, feats.shape[2]), np.float32)
            X[:T] = feats[o:o + T]
            X[T:T + j * s, :, C:] = feats[o + T:o + T + j * s, :, C:]
            X[T:T + j * s, :, :C] = traj[i, :j].reshape(j * s, N, C)
            win = X[j * s:j * s + T]
            assert np.all(np.isfinite(win))
            want.append(fwd(win.reshape(T * N, -1)))
            got.append(traj[i, j, 1:].reshape(N * Hf, C))  # rows 1..Hf: the memory image of the flat output
            prev = win[T - 1, :, :C]
            gaprow = np.float32(0.5) * (prev + traj[i, j, 1]) if gap else prev
            assert gaprow.dtype == np.float32
            assert np.array_equal(traj[i, j, 0], gaprow), f"gap row of origin {o}, cycle {j}"
        r = rel(np.stack(got), np.stack(want))
        worst = max(worst, r)
        print(f"  cycle {j}: teacher-forced pred rel-L2 {r:.3g}")
        assert r <= 1e-5
    return worst


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [1, 0])
def test_teacher_forced_parity_one_full_tile_plus_a_masked_one(gap):
    c = case(CONFIG1)
    d = c.d
    ctx = c.context()
    ctx.variant_counts(reset=True)
    origins = list(range(11))  # 275 rows: one full 256-row gate tile and a masked one
    R = 3  # private rows reach 24 + 2 * 9 - 1 = 41: the slot table (S = T = 24) wraps
    traj, skill = run(c, ctx, origins, 11, R, gap)
    assert not np.any(traj == SENT) and np.all(np.isfinite(traj))
    fwd = oracle_forward(c)
    check_teacher_forced(c, c.feats, traj, origins, R, gap, fwd)
    assert ctx.variant_counts()["fwd_infer"] > 0
    st = ctx.rollout_stats()
    assert st["cycles"] == R and st["append_launches"] == R and st["graph_rows"] == R * 11
    if gap == 1:  # not asserted: how far the free-running rollouts of the GPU and of the oracle drift apart
        free = forecast.rollout_reference(fwd, c.feats, origins, d, R, gap).reshape(traj.shape)
        for j in range(R):
            print(f"  cycle {j}: free-running divergence rel-L2 {rel(traj[:, j], free[:, j]):.3g}")


# 2 ---------------------------------------------------------------------------------------------------
def test_skill_sums():
    c = case(CONFIG1)
    ctx = c.context()
    origins = list(range(11))
    traj, skill = run(c, ctx, origins, 11, 3, 1)
    assert not np.any(skill == SENT)
    want = forecast.rollout_skill_reference(traj, c.feats, origins, c.d, SCALE)
    r = relmax(skill, want)
    print(f"skill sums max rel {r:.3g}")
    assert r <= 1e-5
    _, only = run(c, ctx, origins, 11, 3, 1, traj=False)  # the sums alone (no traj buffer): the same sums
    assert np.array_equal(only, skill)
    _, unscaled = run(c, ctx, origins, 11, 3, 1, traj=False, scale=None)
    assert relmax(unscaled, forecast.rollout_skill_reference(traj, c.feats, origins, c.d)) <= 1e-5


# 3 ---------------------------------------------------------------------------------------------------
def test_reuse_arm_is_bitwise_the_recompute_arm():
    c = case(CONFIG1)
    d = c.d
    T, s, R = d.window_size, d.forecast_horizon + 1, 3
    origins = list(range(11))
    ctx = c.context()
    t1, k1 = run(c, ctx, origins, 11, R, 1)
    st1 = ctx.rollout_stats()
    ctx.set_option("roll_reuse", 0)
    t0, k0 = run(c, ctx, origins, 11, R, 1)
    st0 = ctx.rollout_stats()
    assert np.array_equal(t0, t1) and np.array_equal(k0, k1)
    n = len(origins)
    assert st1["gcn_rows"] == n * ((T - 1) + (R - 1) * s) and st0["gcn_rows"] == n * R * (T - 1)
    assert st1["xg_rows"] == st1["gcn_rows"] + n * R and st0["xg_rows"] == st0["gcn_rows"] + n * R
    assert st0["graph_rows"] == st1["graph_rows"] == n * R


# 4 ---------------------------------------------------------------------------------------------------
def test_pass_regrouping():
    c = case(CONFIG1)
    ctx = c.context()
    seven = [0, 1, 2, 5, 9, 3, 4]
    t3, k3 = run(c, ctx, seven, 3, 3, 1)  # passes of 3, 3 and 1
    assert ctx.rollout_stats()["cycles"] == 9
    t7, k7 = run(c, ctx, seven, 7, 3, 1)
    assert np.array_equal(t3, t7)  # GEMM rows are independent and the K order does not depend on M
    r = relmax(k3, k7)
    print(f"skill sums, 7 origins at batch 3 vs batch 7: max rel {r:.3g}")
    assert r <= 1e-6


# 5 ---------------------------------------------------------------------------------------------------
def test_one_cycle_against_smaml_forecast():
    c = case(CONFIG1)
    d = c.d
    ctx = c.context()
    windows = list(range(11))
    traj, _ = run(c, ctx, windows, 11, 1, 1, skill=False)
    pred = torch.zeros(len(windows), d.num_nodes * d.forecast_horizon, d.output_channels, device=DEV)
    ctx.forecast(_capi.stream_ptr(torch), c.theta, windows, 11, pred=pred)
    torch.cuda.synchronize()
    pred = pred.cpu().numpy()
    mine = traj[:, 0, 1:].reshape(pred.shape)
    r = rel(mine, pred)
    print(f"R = 1 against smaml_forecast: rel-L2 {r:.3g}, bitwise {np.array_equal(mine, pred)}")
    assert r <= 2e-5  # both lie within 1e-5 of the oracle
    assert rel(mine, c.oracle(windows)) <= 1e-5


# 6 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [4, 1])
def test_short_windows(T):
    """T < s = 9: one cycle appends more rows than a window holds (T = 1: a window has no row t >= 1 at all)."""
    d = ModelDims(num_nodes=25, hidden_channels=32, lstm_hidden_size=32, lstm_num_layers=2, window_size=T)
    c = case(d)
    ctx = c.context()
    origins = list(range(11))
    fwd = oracle_forward(c)
    for gap in (1, 0):
        traj, skill = run(c, ctx, origins, 11, 3, gap)
        check_teacher_forced(c, c.feats, traj, origins, 3, gap, fwd)
        assert relmax(skill, forecast.rollout_skill_reference(traj, c.feats, origins, d, SCALE)) <= 1e-5
    st1 = ctx.rollout_stats()
    ctx.set_option("roll_reuse", 0)
    t0, k0 = run(c, ctx, origins, 11, 3, 0)
    assert np.array_equal(t0, traj) and np.array_equal(k0, skill)
    assert st1["gcn_rows"] == ctx.rollout_stats()["gcn_rows"] == 11 * 3 * (T - 1)  # every row t >= 1 is new


@pytest.mark.parametrize("gap", [1, 0])
def test_config2_four_tiles_the_last_masked(gap):
    c = case(CONFIG2)  # 2 origins x 441 = 882 rows: four 256-row tiles (the last masked); the fused GCN
    ctx = c.context()
    origins = [0, 1]
    traj, skill = run(c, ctx, origins, 2, 2, gap)
    check_teacher_forced(c, c.feats, traj, origins, 2, gap, oracle_forward(c))
    assert relmax(skill, forecast.rollout_skill_reference(traj, c.feats, origins, c.d, SCALE)) <= 1e-5
    ctx.set_option("roll_reuse", 0)
    t0, k0 = run(c, ctx, origins, 2, 2, gap)
    assert np.array_equal(t0, traj) and np.array_equal(k0, skill)


# 7 ---------------------------------------------------------------------------------------------------
def test_nan_guard_and_state_isolation():
    c = case(CONFIG1)
    d = c.d
    T, N, C = d.window_size, d.num_nodes, d.output_channels
    st = _capi.stream_ptr(torch)
    t_obs = 50
    nan_stream = forecast.extend_stream(c.feats[:t_obs], c.feats[t_obs:, :, C:])
    assert np.all(np.isnan(nan_stream[t_obs:, :, :C]))
    zero_stream = np.nan_to_num(nan_stream, nan=0.0)
    origins = [20, 26, 23]  # origin 26: its window ends at the last observation; R = 3 reads 18 rows past it
    out = []
    for f in (nan_stream, zero_stream):
        ctx = c.context()
        ctx.set_tasks([torch.from_numpy(f).to(DEV)])
        out.append(run(c, ctx, origins, 2, 3, 1, skill=False)[0])
    assert np.all(np.isfinite(out[0])) and not np.any(out[0] == SENT)
    assert np.array_equal(out[0], out[1])
    check_teacher_forced(c, nan_stream, out[0], origins, 3, 1, oracle_forward(c))

    # a pending smaml_forward / smaml_backward pair stays valid across a rollout; the workspace is not touched
    xs = [c.stream[w:w + T].reshape(T * N, -1) for w in (3, 8)]
    dpred = torch.from_numpy(np.random.default_rng(0).standard_normal((2, N * d.forecast_horizon, C))
                             .astype(np.float32)).to(DEV)

    def pair(cx, between):
        pred, grad = torch.zeros_like(dpred), torch.zeros_like(c.theta)
        cx.forward(st, c.theta, xs, pred)
        ws = cx.workspace_bytes()
        if between:
            cx.variant_counts(reset=True)
            run(c, cx, list(range(9)), 4, 3, 1)
            assert cx.variant_counts()["fwd_infer"] > 0
            assert cx.workspace_bytes() == ws and cx.forecast_bytes() > 0
        cx.backward(st, c.theta, dpred, grad)
        torch.cuda.synchronize()
        assert bool(grad.abs().sum() > 0)
        return pred.cpu(), grad.cpu()

    cx = c.context()
    want_pred, want_grad = pair(cx, False)
    got_pred, got_grad = pair(cx, True)
    assert torch.equal(got_pred, want_pred) and torch.equal(got_grad, want_grad)


# 8 ---------------------------------------------------------------------------------------------------
def test_rejections_leave_stats_and_outputs_alone():
    c = case(CONFIG1)
    d = c.d
    T, s, R = d.window_size, d.forecast_horizon + 1, 3
    tt = c.feats.shape[0]
    ctx = c.context()
    run(c, ctx, [0, 1], 2, R, 1)
    stats = ctx.rollout_stats()
    last_in = tt - T - (R - 1) * s  # o + T + (R - 1) s == t_total
    last_sc = tt - T - R * s        # o + T + R s == t_total
    run(c, ctx, [0, last_in], 2, R, 1, skill=False)  # the boundaries themselves are admitted
    run(c, ctx, [last_sc], 2, R, 1)
    run(c, ctx, [0, 1], 2, R, 1)
    assert ctx.rollout_stats() == stats
    bad = [([-1], True, "origin 0"), ([0, last_in + 1], False, "origin 1"), ([0, 2, last_sc + 1], True, "origin 2"),
           ([last_in], True, "origin 0"), ([tt], False, "origin 0")]
    for origins, with_skill, msg in bad:
        n = len(origins)
        t = torch.full((n, R, s, d.num_nodes, d.output_channels), SENT, device=DEV)
        k = torch.full((3, R * s, d.output_channels), SENT, device=DEV, dtype=torch.float64)
        with pytest.raises(_capi.SmamlError, match=msg) as ei:
            ctx.forecast_rollout(_capi.stream_ptr(torch), c.theta, origins, 2, R, 1, scale=SCALE, traj=t,
                                 skill=k if with_skill else None)
        assert ei.value.code == 1  # SMAML_EINVAL
        torch.cuda.synchronize()
        assert bool((t == SENT).all()) and bool((k == SENT).all())
        assert ctx.rollout_stats() == stats
    # R = 1 reduces to smaml_forecast's rules
    run(c, ctx, [tt - T], 1, 1, 1, skill=False)
    run(c, ctx, [tt - T - s], 1, 1, 1)
    with pytest.raises(_capi.SmamlError, match="origin 0"):
        run(c, ctx, [tt - T - s + 1], 1, 1, 1)


# 9 ---------------------------------------------------------------------------------------------------
def test_rollout_function_physical_units_and_metrics():
    c = case(CONFIG1)
    d = c.d
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    s, R = Hf + 1, 2
    m = build_hybrid(d, c.P)
    rng = np.random.default_rng(1)
    stats = {"mean": rng.standard_normal(6), "std": rng.uniform(0.5, 2.0, 6)}  # six variables, as the checkpoints'
    ei = torch.from_numpy(c.ei).to(DEV)
    res = forecast.rollout(m, c.stream, ei, stats=stats, cycles=R, gap="midpoint", batch=16)
    want_o = forecast.rollout_origins(c.feats.shape[0], T, Hf, R, True)
    assert res.n_origins == want_o.size == c.feats.shape[0] - T - R * s + 1 and list(res.origins) == list(want_o)
    assert res.cycles == R and res.gap == "midpoint"
    assert res.is_gap.shape == (R * s,) and list(np.flatnonzero(res.is_gap)) == [0, s]
    assert res.traj.shape == (want_o.size, R * s, N, C)
    std, mean = np.ones(C), np.zeros(C)
    std[:6], mean[:6] = stats["std"], stats["mean"]
    # the library's own normalised trajectory, in physical units
    raw, sums = run(c, c.context(), want_o, 16, R, 1, scale=std)
    raw = raw.reshape(want_o.size, R * s, N, C)
    assert rel(res.traj, raw * std + mean) <= 1e-6
    # cycle 0 feeds nothing back: the definition with the oracle as the model, at the prediction tolerance
    ref0 = forecast.rollout_reference(oracle_forward(c), c.feats, want_o, d, 1, "midpoint")
    assert rel(res.traj[:, :s], ref0 * std + mean) <= 1e-5
    # the metrics: skill_metrics' formulas on the reference sums of that trajectory, norig * N pairs per lead
    want = forecast.rollout_skill_reference(raw, c.feats, want_o, d, std)
    assert relmax(sums, want) <= 1e-5
    rmse, mae, prmse, skill = forecast.skill_metrics(want, want_o.size * N)
    for got, ref in ((res.rmse, rmse), (res.mae, mae), (res.persistence_rmse, prmse)):
        assert got.shape == (R * s, C) and relmax(got, ref) <= 1e-5
    assert np.max(np.abs(res.skill - skill)) <= 1e-5
    # forecast only, past the scoreable origins; persistence gap rows repeat the row before them
    res2 = forecast.rollout(m, c.stream, ei, stats=stats, cycles=R, gap="persistence", batch=16, score=False)
    assert res2.n_origins == want_o.size + s and res2.rmse is None and res2.gap == "persistence"
    assert np.array_equal(res2.traj[:want_o.size, 1:s], res.traj[:, 1:s])
    last = (c.feats[T - 1, :, :C] * std + mean).astype(np.float32)
    assert rel(res2.traj[0, 0], last) <= 1e-6
