"""GPU tests of ``smaml_forecast_rollout_ensemble`` (MC-dropout members, each fed its own forecast back in)
against the CPU oracle.

Teacher-forced, as test_gpu_rollout.py: for member ``e`` and cycle ``j`` the windows of ALL origins are rebuilt
from the stream and that member's own earlier ``member_traj`` rows, and the oracle member runs on them as one
training batch holding the whole origin list -- ``refcpu.stgcn_features(x_i, ei, Pg, drop, i, norig)`` per origin,
then ``refcpu.batched_forward(P, feats, dims, drop)`` with ``drop = refcpu.Dropout(seed, p_gcn, p_lstm, 0, 64 j +
e)`` -- so the prediction bound stays 1e-5 rel-L2 at every cycle. Gap rows are bitwise the numpy f32 rule.
Statistics: 1e-5 max-relative to ``forecast.ensemble_rollout_reference`` on the GPU's own members; sums regrouped
across passes 1e-6; other groupings / sharing options bitwise.
"""
import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast
from weatherforecast_stgcn_maml_amd.config import CONFIG1, CONFIG2, ModelDims

from test_gpu_forecast import SCALE, case, relmax
from test_gpu_parity import DEV, build_hybrid, rel, split

pytestmark = pytest.mark.gpu

SENT = -777.0  # pre-fill of every output buffer
SEED = 20240607
ELEVEN = list(range(11))  # 11 x 25 = 275 rows: one full 256-row gate tile and a masked one
_RUNS = {}


def run(c, ctx, origins, batch, R, E, p_gcn, p_lstm, gap=1, seed=SEED, scale=SCALE, outputs="tmsp", stream=None):
    """(member_traj, mean, spread, scores) as numpy, each pre-filled with SENT (None where not asked for: letters
    t, m, s, p of `outputs`)."""
    d = c.d
    s, N, C = d.forecast_horizon + 1, d.num_nodes, d.output_channels
    n = len(origins)
    t = torch.full((E, n, R, s, N, C), SENT, device=DEV) if "t" in outputs else None
    m = torch.full((n, R, s, N, C), SENT, device=DEV) if "m" in outputs else None
    sp = torch.full((n, R, s, N, C), SENT, device=DEV) if "s" in outputs else None
    sc = torch.full((4, R * s, C), SENT, device=DEV, dtype=torch.float64) if "p" in outputs else None
    try:
        ctx.forecast_rollout_ensemble(_capi.stream_ptr(torch), c.theta, origins, batch, R, E, p_gcn, p_lstm, seed,
                                      gap=gap, scale=scale, member_traj=t, mean=m, spread=sp, scores=sc)
    finally:
        torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in (t, m, sp, sc))


def oracle_member(c, windows, p_gcn, p_lstm, step, seed=SEED):
    """[norig, N*Hf, C]: the train-mode forward of the windows [norig, T*N, Cin] as one batch under the masks of
    `step`."""
    P = refcpu.to_torch(c.P)
    _, Pg, _ = split(P)
    eic = torch.from_numpy(c.ei).long()
    drop = refcpu.Dropout(seed, p_gcn, p_lstm, 0, step)
    n = len(windows)
    with torch.no_grad():
        feats = [refcpu.stgcn_features(torch.from_numpy(np.ascontiguousarray(x, np.float32)), eic, Pg, drop, i, n)
                 for i, x in enumerate(windows)]
        return np.stack([p.numpy() for p in refcpu.batched_forward(P, feats, c.d, drop)])


def check_teacher_forced(c, feats, mt, origins, R, gap, p_gcn, p_lstm, seed=SEED):
    """Every member's and cycle's prediction rows against the oracle member on the windows rebuilt from the GPU's
    own earlier rows of that member; the gap rows bitwise."""
    d = c.d
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    s = Hf + 1
    worst = 0.0
    assert not np.any(mt == SENT) and np.all(np.isfinite(mt))
    for e in range(mt.shape[0]):
        for j in range(R):
            wins, got = [], []
            for i, o in enumerate(origins):
                X = np.zeros((T + R * s, N, feats.shape[2]), np.float32)
                X[:T] = feats[o:o + T]
                X[T:T + j * s, :, C:] = feats[o + T:o + T + j * s, :, C:]
                X[T:T + j * s, :, :C] = mt[e, i, :j].reshape(j * s, N, C)
                win = X[j * s:j * s + T]
                assert np.all(np.isfinite(win))
                wins.append(win.reshape(T * N, -1))
                got.append(mt[e, i, j, 1:].reshape(N * Hf, C))  # rows 1..Hf: the memory image of the flat output
                prev = win[T - 1, :, :C]
                gaprow = np.float32(0.5) * (prev + mt[e, i, j, 1]) if gap else prev
                assert gaprow.dtype == np.float32
                assert np.array_equal(mt[e, i, j, 0], gaprow), f"gap row of member {e}, origin {o}, cycle {j}"
            want = oracle_member(c, wins, p_gcn, p_lstm, 64 * j + e, seed)
            r = rel(np.stack(got), want)
            worst = max(worst, r)
            print(f"  member {e} cycle {j}: teacher-forced pred rel-L2 {r:.3g}")
            assert r <= 1e-5
    return worst


def base_run(p_gcn, gap):
    """CONFIG1, origins 0..10 in one pass, E = 3, R = 3 (the slot table, S = T = 24, wraps), p_lstm = 0.2: shared
    by the parity, statistics and invariance tests."""
    key = (p_gcn, gap)
    if key not in _RUNS:
        c = case(CONFIG1)
        ctx = c.context()
        ctx.variant_counts(reset=True)
        out = run(c, ctx, ELEVEN, 11, 3, 3, p_gcn, 0.2, gap)
        _RUNS[key] = (out, ctx.rollout_ensemble_stats(), ctx.variant_counts())
    return _RUNS[key]


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [1, 0])
@pytest.mark.parametrize("p_gcn", [0.2, 0.0])
def test_teacher_forced_parity_per_member(p_gcn, gap):
    c = case(CONFIG1)
    (mt, mean, spread, scores), st, vc = base_run(p_gcn, gap)
    for x in (mt, mean, spread, scores):
        assert not np.any(x == SENT) and np.all(np.isfinite(x))
    check_teacher_forced(c, c.feats, mt, ELEVEN, 3, gap, p_gcn, 0.2)
    assert vc["fwd_infer_drop"] > 0 and vc["fwd_infer"] == 0 and vc["fwd"] == 0
    assert st["cycles"] == 3 and st["append_launches"] == 3 and st["member_groups"] == 1
    # the members are different draws from cycle 0 on, and drift further apart
    assert rel(mt[0, :, 0, 1:], mt[1, :, 0, 1:]) > 1e-3 and rel(mt[0, :, 2], mt[2, :, 2]) > 1e-3


# 2 ---------------------------------------------------------------------------------------------------
def test_statistics_against_the_reference():
    c = case(CONFIG1)
    d = c.d
    (mt, mean, spread, scores), _, _ = base_run(0.0, 0)  # persistence: cycle 0's gap row is the same in every member
    m_ref, s_ref, q_ref = forecast.ensemble_rollout_reference(mt, c.feats, ELEVEN, d, SCALE)
    K = 3 * (d.forecast_horizon + 1)
    mean, spread = mean.reshape(m_ref.shape), spread.reshape(s_ref.shape)
    assert np.array_equal(mt[0, :, 0, 0], mt[1, :, 0, 0]) and np.array_equal(mt[0, :, 0, 0], mt[2, :, 0, 0])
    assert np.all(spread[:, 0] == 0.0) and np.all(scores[1, 0] == 0.0)  # exactly, not relatively
    assert np.all(s_ref[:, 0] == 0.0) and np.all(q_ref[1, 0] == 0.0)
    assert np.array_equal(mean[:, 0], mt[0, :, 0, 0])
    lead = np.arange(K) > 0
    r_mean, r_spread = relmax(mean, m_ref), relmax(spread[:, lead], s_ref[:, lead])
    rows = [(k, kk) for k in range(4) for kk in range(K) if not (k == 1 and kk == 0)]
    r_sc = max(relmax(scores[k, kk], q_ref[k, kk]) for k, kk in rows)
    print(f"against the GPU's own members: mean {r_mean:.3g}, spread {r_spread:.3g}, scores {r_sc:.3g} (max rel)")
    assert r_mean <= 1e-5 and r_spread <= 1e-5 and r_sc <= 1e-5
    # the sums alone (no trajectory buffers): bitwise the same; scale = None agrees with the reference too
    ctx = c.context()
    only = run(c, ctx, ELEVEN, 11, 3, 3, 0.0, 0.2, 0, outputs="p")[3]
    assert np.array_equal(only, scores)
    unscaled = run(c, ctx, ELEVEN, 11, 3, 3, 0.0, 0.2, 0, outputs="p", scale=None)[3]
    q1 = forecast.ensemble_rollout_reference(mt, c.feats, ELEVEN, d)[2]
    assert max(relmax(unscaled[k, kk], q1[k, kk]) for k, kk in rows) <= 1e-5 and np.all(unscaled[1, 0] == 0.0)
    # all sites on, midpoint: no exact zeros, every entry relative
    (mt, mean, spread, scores), _, _ = base_run(0.2, 1)
    m_ref, s_ref, q_ref = forecast.ensemble_rollout_reference(mt, c.feats, ELEVEN, d, SCALE)
    r = (relmax(mean.reshape(m_ref.shape), m_ref), relmax(spread.reshape(s_ref.shape), s_ref), relmax(scores, q_ref))
    print(f"all sites on: mean {r[0]:.3g}, spread {r[1]:.3g}, scores {r[2]:.3g} (max rel)")
    assert max(r) <= 1e-5


# 3 ---------------------------------------------------------------------------------------------------
def test_degenerate_ensemble_is_the_rollout():
    c = case(CONFIG1)
    d = c.d
    s, R = d.forecast_horizon + 1, 3
    ctx = c.context()
    mt, mean, spread, scores = run(c, ctx, ELEVEN, 11, R, 3, 0.0, 0.0)
    traj = torch.zeros(11, R, s, d.num_nodes, d.output_channels, device=DEV)
    skill = torch.zeros(3, R * s, d.output_channels, device=DEV, dtype=torch.float64)
    ctx.forecast_rollout(_capi.stream_ptr(torch), c.theta, ELEVEN, 11, R, 1, scale=SCALE, traj=traj, skill=skill)
    torch.cuda.synchronize()
    traj, skill = traj.cpu().numpy(), skill.cpu().numpy()
    for e in range(3):
        assert np.array_equal(mt[e], traj), f"member {e}"
    assert np.all(spread == 0.0) and np.all(scores[1] == 0.0) and np.array_equal(mean, traj)
    for mine, theirs in ((0, 0), (3, 2), (2, 1)):  # the CRPS of identical members is the absolute error
        r = relmax(scores[mine], skill[theirs])
        print(f"scores[{mine}] against the rollout's skill[{theirs}]: max rel {r:.3g}")
        assert r <= 1e-6


# 4 ---------------------------------------------------------------------------------------------------
def test_cycle_zero_is_the_ensemble_forecast():
    c = case(CONFIG1)
    d = c.d
    ctx = c.context()
    mt = run(c, ctx, ELEVEN, 11, 1, 3, 0.0, 0.2, outputs="t")[0]
    mem = torch.zeros(3, 11, d.num_nodes * d.forecast_horizon, d.output_channels, device=DEV)
    ctx.forecast_ensemble(_capi.stream_ptr(torch), c.theta, ELEVEN, 11, 3, 0.0, 0.2, SEED, member_pred=mem)
    torch.cuda.synchronize()
    mem = mem.cpu().numpy()
    mine = mt[:, :, 0, 1:].reshape(mem.shape)
    r = rel(mine, mem)
    print(f"R = 1 against smaml_forecast_ensemble: rel-L2 {r:.3g}, bitwise {np.array_equal(mine, mem)}")
    assert r <= 1e-5


# 5 ---------------------------------------------------------------------------------------------------
def test_invariances_and_what_the_counters_say_was_shared():
    c = case(CONFIG1)
    d = c.d
    T, s, R, E, n = d.window_size, d.forecast_horizon + 1, 3, 3, 11
    ref, st, _ = base_run(0.0, 1)
    assert st["shared_rows"] == n * (T - 1)  # once per pass, not per member
    assert st["member_rows"] == E * n * (R - 1) * min(s, T - 1)
    assert st["graph_rows"] == n + E * n * (R - 1)  # cycle 0's t = 0 block once, then per member
    assert st["xg_rows"] == st["shared_rows"] + st["member_rows"] + st["graph_rows"]
    ctx = c.context()
    per_layer0 = d.window_size + d.lstm_num_layers - 1
    for opt, val, groups in (("ens_group", 1, 3), ("ens_group", 2, 2), ("ens_group", 0, 1), ("ens_share", 0, 1),
                             ("roll_reuse", 0, 1)):
        ctx.set_option(opt, val)
        ctx.variant_counts(reset=True)
        got = run(c, ctx, ELEVEN, 11, R, E, 0.0, 0.2)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), (opt, val)
        now = ctx.rollout_ensemble_stats()
        assert now["member_groups"] == groups and now["cycles"] == groups * R == now["append_launches"]
        assert ctx.variant_counts()["fwd_infer_drop"] == groups * R * per_layer0
        if opt == "roll_reuse":
            assert now["shared_rows"] == 0 and now["member_rows"] == E * n * R * (T - 1)
            assert now["graph_rows"] == E * n * R
        else:
            assert now["shared_rows"] == n * (T - 1) and now["member_rows"] == st["member_rows"]
        ctx.set_option(opt, {"ens_group": -1, "ens_share": 1, "roll_reuse": 1}[opt])
    # a member does not depend on E or R
    fewer = run(c, ctx, ELEVEN, 11, 2, 2, 0.0, 0.2, outputs="t")[0]
    assert np.array_equal(fewer, ref[0][:2, :, :2])
    # passes: 7 origins in passes of 3, 3 and 1 against one pass
    seven = [0, 1, 2, 5, 9, 3, 4]
    for p_gcn in (0.0, 0.2):
        a = run(c, ctx, seven, 3, R, E, p_gcn, 0.2)
        st3 = ctx.rollout_ensemble_stats()
        b = run(c, ctx, seven, 7, R, E, p_gcn, 0.2)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        r = relmax(a[3], b[3])
        print(f"p_gcn {p_gcn}: scores, 7 origins at batch 3 vs batch 7: max rel {r:.3g}")
        assert r <= 1e-6
        if p_gcn == 0.0:
            assert st3["shared_rows"] == 7 * (T - 1) and st3["member_groups"] == 3
    # grouping with GCN dropout too (per-member features)
    ref2 = base_run(0.2, 1)[0]
    ctx.set_option("ens_group", 2)
    for a, b in zip(run(c, ctx, ELEVEN, 11, R, E, 0.2, 0.2), ref2):
        assert np.array_equal(a, b)


# 6 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_gcn", [0.0, 0.2])
def test_config2_four_tiles_the_fused_gcn(p_gcn):
    c = case(CONFIG2)  # 2 origins x 441 = 882 rows: four 256-row tiles (the last masked); H = 128
    ctx = c.context()
    mt, mean, spread, scores = run(c, ctx, [0, 1], 2, 2, 2, p_gcn, 0.2)
    check_teacher_forced(c, c.feats, mt, [0, 1], 2, 1, p_gcn, 0.2)
    m_ref, s_ref, q_ref = forecast.ensemble_rollout_reference(mt, c.feats, [0, 1], c.d, SCALE)
    assert relmax(mean.reshape(m_ref.shape), m_ref) <= 1e-5 and relmax(scores, q_ref) <= 1e-5
    if p_gcn == 0.0:
        ctx.set_option("roll_reuse", 0)
        again = run(c, ctx, [0, 1], 2, 2, 2, p_gcn, 0.2)
        for a, b in zip(again, (mt, mean, spread, scores)):
            assert np.array_equal(a, b)


def test_one_layer_lstm_on_rings_a_previous_call_left_full():
    d = ModelDims(num_nodes=25, hidden_channels=32, lstm_hidden_size=32, lstm_num_layers=1)
    c = case(d)
    ctx = c.context()
    run(c, ctx, ELEVEN, 11, 2, 3, 0.0, 0.5, seed=99)  # leaves the rings, tables and sequences full of other values
    out = {}
    for share in (1, 0):  # a one-layer LSTM has no layer above to read a shared layer 0: off whatever the option
        ctx.set_option("ens_share", share)
        out[share] = run(c, ctx, ELEVEN, 11, 2, 2, 0.0, 0.2)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    check_teacher_forced(c, c.feats, out[1][0], ELEVEN, 2, 1, 0.0, 0.2)
    assert rel(out[1][0][0, :, 0, 1:], out[1][0][1, :, 0, 1:]) > 1e-3  # the head-input mask differs per member


def test_short_window():
    """T = 4 < s = 9: one cycle appends more rows than a window holds; every row t >= 1 of a later window is a
    member's own."""
    d = ModelDims(num_nodes=25, hidden_channels=32, lstm_hidden_size=32, lstm_num_layers=2, window_size=4)
    c = case(d)
    ctx = c.context()
    for p_gcn, gap in ((0.0, 1), (0.2, 0)):
        mt = run(c, ctx, ELEVEN, 11, 3, 2, p_gcn, 0.2, gap, outputs="t")[0]
        check_teacher_forced(c, c.feats, mt, ELEVEN, 3, gap, p_gcn, 0.2)
        if p_gcn == 0.0:
            st = ctx.rollout_ensemble_stats()
            assert st["shared_rows"] == 11 * 3 and st["member_rows"] == 2 * 11 * 2 * 3


def test_sixty_four_members():
    """More than 32 members: k_rens_stats needs its dynamic-LDS limit raised (64 KB at E = 64, its largest
    footprint). Member 0 teacher-forced against the oracle (test 1's bound), the statistics against the reference
    on the GPU's own members (test 2's bound)."""
    c = case(CONFIG1)
    ctx = c.context()
    mt, mean, spread, scores = run(c, ctx, [0, 1], 2, 2, 64, 0.0, 0.2)
    for x in (mt, mean, spread, scores):
        assert not np.any(x == SENT) and np.all(np.isfinite(x))
    check_teacher_forced(c, c.feats, mt[:1], [0, 1], 2, 1, 0.0, 0.2)
    assert rel(mt[0, :, 1], mt[63, :, 1]) > 1e-3  # the last member is another draw
    m_ref, s_ref, q_ref = forecast.ensemble_rollout_reference(mt, c.feats, [0, 1], c.d, SCALE)
    r = (relmax(mean.reshape(m_ref.shape), m_ref), relmax(spread.reshape(s_ref.shape), s_ref), relmax(scores, q_ref))
    print(f"64 members: mean {r[0]:.3g}, spread {r[1]:.3g}, scores {r[2]:.3g} (max rel)")
    assert max(r) <= 1e-5


# 7 ---------------------------------------------------------------------------------------------------
def test_nan_guard_and_state_isolation():
    c = case(CONFIG1)
    d = c.d
    T, N, C = d.window_size, d.num_nodes, d.output_channels
    st = _capi.stream_ptr(torch)
    t_obs = 50
    nan_stream = forecast.extend_stream(c.feats[:t_obs], c.feats[t_obs:, :, C:])
    zero_stream = np.nan_to_num(nan_stream, nan=0.0)
    origins = [20, 26, 23]  # origin 26: its window ends at the last observation; R = 3 reads 18 rows past it
    out = []
    for f in (nan_stream, zero_stream):
        ctx = c.context()
        ctx.set_tasks([torch.from_numpy(f).to(DEV)])
        out.append(run(c, ctx, origins, 2, 3, 2, 0.0, 0.2, outputs="tms"))
    for a, b in zip(out[0][:3], out[1][:3]):
        assert np.all(np.isfinite(a)) and not np.any(a == SENT) and np.array_equal(a, b)
    check_teacher_forced(c, nan_stream, out[0][0], origins, 3, 1, 0.0, 0.2)

    # a pending smaml_forward / smaml_backward pair stays valid across the call; the workspace is not touched
    xs = [c.stream[w:w + T].reshape(T * N, -1) for w in (3, 8)]
    dpred = torch.from_numpy(np.random.default_rng(0).standard_normal((2, N * d.forecast_horizon, C))
                             .astype(np.float32)).to(DEV)

    def pair(cx, between):
        pred, grad = torch.zeros_like(dpred), torch.zeros_like(c.theta)
        cx.forward(st, c.theta, xs, pred)
        ws = cx.workspace_bytes()
        if between:
            fb = cx.forecast_bytes()
            for p_gcn in (0.0, 0.2):
                run(c, cx, list(range(9)), 4, 2, 3, p_gcn, 0.2)
            assert cx.workspace_bytes() == ws and cx.forecast_bytes() > fb
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
    T, s, R, E = d.window_size, d.forecast_horizon + 1, 2, 2
    N, C = d.num_nodes, d.output_channels
    tt = c.feats.shape[0]
    ctx = c.context()
    run(c, ctx, [0, 1], 2, R, E, 0.0, 0.2)
    stats = ctx.rollout_ensemble_stats()
    last_in = tt - T - (R - 1) * s  # o + T + (R - 1) s == t_total
    last_sc = tt - T - R * s        # o + T + R s == t_total
    run(c, ctx, [0, last_in], 2, R, E, 0.0, 0.2, outputs="tms")  # the boundaries themselves are admitted
    run(c, ctx, [last_sc], 2, R, E, 0.0, 0.2)
    run(c, ctx, [0, 1], 2, R, E, 0.0, 0.2)
    assert ctx.rollout_ensemble_stats() == stats
    bad = [([-1], True, "origin 0"), ([0, last_in + 1], False, "origin 1"), ([0, 2, last_sc + 1], True, "origin 2"),
           ([last_in], True, "origin 0"), ([tt], False, "origin 0")]
    for origins, with_scores, msg in bad:
        n = len(origins)
        t = torch.full((E, n, R, s, N, C), SENT, device=DEV)
        m = torch.full((n, R, s, N, C), SENT, device=DEV)
        k = torch.full((4, R * s, C), SENT, device=DEV, dtype=torch.float64)
        with pytest.raises(_capi.SmamlError, match=msg) as ei:
            ctx.forecast_rollout_ensemble(_capi.stream_ptr(torch), c.theta, origins, 2, R, E, 0.0, 0.2, SEED, scale=SCALE,
                                          member_traj=t, mean=m, spread=m, scores=k if with_scores else None)
        assert ei.value.code == 1  # SMAML_EINVAL
        torch.cuda.synchronize()
        assert bool((t == SENT).all()) and bool((m == SENT).all()) and bool((k == SENT).all())
        assert ctx.rollout_ensemble_stats() == stats


# 9 ---------------------------------------------------------------------------------------------------
def test_ensemble_rollout_function_physical_units_and_metrics():
    c = case(CONFIG1)
    d = c.d
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    s, R, E = Hf + 1, 2, 3
    m = build_hybrid(d, c.P)
    rng = np.random.default_rng(1)
    stats = {"mean": rng.standard_normal(6), "std": rng.uniform(0.5, 2.0, 6)}  # six variables, as the checkpoints'
    ei = torch.from_numpy(c.ei).to(DEV)
    res = forecast.ensemble_rollout(m, c.stream, ei, stats=stats, cycles=R, members=E, p_gcn=0.0, p_lstm=0.2, seed=SEED,
                                    gap="midpoint", batch=16, return_members=True)
    want_o = forecast.rollout_origins(c.feats.shape[0], T, Hf, R, True)
    n = want_o.size
    assert res.n_origins == n and list(res.origins) == list(want_o) and res.n_members == E and res.cycles == R
    assert res.gap == "midpoint" and res.seed == SEED and res.p_gcn == 0.0 and res.p_lstm == 0.2
    assert res.is_gap.shape == (R * s,) and list(np.flatnonzero(res.is_gap)) == [0, s]
    assert res.mean.shape == res.spread.shape == (n, R * s, N, C) and res.members.shape == (E, n, R * s, N, C)
    std, mean = np.ones(C), np.zeros(C)
    std[:6], mean[:6] = stats["std"], stats["mean"]
    # the library's own normalised members, and the reference on them, in physical units
    mt, _, _, sums = run(c, c.context(), want_o, 16, R, E, 0.0, 0.2, scale=std)
    assert rel(res.members, mt.reshape(E, n, R * s, N, C) * std + mean) <= 1e-6
    m_ref, s_ref, q_ref = forecast.ensemble_rollout_reference(mt, c.feats, want_o, d, std)
    assert rel(res.mean, m_ref * std + mean) <= 1e-6 and rel(res.spread, s_ref * std) <= 1e-5
    assert relmax(sums, q_ref) <= 1e-5
    rmse, rms, ratio, crps, prmse, skill = forecast.ensemble_rollout_metrics(q_ref, n * N)
    for got, ref in ((res.rmse, rmse), (res.rms_spread, rms), (res.crps, crps), (res.persistence_rmse, prmse),
                     (res.spread_skill, ratio)):
        assert got.shape == (R * s, C) and relmax(got, ref) <= 1e-5
    assert np.max(np.abs(res.skill - skill)) <= 1e-5
    assert relmax(res.spread_skill, res.rms_spread / res.rmse) <= 1e-12
    # forecast only, past the scoreable origins; the model's own rates and a drawn seed by default
    res2 = forecast.ensemble_rollout(m, c.stream, ei, stats=stats, cycles=R, members=2, gap="persistence", batch=16,
                                     score=False)
    assert res2.n_origins == n + s and res2.rmse is None and res2.members is None and res2.gap == "persistence"
    assert res2.p_gcn == float(m.base_stgcn.dropout.p) and res2.p_lstm == float(m.dropout.p)
    last = (c.feats[T - 1, :, :C] * std + mean).astype(np.float32)
    assert rel(res2.mean[0, 0], last) <= 1e-6 and np.all(res2.spread[:, 0] == 0.0)
