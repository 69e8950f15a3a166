"""CPU checks of the weighted loss and the weighted forecast scores: the four new C functions (names, host-only
argument check), the ``loss`` helpers, the ``*_reference`` functions' ``node_weights``, and the oracle that the
GPU tests (test_gpu_weighted_loss.py) hold the library to -- that with ones it is bitwise ``refcpu``'s, and that in
float32 it agrees with a float64 run of itself within a tenth of each of the project's tolerances on the GPU
tests' own tables, so the reference alone is well inside the bounds."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast as fc, loss as L, synth
from weatherforecast_stgcn_maml_amd.config import ModelDims

import weighted_loss_oracle as wlo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smaml_loss_weights_check", "smaml_set_loss_weights", "smaml_set_score_weights", "smaml_loss_stats")
TINY = ModelDims(num_nodes=9, window_size=3, hidden_channels=16, lstm_hidden_size=32, lstm_num_layers=2)
D3 = ModelDims(num_nodes=3, window_size=2, input_channels=4, hidden_channels=8, lstm_hidden_size=8, lstm_num_layers=1,
               forecast_horizon=2, output_channels=2)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def grid_edges(d):
    from weatherforecast_stgcn_maml_amd.graph import build_spatial_graph

    side = int(round(d.num_nodes ** 0.5))
    lats, lons = synth.region_grid(n_lat=side, n_lon=side)
    return build_spatial_graph(lats, lons, 4)[0]


# ----------------------------------------------------------------------------- C ABI
def test_header_exports_sigs_and_library_agree_on_the_new_names():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    decl = set(re.findall(r"\b(smaml_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    lib = _capi.lib()
    for name in NEW:
        assert name in decl and name in _capi.EXPORTS and name in _capi._SIGS and hasattr(lib, name), name
    assert lib.smaml_abi_version() == _capi.ABI_VERSION == 9
    assert len(_capi.LOSS_STATS) == 6


def _bad_tables():
    rows, C = TINY.forecast_horizon * TINY.num_nodes, TINY.output_channels
    ones = np.ones((2, rows, C), np.float32)

    def with_(z, i, v):
        a = ones.copy()
        a.reshape(2, -1)[z, i] = v
        return a

    allzero = ones.copy()
    allzero[1] = 0.0
    return {"negative": (with_(1, 17, -0.5), "set 1", "element 17"), "nan": (with_(0, 5, np.nan), "set 0", "element 5"),
            "inf": (with_(1, rows * C - 1, np.inf), "set 1", f"element {rows * C - 1}"),
            "no_positive": (allzero, "set 1", "no positive")}


@pytest.mark.parametrize("name", ["negative", "nan", "inf", "no_positive"])
def test_loss_weights_check_rejects_and_names_set_and_element(name):
    table, set_word, elem_word = _bad_tables()[name]
    with pytest.raises(_capi.SmamlError) as e:
        _capi.loss_weights_check(TINY, table)
    assert e.value.code == 1 and set_word in str(e.value) and elem_word in str(e.value), str(e.value)


def test_loss_weights_check_accepts_good_tables_and_rejects_null_and_nsets():
    sep, rnd = wlo.draw_tables(TINY, 7)
    _capi.loss_weights_check(TINY, sep)
    _capi.loss_weights_check(TINY, [sep, rnd])
    lib, d = _capi.lib(), _capi.Dims.from_model(TINY)
    import ctypes

    assert lib.smaml_loss_weights_check(ctypes.byref(d), None, 1) == 1  # SMAML_EINVAL
    assert lib.smaml_loss_weights_check(ctypes.byref(d), sep.ctypes.data_as(_capi.PF32), 0) == 1
    with pytest.raises(ValueError):
        _capi.loss_weights_check(TINY, sep.T)  # transposed: not [Hf*N, C]


# ----------------------------------------------------------------------------- loss.py
def test_latitude_weights():
    lat = np.array([0.0, 30.0, 60.0, -60.0])
    w = L.latitude_weights(lat)
    assert w.shape == (4,) and abs(w.mean() - 1.0) < 1e-12
    np.testing.assert_allclose(w / w[0], np.cos(np.deg2rad(lat)), rtol=1e-12)
    with pytest.raises(ValueError):
        L.latitude_weights([91.0])


def test_make_loss_weights_shape_layout_and_mean():
    d = TINY
    Hf, N, C = d.forecast_horizon, d.num_nodes, d.output_channels
    rng = np.random.default_rng(1)
    node, var, lead = rng.uniform(0.5, 2, N), rng.uniform(0.5, 2, C), rng.uniform(0.5, 2, Hf)
    node[4] = 0.0
    W = L.make_loss_weights(d, node=node, variable=var, lead=lead)
    assert W.shape == (Hf * N, C) and W.dtype == np.float32 and abs(float(W.astype(np.float64).mean()) - 1.0) < 1e-6
    raw = L.make_loss_weights(d, node=node, variable=var, lead=lead, normalize=False)
    for hp, n, c in [(0, 0, 0), (3, 4, 5), (Hf - 1, N - 1, C - 1), (2, 7, 1)]:
        assert raw[hp * N + n, c] == np.float32(lead[hp] * node[n] * var[c]), (hp, n, c)  # row h'*N + n'
    assert np.all(W[4::N] == 0) and np.all(W[3::N] > 0)  # node 4 masked at every lead
    assert np.array_equal(L.make_loss_weights(d), np.ones((Hf * N, C), np.float32))
    with pytest.raises(ValueError):
        L.make_loss_weights(d, node=np.ones(N + 1))
    with pytest.raises(ValueError):
        L.make_loss_weights(d, variable=-np.ones(C))


def test_weighted_mse_reference_numpy_torch_and_masked_nan():
    rng = np.random.default_rng(2)
    p, y, W = rng.normal(size=(2, 6, 3)), rng.normal(size=(2, 6, 3)), rng.uniform(0, 2, (6, 3))
    W[1, 2] = 0.0
    want = float((W * (p - y) ** 2).mean())
    assert abs(L.weighted_mse_reference(p, y, W) - want) < 1e-15
    y[:, 1, 2] = np.nan
    assert abs(L.weighted_mse_reference(p, y, W) - want) < 1e-15
    got = L.weighted_mse_reference(torch.from_numpy(p), torch.from_numpy(y), W)
    assert abs(float(got) - want) < 1e-15


# ----------------------------------------------------------------------------- the score references
def _score_inputs(seed=3, E=3, nwin=2, R=2):
    d = D3
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    rng = np.random.default_rng(seed)
    K = R * (Hf + 1)
    f = rng.normal(size=(T + K + nwin + 1, N, d.input_channels)).astype(np.float32)
    mem = rng.normal(size=(E, nwin, N * Hf, C)).astype(np.float32)
    mtraj = rng.normal(size=(E, nwin, K, N, C)).astype(np.float32)
    scale = rng.uniform(0.5, 2.0, C)
    return d, f, list(range(nwin)), mem, mtraj, scale, K


def _brute(d, f, starts, x, v, scale, rollout):
    """sum v (s e)^2, sum v |s e|, sum v (s q)^2 by a triple loop (leads, nodes, variables) per window."""
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    K = x.shape[1] if rollout else Hf
    out = np.zeros((3, K, C))
    for i, w in enumerate(starts):
        xi = x[i] if rollout else x[i].reshape(Hf, N, C)
        for k in range(K):
            for n in range(N):
                for c in range(C):
                    y = float(f[w + T + k + (0 if rollout else 1), n, c])
                    e = scale[c] * (float(xi[k, n, c]) - y)
                    q = scale[c] * (float(f[w + T - 1, n, c]) - y)
                    out[0, k, c] += v[n] * e * e
                    out[1, k, c] += v[n] * abs(e)
                    out[2, k, c] += v[n] * q * q
    return out


def test_references_with_ones_are_their_unweighted_selves():
    d, f, starts, mem, mtraj, scale, K = _score_inputs()
    ones = np.ones(d.num_nodes)
    assert np.array_equal(fc.skill_reference(mem[0], f, starts, d, scale),
                          fc.skill_reference(mem[0], f, starts, d, scale, node_weights=ones))
    assert np.array_equal(fc.rollout_skill_reference(mtraj[0], f, starts, d, scale),
                          fc.rollout_skill_reference(mtraj[0], f, starts, d, scale, node_weights=ones))
    for a, b in zip(fc.ensemble_reference(mem, f, starts, d, scale),
                    fc.ensemble_reference(mem, f, starts, d, scale, node_weights=ones)):
        assert np.array_equal(a, b)
    for a, b in zip(fc.ensemble_rollout_reference(mtraj, f, starts, d, scale),
                    fc.ensemble_rollout_reference(mtraj, f, starts, d, scale, node_weights=ones)):
        assert np.array_equal(a, b)


def test_references_match_a_brute_force_loop_and_mask_nan_targets():
    d, f, starts, mem, mtraj, scale, K = _score_inputs()
    T, Hf, N, C = d.window_size, d.forecast_horizon, d.num_nodes, d.output_channels
    v = np.array([0.5, 0.0, 1.75])
    want = _brute(d, f, starts, mem[0], v, scale, False)
    want_r = _brute(d, f, starts, mtraj[0], v, scale, True)
    f = f.copy()
    f[T:, 1, :C] = np.nan  # every target of the masked node (never y_last of a window start: rows >= T)
    got = fc.skill_reference(mem[0], f, starts, d, scale, node_weights=v)
    np.testing.assert_allclose(got, want, rtol=1e-12)
    got_r = fc.rollout_skill_reference(mtraj[0], f, starts, d, scale, node_weights=v)
    np.testing.assert_allclose(got_r, want_r, rtol=1e-12)
    # the ensembles: the mean's error and the persistence are the deterministic sums of the member mean
    mean, spread, sums = fc.ensemble_reference(mem, f, starts, d, scale, node_weights=v)
    np.testing.assert_allclose(sums[0], _brute(d, np.nan_to_num(f), starts, mean, v, scale, False)[0], rtol=1e-12)
    np.testing.assert_allclose(sums[3], want[2], rtol=1e-12)
    var = (spread ** 2).reshape(len(starts), Hf, N, C)
    np.testing.assert_allclose(sums[1], (var * v[None, None, :, None] * scale ** 2).sum(axis=(0, 2)), rtol=1e-12)
    assert np.isfinite(sums).all()
    mean_r, _, sums_r = fc.ensemble_rollout_reference(mtraj, f, starts, d, scale, node_weights=v)
    np.testing.assert_allclose(sums_r[0], _brute(d, np.nan_to_num(f), starts, mean_r, v, scale, True)[0], rtol=1e-12)
    np.testing.assert_allclose(sums_r[3], want_r[2], rtol=1e-12)
    assert np.isfinite(sums_r).all()
    # without the weights the NaN targets reach the sums: the masking is what keeps them out
    assert np.isnan(fc.skill_reference(mem[0], f, starts, d, scale)).any()
    assert fc.score_count(5, N) == 5 * N and abs(fc.score_count(5, N, v) - 5 * 2.25) < 1e-12
    with pytest.raises(ValueError):
        fc.skill_reference(mem[0], f, starts, d, scale, node_weights=[1.0, -1.0, 1.0])


# ----------------------------------------------------------------------------- the oracle
def _tiny_case(dtype=torch.float32):
    d = TINY
    P = synth.init_params(91, d, gcn_bias_scale=0.1)
    PT = wlo.to_dtype(refcpu.to_torch(P), dtype)
    names = refcpu.trainable_names(PT)
    Pt, Pg = {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names}
    ei = grid_edges(d)
    np_t = np.float64 if dtype == torch.float64 else np.float32
    tasks = [refcpu.TaskData(synth.make_features(9100 + j, d.num_nodes, synth.t_total_for(12, d.window_size,
                                                                                        d.forecast_horizon)).astype(np_t),
                             ei, d) for j in range(2)]
    windows = np.array([[[0, 1], [4, 5]], [[2, 3], [1, 7]], [[6, 7], [8, 9]]], np.int32)  # K = 2, 2 tasks, B = 2
    return d, Pt, Pg, tasks, windows, names


def test_patched_oracle_with_ones_is_bitwise_refcpu():
    d, Pt, Pg, tasks, windows, names = _tiny_case()
    ones = np.ones((d.forecast_horizon * d.num_nodes, d.output_channels), np.float32)
    ref = refcpu.meta_step(Pt, Pg, tasks, None, 2, 2, None, 0.01, 1.0, 2, windows=windows)
    got = wlo.meta_step(Pt, Pg, tasks, [ones, ones], windows, 2, 2, 0.01, 1.0, 2)
    assert got["query_losses"] == ref["query_losses"] and got["step_records"] == ref["step_records"]
    for k in names:
        assert torch.equal(got["meta_grad"][k], ref["meta_grad"][k]), k
        for j in range(2):
            assert torch.equal(got["adapted"][j][k], ref["adapted"][j][k]), (j, k)
    assert refcpu.mse.__module__ == "oracle.refcpu"  # the patch is undone


def test_float32_oracle_is_within_a_tenth_of_each_tolerance_of_its_float64_self():
    """The GPU tests' tables (draw_tables: separable for task 0, random for task 1) at a tiny shape, second order:
    per-step losses and adapted parameters 1e-6 rel-L2, query loss and meta-gradient 1e-5."""
    d, Pt, Pg, tasks, windows, names = _tiny_case()
    tables = wlo.draw_tables(d, 17)
    a = wlo.meta_step(Pt, Pg, tasks, tables, windows, 2, 2, 0.01, 1.0, 2)
    d, Pt64, Pg64, tasks64, _, _ = _tiny_case(torch.float64)
    b = wlo.meta_step(Pt64, Pg64, tasks64, tables, windows, 2, 2, 0.01, 1.0, 2)
    plain = refcpu.meta_step(Pt, Pg, tasks, None, 2, 2, None, 0.01, 1.0, 2, windows=windows)
    for j in range(2):
        e_step = rel([r[0] for r in a["step_records"][j]], [r[0] for r in b["step_records"][j]])
        e_q = abs(a["query_losses"][j] - b["query_losses"][j]) / b["query_losses"][j]
        e_ad = max(rel(a["adapted"][j][k].numpy(), b["adapted"][j][k].numpy()) for k in names)
        print(f"task {j}: step losses {e_step:.3g} (1e-6), query {e_q:.3g} (1e-5), adapted {e_ad:.3g} (1e-6)")
        assert e_step < 1e-6 and e_q < 1e-5 and e_ad < 1e-6
        # and the tables matter: the weighted losses are not the unweighted ones
        assert abs(a["query_losses"][j] - plain["query_losses"][j]) > 1e-3 * plain["query_losses"][j]
    e_mg = max(rel(a["meta_grad"][k].numpy(), b["meta_grad"][k].numpy()) for k in names)
    print(f"meta-gradient {e_mg:.3g} (1e-5)")
    assert e_mg < 1e-5


def test_float32_adapt_oracle_is_within_a_tenth_of_the_tolerance_of_its_float64_self():
    d = TINY
    P = synth.init_params(92, d, gcn_bias_scale=0.1)
    feats = synth.make_features(9200, d.num_nodes, synth.t_total_for(8, d.window_size, d.forecast_horizon))
    W = wlo.draw_tables(d, 18)[1]
    windows, lrs = np.array([[3, 0], [1, 5], [3, 6]]), [6e-4, 5e-4, 4e-4]
    for train_base in (False, True):
        a, la = wlo.adam_steps(d, P, feats, grid_edges(d), windows, lrs, W, 1e-4, train_base=train_base)
        b, lb = wlo.adam_steps(d, P, feats, grid_edges(d), windows, lrs, W, 1e-4, train_base=train_base,
                               dtype=torch.float64)
        assert rel(la, lb) < 1e-6
        assert max(rel(a[k], b[k]) for k in a) < 1e-6
