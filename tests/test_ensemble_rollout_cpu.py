"""CPU statement of the ensemble rollout: ``forecast.ensemble_rollout_reference`` on hand cases and against the
ensemble's and the rollout's references, the mask step ``64 j + e``, the binding of
``smaml_forecast_rollout_ensemble`` / ``smaml_rollout_ensemble_stats`` and the argument errors that need no
device."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, forecast
from weatherforecast_stgcn_maml_amd.config import ModelDims

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dims(T, Hf=2, N=3, C=2, Cin=4):
    return ModelDims(num_nodes=N, window_size=T, input_channels=Cin, hidden_channels=16, lstm_hidden_size=32,
                     lstm_num_layers=1, forecast_horizon=Hf, output_channels=C)


# 1 ---------------------------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("smaml_forecast_rollout_ensemble", 18), ("smaml_rollout_ensemble_stats", 4)):
        m = re.search(name + r"\s*\((.*?)\);", txt, flags=re.S)
        assert m, f"include/smaml.h does not declare {name}"
        assert name in _capi.EXPORTS and name in _capi._SIGS
        assert hasattr(_capi.lib(), name)
        assert len(m.group(1).split(",")) == len(_capi._SIGS[name][0]) == nargs
    src = open(_capi.__file__).read()  # (another test module may have swapped _capi.Context for a stub)
    assert "def forecast_rollout_ensemble(self" in src and "def rollout_ensemble_stats(self" in src
    assert len(_capi.ROLLOUT_ENSEMBLE_STATS) == 7
    assert _capi.ABI_VERSION == 9 and _capi.lib().smaml_abi_version() == 9
    for name in ("ensemble_rollout", "ensemble_rollout_reference", "EnsembleRolloutResult"):
        assert hasattr(forecast, name)


# 2 ---------------------------------------------------------------------------------------------------
def hand_case():
    """T = 2, Hf = 1 (s = 2), R = 2, N = 2, C = 2; variable 0 of the stream rises by 10 per step, variable 1 is 0.
    Members e = 0, 1, 2 sit at y + (k + 1) + d_e on variable 0 and at y - 2 (k + 1) - d_e on variable 1, with
    d = (-1, 0, 1): the mean errs by +(k + 1) / -2 (k + 1), the unbiased variance is 1 on both."""
    d = dims(T=2, Hf=1, N=2, C=2)
    K = 4
    f = np.zeros((12, 2, 4), np.float32)
    f[:, :, 0] = np.arange(12)[:, None] * 10.0
    origins = [0, 3]
    x = np.zeros((3, 2, K, 2, 2), np.float32)
    for e, de in enumerate((-1.0, 0.0, 1.0)):
        for i, o in enumerate(origins):
            for k in range(K):
                y = f[o + 2 + k, :, :2]
                x[e, i, k, :, 0] = y[:, 0] + (k + 1) + de
                x[e, i, k, :, 1] = y[:, 1] - 2.0 * (k + 1) - de
    return d, f, origins, x


def test_reference_hand_case():
    d, f, origins, x = hand_case()
    K = 4
    scale = np.array([2.0, 0.5])
    mean, spread, sums = forecast.ensemble_rollout_reference(x, f, origins, d, scale)
    assert mean.shape == spread.shape == (2, K, 2, 2) and sums.shape == (4, K, 2) and sums.dtype == np.float64
    np.testing.assert_array_equal(mean, x[1].astype(np.float64))
    np.testing.assert_array_equal(spread, np.ones_like(spread))
    count = len(origins) * d.num_nodes
    for k in range(K):
        np.testing.assert_array_equal(sums[0, k], count * np.array([(2.0 * (k + 1)) ** 2, (1.0 * (k + 1)) ** 2]))
        np.testing.assert_array_equal(sums[1, k], count * np.array([4.0, 0.25]))
        # CRPS of members at errors a - 1, a, a + 1: (1/3) sum |.| - (1/9)(1 + 2 + 1)
        crps = []
        for a in ((k + 1.0), -2.0 * (k + 1)):
            crps.append((abs(a - 1) + abs(a) + abs(a + 1)) / 3.0 - 4.0 / 9.0)
        np.testing.assert_allclose(sums[2, k], count * np.array([2.0 * crps[0], 0.5 * crps[1]]), rtol=1e-14)
        np.testing.assert_array_equal(sums[3, k], count * np.array([(2.0 * 10.0 * (k + 1)) ** 2, 0.0]))
    # the library's 6-D layout is accepted; no scale = factors of 1
    m6, s6, q6 = forecast.ensemble_rollout_reference(x.reshape(3, 2, 2, 2, 2, 2), f, origins, d, scale)
    np.testing.assert_array_equal(q6, sums)
    np.testing.assert_array_equal(forecast.ensemble_rollout_reference(x, f, origins, d)[2][0], sums[0] / scale ** 2)
    with pytest.raises(ValueError):
        forecast.ensemble_rollout_reference(x, f, [0, 7], d)  # 7 + 2 + 4 > 12
    rmse, rms, ratio, crps_m, prmse, skill = forecast.ensemble_rollout_metrics(sums, count)
    np.testing.assert_allclose(rmse[:, 0], 2.0 * np.arange(1, 5))
    np.testing.assert_allclose(ratio, rms / rmse)
    assert np.all(np.isnan(skill[:, 1])) and np.allclose(skill[:, 0], 1 - 1 / 100.0)


def test_reference_one_member_and_identical_members():
    d, f, origins, x = hand_case()
    one = x[2:3]
    mean, spread, sums = forecast.ensemble_rollout_reference(one, f, origins, d)
    np.testing.assert_array_equal(mean, one[0].astype(np.float64))
    assert np.all(spread == 0.0) and np.all(sums[1] == 0.0)
    # E = 1: CRPS = |x - y|, and sums [0] / [3] are the rollout's skill sums [0] / [2]
    ro = forecast.rollout_skill_reference(one[0], f, origins, d)
    np.testing.assert_array_equal(sums[2], ro[1])
    np.testing.assert_array_equal(sums[0], ro[0])
    np.testing.assert_array_equal(sums[3], ro[2])
    scale = np.array([3.0, 0.25])
    ro = forecast.rollout_skill_reference(one[0], f, origins, d, scale)
    s1 = forecast.ensemble_rollout_reference(one, f, origins, d, scale)[2]
    np.testing.assert_array_equal(s1[0], ro[0])
    np.testing.assert_array_equal(s1[3], ro[2])
    # identical members: variance sum exactly 0, CRPS the absolute error
    same = np.repeat(one, 4, axis=0)
    mean4, spread4, sums4 = forecast.ensemble_rollout_reference(same, f, origins, d)
    assert np.all(spread4 == 0.0) and np.all(sums4[1] == 0.0)
    np.testing.assert_allclose(sums4[2], sums[2], rtol=1e-14)


def test_reference_agrees_with_ensemble_reference_on_one_cycle():
    """A one-cycle trajectory's rows 1..Hf are the memory image of the flat prediction: read as [N*Hf, C] they are
    ``ensemble_reference``'s input, whose F4 pairing puts flat row r at lead r // N -- trajectory row 1 + r // N."""
    d = dims(T=3, Hf=2, N=3, C=2)
    T, Hf, N, C, s = 3, 2, 3, 2, 3
    rng = np.random.default_rng(5)
    f = rng.standard_normal((20, N, 4)).astype(np.float32)
    origins = [0, 4, 9]
    E = 4
    x = rng.standard_normal((E, len(origins), 1, s, N, C)).astype(np.float32)
    scale = np.array([1.5, 0.75])
    mean, spread, sums = forecast.ensemble_rollout_reference(x, f, origins, d, scale)
    flat = x[:, :, 0, 1:].reshape(E, len(origins), N * Hf, C)
    m_e, s_e, q_e = forecast.ensemble_reference(flat, f, origins, d, scale)
    np.testing.assert_allclose(mean[:, 1:].reshape(m_e.shape), m_e, rtol=1e-14)
    np.testing.assert_allclose(spread[:, 1:].reshape(s_e.shape), s_e, rtol=1e-14)
    np.testing.assert_allclose(sums[:, 1:], q_e, rtol=1e-13)


# 3 ---------------------------------------------------------------------------------------------------
def test_mask_step_is_distinct_and_stays_inside_its_bits():
    R, E = _capi.ROLLOUT_ENSEMBLE_MAX_CYCLES, 64
    assert R == 1024
    steps = {64 * j + e for j in range(R) for e in range(E)}
    assert len(steps) == R * E and max(steps) == 64 * (R - 1) + (E - 1) == 0xFFFF  # 16 bits, all of them used
    top = max(steps)
    # drop_site packs (kind << 24) ^ (step << 8) ^ layer: the largest step must not reach the kind field
    assert (top << 8) < (1 << 24) and ((top + 1) << 8) == (1 << 24)
    seed = 20240607
    for kind in (1, 2, 3):
        for layer in (0, 7):
            assert refcpu.drop_site(seed, kind, top, layer) != refcpu.drop_site(seed, kind + 1, top, layer)
            # one step further would flip the kind field's low bit (the fields are xor-ed): another kind's step 0
            assert refcpu.drop_site(seed, kind, top + 1, layer) == refcpu.drop_site(seed, kind ^ 1, 0, layer)
    sites = {int(refcpu.drop_site(seed, 2, st, 1)) for st in (0, 1, 63, 64, 65, 64 * 1023, top)}
    assert len(sites) == 7
    # the kernels' packing is the oracle's (kernels.h drop_site)
    src = open(os.path.join(REPO, "weatherforecast_stgcn_maml_amd", "csrc", "kernels.h")).read()
    assert "((uint32_t)kind << 24) ^ ((uint32_t)step << 8) ^ (uint32_t)layer" in src


# 4 ---------------------------------------------------------------------------------------------------
def test_argument_errors_are_rejected_without_a_device():
    L = _capi.lib()
    P = ctypes.c_void_p
    fake = 256  # never dereferenced: every call below fails its argument checks first
    org = (ctypes.c_int32 * 1)(0)

    def call(norig=1, batch=1, cycles=1, gap=1, members=2, p_gcn=0.0, p_lstm=0.2, outs=(fake,) * 4, origins=org):
        f = L.smaml_forecast_rollout_ensemble
        return f(None, None, P(fake), 0, origins, norig, batch, cycles, gap, members, p_gcn, p_lstm, 7, None,
                 *[P(o) if o else None for o in outs])

    def msg():
        return L.smaml_last_error().decode()

    assert call() == 1 and "ctx is NULL" in msg()  # every argument check passed
    for k in range(4):  # any one output is enough
        outs = [0] * 4
        outs[k] = fake
        assert call(outs=tuple(outs)) == 1 and "ctx is NULL" in msg()
    assert call(cycles=1024, members=64) == 1 and "ctx is NULL" in msg()  # the largest accepted values
    assert call(outs=(0, 0, 0, 0)) == 1 and "all NULL" in msg()
    for m in (0, 65, -1):
        assert call(members=m) == 1 and "members must be in 1..64" in msg() and str(m) in msg()
    for r in (0, 1025, -3):
        assert call(cycles=r) == 1 and "cycles must be in 1..1024" in msg() and str(r) in msg()
    for kw in (dict(p_gcn=1.0), dict(p_lstm=1.0), dict(p_gcn=-0.1), dict(p_lstm=-1e-3), dict(p_lstm=float("nan"))):
        assert call(**kw) == 1 and "probabilities must be in [0, 1)" in msg()
    for g in (-1, 2):
        assert call(gap=g) == 1 and "gap must be 0" in msg() and str(g) in msg()
    for kw in (dict(norig=0), dict(norig=-1), dict(batch=0), dict(batch=-4), dict(origins=None)):
        assert call(**kw) == 1 and "norig and batch must be positive" in msg()
    cnt = ctypes.c_int32()
    assert L.smaml_rollout_ensemble_stats(None, None, 0, ctypes.byref(cnt)) == 1
