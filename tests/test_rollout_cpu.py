"""CPU statement of the autoregressive rollout (``forecast.rollout_reference`` / ``rollout_skill_reference`` /
``rollout_origins`` / ``extend_stream``), the binding of ``smaml_forecast_rollout`` / ``smaml_rollout_stats`` and
the argument errors that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from weatherforecast_stgcn_maml_amd import _capi, forecast
from weatherforecast_stgcn_maml_amd.config import ModelDims

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dims(T, Hf=2, N=3, C=2, Cin=4):
    return ModelDims(num_nodes=N, window_size=T, input_channels=Cin, hidden_channels=16, lstm_hidden_size=32,
                     lstm_num_layers=1, forecast_horizon=Hf, output_channels=C)


def stream(t_total, N=3, Cin=4, nan_from=None, C=2):
    """features[t, n, c] = 1000 t + 10 n + c: every value names its place; optionally NaN weather from a row on."""
    t, n, c = np.meshgrid(np.arange(t_total), np.arange(N), np.arange(Cin), indexing="ij")
    f = (1000.0 * t + 10.0 * n + c).astype(np.float32)
    if nan_from is not None:
        f[nan_from:, :, :C] = np.nan
    return f


class Stub:
    """forward(window) -> flat [N*Hf, C] whose memory image read as [Hf, N, C] is
    P[h', n', c] = last[n', c] / 8 + 64 h' + 8 n' + c + 0.5, last = the window's last row; records every window."""

    def __init__(self, d):
        self.d = d
        self.windows = []

    def __call__(self, x):
        d = self.d
        T, N, Hf, C = d.window_size, d.num_nodes, d.forecast_horizon, d.output_channels
        assert x.shape == (T * N, d.input_channels) and x.dtype == np.float32
        self.windows.append(x.copy())
        last = x.reshape(T, N, -1)[T - 1, :, :C]
        h, n, c = np.meshgrid(np.arange(Hf), np.arange(N), np.arange(C), indexing="ij")
        P = last[None] / np.float32(8) + (64.0 * h + 8.0 * n + c + 0.5).astype(np.float32)
        return P.astype(np.float32).reshape(N * Hf, C)  # flat rows: the F4 view is the memory image


@pytest.mark.parametrize("gap", ["midpoint", "persistence", 1, 0])
def test_reference_places_predictions_gap_rows_and_exogenous_channels(gap):
    d = dims(T=5)
    T, Hf, N, C, s, R = 5, 2, 3, 2, 3, 3
    t_total = 30
    # weather channels of rows past each origin's window are NaN where the origin's rollout could read them
    origins = [4, 0]
    f = stream(t_total)
    stub = Stub(d)
    traj = forecast.rollout_reference(stub, f, origins, d, R, gap)
    assert traj.shape == (2, R * s, N, C) and traj.dtype == np.float32
    assert len(stub.windows) == 2 * R
    mid = gap in ("midpoint", 1)
    for i, o in enumerate(origins):
        X = np.zeros((T + (R - 1) * s, N, 4), np.float32)
        X[:T] = f[o:o + T]
        for j in range(R):
            w = stub.windows[i * R + j].reshape(T, N, 4)
            # window j starts at private row j s; its exogenous channels are those of the same absolute time
            np.testing.assert_array_equal(w[:, :, C:], f[o + j * s:o + j * s + T, :, C:])
            np.testing.assert_array_equal(w[:, :, :C], X[j * s:j * s + T, :, :C])
            last = w[T - 1, :, :C]
            blk = traj[i, j * s:(j + 1) * s]
            for h in range(Hf):
                for n in range(N):
                    for c in range(C):  # F4 placement: P[h', n', c] lands in appended row 1 + h', node n'
                        want = np.float32(last[n, c] / np.float32(8)) + np.float32(64 * h + 8 * n + c + 0.5)
                        assert blk[1 + h, n, c] == want
            want_gap = np.float32(0.5) * (last + blk[1]) if mid else last
            assert want_gap.dtype == np.float32
            np.testing.assert_array_equal(blk[0], want_gap)  # bitwise in f32
            if j + 1 < R:
                X[j * s + T:(j + 1) * s + T, :, :C] = blk


def test_nan_weather_past_the_window_never_reaches_an_output():
    d = dims(T=5)
    o, R = 2, 4
    clean = stream(40)
    dirty = stream(40, nan_from=o + d.window_size)
    a = forecast.rollout_reference(Stub(d), clean, [o], d, R, "midpoint")
    b = forecast.rollout_reference(Stub(d), dirty, [o], d, R, "midpoint")
    assert np.all(np.isfinite(b))
    np.testing.assert_array_equal(a, b)
    # extend_stream builds such a stream
    exo = clean[20:, :, 2:]
    ext = forecast.extend_stream(clean[:20], exo)
    assert ext.shape == clean.shape and ext.dtype == np.float32
    assert np.all(np.isnan(ext[20:, :, :2])) and np.array_equal(ext[20:, :, 2:], exo)
    np.testing.assert_array_equal(ext[:20], clean[:20])
    c = forecast.rollout_reference(Stub(d), ext, [15], d, 3, "persistence")  # 15 + 5 = 20: runs off the observed end
    np.testing.assert_array_equal(c, forecast.rollout_reference(Stub(d), clean, [15], d, 3, "persistence"))
    with pytest.raises(ValueError):
        forecast.extend_stream(clean[:20], clean[20:, :2, 2:])


@pytest.mark.parametrize("T,Hf", [(5, 2), (3, 2), (4, 8), (1, 2)])  # T > s, T = s, T = 4 < s = 9, T = 1
def test_window_j_starts_at_j_s(T, Hf):
    d = dims(T=T, Hf=Hf)
    s, R, N, C = Hf + 1, 4, 3, 2
    f = stream(60)
    stub = Stub(d)
    o = 3
    traj = forecast.rollout_reference(stub, f, [o], d, R, "persistence")
    # the full private sequence, built from the outputs
    rows = T + (R - 1) * s
    X = np.zeros((rows + s, N, 4), np.float32)
    X[:T] = f[o:o + T]
    X[T:, :, C:] = f[o + T:o + rows + s, :, C:]
    X[T:, :, :C] = traj[0]
    for j in range(R):
        np.testing.assert_array_equal(stub.windows[j].reshape(T, N, 4), X[j * s:j * s + T])


def test_skill_reference_hand_case():
    d = dims(T=2, Hf=1, N=2, C=2)
    s, R = 2, 2
    f = np.zeros((12, 2, 4), np.float32)
    f[:, :, 0] = np.arange(12)[:, None] * 10.0  # variable 0 rises by 10 per step; variable 1 stays 0
    origins = [0, 3]
    traj = np.zeros((2, R * s, 2, 2), np.float32)
    for i, o in enumerate(origins):
        for k in range(R * s):
            y = f[o + d.window_size + k, :, :2]
            traj[i, k, :, 0] = y[:, 0] + (k + 1)         # error +(k + 1) on variable 0
            traj[i, k, :, 1] = y[:, 1] - 2.0 * (k + 1)   # error -2 (k + 1) on variable 1
    scale = np.array([2.0, 0.5])
    out = forecast.rollout_skill_reference(traj, f, origins, d, scale)
    assert out.shape == (3, R * s, 2) and out.dtype == np.float64
    count = len(origins) * d.num_nodes  # per lead: norig * N
    for k in range(R * s):
        np.testing.assert_array_equal(out[0, k], count * np.array([(2.0 * (k + 1)) ** 2, (1.0 * (k + 1)) ** 2]))
        np.testing.assert_array_equal(out[1, k], count * np.array([2.0 * (k + 1), 1.0 * (k + 1)]))
        # persistence: y_last = f[o + T - 1], y = f[o + T + k]: -10 (k + 1) on variable 0, 0 on variable 1
        np.testing.assert_array_equal(out[2, k], count * np.array([(2.0 * 10.0 * (k + 1)) ** 2, 0.0]))
    # the 5-D layout of the library's traj is accepted too; no scale = factors of 1
    out5 = forecast.rollout_skill_reference(traj.reshape(2, R, s, 2, 2), f, origins, d, scale)
    np.testing.assert_array_equal(out5, out)
    np.testing.assert_array_equal(forecast.rollout_skill_reference(traj, f, origins, d)[0], out[0] / scale ** 2)
    rmse, mae, prmse, skill = forecast.skill_metrics(out, count)
    np.testing.assert_allclose(rmse[:, 0], 2.0 * np.arange(1, 5))
    assert np.all(np.isnan(skill[:, 1])) and np.allclose(skill[:, 0], 1 - 1 / 100.0)
    with pytest.raises(ValueError):
        forecast.rollout_skill_reference(traj, f, [0, 7], d)  # 7 + 2 + 4 > 12


def test_range_rule_boundaries():
    T, Hf = 5, 2
    s = Hf + 1
    d = dims(T=T)
    for R in (1, 2, 4):
        t_total = 40
        o_in = forecast.rollout_origins(t_total, T, Hf, R, score=False)
        o_sc = forecast.rollout_origins(t_total, T, Hf, R, score=True)
        assert o_in[-1] + T + (R - 1) * s == t_total  # the boundary itself is admitted
        assert o_sc[-1] + T + R * s == t_total
        assert list(o_in) == list(range(len(o_in))) and o_in.dtype == np.int32
        f = stream(t_total)
        forecast.rollout_reference(Stub(d), f, [int(o_in[-1])], d, R, 0)
        with pytest.raises(ValueError):
            forecast.rollout_reference(Stub(d), f, [int(o_in[-1]) + 1], d, R, 0)
        with pytest.raises(ValueError):
            forecast.rollout_reference(Stub(d), f, [-1], d, R, 0)
        tr = forecast.rollout_reference(Stub(d), f, [int(o_sc[-1]), int(o_sc[-1]) + 1], d, R, 0)
        forecast.rollout_skill_reference(tr[:1], f, [int(o_sc[-1])], d)
        with pytest.raises(ValueError):
            forecast.rollout_skill_reference(tr[1:], f, [int(o_sc[-1]) + 1], d)
    for score in (False, True):  # one cycle admits what default_windows admits
        for t_total in (T, T + Hf, T + Hf + 1, 23):
            np.testing.assert_array_equal(forecast.rollout_origins(t_total, T, Hf, 1, score),
                                          forecast.default_windows(t_total, T, Hf, score))
    assert forecast.rollout_origins(6, T, Hf, 3, True).size == 0
    with pytest.raises(ValueError):
        forecast.rollout_origins(40, T, Hf, 0, True)
    with pytest.raises(ValueError):
        forecast.rollout_reference(Stub(d), stream(40), [0], d, 2, "linear")


def test_header_exports_and_bindings_agree():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, nargs in (("smaml_forecast_rollout", 12), ("smaml_rollout_stats", 4)):
        m = re.search(name + r"\s*\((.*?)\);", txt, flags=re.S)
        assert m, f"include/smaml.h does not declare {name}"
        assert name in _capi.EXPORTS and name in _capi._SIGS
        assert hasattr(_capi.lib(), name)
        assert len(m.group(1).split(",")) == len(_capi._SIGS[name][0]) == nargs
    src = open(_capi.__file__).read()  # (another test module may have swapped _capi.Context for a stub)
    assert "def forecast_rollout(self" in src and "def rollout_stats(self" in src
    assert len(_capi.ROLLOUT_STATS) == 5
    assert _capi.ROLLOUT_GAPS == forecast.GAPS == {"persistence": 0, "midpoint": 1}
    assert _capi.ABI_VERSION == 9 and _capi.lib().smaml_abi_version() == 9
    assert _capi.VARIANTS[-1] == "fwd_infer_drop"


def test_argument_errors_are_rejected_without_a_device():
    L = _capi.lib()
    P = ctypes.c_void_p
    fake = 256  # never dereferenced: every call below fails its argument checks first
    org = (ctypes.c_int32 * 1)(0)

    def call(norig=1, batch=1, cycles=1, gap=1, traj=fake, skill=fake, origins=org):
        return L.smaml_forecast_rollout(None, None, P(fake), 0, origins, norig, batch, cycles, gap, None,
                                        P(traj) if traj else None, P(skill) if skill else None)

    def msg():
        return L.smaml_last_error().decode()

    assert call() == 1 and "ctx is NULL" in msg()  # every argument check passed
    assert call(traj=0) == 1 and "ctx is NULL" in msg() and call(skill=0) == 1 and "ctx is NULL" in msg()
    assert call(traj=0, skill=0) == 1 and "both NULL" in msg()
    for kw in (dict(cycles=0), dict(cycles=-2)):
        assert call(**kw) == 1 and "cycles must be positive" in msg()
    for g in (-1, 2, 7):
        assert call(gap=g) == 1 and "gap must be 0" in msg() and str(g) in msg()
    for kw in (dict(norig=0), dict(norig=-1), dict(batch=0), dict(origins=None)):
        assert call(**kw) == 1 and "norig and batch must be positive" in msg()
    cnt = ctypes.c_int32()
    assert L.smaml_rollout_stats(None, None, 0, ctypes.byref(cnt)) == 1
