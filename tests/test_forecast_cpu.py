"""CPU statement of the forecast skill sums (``forecast.skill_reference``) and the default window lists."""
import numpy as np
import torch

from weatherforecast_stgcn_maml_amd import forecast
from weatherforecast_stgcn_maml_amd.config import ModelDims
from weatherforecast_stgcn_maml_amd.dataset import WeatherGraphDataset

# the hand-built case: 2 windows, N = 3, Hf = 2, C = 2 (T = 2, 4 input channels)
D = ModelDims(num_nodes=3, window_size=2, input_channels=4, hidden_channels=4, lstm_hidden_size=32,
              lstm_num_layers=1, forecast_horizon=2, output_channels=2)


def hand_case():
    """features[t, n, c] = 10 t + 3 n + c; the prediction of flat row r (= n Hf + h in the model's own
    order) is the target that the F4 pairing gives it -- (h' = r // N, n' = r % N) -- plus r + 1 for
    variable 0 and minus (r + 1) for variable 1."""
    T, Hf, N, C = D.window_size, D.forecast_horizon, D.num_nodes, D.output_channels
    t, n, c = np.meshgrid(np.arange(7), np.arange(N), np.arange(4), indexing="ij")
    feats = (10 * t + 3 * n + c).astype(np.float32)
    windows = [0, 1]
    pred = np.zeros((2, N * Hf, C), np.float32)
    for i, w in enumerate(windows):
        for r in range(N * Hf):
            hp, np_ = r // N, r % N
            pred[i, r, 0] = feats[w + T + 1 + hp, np_, 0] + (r + 1)
            pred[i, r, 1] = feats[w + T + 1 + hp, np_, 1] - (r + 1)
    return feats, windows, pred


def test_skill_reference_hand_case():
    feats, windows, pred = hand_case()
    scale = [2.0, 0.5]
    s = forecast.skill_reference(pred, feats, windows, D, scale)
    assert s.shape == (3, 2, 2) and s.dtype == np.float64
    # errors of lead 0 are 1, 2, 3 (rows 0..2), of lead 1 are 4, 5, 6 (rows 3..5), in both windows
    sse = [[4 * 2 * (1 + 4 + 9), 0.25 * 2 * (1 + 4 + 9)], [4 * 2 * (16 + 25 + 36), 0.25 * 2 * (16 + 25 + 36)]]
    sae = [[2 * 2 * (1 + 2 + 3), 0.5 * 2 * (1 + 2 + 3)], [2 * 2 * (4 + 5 + 6), 0.5 * 2 * (4 + 5 + 6)]]
    # persistence: y_last - y = f[w+T-1] - f[w+T+1+h'] = -10 (2 + h') at every node, 2 windows x 3 nodes
    pers = [[6 * (2 * 20) ** 2, 6 * (0.5 * 20) ** 2], [6 * (2 * 30) ** 2, 6 * (0.5 * 30) ** 2]]
    np.testing.assert_array_equal(s[0], np.array(sse, np.float64))
    np.testing.assert_array_equal(s[1], np.array(sae, np.float64))
    np.testing.assert_array_equal(s[2], np.array(pers, np.float64))
    assert forecast.SUMS == ("sse", "sae", "persistence_sse")
    # without a scale the factors are 1
    s1 = forecast.skill_reference(pred, feats, windows, D)
    np.testing.assert_array_equal(s1[0], np.array(sse) / np.array([4, 0.25]))


def test_skill_reference_is_the_f4_pairing_not_the_model_order():
    """Read in the model's own (node, horizon) order the same predictions are wrong: the sums differ."""
    feats, windows, pred = hand_case()
    T, Hf, N, C = D.window_size, D.forecast_horizon, D.num_nodes, D.output_channels
    model_order = 0.0
    for i, w in enumerate(windows):
        for n in range(N):
            for h in range(Hf):
                model_order += float(pred[i, n * Hf + h, 0] - feats[w + T + 1 + h, n, 0]) ** 2
    assert model_order != forecast.skill_reference(pred, feats, windows, D)[0, :, 0].sum()


def test_skill_reference_rejects_windows_without_targets():
    feats, _, pred = hand_case()
    T, Hf = D.window_size, D.forecast_horizon
    last = feats.shape[0] - T - Hf - 1  # the last window with targets
    forecast.skill_reference(pred[:1], feats, [last], D)
    for w in (last + 1, -1):
        try:
            forecast.skill_reference(pred[:1], feats, [w], D)
        except ValueError:
            continue
        raise AssertionError(f"window {w} accepted")


def test_skill_metrics():
    sums = np.array([[[8.0, 2.0]], [[4.0, 2.0]], [[32.0, 0.0]]])  # [3, Hf = 1, C = 2], 2 pairs each
    rmse, mae, prmse, skill = forecast.skill_metrics(sums, 2)
    np.testing.assert_allclose(rmse, [[2.0, 1.0]])
    np.testing.assert_allclose(mae, [[2.0, 1.0]])
    np.testing.assert_allclose(prmse, [[4.0, 0.0]])
    assert skill[0, 0] == 0.75 and np.isnan(skill[0, 1])  # NaN where the baseline error is 0


def test_default_windows_match_the_dataset_and_extend_past_the_end():
    T, Hf, t_total = 24, 8, 40
    feats = torch.zeros(t_total, 3, 24)
    ds = WeatherGraphDataset(feats, None, T, Hf)
    scored = forecast.default_windows(t_total, T, Hf, True)
    assert scored.dtype == np.int32
    assert list(scored) == [ds.window_start(i) for i in range(len(ds))] == list(range(t_total - T - Hf))
    every = forecast.default_windows(t_total, T, Hf, False)
    assert list(every[:len(scored)]) == list(scored)
    assert len(every) == len(scored) + Hf + 1 and every[-1] + T == t_total  # the last one ends with the stream
    # streams too short for a sample / a window
    assert forecast.default_windows(T + Hf, T, Hf, True).size == 0
    assert list(forecast.default_windows(T + Hf, T, Hf, False)) == list(range(Hf + 1))
    assert forecast.default_windows(T - 1, T, Hf, False).size == 0
