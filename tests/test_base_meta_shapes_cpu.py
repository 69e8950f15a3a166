"""The cases of tests/test_gpu_base_meta_shapes.py (the base meta-gradient over every accepted shape) and, without a
device, the conditions that keep them from being vacuous -- modelled on test_base_meta_cpu.py's
``test_gpu_cases_discriminate``.

Cases (K = 2 inner steps, two tasks, a 4-neighbour grid graph; G: one task):

====  =========================================  =====  =============================================================
 id   dims                                       batch  the first to reach
====  =========================================  =====  =============================================================
 A    N=49, Hc=32, H=256, L=2, T=4               6      K = 1024 / 2048 in ``k_lstm_dx0_meta``, ``Cat2*`` switching at
                                                        k = 1024; a quarter-full column tile; 686 distinct rows =
                                                        10 row tiles + 46
 B    N=25, Hc=48, H=64, L=3, T=3                11     K = 256 / 512; the Hc = 48 column tail, 3 K tiles through
                                                        ``gcn_backward_chain``; an odd layer count
 C    N=36, Hc=16, H=32, L=4, T=2                8      T = 2: the compact rows fill a task's slab exactly, the block
                                                        past t = 0 is exactly B N rows; T < L
 D    N=25, Hc=64, H=128, L=2, T=1               11     T = 1 with two LSTM layers: no block past t = 0
 F    N=25, T=7, Cin=8, Hc=32, H=64, L=2,        3      T > B: the window slots that hold a stream row are capped by
      Hf=2, C=4                                         B; Cin0 = 8 in ``xcat``, the stream slices and conv1's dW
 G    CONFIG2 (N=441, T=24, Hc=256, H=128, L=4)  2      the shipped shape (order 2, unclipped, consecutive only)
====  =========================================  =====  =============================================================

A..D are test_gpu_shapes.py's shapes and batches. Tables per case: ``consec`` (task j reads the runs starting at
j, B + 1 + j and 2B + 3 + j) and ``mixed`` (step 0 that run, step 1 and the query B scattered windows, among them the
first and the last window of the stream). Settings: test_base_meta_cpu.SETTINGS.
"""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import synth
from weatherforecast_stgcn_maml_amd.config import CONFIG2, ModelDims

import base_meta_oracle as bmo
import test_gpu_shapes as gs
from test_base_meta_cpu import GRAD_TOL, SETTINGS, rel
from test_gpu_parity import grid_edges, split

K = 2
SEED = 70
BIAS_SCALE = 0.1
CASES = {  # tag: (dims, batch, tasks)
    "A": (gs.SHAPES["A"], gs.BATCH["A"], 2),
    "B": (gs.SHAPES["B"], gs.BATCH["B"], 2),
    "C": (gs.SHAPES["C"], gs.BATCH["C"], 2),
    "D": (gs.SHAPES["D"], gs.BATCH["D"], 2),
    "F": (ModelDims(num_nodes=25, window_size=7, input_channels=8, hidden_channels=32, lstm_hidden_size=64,
                    lstm_num_layers=2, forecast_horizon=2, output_channels=4), 3, 2),
    "G": (CONFIG2, 2, 1),
}
SWEEP = ("A", "B", "C", "D", "F")
# (table, setting) of every case: A..F the full set, G the shipped shape once
RUNS = {t: (("consec", "unclipped"), ("consec", "clipped"), ("mixed", "unclipped")) for t in SWEEP}
RUNS["G"] = (("consec", "unclipped"),)
ALL_RUNS = [(t, tab, s) for t in CASES for tab, s in RUNS[t]]
ROW_TILE, COL_TILE, K_TILE = 64, 128, 16  # CfgNN's BM and BN (k_lstm_dx0_meta), the loaders' BK


def nwin(tag):
    return 3 * CASES[tag][1] + 6


@functools.lru_cache(maxsize=None)
def model(tag):
    d = CASES[tag][0]
    P = synth.init_params(SEED, d, gcn_bias_scale=BIAS_SCALE)
    return d, P, split(P)[2], grid_edges(d)


@functools.lru_cache(maxsize=None)
def stream(tag, j):
    d = CASES[tag][0]
    f = synth.make_features(7700 + j, d.num_nodes, synth.t_total_for(nwin(tag), d.window_size, d.forecast_horizon))
    return np.ascontiguousarray(f[:, :, :d.input_channels])


def scattered(tag, j):
    """Two rows of B windows of task j, none consecutive, all distinct, the stream's first and last window among them."""
    B, n = CASES[tag][1], nwin(tag)
    rng = np.random.default_rng(1000 * B + j)
    pool = np.concatenate([[0, n - 1], 1 + rng.permutation(n - 2)])[:2 * B]
    rows = rng.permutation(pool).reshape(2, B)
    for r in rows:
        if np.all(np.diff(r) == 1):
            r[:] = r[::-1]
    return rows


@functools.lru_cache(maxsize=None)
def table(tag, name):
    """int32 [K + 1][tasks][B]."""
    _, B, Z = CASES[tag]
    run = lambda a: list(range(a, a + B))  # noqa: E731
    steps = [[run(0 + j) for j in range(Z)], [run(B + 1 + j) for j in range(Z)], [run(2 * B + 3 + j) for j in range(Z)]]
    if name == "mixed":
        for j in range(Z):
            s = scattered(tag, j)
            steps[1][j], steps[2][j] = list(s[0]), list(s[1])
    w = np.asarray(steps, np.int32)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def oracle(tag, name, order, setting, dtype=torch.float64):
    d, P, names, ei = model(tag)
    PT = refcpu.to_torch(P)
    Pt, Pg = {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names}
    w = table(tag, name)
    tasks = [refcpu.TaskData(stream(tag, j), ei, d) for j in range(w.shape[1])]
    lr, mn = SETTINGS[setting]
    return bmo.meta_step(Pt, Pg, tasks, w, lr, mn, order, dtype=dtype)


def consecutive(w):
    return [bool(w.shape[2] > 1 and np.all(w[k] == w[k][:, :1] + np.arange(w.shape[2]))) for k in range(w.shape[0])]


# ----------------------------------------------------------------------------- the tables
@pytest.mark.parametrize("tag", list(CASES))
def test_tables_are_what_the_docstring_says(tag):
    d, B, Z = CASES[tag]
    for name in ("consec", "mixed"):
        w = table(tag, name)
        assert w.shape == (K + 1, Z, B) and w.min() >= 0 and w.max() <= nwin(tag) - 1
        assert consecutive(w) == ([True] * 3 if name == "consec" else [True, False, False])
        for j in range(Z):
            assert stream(tag, j).shape == (nwin(tag) + d.window_size + d.forecast_horizon, d.num_nodes, d.input_channels)
    m = table(tag, "mixed")
    for j in range(Z):
        s = m[1:, j].ravel()
        assert len(set(s)) == 2 * B and 0 in s and nwin(tag) - 1 in s
    if Z > 1:  # the tasks read different rows
        assert not np.array_equal(table(tag, "consec")[:, 0], table(tag, "consec")[:, 1])


def test_shapes_reach_what_the_table_claims():
    """The row and tile counts behind the "first to reach" column."""
    rows = {}
    for tag, (d, B, _) in CASES.items():
        N, T = d.num_nodes, d.window_size
        rows[tag] = dict(distinct=(2 * B + T - 2) * N if T > 1 else B * N, per_sample=T * B * N, past0=(B + T - 2) * N if T > 1 else 0)
    d, B, _ = CASES["A"]
    assert 4 * d.lstm_hidden_size == 1024 and 8 * d.lstm_hidden_size == 2048
    assert d.hidden_channels * 4 == COL_TILE
    assert rows["A"]["distinct"] == 686 == 10 * ROW_TILE + 46
    d, B, _ = CASES["B"]
    assert 4 * d.lstm_hidden_size == 256 and d.hidden_channels == 3 * K_TILE and d.hidden_channels % 32 != 0
    assert d.lstm_num_layers % 2 == 1
    d, B, _ = CASES["C"]
    assert d.window_size == 2 < d.lstm_num_layers
    assert rows["C"]["distinct"] == rows["C"]["per_sample"] and rows["C"]["past0"] == B * d.num_nodes
    d, B, _ = CASES["D"]
    assert d.window_size == 1 and d.lstm_num_layers == 2 and rows["D"]["past0"] == 0
    assert rows["D"]["distinct"] == B * d.num_nodes == rows["D"]["per_sample"]
    d, B, _ = CASES["F"]
    assert d.window_size > B and d.input_channels == 8 and d.output_channels <= d.input_channels
    assert min(B, d.window_size) == B  # a stream row sits in at most B window slots, not T
    assert rows["F"]["distinct"] == 275 and rows["F"]["per_sample"] == 525
    d, B, _ = CASES["G"]
    assert (d.num_nodes, d.window_size, d.hidden_channels, d.lstm_hidden_size, d.lstm_num_layers) == (441, 24, 256, 128, 4)
    assert rows["G"]["distinct"] == 11466 and rows["G"]["per_sample"] == 21168
    # every T, H and Hc class differs from test_gpu_base_meta.py's (T = 3, H = 32; Hc 16 / 256; Cin 24)
    assert {CASES[t][0].lstm_hidden_size for t in CASES} == {32, 64, 128, 256}
    assert {CASES[t][0].hidden_channels for t in CASES} == {16, 32, 48, 64, 256}
    assert {CASES[t][0].window_size for t in CASES} == {1, 2, 3, 4, 7, 24}


# ----------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("tag,name,setting", ALL_RUNS, ids=["-".join(r) for r in ALL_RUNS])
def test_gpu_cases_discriminate(tag, name, setting):
    """Each base tensor's order-1-versus-order-2 difference is at least 10 times the gradient tolerance, the clip
    engages at every step of the clipped setting and at none of the other, and no gradient tensor is zero."""
    r1, r2 = oracle(tag, name, 1, setting), oracle(tag, name, 2, setting)
    for r in (r1, r2):
        coefs = [c for rec in r["step_records"] for _, _, c in rec]
        print(tag, name, setting, "coefs", [round(c, 4) for c in coefs])
        assert len(coefs) == K * CASES[tag][2]
        assert all(c < 1.0 for c in coefs) if setting == "clipped" else all(c == 1.0 for c in coefs), coefs
    for k in r2["gcn_grad"]:
        share = rel(r1["gcn_grad"][k].numpy(), r2["gcn_grad"][k].numpy())
        print(f"  {k}: order-1 vs order-2 {share:.3e}")
        assert share >= 10 * GRAD_TOL, (k, share)
    one_step = CASES[tag][0].window_size == 1
    for r in (r1, r2):
        for grp in ("gcn_grad", "meta_grad"):
            for k, v in r[grp].items():
                assert bool(torch.isfinite(v).all()), (grp, k)
                if one_step and k.startswith("lstm.weight_hh_l"):  # h_{t-1} never exists: zero by structure
                    assert float(v.abs().max()) == 0, (grp, k)
                else:
                    assert float(v.abs().max()) > 0, (grp, k)


@pytest.mark.parametrize("tag,name", [(t, n) for t, n, s in ALL_RUNS if s == "unclipped"])
def test_relu_mask_is_not_trivial(tag, name):
    """The share of zero entries of conv4's output over the query batch lies strictly inside (0.05, 0.95): the
    stage's ``F > 0`` mask neither passes nor blocks everything."""
    d, P, names, ei = model(tag)
    base = {k: v.double() for k, v in refcpu.to_torch(P).items() if k.startswith("base_stgcn.conv")}
    w = table(tag, name)
    eit = torch.from_numpy(np.ascontiguousarray(ei)).long()
    zeros = total = 0
    for j in range(w.shape[1]):
        task = refcpu.TaskData(stream(tag, j), ei, d)
        for i in w[K, j]:
            with torch.no_grad():
                f = refcpu.stgcn_features(task.xy(int(i))[0].double(), eit, base)
            assert f.shape == (d.window_size * d.num_nodes, d.hidden_channels) and float(f.min()) >= 0
            zeros += int((f == 0).sum())
            total += f.numel()
    share = zeros / total
    print(f"{tag} {name}: conv4 zero share {share:.3f}")
    assert 0.05 < share < 0.95, share


def test_float32_oracle_is_close_to_float64_at_h256():
    """The float32 oracle's own distance to float64 at A (K = 1024 / 2048 products): the size of error that f32
    arithmetic alone gives a case of the sweep."""
    r64, r32 = oracle("A", "mixed", 2, "unclipped"), oracle("A", "mixed", 2, "unclipped", torch.float32)
    for k in r64["gcn_grad"]:
        e = rel(r32["gcn_grad"][k].numpy(), r64["gcn_grad"][k].numpy())
        print(k, f"{e:.2e}")
        assert e < 1e-5, (k, e)


def test_f_has_eight_channel_streams():
    d = CASES["F"][0]
    assert dataclasses.asdict(d)["input_channels"] == 8
    P = model("F")[1]
    assert P["base_stgcn.conv1.lin.weight"].shape == (d.hidden_channels, 8)
