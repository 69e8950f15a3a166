"""Meta-steps over window tables the default schedule never produces.

``smaml_meta_step`` takes the caller's window table, int32 [K+1][tasks][B], and decides per step from it
(``is_consec`` in api.cpp: B > 1 and every task's row is w0, w0+1, .., w0+B-1) whether the GCN and layer 0's
projection / weight gradient run once per distinct stream row and whether the step's features are stored
compact. ``window_table()`` with S = K B only ever yields steps that are all consecutive, equal for every
task and start at k B. The tables here (``TABLES``; C = a consecutive run, S = six scattered windows):

=========  =====  ==============================================================================================
 table     tasks  the first to reach
=========  =====  ==============================================================================================
 mixed_a   2      steps C S C, query S: compact and expanded ``so_F`` slots side by side, ``so_fc`` alternating in
                  the sweep, the ``xgd`` scratch used on one step and not the next; rows differ per task
 mixed_b   2      steps S C S, query C: the complement (first step, last step and query in the other state)
 per_task  3      every step consecutive, every task somewhere else (task 1's runs overlap, task 2's stream is
                  shorter): the per-task first-window table, and the table slices of task groups; the query
                  batches of tasks 0 and 2 end at the last valid window of their streams, task 0 starts at 0
 traps     2      K = 5: task 0 consecutive at every step, task 1 one near-consecutive row per step (last
                  window off by one, a repeat, descending, stride 2, a break after the first pair, all equal):
                  the whole step must take the per-window path
 wrap      2      ``window_table`` itself with S = 8, B = 6: (k B + b) mod S wraps inside a batch
 perm      2      per_task's first two tasks with every row permuted: the same batches, none consecutive
=========  =====  ==============================================================================================

Two shapes, both B = 6 x N = 49 = 294 rows (one full 256-row gate tile plus a partial one, the batch rule of
test_gpu_shapes.py): P (Hc = 16, L = 2: the per-layer GCN with ``k_gcn_expand``) and Q (Hc = 256, L = 1: the
fused ``k_gcn_mlp`` with its dedup and compact forms). Two arms as in test_gpu_shapes.py: the default knobs,
and ``big`` (``BIG_ARM``), in which ``f_compact``, ``xg_dedup`` and ``wgrad_dedup`` engage.

Launch counters. ``dedup_counts`` derives the four dedup counters of the big arm from the ``count_variant``
sites: ``run_gcn`` counts ``gcn_dedup`` and ``f_compact`` once per forward of a consecutive step (K inner steps
+ the query; the sweep reads the kept ``so_F`` slot and runs no GCN); ``launch_xg_dedup`` counts once per
primal forward of a consecutive step and, in the second-order sweep, once (the tangent table; the step's
primal kept) or twice (+ the primal table; recomputed) per consecutive inner step; ``timed_wgrad_ih0_dedup``
counts once per backward of a consecutive step (every inner step + the query, at order 1 and 2) and once per
consecutive inner step in the sweep's tangent backward.

Guard bands. Every stream here is the middle slice of a larger device tensor whose rows before and after
it are NaN, so a read outside the stream that reaches arithmetic turns a loss or a gradient into NaN.

Tolerances are the project's (test_gpu_parity.py): per-step losses and adapted parameters 1e-5 rel-L2, query
MSE and meta-gradient 1e-4. tests/test_oracle_windows_cpu.py checks on the CPU that the tables are what this
docstring says (classification, ranges) and that they discriminate.
"""
import numpy as np
import pytest
import torch

from oracle import refcpu
from weatherforecast_stgcn_maml_amd import _capi, params, synth
from weatherforecast_stgcn_maml_amd.config import MamlConfig, ModelDims
from weatherforecast_stgcn_maml_amd.maml import MetaLearner, query_starts, window_table

from test_gpu_parity import DEV, _check_meta_step, grid_edges, rel, split
from test_gpu_shapes import check_adapted

pytestmark = pytest.mark.gpu

SHAPES = {
    "P": ModelDims(num_nodes=49, window_size=3, hidden_channels=16, lstm_hidden_size=32, lstm_num_layers=2),
    "Q": ModelDims(num_nodes=49, window_size=3, hidden_channels=256, lstm_hidden_size=32, lstm_num_layers=1),
}
SEEDS = {"P": 81, "Q": 82}
B, N, T, HF = 6, 49, 3, SHAPES["P"].forecast_horizon
BIG_ARM = (("wgrad_group_max_rows", 0), ("bwd_big_min", 0), ("bwdd_big_min", 0), ("split_max", 1))
DEDUP = ("gcn_dedup", "f_compact", "xg_dedup", "wgrad_dedup")

# ----------------------------------------------------------------------------- streams
WINDOWS = (40, 40, 33)  # windows of task 0, 1, 2: task 2's stream is shorter
T_TOTAL = tuple(synth.t_total_for(n, T, HF) for n in WINDOWS)
LAST = tuple(t - T - HF - 1 for t in T_TOTAL)  # last valid window start: w + T + Hf = t_total - 1
PAD = 16  # NaN rows before and after each stream (more than the B + T - 1 rows a distinct-row pass reads)
_STREAMS = {}


def stream(j):
    if j not in _STREAMS:
        _STREAMS[j] = synth.make_features(8100 + j, N, T_TOTAL[j])
    return _STREAMS[j]


def guarded(feats):
    """The stream as the middle slice of a device tensor with PAD NaN rows on either side. A row is N x 24
    floats = 4,704 bytes, so the slice is contiguous and 16-byte aligned; MetaLearner.set_tasks keeps it."""
    t = feats.shape[0]
    big = torch.full((PAD + t + PAD,) + feats.shape[1:], float("nan"), device=DEV)
    big[PAD:PAD + t] = torch.from_numpy(feats)
    view = big[PAD:PAD + t]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    assert bool(torch.isnan(big[:PAD]).all()) and bool(torch.isnan(big[PAD + t:]).all())
    return view


# ----------------------------------------------------------------------------- tables
def run(w0):
    return list(range(w0, w0 + B))


def table(*steps):
    """int32 [K+1][tasks][B] from one list of per-task rows per step, the query batch last."""
    return np.asarray(steps, np.int32)


# six scattered, non-monotonic windows; between them the first (0) and the last (39) window of a stream
S0, S1 = [17, 3, 39, 8, 22, 11], [31, 5, 14, 26, 2, 19]
S2, S3 = [9, 33, 1, 24, 12, 28], [6, 35, 18, 0, 27, 13]


def permuted(w, seed):
    """Every row of the table in another (never the identity) order."""
    rng = np.random.default_rng(seed)
    out = np.array(w, np.int32)
    for row in out.reshape(-1, out.shape[-1]):
        p = rng.permutation(len(row))
        while np.array_equal(p, np.arange(len(row))):
            p = rng.permutation(len(row))
        row[:] = row[p]
    return out


WRAP_CFG = dict(inner_steps=3, batch=B, support_samples=8)
DEFAULT_CFG = MamlConfig(inner_steps=3, batch=B)

TABLES = {
    "mixed_a": table([run(4), run(20)], [S0, S1], [run(30), run(9)], [S2, S3]),
    "mixed_b": table([S0, S1], [run(13), run(27)], [S2, S3], [run(LAST[0] - B + 1), run(0)]),
    "per_task": table([run(0), run(11), run(7)], [run(6), run(13), run(2)], [run(12), run(15), run(21)],
                      [run(LAST[0] - B + 1), run(24), run(LAST[2] - B + 1)]),
    "traps": table([run(0), [5, 6, 7, 8, 9, 11]], [run(7), [5, 6, 7, 7, 8, 9]], [run(14), [10, 9, 8, 7, 6, 5]],
                   [run(21), [0, 2, 4, 6, 8, 10]], [run(28), [3, 4, 6, 7, 8, 9]], [run(33), [4, 4, 4, 4, 4, 4]]),
    "wrap": window_table(MamlConfig(**WRAP_CFG), 2),
}
TABLES["perm_base"] = TABLES["per_task"][:, :2].copy()
TABLES["perm"] = permuted(TABLES["perm_base"], 5)
# not run on the GPU: what the discrimination tests compare with
TABLES["default"] = window_table(DEFAULT_CFG, 2, query_start=query_starts(DEFAULT_CFG, WINDOWS[:2]))
TABLES["per_task_swapped"] = TABLES["per_task"][:, [1, 0, 2]].copy()

# whether each step (the query batch last) is meant to be consecutive
INTENT = {
    "mixed_a": [True, False, True, False],
    "mixed_b": [False, True, False, True],
    "per_task": [True] * 4,
    "traps": [False] * 6,
    "wrap": [True, False, False, True],
    "perm_base": [True] * 4,
    "perm": [False] * 4,
    "default": [True] * 4,
    "per_task_swapped": [True] * 4,
}


def rejected_tables():
    """{name: (table, task the error must name)}: per_task with one entry out of range."""
    past = TABLES["per_task"].copy()
    past[-1, -1, -1] = LAST[2] + 1
    neg = TABLES["per_task"].copy()
    neg[1, 1, 0] = -1
    return {"past_end": (past, 2), "negative": (neg, 1)}


def consecutive_steps(w):
    """api.cpp's is_consec: step k is consecutive iff B > 1 and every task's row is w0, w0 + 1, .., w0 + B - 1."""
    w = np.asarray(w)
    nb = w.shape[2]
    return [bool(nb > 1 and np.all(w[k] == w[k][:, :1] + np.arange(nb))) for k in range(w.shape[0])]


def dedup_counts(w, order, kept=0, groups=None):
    """The four dedup counters of one meta-step over table `w` in the big arm (module docstring), `kept` =
    inner steps whose primal the sweep keeps (the last `kept` ones); groups: the task slices of a MetaLearner
    that runs in task groups (one smaml_meta_step per group)."""
    if groups is not None:
        parts = [dedup_counts(w[:, z0:z0 + n], order, kept) for z0, n in groups]
        return {k: sum(p[k] for p in parts) for k in DEDUP}
    c = consecutive_steps(w)
    K = len(c) - 1
    exp = {k: sum(c) for k in DEDUP}
    if order == 2:
        for k in range(K):
            if c[k]:
                exp["xg_dedup"] += 1 if K - 1 - k < kept else 2
                exp["wgrad_dedup"] += 1
    return exp


# ----------------------------------------------------------------------------- oracle
_MODEL, _ORACLE = {}, {}


def model(tag):
    if tag not in _MODEL:
        d = SHAPES[tag]
        P = synth.init_params(SEEDS[tag], d, gcn_bias_scale=0.1)
        _MODEL[tag] = (d, P, split(P)[2], grid_edges(d))
    return _MODEL[tag]


def oracle(tag, name, order):
    """refcpu.meta_step under table `name` (computed once per key; finite, or it is no reference)."""
    key = (tag, name, order)
    if key not in _ORACLE:
        d, P, names, ei = model(tag)
        w = TABLES[name]
        K, Z = w.shape[0] - 1, w.shape[1]
        cfg = MamlConfig(inner_steps=K, batch=B, order=order)
        PT = refcpu.to_torch(P)
        Pt, Pg = {k: PT[k] for k in names}, {k: v for k, v in PT.items() if k not in names}
        tasks = [refcpu.TaskData(stream(j), ei, d) for j in range(Z)]
        if name == "wrap":  # the schedule the existing arguments express: (k B + b) mod S, query at S
            S = WRAP_CFG["support_samples"]
            ref = refcpu.meta_step(Pt, Pg, tasks, run(S), K, B, S, cfg.inner_lr, cfg.max_norm, order)
        else:
            ref = refcpu.meta_step(Pt, Pg, tasks, None, K, B, None, cfg.inner_lr, cfg.max_norm, order, windows=w)
        assert oracle_finite(ref), key
        _ORACLE[key] = ref
    return _ORACLE[key]


def oracle_finite(ref):
    vals = [np.asarray(ref["query_losses"]), np.asarray(ref["step_records"])]
    vals += [v.numpy() for v in ref["meta_grad"].values()]
    vals += [v.numpy() for ad in ref["adapted"] for v in ad.values()]
    return all(np.isfinite(v).all() for v in vals)


def flat_meta_grad(ref, names):
    return np.concatenate([ref["meta_grad"][k].numpy().ravel() for k in names])


# ----------------------------------------------------------------------------- running a case
def learner(tag, w, order, arm, keep=None, task_group=None):
    """A MetaLearner of shape `tag` for table `w` (its K and its tasks, each stream between guard bands)."""
    d, P, names, ei = model(tag)
    theta, gcn, _ = split(P)
    cfg = MamlConfig(inner_steps=w.shape[0] - 1, batch=B, order=order)
    ml = MetaLearner(d, cfg, gcn, theta, ei, device=DEV, task_group=task_group)
    ml.set_tasks([guarded(stream(j)) for j in range(w.shape[1])])
    if arm == "big":
        for k, v in BIG_ARM:
            ml.ctx.set_option(k, v)
    if keep is not None:
        ml.ctx.set_option("keep", keep)
    return ml


def meta_step(ml, w, label):
    """One meta-step over table `w`: (result, adapted parameters, launch counters since a reset)."""
    assert ml.cfg.inner_steps == w.shape[0] - 1 and len(ml.tasks) == w.shape[1]
    fast = torch.zeros(w.shape[1], ml.theta.numel(), device=DEV)
    ml.ctx.variant_counts(reset=True)
    res = ml.meta_step(windows=w, fast_out=fast)
    vc = ml.ctx.variant_counts()
    print(f"{label}: {({k: v for k, v in vc.items() if v})}")
    return res, fast, vc


def check_against_oracle(label, res, ml, fast, ref, tag):
    """Finite outputs, then the project's tolerances; prints the largest error of each kind first."""
    d, _, names, _ = model(tag)
    K, Z = res.losses.shape[0] - 1, res.losses.shape[1]
    losses, norms = res.losses.cpu().numpy(), res.norms.cpu().numpy()
    mg = params.unpack(ml.meta_grad, d, 0)
    for what, a in (("losses", losses), ("norms", norms), ("meta-gradient", ml.meta_grad.cpu().numpy()),
                    ("adapted parameters", fast.cpu().numpy())):
        assert np.isfinite(a).all(), f"{label}: {what} not finite (a read outside a stream reaches them as NaN)"
    e_step = max(rel(losses[:K, j], [r[0] for r in ref["step_records"][j]]) for j in range(Z))
    e_query = max(abs(losses[-1, j] - ref["query_losses"][j]) / ref["query_losses"][j] for j in range(Z))
    e_mg = max(rel(mg[k].cpu().numpy(), ref["meta_grad"][k].numpy()) for k in names)
    e_ad = max(rel(params.unpack(fast[j], d, 0)[k].cpu().numpy(), ref["adapted"][j][k].numpy())
               for j in range(Z) for k in names)
    print(f"ERR {label}: step losses {e_step:.3g} (1e-5), adapted {e_ad:.3g} (1e-5), query MSE {e_query:.3g} (1e-4), "
          f"meta-gradient {e_mg:.3g} (1e-4)")
    _check_meta_step(res, ml, ref, d, names, Z, K)
    check_adapted(fast, ref, d, names)


def check_dedup(vc, w, order, arm, kept=0, groups=None):
    exp = dedup_counts(w, order, kept, groups)
    if arm == "big":
        assert {k: vc[k] for k in DEDUP} == exp, (vc, exp)
    else:  # the distinct-row GCN does not depend on the tiles
        assert vc["gcn_dedup"] == exp["gcn_dedup"], (vc, exp)


def kept_steps(ml, w, keep):
    """Inner steps whose primal the sweep kept: all of them unless `keep` says 0 (asserted, since the
    xg_dedup count depends on it)."""
    K = w.shape[0] - 1
    kept = ml.ctx.so_kept_steps()
    assert kept == (0 if keep == 0 else K), (kept, keep)
    return kept


# ----------------------------------------------------------------------------- a. mixed steps
MIXED_ARMS = [(1, "default", None), (1, "big", None), (2, "default", None), (2, "big", -1), (2, "big", 0)]


@pytest.mark.parametrize("order,arm,keep", MIXED_ARMS, ids=[f"o{o}-{a}" + ("" if k is None else f"-keep{k}")
                                                          for o, a, k in MIXED_ARMS])
@pytest.mark.parametrize("name", ["mixed_a", "mixed_b"])
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_mixed_steps_match_oracle(tag, name, order, arm, keep):
    """K = 3, 2 tasks, consecutive and scattered steps in one meta-step (C S C | S and S C S | C): the dedup and
    compact kernels run on exactly the consecutive steps, and the result is the oracle's."""
    w = TABLES[name]
    ml = learner(tag, w, order, arm, keep)
    label = f"{tag} {name} order {order} {arm}" + ("" if keep is None else f" keep {keep}")
    res, fast, vc = meta_step(ml, w, label)
    kept = kept_steps(ml, w, keep) if order == 2 else 0
    check_dedup(vc, w, order, arm, kept)
    check_against_oracle(label, res, ml, fast, oracle(tag, name, order), tag)


# ----------------------------------------------------------------------------- b, c. per-task tables, guard bands
@pytest.mark.parametrize("arm", ["default", "big"])
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_per_task_tables_match_oracle(tag, arm):
    """Second order, 3 tasks, every step consecutive but every task somewhere else, one stream shorter; the
    query batches of tasks 0 and 2 end at their streams' last valid window, task 0 starts at row 0 of its
    stream, and the rows outside every stream are NaN."""
    w = TABLES["per_task"]
    ml = learner(tag, w, 2, arm)
    label = f"{tag} per_task order 2 {arm}"
    res, fast, vc = meta_step(ml, w, label)
    kept = kept_steps(ml, w, None)
    check_dedup(vc, w, 2, arm, kept)
    assert dedup_counts(w, 2, kept) == dedup_counts(TABLES["default"], 2, kept)  # as an all-consecutive table
    check_against_oracle(label, res, ml, fast, oracle(tag, "per_task", 2), tag)


@pytest.mark.parametrize("tag", ["P", "Q"])
def test_per_task_tables_in_task_groups(tag):
    """The same table with the 3 tasks run in task groups of 2 (MetaLearner slices windows[:, z0:z0+n] and
    sets each group's streams): big arm, second order."""
    w = TABLES["per_task"]
    ml = learner(tag, w, 2, "big", task_group=2)
    groups = [(z0, len(g)) for z0, g in ml._groups]
    assert groups == [(0, 2), (2, 1)]
    label = f"{tag} per_task order 2 big groups of 2"
    res, fast, vc = meta_step(ml, w, label)
    check_dedup(vc, w, 2, "big", kept_steps(ml, w, None), groups)
    check_against_oracle(label, res, ml, fast, oracle(tag, "per_task", 2), tag)


# ----------------------------------------------------------------------------- d. near-consecutive rows
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_one_task_breaks_the_run(tag, order):
    """K = 5, big arm: task 0 consecutive at every step, task 1 near-consecutive in six ways. No step may take
    a distinct-row kernel (all four counters 0), and the result is the oracle's."""
    w = TABLES["traps"]
    ml = learner(tag, w, order, "big")
    label = f"{tag} traps order {order} big"
    res, fast, vc = meta_step(ml, w, label)
    assert all(vc[k] == 0 for k in DEDUP), vc
    check_against_oracle(label, res, ml, fast, oracle(tag, "traps", order), tag)


# ----------------------------------------------------------------------------- e. wrap-around
@pytest.mark.parametrize("tag", ["P", "Q"])
def test_support_schedule_wraps_inside_a_batch(tag):
    """window_table with S = 8, B = 6: [0..5], [6,7,0,1,2,3], [4,5,6,7,0,1], query [8..13]; big arm, second order,
    against the oracle's own (k B + b) mod S schedule."""
    w = TABLES["wrap"]
    assert w[1, 0].tolist() == [6, 7, 0, 1, 2, 3] and w[2, 1].tolist() == [4, 5, 6, 7, 0, 1]
    ml = learner(tag, w, 2, "big")
    label = f"{tag} wrap order 2 big"
    res, fast, vc = meta_step(ml, w, label)
    check_dedup(vc, w, 2, "big", kept_steps(ml, w, None))
    check_against_oracle(label, res, ml, fast, oracle(tag, "wrap", 2), tag)


# ----------------------------------------------------------------------------- f. permutation invariance
def test_permuted_batches_give_the_same_step():
    """A consecutive table through the distinct-row kernels and the same batches permuted through the
    per-window kernels compute the same means over samples: losses and norms to 1e-6, the meta-gradient to
    1e-5 (the bounds of test_xg_dedup_against_oracle_and_off for the same comparison). Q, big arm, order 2."""
    out = []
    for name in ("perm_base", "perm"):
        w = TABLES[name]
        ml = learner("Q", w, 2, "big")
        res, fast, vc = meta_step(ml, w, f"Q {name} order 2 big")
        if name == "perm":
            assert all(vc[k] == 0 for k in DEDUP), vc
        else:
            check_dedup(vc, w, 2, "big", kept_steps(ml, w, None))
        out.append((res.losses.cpu().numpy(), res.norms.cpu().numpy(), ml.meta_grad.cpu().numpy().copy()))
        assert all(np.isfinite(a).all() for a in out[-1])
    e = [rel(out[1][i], out[0][i]) for i in range(3)]
    print(f"ERR Q perm vs perm_base: losses {e[0]:.3g} (1e-6), norms {e[1]:.3g} (1e-6), meta-gradient {e[2]:.3g} (1e-5)")
    assert e[0] < 1e-6 and e[1] < 1e-6
    assert e[2] < 1e-5


# ----------------------------------------------------------------------------- g. rejection
@pytest.mark.parametrize("name", ["past_end", "negative"])
def test_out_of_range_window_is_rejected_before_any_launch(name):
    """One entry past a stream's last valid window (the last task's query row) or one -1: smaml_meta_step and
    smaml_inner_loop return SMAML_EINVAL naming the task and launch nothing; the context then runs a valid
    meta-step that matches the oracle."""
    bad, z = rejected_tables()[name]
    good = TABLES["per_task"]
    assert int((bad != good).sum()) == 1
    ml = learner("P", good, 2, "big")
    K = good.shape[0] - 1
    cfg = ml.cfg
    st = _capi.stream_ptr(torch)
    fast = torch.zeros(3, ml.theta.numel(), device=DEV)
    losses, norms = torch.zeros(K + 1, 3, device=DEV), torch.zeros(K, 3, device=DEV)
    calls = {
        "smaml_meta_step": lambda: ml.ctx.meta_step(st, ml.theta, 2, K, B, bad, cfg.inner_lr, cfg.max_norm,
                                                    cfg.query_loss_scale, meta_grad=ml.meta_grad, losses=losses,
                                                    norms=norms, fast_out=fast),
        "smaml_inner_loop": lambda: ml.ctx.inner_loop(st, ml.theta, K, B, bad, cfg.inner_lr, cfg.max_norm, fast,
                                                      losses=losses, norms=norms),
    }
    ml.ctx.variant_counts(reset=True)
    for entry, call in calls.items():
        with pytest.raises(_capi.SmamlError, match=f"EINVAL.*window start out of range for task {z}"):
            call()
    torch.cuda.synchronize()
    assert not any(ml.ctx.variant_counts().values()), ml.ctx.variant_counts()
    assert float(fast.abs().max()) == 0.0 and float(losses.abs().max()) == 0.0  # nothing was written either
    label = f"P per_task order 2 big after {name}"
    res, fast, vc = meta_step(ml, good, label)
    check_dedup(vc, good, 2, "big", kept_steps(ml, good, None))
    check_against_oracle(label, res, ml, fast, oracle("P", "per_task", 2), "P")
