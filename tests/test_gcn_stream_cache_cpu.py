"""Host side of the per-stream GCN feature cache: the memory plan (``maml.task_bytes`` without the per-step
feature store that ``ensure_so_store`` no longer makes for cached meta-steps, the cache's own bytes), the binding of
``smaml_gcn_cache_invalidate`` and the two counters."""
import os
import re

from weatherforecast_stgcn_maml_amd import _capi
from weatherforecast_stgcn_maml_amd.config import CONFIG2, CONFIG5, MamlConfig
from weatherforecast_stgcn_maml_amd.maml import (KEEP_MARGIN, gcn_cache_applies, plan_task_group, stream_cache_bytes,
                                                  stream_len_for, task_bytes)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 1 << 30
HBM = 268 * GIB


def test_task_bytes_drops_exactly_the_per_step_feature_store():
    """ensure_so_store's store is float [K][Z][B][T][N][Hc]: per task K B T N Hc 4 bytes, at any kept count."""
    for d, cfg in ((CONFIG2, MamlConfig(inner_steps=5, batch=32, order=2)),
                   (CONFIG5, MamlConfig(inner_steps=10, batch=32, order=2))):
        store = cfg.inner_steps * cfg.batch * d.window_size * d.num_nodes * d.hidden_channels * 4
        for kept in (0, 1, cfg.inner_steps):
            assert task_bytes(d, cfg, kept) - task_bytes(d, cfg, kept, gcn_cached=True) == store
            assert task_bytes(d, cfg, kept, gcn_cached=False) == task_bytes(d, cfg, kept)


def test_stream_cache_bytes_and_when_it_applies():
    cfg = MamlConfig(inner_steps=5, batch=32, order=2)
    rows = stream_len_for(cfg, CONFIG2)
    b = stream_cache_bytes(CONFIG2, rows)
    assert b == 2 * rows * 441 * 256 * 4
    # two tables of one stream against the store of ONE task's meta-step: far smaller
    assert 15 * b < 5 * (task_bytes(CONFIG2, cfg, 5) - task_bytes(CONFIG2, cfg, 5, True))
    assert gcn_cache_applies(cfg, 0.0)
    assert not gcn_cache_applies(cfg, 0.2)
    assert not gcn_cache_applies(MamlConfig(inner_steps=5, batch=1, order=2), 0.0)


def test_plan_counts_the_cache_of_every_stream():
    cfg = MamlConfig(inner_steps=5, batch=32, order=2)
    rows = stream_len_for(cfg, CONFIG2)
    per = task_bytes(CONFIG2, cfg, 5, True)
    for n in (15, 8, 7, 4, 2):
        g = plan_task_group(CONFIG2, cfg, n, HBM, True, rows)
        assert g == plan_task_group(CONFIG2, cfg, n, HBM), n  # the bench's groups stay what they were
        assert g * per + n * stream_cache_bytes(CONFIG2, rows) <= HBM - KEEP_MARGIN
    # the cache of many long streams takes room from the groups
    assert plan_task_group(CONFIG2, cfg, 15, HBM, True, 200 * rows) < plan_task_group(CONFIG2, cfg, 15, HBM, True, rows)
    cfg5 = MamlConfig(inner_steps=10, batch=32, order=2)
    assert plan_task_group(CONFIG5, cfg5, 8, HBM, True, stream_len_for(cfg5, CONFIG5)) == 1


def test_binding_and_counters():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+smaml_gcn_cache_invalidate\s*\(\s*smaml_ctx\s*\*\s*ctx\s*\)\s*;", code)
    assert "smaml_gcn_cache_invalidate" in _capi.EXPORTS
    args, res = _capi._SIGS["smaml_gcn_cache_invalidate"]
    assert len(args) == 1 and res is _capi.I32
    assert hasattr(_capi.lib(), "smaml_gcn_cache_invalidate")
    # VARIANTS names the counters of kernels.h's enum Variant, in its order
    kh = open(os.path.join(REPO, "weatherforecast_stgcn_maml_amd", "csrc", "kernels.h")).read()
    body = re.search(r"enum Variant\s*\{(.*?)\bNVAR\b", kh, flags=re.S).group(1)
    names = re.findall(r"^\s*(V_[A-Z0-9_]+)\s*(?:=\s*\d+\s*)?,", body, flags=re.M)
    assert len(names) == len(_capi.VARIANTS)
    i = names.index("V_GCN_CACHE")
    assert names[i + 1] == "V_GCN_CACHE_ROWS"
    assert _capi.VARIANTS[i:i + 2] == ("gcn_cache", "gcn_cache_rows")
    assert "smaml_gcn_cache_invalidate" in open(os.path.join(REPO, "INTEGRATION.md")).read()
