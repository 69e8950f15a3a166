"""bench.py's command line: --full gates the extra legs, --dump-outputs writes the last step's arrays."""
import sys
import types

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_float32_arrays(tmp_path):
    g = torch.Generator().manual_seed(0)
    res = types.SimpleNamespace(losses=torch.rand(6, 15, generator=g), norms=torch.rand(5, 15, generator=g))
    ml = types.SimpleNamespace(meta_grad=torch.rand(640, generator=g), theta=torch.rand(640, generator=g).double())
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), res, ml)
    assert sorted(p.name for p in out.iterdir()) == ["losses.npy", "meta_grad.npy", "norms.npy", "theta.npy"]
    for name, t in (("losses", res.losses), ("norms", res.norms), ("meta_grad", ml.meta_grad), ("theta", ml.theta)):
        a = np.load(out / (name + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        np.testing.assert_array_equal(a, t.float().numpy())
