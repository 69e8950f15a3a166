"""The ABI of ``smaml_backward_base`` and the module API's ``base_grad`` switch: no GPU."""
import ctypes
import os
import re

import torch

from weatherforecast_stgcn_maml_amd import _capi
from weatherforecast_stgcn_maml_amd.config import CONFIG1

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_backward_base_is_declared_exported_and_bound():
    txt = open(os.path.join(REPO, "include", "smaml.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"smaml_backward_base\s*\((.*?)\);", txt, flags=re.S)
    assert m, "include/smaml.h does not declare smaml_backward_base"
    assert "smaml_backward_base" in _capi.EXPORTS and "smaml_backward_base" in _capi._SIGS
    assert hasattr(_capi.lib(), "smaml_backward_base")
    assert len(m.group(1).split(",")) == len(_capi._SIGS["smaml_backward_base"][0]) == 9
    assert hasattr(_capi.Context, "backward_base")
    # one new symbol, the same ABI number
    assert _capi.ABI_VERSION == 9 and _capi.lib().smaml_abi_version() == 9


def test_null_arguments_are_rejected_without_a_device():
    L = _capi.lib()
    P = ctypes.c_void_p
    one = (P * 1)(P(256))
    fake = P(256)  # never dereferenced: every call below fails its argument checks first

    def msg():
        return L.smaml_last_error().decode()

    # NULL context
    assert L.smaml_backward_base(None, None, fake, one, 1, fake, fake, fake, one) == 1
    assert "ctx is NULL" in msg()
    # nothing to compute: gcn_grad and dx_host both NULL
    assert L.smaml_backward_base(None, None, fake, one, 1, fake, fake, None, None) == 1
    assert "both NULL" in msg()
    # NULL theta / samples / dpred / grad, no samples
    for args in ((None, one, 1, fake, fake), (fake, None, 1, fake, fake), (fake, one, 1, None, fake),
                 (fake, one, 1, fake, None), (fake, one, 0, fake, fake)):
        assert L.smaml_backward_base(None, None, *args, fake, None) == 1
        assert "bad backward_base arguments" in msg()


def _hybrid(**kw):
    from weatherforecast_stgcn_maml_amd.hybrid_model import HybridSTGCN_LSTM
    from weatherforecast_stgcn_maml_amd.model import STGCN

    d = CONFIG1
    base = STGCN(d.input_channels, d.hidden_channels, d.output_channels, d.window_size, d.forecast_horizon)
    return HybridSTGCN_LSTM(base, d.lstm_hidden_size, d.lstm_num_layers, 0.2, d.output_channels, d.forecast_horizon,
                            **kw)


def test_base_grad_defaults_to_off_and_stays_out_of_the_state_dict():
    torch.manual_seed(0)
    off = _hybrid(freeze_base=False)
    assert off.base_grad is False
    on = _hybrid(freeze_base=False, base_grad=True)
    assert on.base_grad is True
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert off.enable_base_grad() is off and off.base_grad is True
    assert list(off.state_dict().keys()) == list(on.state_dict().keys())
    off.enable_base_grad(False)
    assert off.base_grad is False
    # the switch alone changes no requires_grad
    assert all(p.requires_grad for p in on.base_stgcn.parameters())
    assert not any(p.requires_grad for p in _hybrid(freeze_base=True, base_grad=True).base_stgcn.parameters())
