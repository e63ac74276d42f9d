"""The one way to make a native call (``_hip.call`` / ``launch`` / ``workspace``), against a stub library: no device, and
no built library for anything but the package's own source."""
import os
import re

import pytest
import torch

from diffsound_amd import _hip

STREAM = 0x5EED


class _Stub:
    """A library whose every entry point records its arguments and returns ``status``."""

    def __init__(self, status=0, error=b""):
        self.calls, self.status, self.error = [], status, error

    def ds_last_error(self):
        return self.error

    def __getattr__(self, symbol):
        if not symbol.startswith("ds_"):
            raise AttributeError(symbol)
        return lambda *args: self.calls.append((symbol, args)) or self.status


@pytest.fixture
def stub(monkeypatch):
    s = _Stub()
    monkeypatch.setattr(_hip, "lib", lambda: s)
    monkeypatch.setattr(_hip, "stream_ptr", lambda: STREAM)
    return s


def test_arguments_pass_through_and_only_launch_adds_the_stream(stub):
    t = torch.zeros(3)
    args = (t.data_ptr(), None, 7, 2.5, t)
    _hip.call("ds_host_thing", *args)
    _hip.launch("ds_thing_fwd", *args)
    _hip.launch("ds_thing_fwd", device=None)
    assert stub.calls == [("ds_host_thing", args), ("ds_thing_fwd", args + (STREAM,)), ("ds_thing_fwd", (STREAM,))]
    assert all(a is b for a, b in zip(stub.calls[1][1], args))


def test_the_stream_of_a_guarded_launch_is_taken_inside_the_guard(stub, monkeypatch):
    current = [0]

    class Guard:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            self.before, current[0] = current[0], self.device

        def __exit__(self, *exc):
            current[0] = self.before

    monkeypatch.setattr(torch.cuda, "device", Guard)
    monkeypatch.setattr(_hip, "stream_ptr", lambda: 100 + current[0])  # (one stream per device)
    _hip.launch("ds_thing_fwd", 7, device=1)
    _hip.launch("ds_thing_fwd", 7)
    assert stub.calls == [("ds_thing_fwd", (7, 101)), ("ds_thing_fwd", (7, 100))] and current == [0]
    stub.status = 1
    with pytest.raises(RuntimeError, match="ds_thing_bwd failed"):
        _hip.launch("ds_thing_bwd", device=1)
    assert current == [0]


@pytest.mark.parametrize("helper", ["call", "launch"])
@pytest.mark.parametrize("symbol", ["ds_spmm_f64_polish_f32out", "ds_osc_bank_bwd"])
def test_a_failure_names_the_symbol_that_was_called(stub, helper, symbol):
    stub.status, stub.error = 3, b"what the library said"
    with pytest.raises(RuntimeError) as e:
        getattr(_hip, helper)(symbol, 1, 2)
    assert str(e.value) == f"{symbol} failed (status 3): what the library said"
    assert [c[0] for c in stub.calls] == [symbol]


def test_workspace_is_the_query_and_its_allocation(stub):
    stub.status = 40
    w, n = _hip.workspace("ds_x_workspace_bytes", 2, 3, device="cpu")
    assert n == 40 and w.shape == (40,) and w.dtype == torch.uint8 and w.device.type == "cpu"
    w, n = _hip.workspace("ds_x_workspace_floats", 5, device="cpu", dtype=torch.float32)
    assert n == 40 and w.shape == (40,) and w.dtype == torch.float32
    assert stub.calls == [("ds_x_workspace_bytes", (2, 3)), ("ds_x_workspace_floats", (5,))]
    stub.status = 0
    w, n = _hip.workspace("ds_x_workspace_doubles", 1, device="cpu", dtype=torch.float64)
    assert n == 0 and w.shape == (0,) and w.dtype == torch.float64


def test_the_package_calls_the_library_through_the_helpers_only():
    """Outside _hip.py nothing checks a status by hand or hands ``stream_ptr()`` to an entry point: a new operator that does
    types the symbol twice again and chooses its own device."""
    pkg = os.path.dirname(os.path.abspath(_hip.__file__))
    seen = 0
    for folder, _, files in os.walk(pkg):
        for name in files:
            path = os.path.join(folder, name)
            if not name.endswith(".py") or path == os.path.abspath(_hip.__file__):
                continue
            seen += 1
            text = open(path).read()
            for pattern in (r"_hip\.check\(", r"[(,]\s*_hip\.stream_ptr\(\)\s*[,)]", r"=\s*_hip\.stream_ptr\(\)"):
                assert not re.search(pattern, text), f"{os.path.relpath(path, pkg)}: {pattern}"
    assert seen > 30
