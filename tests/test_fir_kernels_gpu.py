"""The kernels of diffsound_amd/csrc/fir.hip behind ds_fir_fwd / ds_fir_bwd, element by element against the plain fp64 sums of
tests/_fir_ref.py at the bounds derived there (tests/test_fir_ref_cpu.py anchors both without a GPU).

Every output and the workspace (sized exactly to ds_fir_workspace_bytes) live inside NaN-filled guard zones; each case is run
twice and every output must come out with the same bits, and a gradient computed alone must have the bits it has beside the
other.  Each case prints its largest error / bound ratio per output (``pytest -s``); every element must be <= 1 and none is
left out."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fir_ref as F  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, outside_untouched as _outside_untouched, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [F.case_id(c) for c in F.CASES]


def _call(case, inputs, want=("y", "gx", "gh")):
    """One forward and one backward call on fresh guarded buffers; ``want``: the outputs asked for (NULL for the others)."""
    _hip, L = _lib()
    B, H, N, Lt = case
    x, h, gy = inputs
    p = _hip.ptr
    d_x, d_h, d_gy = map(_up, (x, h, gy))
    out = {}
    if "y" in want:
        out["y"] = Guarded((B, N))
        _hip.check(L.ds_fir_fwd(p(d_x), p(d_h), B, H, N, Lt, out["y"].ptr, _hip.stream_ptr()), "ds_fir_fwd")
    nbytes = L.ds_fir_workspace_bytes(B, H, N, Lt)
    assert nbytes == 8 * B * -(-N // F.GH_CHUNK) * min(Lt, N)
    if "gx" in want:
        out["gx"] = Guarded((B, N))
    if "gh" in want:
        out["gh"], out["work"] = Guarded((H, Lt), torch.float64), Guarded((nbytes // 8,), torch.float64)
    if "gx" in want or "gh" in want:
        ptr = lambda k: out[k].ptr if k in out else None
        _hip.check(L.ds_fir_bwd(p(d_gy), p(d_x), p(d_h), B, H, N, Lt, ptr("work"), nbytes if "gh" in want else 0, ptr("gx"),
                                ptr("gh"), _hip.stream_ptr()), "ds_fir_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(case):
    inputs, f, b = F.reference(case)
    return inputs, f, b, _call(case, inputs), _call(case, inputs)


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_forward(case):
    _, f, _, out, again = _run(case)
    out["y"].check("y")
    assert _same_bits(out["y"], again["y"])
    assert _ratio("fir.y", case, out["y"].numpy(), f["y"], f["bound"]) <= 1.0


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_backward(case):
    inputs, _, b, out, again = _run(case)
    for k in ("gx", "gh"):
        out[k].check(k)
    _outside_untouched(out["work"], "work")
    assert _same_bits(out["gx"], again["gx"]) and _same_bits(out["gh"], again["gh"])
    assert _ratio("fir.gx", case, out["gx"].numpy(), b["gx"], b["gx_bound"]) <= 1.0
    assert _ratio("fir.gh", case, out["gh"].numpy(), b["gh"], b["gh_bound"]) <= 1.0
    N = case[2]
    assert not out["gh"].numpy()[:, N:].any()                          # an empty sum: exactly 0
    # a gradient alone has the bits it has beside the other
    alone_x, alone_h = _call(case, inputs, ("gx",)), _call(case, inputs, ("gh",))
    alone_x["gx"].check("gx"), alone_h["gh"].check("gh")
    assert _same_bits(alone_x["gx"], out["gx"]) and _same_bits(alone_h["gh"], out["gh"])


@pytest.mark.parametrize("case", [(2, 1, 37, 100), (2, 2, 2 * F.TILE + 1, 2 * F.TAPS + 1), (4, 2, 4097, 4096)], ids=F.case_id)
def test_unit_tap_shifts_bit_for_bit(case):
    B, H, N, L = case
    x, _, gy = F.inputs(case)
    for k in (0, 1, L - 1):
        h = np.zeros((H, L))
        h[:, k] = 1.0
        out = _call(case, (x, h, gy), ("y", "gx"))
        out["y"].check("y"), out["gx"].check("gx")
        assert np.array_equal(out["y"].numpy().view(np.uint32), F.shifted(x, k).view(np.uint32)), k
        assert np.array_equal(out["gx"].numpy().view(np.uint32), F.advanced(gy, k).view(np.uint32)), k


def test_long_addressing():
    """B = H = 2, N = 70001, L = 65536 with 32 non-zero taps (lags 0 and L - 1 among them): y and gx at every element, gh at
    the 32 non-zero lags and at 32 zero lags."""
    x, h, gy, lags, zero_lags, f, b = F.long_case()
    out = _call(F.LONG, (x, h, gy))
    for k in ("y", "gx", "gh"):
        out[k].check(k)
    _outside_untouched(out["work"], "work")
    assert _ratio("fir.long.y", F.LONG, out["y"].numpy(), f["y"], f["bound"]) <= 1.0
    assert _ratio("fir.long.gx", F.LONG, out["gx"].numpy(), b["gx"], b["gx_bound"]) <= 1.0
    at = np.concatenate([lags, zero_lags])
    assert _ratio("fir.long.gh", F.LONG, out["gh"].numpy()[:, at], b["gh"], b["gh_bound"]) <= 1.0


def test_a_nan_stays_in_its_row():
    case = (6, 3, 70, 9)
    (x, h, gy), f, _ = F.reference(case)
    x = x.copy()
    x[1, 5] = np.nan
    out = _call(case, (x, h, gy), ("y",))
    _outside_untouched(out["y"], "y")
    y = out["y"].numpy()
    rest = [r for r in range(6) if r != 1]
    assert np.isnan(y[1, 5:5 + 9]).all() and np.isfinite(y[1, :5]).all() and np.isfinite(y[rest]).all()
    assert _ratio("fir.nan.y", case, y[rest], f["y"][rest], f["bound"][rest]) <= 1.0


def test_zero_gradient_gives_exact_zeros():
    case = (2, 2, F.GH_CHUNK + 1, 300)
    x, h, _ = F.inputs(case)
    out = _call(case, (x, h, np.zeros_like(x)), ("gx", "gh"))
    out["gx"].check("gx"), out["gh"].check("gh")
    assert not out["gx"].numpy().any() and not out["gh"].numpy().any()


def test_workspace_bytes():
    _, L = _lib()
    for a in [(0, 1, 1, 1), (65536, 1, 1, 1), (1, 0, 1, 1), (2, 3, 1, 1), (3, 2, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 65537)]:
        assert L.ds_fir_workspace_bytes(*a) == 0
    for B, H, N, Lt in [(1, 1, 1, 1), (6, 3, 5000, 300), (16, 2, 32000, 65536)]:
        assert L.ds_fir_workspace_bytes(B, H, N, Lt) == 8 * B * -(-N // F.GH_CHUNK) * min(Lt, N)
