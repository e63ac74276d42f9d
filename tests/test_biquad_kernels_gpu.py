"""The kernels of diffsound_amd/csrc/biquad.hip behind ds_biquad_fwd / ds_biquad_bwd, element by element against the plain
fp64 recurrences of tests/_biquad_ref.py at the bounds derived there (tests/test_biquad_ref_cpu.py anchors both without a
GPU).

Every output and the workspace (sized exactly to ds_biquad_workspace_bytes) live inside NaN-filled guard zones; each case is
run twice and every output must come out with the same bits.  Each case prints its largest error / bound ratio per output
(``pytest -s``); every element must be <= 1 and none is left out."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _biquad_ref as BQ  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [BQ.case_id(c) for c in BQ.CASES]


def _call(case, inputs):
    """One forward and one backward call on fresh guarded buffers."""
    _hip, L = _lib()
    B, N, S, per_clip = case[:4]
    x, sos, gy = inputs
    p = _hip.ptr
    d_x, d_sos, d_gy = map(_up, (x, sos, gy))
    nbytes = L.ds_biquad_workspace_bytes(B, N, S)
    assert nbytes == 8 * B * S * N
    out = dict(work=Guarded((nbytes // 8,), torch.float64), y=Guarded((B, N)), gx=Guarded((B, N)),
               gsos=Guarded((B, S, 5), torch.float64))
    _hip.check(L.ds_biquad_fwd(p(d_x), p(d_sos), per_clip, B, N, S, out["y"].ptr, _hip.stream_ptr()), "ds_biquad_fwd")
    _hip.check(L.ds_biquad_bwd(p(d_gy), p(d_x), p(d_sos), per_clip, B, N, S, out["work"].ptr, nbytes, out["gx"].ptr,
                               out["gsos"].ptr, _hip.stream_ptr()), "ds_biquad_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=4)
def _run(case):
    inputs = BQ.inputs(case)
    f = BQ.forward(inputs[0], inputs[1])
    return inputs, f, _call(case, inputs), _call(case, inputs)


@pytest.mark.parametrize("case", BQ.CASES, ids=IDS)
def test_forward(case):
    _, f, out, again = _run(case)
    out["y"].check("y")
    assert _same_bits(out["y"], again["y"])
    assert _ratio("biquad.y", case, out["y"].numpy(), f["y"], f["y_bound"]) <= 1.0


@pytest.mark.parametrize("case", BQ.CASES, ids=IDS)
def test_backward(case):
    (x, sos, gy), f, out, again = _run(case)
    for k in ("gx", "gsos", "work"):
        out[k].check(k)
    assert _same_bits(out["gx"], again["gx"]) and _same_bits(out["gsos"], again["gsos"])
    b = BQ.backward(gy, x, sos, f)
    assert _ratio("biquad.gx", case, out["gx"].numpy(), b["gx"], b["gx_bound"]) <= 1.0
    assert _ratio("biquad.gsos", case, out["gsos"].numpy(), b["gsos"], b["gsos_bound"]) <= 1.0
    # the recomputed w of every section, as the workspace holds it: (B, S, N)
    B, N, S = case[:3]
    w = out["work"].numpy().reshape(B, S, N)
    for s in range(S):
        assert _ratio("biquad.w", case, w[:, s], f["w"][s], f["ew"][s] + 1e-300) <= 1.0


def test_sixteen_sections():
    """S = DS_BIQUAD_MAX_SECTIONS once, at N = 1025 (two tiles), per clip: every LDS slot of the powers, carries and sums."""
    case = (3, 1025, 16, 1, "sixteen")
    x, _, gy = BQ.inputs((3, 1025, 16, 1, "real"))
    sos = BQ.sixteen(3)
    f = BQ.forward(x, sos)
    out, again = _call(case, (x, sos, gy)), _call(case, (x, sos, gy))
    for k in ("y", "gx", "gsos", "work"):
        out[k].check(k)
    assert all(_same_bits(out[k], again[k]) for k in ("y", "gx", "gsos"))
    b = BQ.backward(gy, x, sos, f)
    assert _ratio("biquad.y", case, out["y"].numpy(), f["y"], f["y_bound"]) <= 1.0
    assert _ratio("biquad.gx", case, out["gx"].numpy(), b["gx"], b["gx_bound"]) <= 1.0
    assert _ratio("biquad.gsos", case, out["gsos"].numpy(), b["gsos"], b["gsos_bound"]) <= 1.0


def test_zero_gradient_gives_exact_zeros():
    case = (3, 2051, 3, 1, "complex")
    x, sos, _ = BQ.inputs(case)
    out = _call(case, (x, sos, np.zeros_like(x)))
    out["gx"].check("gx"), out["gsos"].check("gsos")
    assert not out["gx"].numpy().any() and not out["gsos"].numpy().any()


def test_unstable_coefficients_are_only_numbers():
    """What the header promises for EVERY sos: an unstable section (a2 = 1.01, N = 2051) returns without error, the outputs
    are non-finite or huge, and nothing outside them is written."""
    case = (2, 2051, 2, 0, "unstable")
    B, N, S = case[:3]
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, N)).astype(np.float32)
    gy = rng.standard_normal((B, N)).astype(np.float32)
    sos = np.stack([BQ.SETS["real"], np.array([1.0, 0.0, 0.0, 0.0, 1.01])])
    out = _call(case, (x, sos, gy))
    y = out["y"].numpy()
    assert (~np.isfinite(y)).any() or np.abs(y).max() > 1e3
    for k in ("y", "gx", "gsos", "work"):
        whole = out[k].buf.cpu().numpy()
        assert np.isnan(whole[:64]).all() and np.isnan(whole[-64:]).all(), f"{k}: written outside"


def test_workspace_bytes():
    _, L = _lib()
    for a in [(0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 17)]:
        assert L.ds_biquad_workspace_bytes(*a) == 0
    for B, N, S in [(1, 1, 1), (3, 1025, 3), (64, 160000, 4)]:
        assert L.ds_biquad_workspace_bytes(B, N, S) == 8 * B * S * N
