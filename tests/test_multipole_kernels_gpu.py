"""The kernels of diffsound_amd/csrc/multipole.hip behind ds_multipole_fwd / ds_multipole_bwd, element by element against the
truth of tests/_multipole_ref.py (mpmath's h_l, longdouble harmonics and sums) at its counted bounds;
tests/test_multipole_ref_cpu.py vouches for the truth and the bounds without a GPU.

Every output and the workspace (sized exactly to ds_multipole_workspace_bytes) live inside NaN-filled guard zones; each case is
run twice and every output and the workspace must come out with the same bits; a NULL gradient output leaves the other's bits
unchanged.  Each case prints its largest error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _multipole_ref as R  # noqa: E402
from _guarded import Guarded, _lib, _up  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
IDS = ["-".join(map(str, c)) for c in R.CASES]


def _pairs(z):
    """complex array -> interleaved (re, im) fp64."""
    return np.ascontiguousarray(np.stack([z.real, z.imag], -1))


def _call(case, P, m, L, gpts=True, gcoef=True):
    """One forward and one backward call on fresh guarded buffers; a gradient that is switched off gets NULL."""
    _hip, lib = _lib()
    N = R.nterms(L)
    ops = [_up(x) for x in (case["pts"], R.CENTER, case["k"], _pairs(case["coef"]))]
    g = _up(_pairs(case["gout"]))
    ptr = _hip.ptr
    nbytes = lib.ds_multipole_workspace_bytes(P, m, L)
    assert nbytes == 16 * min(P, R.GCOEF_BLOCKS) * N * m
    out = dict(out=Guarded((P, m, 2), F64), gpts=Guarded((P, 3), F64), gcoef=Guarded((N, m, 2), F64), work=Guarded((nbytes // 8,), F64))
    _hip.check(lib.ds_multipole_fwd(*map(ptr, ops), P, m, L, out["out"].ptr, _hip.stream_ptr()), "ds_multipole_fwd")
    _hip.check(lib.ds_multipole_bwd(ptr(g), *map(ptr, ops), P, m, L, out["work"].ptr if gcoef else None, nbytes if gcoef else 0,
                                    out["gpts"].ptr if gpts else None, out["gcoef"].ptr if gcoef else None, _hip.stream_ptr()),
               "ds_multipole_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(i):
    P, m, L = R.CASES[i]
    case = R.case_truth(P, m, L)
    return case, _call(case, P, m, L), _call(case, P, m, L)


def _cplx(a):
    return a[..., 0] + 1j * a[..., 1]


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_outputs_within_the_bound(i):
    case, first, _ = _run(i)
    for k, v in first.items():
        v.check(k)
    q = R.ratios(case, _cplx(first["out"].numpy()), first["gpts"].numpy(), _cplx(first["gcoef"].numpy()))
    print("RATIO multipole", IDS[i], " ".join(f"{k} {v:.4g}" for k, v in q.items()))
    assert max(q.values()) < 1, q
    if R.CASES[i][1] >= 5:  # a column of zero coefficients: exact zeros
        assert (first["out"].numpy()[:, 3] == 0).all()


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_two_calls_give_the_same_bits(i):
    _, first, second = _run(i)
    for k in ("out", "gpts", "gcoef", "work"):
        assert torch.equal(first[k].buf[64:-64].view(torch.int64), second[k].buf[64:-64].view(torch.int64)), k


@pytest.mark.parametrize("i", [0, 22, 38, 59], ids=[IDS[j] for j in (0, 22, 38, 59)])
def test_a_null_output_leaves_the_other_unchanged(i):
    P, m, L = R.CASES[i]
    case, first, _ = _run(i)
    only_p = _call(case, P, m, L, gcoef=False)
    only_c = _call(case, P, m, L, gpts=False)
    assert torch.equal(only_p["gpts"].buf[64:-64].view(torch.int64), first["gpts"].buf[64:-64].view(torch.int64))
    assert torch.equal(only_c["gcoef"].buf[64:-64].view(torch.int64), first["gcoef"].buf[64:-64].view(torch.int64))
    assert only_p["gcoef"].untouched() and only_p["work"].untouched() and only_c["gpts"].untouched()


def test_kernels_agree_with_the_restatement_closely():
    """Not a bound, a sanity figure: the device and the fp64 numpy restatement differ by the device's sqrt / sincos / division
    only; both are inside the bound, so they are within twice the bound of each other."""
    i = R.CASES.index((63, 5, 7))
    case, first, _ = _run(i)
    out, gp, gc, _ = R.restate(case["pts"], R.CENTER, case["k"], case["coef"], 7, case["gout"])
    assert (np.abs(_cplx(first["out"].numpy()) - out) <= 2 * case["b_out"]).all()
    assert (np.abs(first["gpts"].numpy() - gp) <= 2 * case["b_gpts"]).all()
    assert (np.abs(_cplx(first["gcoef"].numpy()) - gc) <= 2 * case["b_gcoef"]).all()
