"""The references of tests/_fir_ref.py are anchored without a GPU: against numpy.longdouble sums on every case, against torch's
fp64 autograd of the same sums on the two smallest, and the exact statements - a unit tap shifts bit for bit, gh is exactly 0
from lag N on - hold for the reference itself."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fir_ref as F  # noqa: E402

IDS = [F.case_id(c) for c in F.CASES]
LD = np.longdouble
U_LD = float(np.finfo(LD).eps) / 2


def _longdouble(case):
    """y, gx (B, N), gh (H, L) as plain longdouble sums, every product formed in longdouble."""
    B, H, N, L = case
    x, h, gy = (a.astype(LD) for a in F.inputs(case))
    rows = np.arange(B) % H
    y, gx, ghb = np.zeros((B, N), LD), np.zeros((B, N), LD), np.zeros((B, L), LD)
    for j in range(min(L, N)):
        y[:, j:] += h[rows, j:j + 1] * x[:, :N - j]
        gx[:, :N - j] += h[rows, j:j + 1] * gy[:, j:]
        ghb[:, j] = (gy[:, j:] * x[:, :N - j]).sum(1)
    return y, gx, ghb.reshape(B // H, H, L).sum(0)


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_reference_against_longdouble(case):
    """|fp64 reference - longdouble sum| <= 2 U64 P (what the bound's derivation grants the reference: its products and its
    last addition) + the longdouble sum's own 2 n u_ld P."""
    B, H, N, L = case
    _, f, b = F.reference(case)
    y, gx, gh = _longdouble(case)
    for name, ref, ld, P, n in (("y", f["y"], y, f["P"], f["n"]), ("gx", b["gx"], gx, b["gx_P"], f["n"][::-1])):
        err = np.abs((ref.astype(LD) - ld).astype(np.float64))
        tol = (2 * F.U64 + 2 * n * U_LD) * P
        assert (err <= tol).all(), (name, float((err / np.where(tol > 0, tol, 1)).max()))
    nj = np.maximum(N - np.arange(L), 0.0)
    err = np.abs((b["gh"].astype(LD) - gh).astype(np.float64))
    assert (err <= (2 * F.U64 + B // H * F.U64 + 2 * (nj + B // H) * U_LD) * b["gh_P"]).all()


def test_cases_cover_the_kernel_paths():
    Ns, Ls = {c[2] for c in F.CASES}, {c[3] for c in F.CASES}
    assert {1, F.TILE - 1, F.TILE, F.TILE + 1, 2 * F.TILE + 1, F.GH_CHUNK - 1, F.GH_CHUNK, F.GH_CHUNK + 1} <= Ns
    assert {1, F.TAPS - 1, F.TAPS, F.TAPS + 1, 2 * F.TAPS + 1} <= Ls
    assert any(c[3] == c[2] for c in F.CASES) and (2, 1, 37, 100) in F.CASES and (4, 2, 4097, 4096) in F.CASES
    assert any(c[1] == 1 and c[0] > 1 for c in F.CASES) and any(c[1] == c[0] > 1 for c in F.CASES) and (6, 3, 70, 9) in F.CASES
    for case in F.CASES:
        x, h, gy = F.inputs(case)
        if x.size >= 64:   # several decades, both signs
            a = np.abs(x[x != 0])
            assert a.max() / a.min() > 1e3 and (x > 0).any() and (x < 0).any() and (gy > 0).any() and (gy < 0).any()
        if h.size >= 8:
            assert (h > 0).any() and (h < 0).any() and np.abs(h).max() / np.abs(h).min() > 1e2


@pytest.mark.parametrize("case", F.SMALLEST + [(6, 3, 70, 9), (2, 1, 37, 100)], ids=F.case_id)
def test_gradients_against_autograd(case):
    """The same sums written with torch on the CPU in fp64 - an explicit loop over the lag - and differentiated by autograd."""
    B, H, N, L = case
    (x, h, gy), f, b = F.reference(case)
    tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    th = torch.from_numpy(h).requires_grad_(True)
    y = torch.zeros(B, N, dtype=torch.float64)
    for j in range(min(L, N)):
        y = y + torch.nn.functional.pad(th[torch.arange(B) % H, j:j + 1] * tx[:, :N - j], (j, 0))
    y.backward(torch.from_numpy(gy.astype(np.float64)))
    for got, ref, P in ((y.detach().numpy(), f["y"], f["P"]), (tx.grad.numpy(), b["gx"], b["gx_P"]),
                        (th.grad.numpy(), b["gh"], b["gh_P"])):
        assert (np.abs(got - ref) <= 2 * (min(L, N) + B) * F.U64 * P + 1e-300).all()


@pytest.mark.parametrize("k", [0, 1, 5, 36, 37, 99])
def test_unit_tap_shifts_bit_for_bit(k):
    case = (2, 1, 37, 100)
    x, _, gy = F.inputs(case)
    h = np.zeros((1, 100))
    h[0, k] = 1.0
    f, b = F.forward(x, h), F.input_gradient(gy, h)
    y32, gx32 = f["y"].astype(np.float32), b["gx"].astype(np.float32)
    assert np.array_equal(y32.view(np.uint32), F.shifted(x, k).view(np.uint32))
    assert np.array_equal(gx32.view(np.uint32), F.advanced(gy, k).view(np.uint32))
    assert not y32[:, :k].any()


def test_tap_gradient_is_exactly_zero_from_lag_n_on():
    for case in [(2, 1, 37, 100), (2, 1, 1, 5)]:
        N = case[2]
        _, _, b = F.reference(case)
        assert not b["gh"][:, N:].any() and not b["gh_bound"][:, N:].any() and b["gh"][:, :N].all()


def test_long_case_has_its_ends():
    x, h, gy, lags, zero_lags, f, b = F.long_case()
    assert len(lags) == 32 and len(zero_lags) == 32 and lags[0] == 0 and lags[-1] == F.LONG[3] - 1
    assert (h[:, lags] != 0).all() and np.count_nonzero(h) == 64 and not h[:, zero_lags].any()
    assert f["y"].shape == x.shape and b["gh"].shape == (2, 64)
    assert b["gh"].all()   # the taps' gradient does not ask whether the tap is zero
