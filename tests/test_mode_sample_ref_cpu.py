"""tests/_mode_sample_ref.py against itself, without a GPU: the analytic gradients against central differences of the
forward, the interpolant at the element's own nodes, and P1 / P2 reproduction of linear / quadratic fields.

Tolerances.  Every quantity compared is a sum of products evaluated in fp64, so each side is within
gamma_k * sum |terms| of the exact value, k the number of terms plus the roundings of one term (any summation order
has a chain no longer than the number of terms).  The forward is a polynomial of degree <= 2 in L and of degree 1 in
dir, for which a central difference has no truncation error; what is left is the rounding of the two forward values,
divided by 2 h, and the rounding of (x + h) - (x - h) against 2 h, a relative 2 u |x| / h <= 2 u / h of the derivative.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mode_sample_ref as R  # noqa: E402

from diffsound_amd import fem_tables  # noqa: E402

M, P, H = 5, 24, 2.0 ** -10


def _case(order):
    verts, tets = R.mesh(order)
    elem, L, dirs = R.sample_points(tets.shape[0], P, seed=10 + order)
    U = R.random_modes(verts.shape[0], M, M + 3, seed=20 + order)
    gout = np.random.default_rng(30 + order).standard_normal((P, M))
    return verts, tets, elem, L.astype(np.float64), dirs.astype(np.float64), U, gout


@pytest.mark.parametrize("order", [1, 2])
def test_gradients_agree_with_central_differences(order):
    verts, tets, elem, L, dirs, U, gout = _case(order)
    N = tets.shape[1]
    gL, gdir, agL, agdir = R.backward(tets, U, M, elem, L, dirs, gout, with_abs=True)
    k = 3 * N * M + 8  # terms of one point's loss sum_i gout_i out_i, and the roundings of one term
    loss = lambda L_, d_: (gout * R.forward(tets, U, M, elem, L_, d_)[0]).sum(1)
    aloss = (np.abs(gout) * R.forward(tets, U, M, elem, L, dirs, with_abs=True)[2]).sum(1)
    # |terms| at the shifted points: the shape functions move by at most 4 h (1 + h) each, covered by the factor 1 + 8 h
    fd_round = R.gamma(k) * aloss * (1 + 8 * H) / H
    for j in range(4):
        e = np.zeros(4)
        e[j] = H
        fd = (loss(L + e, dirs) - loss(L - e, dirs)) / (2 * H)
        tol = fd_round + (R.gamma(k) + 2 * R.U64 / H) * agL[:, j]
        assert np.all(np.abs(fd - gL[:, j]) <= tol), (order, j, np.abs(fd - gL[:, j]).max(), tol.min())
    for c in range(3):
        e = np.zeros(3)
        e[c] = H
        fd = (loss(L, dirs + e) - loss(L, dirs - e)) / (2 * H)
        # (the shifted direction adds h |vec_c| to the |terms| of the forward)
        tol = fd_round + R.gamma(k) * agdir[:, c] + (R.gamma(k) + 2 * R.U64 * (np.abs(dirs[:, c]) + H) / H) * agdir[:, c]
        assert np.all(np.abs(fd - gdir[:, c]) <= tol), (order, c, np.abs(fd - gdir[:, c]).max(), tol.min())
    assert np.abs(gL).max() > 0.1 and np.abs(gdir).max() > 0.1  # the comparison is not between zeros


@pytest.mark.parametrize("order", [1, 2])
def test_a_node_returns_its_own_row(order):
    """At a corner node, and at a mid-edge node of the P2 element, exactly one shape function is 1 and the others are
    exactly 0, so the interpolant is the node's row of U to the last bit."""
    verts, tets = R.mesh(order)
    N = tets.shape[1]
    U = R.random_modes(verts.shape[0], M, M + 3, seed=5)
    nodal_L = np.zeros((N, 4))
    if order == 1:
        nodal_L[:] = np.eye(4)
    else:
        for slot, k in fem_tables._CORNER.items():
            nodal_L[slot, k] = 1.0
        for slot, (p, q) in fem_tables._MID.items():
            nodal_L[slot, p] = nodal_L[slot, q] = 0.5
    for e in (0, tets.shape[0] - 1):
        elem = np.full(N, e, dtype=np.int32)
        for c in range(3):
            d = np.zeros((N, 3))
            d[:, c] = 1.0
            out, vec = R.forward(tets, U, M, elem, nodal_L, d)
            rows = U[3 * tets[e].astype(np.int64) + c, :M]
            assert np.array_equal(out, rows) and np.array_equal(vec[:, :, c], rows)


@pytest.mark.parametrize("order", [1, 2])
def test_interpolation_reproduces_polynomials_of_its_degree(order):
    """A field of degree ``order`` sampled at the nodes comes back exactly at any point of any element (the element map
    is affine: x(L) = sum_k L_k X_k)."""
    verts, tets = R.mesh(order)
    rng = np.random.default_rng(7)
    nv, N = verts.shape[0], tets.shape[1]
    x = verts / np.abs(verts).max()  # O(1) coordinates
    A, b, Q = rng.standard_normal((3 * M, 3)), rng.standard_normal(3 * M), rng.standard_normal((3 * M, 3, 3))
    if order == 1:
        Q[:] = 0.0
    field = lambda y: np.einsum("fk,nk->nf", A, y) + b + np.einsum("fkl,nk,nl->nf", Q, y, y)  # (n, 3 M), column c * M + i
    U = field(x).reshape(nv, 3, M).reshape(3 * nv, M)
    elem, L, _ = R.sample_points(tets.shape[0], P, seed=8)
    L = L.astype(np.float64)
    L[:, 3] = 1.0 - L[:, :3].sum(1)  # a partition of unity to fp64 rounding
    y = np.einsum("pk,pkx->px", L, R.element_frame(x, tets, elem))
    want = field(y).reshape(P, 3, M).transpose(0, 2, 1)
    _, vec, _, avec = R.forward(tets, U, M, elem, L, np.zeros((P, 3)), with_abs=True)
    # both sides are sums of at most 13 products of O(1) numbers per entry, the nodal values through the interpolant's
    # N weights; the partition of unity itself holds to 4 u
    tol = R.gamma(N + 16) * (avec + np.abs(A).sum() + np.abs(b).max() + np.abs(Q).sum())
    assert np.all(np.abs(vec - want) <= tol), (np.abs(vec - want).max(), tol.min())
    assert np.abs(want).max() > 1.0


def test_position_recovery_on_the_restatement():
    """Where RECOVER_MARGIN of the GPU test comes from: the same loop on the fp64 restatement, with ARPACK's modes."""
    import torch

    from diffsound_amd import meshgen
    from oracle import fem, modal

    v, t = meshgen.kuhn_box(R.RECOVER_CELLS)
    vo, to = torch.from_numpy(v), torch.from_numpy(t).long()
    lam, mu = fem.lame(5e10, 0.25)
    K = fem.assemble_stiffness(fem.OracleDeform(vo, to, 1), lam, mu)
    M3, _ = fem.assemble_mass(vo, to, 1, 2700.0)
    _, U, _, _ = modal.eigsh_shift_invert(K, M3, R.RECOVER_MODES)
    elem, corner, normal = R.boundary_faces(v, t)
    cent = v.astype(np.float64)[np.take_along_axis(t[elem].astype(np.int64), corner, 1)].mean(1)
    f = int(np.argmin(((cent - np.array(R.RECOVER_SPOT)) ** 2).sum(1)))
    gains = R.numpy_gains(t, np.asarray(U, dtype=np.float64), R.RECOVER_MODES, int(elem[f]), corner[f], normal[f])
    first, last, b = R.recover(gains)
    print(f"recovery on the restatement: start {first:.3g}, end {last:.3g}, ratio {last / first:.3g}, bary3 {b}")
    assert first > 0.1
    # the figure the margin is derived from (ARPACK's start vector is random: the modes, and with them the late
    # trajectory, move in their last digits from run to run)
    assert last / first <= 10 * R.RECOVER_MEASURED <= R.RECOVER_MARGIN / 40
    assert np.abs(b - np.array(R.RECOVER_TARGET)).max() < 2e-3
