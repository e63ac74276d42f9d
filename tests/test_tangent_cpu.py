"""Anisotropic tangents without a device: ``elastic_tangent``, ``TrainableOrthotropic``, and an fp64 restatement of the
reference's general-C assembly (per Gauss point A^T C A, reference src/diffelastic/diff_model.py:204-219) built from
``oracle.fem.OracleDeform``'s tables, against the fixture made from the reference (tests/golden/g10_aniso_cube2.npz).

Also the shared helpers of tests/test_tangent_gpu.py.  ``python tests/test_tangent_cpu.py`` prints the error of the
reference's own fp32 arithmetic against fp64 - the figures the GPU tests' measured tolerances are 4x of (DESIGN.md
section 14)."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import test_deform_cpu as dref  # noqa: E402
from oracle import fem  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TANGENTS = ("ortho", "tri")
READOUT_LOG_SCALE = (0.30, -0.20, 0.10, 0.15, -0.25, 0.05, 0.20, -0.10, -0.30)  # a fixed orthotropic state off isotropy


# ---------------------------------------------------------------------------------------------- shared helpers
def g10():
    return np.load(os.path.join(GOLDEN, "g10_aniso_cube2.npz"))


def voigt_expand(voigt):
    idx = np.asarray((0, 5, 4, 5, 1, 3, 4, 3, 2))
    return np.ascontiguousarray(np.asarray(voigt)[idx][:, idx])


def assemble_general(v, t, order, C, tables="fp32"):
    """K = sum over Gauss points of w A^T C A in fp64, A = the 9 x 3N matrix with the shape gradients at rows 3i..3i+2,
    columns i::3 (reference :204-219).  ``tables``: "fp32" - the reference's own fp32 shape gradients and weights, as it
    assembles; "fp64" - the same tables formed in fp64 from the fp32 coordinates.  scipy CSR."""
    r = dref.Restatement(v, t, order, torch.float32 if tables == "fp32" else torch.float64)
    d = r.d
    T, G, N = d.T, d.G, d.N
    SFDT = r.B.double().transpose(1, 2).reshape(T, G, 3, N)
    w = r.w.double().reshape(T, G)
    A = torch.zeros(T, G, 9, 3 * N, dtype=torch.float64)
    A[:, :, 0:3, 0::3] = SFDT
    A[:, :, 3:6, 1::3] = SFDT
    A[:, :, 6:9, 2::3] = SFDT
    Ke = torch.einsum("tgri,rs,tgsj,tg->tij", A, torch.as_tensor(np.asarray(C, np.float64)), A, w)
    dof = d.dof_index().numpy()
    m, n = dof.shape[1], 3 * d.verts.shape[0]
    rows, cols = np.repeat(dof, m, axis=1).reshape(-1), np.tile(dof, (1, m)).reshape(-1)
    return sp.coo_matrix((Ke.reshape(-1).numpy(), (rows, cols)), shape=(n, n)).tocsr()


def eigsh_modes(K, M3, mode_num):
    """The reference's eigen_decomposition_arpack (:356-369): eigsh(k = mode_num + 6, sigma = 20000), six rigid pairs dropped."""
    import scipy.sparse.linalg as spla

    S, U = spla.eigsh(sp.csr_matrix(K), M=sp.csr_matrix(M3), k=mode_num + 6, sigma=20000)
    o = np.argsort(S)
    return S[o][6:], U[:, o][:, 6:]


def orthotropic_model(mat, log_scale=READOUT_LOG_SCALE):
    from diffsound_amd.diffelastic.diff_model import Material, TrainableOrthotropic

    m = TrainableOrthotropic(Material(mat))
    with torch.no_grad():
        m.log_scale.copy_(torch.tensor(log_scale, dtype=torch.float64))
    return m


def moment_tensors(r, U):
    """Q[m] = sum_g w_g vec(F_g) vec(F_g)^T of every column of U (n x k) through the restatement ``r``: u^T K(C) u = <C, Q>."""
    F = r.gradient(torch.as_tensor(U).T.reshape(U.shape[1], -1, 3).to(r.dtype)).reshape(U.shape[1], -1, 9)
    return torch.einsum("mgp,mgq,g->mpq", F, F, r.w)


# ---------------------------------------------------------------------------------------------- elastic_tangent
def _shipped():
    lam, mu = fem.lame(5e10, 0.25)
    return fem.piola_jacobian(lam, mu), lam, mu


def test_elastic_tangent_accepts_valid_tangents():
    from diffsound_amd.diffelastic.diff_model import elastic_tangent

    iso, lam, mu = _shipped()
    g = g10()
    for C in (iso, dref.orthotropic_tangent(lam, mu), g["ortho_C"], g["tri_C"], torch.from_numpy(g["tri_C"]).float()):
        out = elastic_tangent(C)
        assert out.dtype == np.float64 and out.shape == (9, 9)
        C64 = np.asarray(C, dtype=np.float64)
        assert np.abs(out - C64).max() <= 1e-15 * np.abs(C64).max()
        o4 = out.reshape(3, 3, 3, 3)  # symmetrised exactly
        assert np.array_equal(o4, o4.transpose(2, 3, 0, 1)) and np.array_equal(o4, o4.transpose(0, 1, 3, 2))
        assert np.array_equal(o4, o4.transpose(1, 0, 2, 3))
    noisy = iso.copy()
    noisy[1, 3] *= 1 + 1e-6  # fp32-parameter noise passes (a test of form) and comes back symmetric
    out = elastic_tangent(noisy)
    assert out[1, 3] == out[3, 1] == out[1, 1]


def test_elastic_tangent_names_the_failed_condition():
    from diffsound_amd.diffelastic.diff_model import elastic_tangent

    iso, lam, mu = _shipped()
    major = iso.copy()
    major[0, 4] *= 1.01  # C_0011 != C_1100
    with pytest.raises(ValueError, match="major symmetry"):
        elastic_tangent(major)
    minor = iso.copy()
    minor[1, 3] = 0.0  # P_01 no longer sees F_10 (tests/test_deform_cpu.py); kept major-symmetric
    minor[3, 1] = 0.0
    with pytest.raises(ValueError, match="minor symmetry"):
        elastic_tangent(minor)
    voigt = np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -0.5]) * 5e10
    with pytest.raises(ValueError, match="positive definite"):
        elastic_tangent(voigt_expand(voigt))
    with pytest.raises(ValueError, match="zero"):
        elastic_tangent(np.zeros((9, 9)))
    with pytest.raises(ValueError, match="shape"):
        elastic_tangent(np.eye(6))
    bad = iso.copy()
    bad[2, 2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        elastic_tangent(bad)


# ---------------------------------------------------------------------------------------------- TrainableOrthotropic
def test_orthotropic_model_starts_isotropic_and_differentiates():
    from diffsound_amd.diffelastic.diff_model import Material, MatSet, TrainableOrthotropic, elastic_tangent

    m = TrainableOrthotropic(Material(MatSet.Wood))
    assert m.mat.density == MatSet.Wood[0] and tuple(m.log_scale.shape) == (9,) and m.log_scale.dtype == torch.float64
    assert [n for n, _ in m.named_parameters()] == ["log_scale"]
    iso = fem.piola_jacobian(*fem.lame(MatSet.Wood[1], MatSet.Wood[2]))
    C = m.tangent()
    assert C.dtype == torch.float64 and tuple(C.shape) == (9, 9) and C.requires_grad
    assert np.abs(C.detach().numpy() - iso).max() <= 1e-12 * np.abs(iso).max()
    assert tuple(m.jacobian_F().shape) == (1, 3, 3, 1, 3, 3) and not m.jacobian_F().requires_grad
    F = torch.randn((2, 5, 3, 3), generator=torch.Generator().manual_seed(0))
    want = dref.linear_stress(F.double(), *fem.lame(MatSet.Wood[1], MatSet.Wood[2]))
    assert m(F).dtype == torch.float32 and dref.relmax(m(F).detach(), want) < 1e-6

    class Tangent(torch.nn.Module):
        def __init__(self, model):
            super().__init__()
            self.model = model

        def forward(self):
            return self.model.tangent() / 1e10

    moved = orthotropic_model(MatSet.Wood)
    f = lambda p: torch.func.functional_call(Tangent(moved), {"model.log_scale": p}, ())
    assert torch.autograd.gradcheck(f, (moved.log_scale.detach().clone().requires_grad_(True),))
    elastic_tangent(moved.tangent())  # a valid elasticity tensor off isotropy too
    E1, E2 = (float(x) for x in moved.constants().detach()[:2])
    assert E1 / E2 == pytest.approx(np.exp(0.5), rel=1e-12)


def test_axes_rotate_the_tangent_as_a_fourth_order_tensor():
    from diffsound_amd.diffelastic.diff_model import Material, MatSet, TrainableOrthotropic

    a = 0.7
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    R = R @ np.array([[1.0, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
    base, turned = orthotropic_model(MatSet.Wood), TrainableOrthotropic(Material(MatSet.Wood), axes=R)
    with torch.no_grad():
        turned.log_scale.copy_(base.log_scale)
    C4 = base.tangent().detach().numpy().reshape(3, 3, 3, 3)
    want = np.einsum("ia,jb,kc,ld,abcd->ijkl", R, R, R, R, C4).reshape(9, 9)
    got = turned.tangent().detach().numpy()
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max() and np.abs(got - C4.reshape(9, 9)).max() > 1e-2 * np.abs(want).max()
    # the rotated material answers a rotated strain with the rotated stress: P'(R F R^T) = R P(F) R^T
    F = torch.randn((4, 3, 3), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    Rt = torch.from_numpy(R)
    assert dref.relmax(turned(Rt @ F @ Rt.T).detach(), (Rt @ base(F) @ Rt.T).detach()) < 1e-13


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", TANGENTS)
def test_restatement_matches_the_fixture(name, order):
    g = g10()
    v, t = dref.mesh_case("cube", order)
    C = g[f"{name}_C"]
    K = assemble_general(v, t, order, C).toarray()
    want = g[f"{name}_o{order}_K"]
    # 1e-6 as tests/test_oracle_golden.py grants the isotropic fixture: the fp32 inverse differs in the last ulp across torch builds
    assert dref.relmax(K, want) < 1e-6
    assert np.abs(K - K.T).max() <= 1e-12 * np.abs(K).max()
    M3, _ = fem.assemble_mass(v, t, order, float(g["mat"][0]))
    ev, _ = eigsh_modes(K, M3, int(g["mode_num"]))
    assert np.abs(ev / g[f"{name}_o{order}_eigenvalues"] - 1).max() < 1e-6
    assert np.abs(np.sqrt(ev) / 2 / np.pi / g[f"{name}_o{order}_freqs"].reshape(-1) - 1).max() < 1e-5  # (its fp32 bracket)


def test_isotropic_tangent_restates_the_isotropic_assembly():
    v, t = dref.mesh_case("cube", 2)
    iso, lam, mu = _shipped()
    K = assemble_general(v, t, 2, iso)
    want = fem.assemble_stiffness(fem.OracleDeform(v, t, 2), lam, mu)
    assert abs(K - want).max() <= 1e-13 * abs(want).max()


def test_moment_tensors_reproduce_the_quadratic_forms():
    g = g10()
    v, t = dref.mesh_case("cube", 1)
    r64 = dref.Restatement(v, t, 1, torch.float64)
    U = torch.randn((3 * v.shape[0], 3), generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    Q = moment_tensors(r64, U)
    for name in TANGENTS:
        C = g[f"{name}_C"]
        K = torch.from_numpy(assemble_general(v, t, 1, C, tables="fp64").toarray())
        want = ((K @ U) * U).sum(0)
        got = (torch.from_numpy(C) * Q).sum((-1, -2))
        assert float(((got - want).abs() / want.abs()).max()) < 1e-12


# ---------------------------------------------------------------------------------------------- the tolerance figures
def reference_fp32_table_errors(log=print):
    """K of the reference's arithmetic (fp32 shape gradients and weights, fp64 sums) against the same assembly on fp64
    tables, relative to max|K|: per tangent and order on the cube."""
    g = g10()
    worst = 0.0
    for name in TANGENTS:
        for order in (1, 2):
            v, t = dref.mesh_case("cube", order)
            e = dref.relmax(assemble_general(v, t, order, g[f"{name}_C"]).toarray(),
                            assemble_general(v, t, order, g[f"{name}_C"], tables="fp64").toarray())
            log(f"cube order {order} {name}: K on fp32 tables against fp64 tables {e:.3e}")
            worst = max(worst, e)
    return {"stiff_matrix": worst}


def reference_fp32_readout_errors(log=print):
    """get_undamped_freqs of the reference's formula (the fp32 bracket through its matrix-free chain, :371-388) for the
    orthotropic model at READOUT_LOG_SCALE on the cube, orders 1 and 2: the frequencies and d sum(f) / d log_scale
    against the fp64 closed form sqrt(lambda + <C, Q> - lambda m) / 2 pi."""
    g = g10()
    mat = tuple(float(x) for x in g["mat"])
    worst = {"freqs": 0.0, "scale_grad": 0.0}
    for order in (1, 2):
        v, t = dref.mesh_case("cube", order)
        model = orthotropic_model(mat)
        K = assemble_general(v, t, order, model.tangent().detach().numpy())
        M3, _ = fem.assemble_mass(v, t, order, mat[0])
        ev, U = eigsh_modes(K, M3, int(g["mode_num"]))
        r32, r64 = dref.Restatement(v, t, order, torch.float32), dref.Restatement(v, t, order, torch.float64)
        ev_t, U_t, M_t = torch.from_numpy(ev), torch.from_numpy(U), torch.from_numpy(M3.toarray())
        # fp32, as the reference evaluates it
        U32 = U_t.float()
        F = r32.gradient(U32.T.reshape(U32.shape[1], -1, 3))
        C32 = model.tangent().float()  # (a plain fp32 product with torch's own backward, as a model of the reference's would be)
        KU = r32.force((F.reshape(*F.shape[:-2], 9) @ C32.T).reshape(F.shape)).T
        pred = ev_t.float() + (U32.T @ KU).diagonal() - ev_t.float() * (U32.T @ (M_t.float() @ U32)).diagonal()
        f32 = torch.sqrt(pred) / 2 / np.pi
        model.zero_grad()
        f32.sum().backward()
        g32 = model.log_scale.grad.clone()
        # fp64 closed form
        model.zero_grad()
        Q = moment_tensors(r64, U_t)
        m = ((M_t @ U_t) * U_t).sum(0)
        f64 = torch.sqrt(ev_t + (model.tangent() * Q).sum((-1, -2)) - ev_t * m) / 2 / np.pi
        f64.sum().backward()
        e = {"freqs": dref.relmax(f32.detach(), f64.detach()), "scale_grad": dref.relmax(g32, model.log_scale.grad)}
        log(f"cube order {order} orthotropic read-out: {e}")
        worst = {k_: max(worst[k_], e[k_]) for k_ in worst}
    return worst


if __name__ == "__main__":
    out = reference_fp32_table_errors()
    out.update(reference_fp32_readout_errors())
    print(out)
