"""Anisotropic tangents on the device: ds_combine_tangent / ds_tangent_forms (csrc/tangent.hip), HipModalOps.set_tangent
and the tangent-model path of DiffSoundObj, against the fixture made from the reference (g10_aniso_cube2.npz) and the
fp64 restatement of tests/test_tangent_cpu.py.

Tolerances.  Derived ones are stated where they are used.  The measured ones are 4x the error of the REFERENCE's own
fp32 arithmetic against fp64 on the same cases, as in tests/test_deform_gpu.py; ``python tests/test_tangent_cpu.py``
prints the REF_* figures and DESIGN.md section 14 lists them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_deform_cpu as dref  # noqa: E402
import test_tangent_cpu as tref  # noqa: E402
from conftest import load_golden  # noqa: E402
from oracle import fem  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REF_TANGENT_FREQS = 3.025e-7  # get_undamped_freqs of the orthotropic model through the reference's fp32 bracket
REF_SCALE_GRAD = 6.182e-7  # d sum(freqs) / d log_scale through that bracket
REF_TABLES = 1.164e-7  # K on the reference's fp32 tables against fp64 tables (not needed by a bound below; for the record)
K_RTOL = 2e-6  # assembled K, device against reference, relative to the largest entry (tests/test_hip_kernels.py, test_api_gpu.py)
EIG_TOL = 1e-4  # per eigenvalue (tests/test_parity_gpu.py)
EIG_RTOL = 2e-8  # two solves of one pencil by one deterministic solver (tests/test_deform_gpu.py)
ULP32 = 2.0 ** -23
U64 = 2.0 ** -52

_cache = {}


def _g10():
    return load_golden("g10_aniso_cube2.npz")


def _mat():
    return tuple(float(x) for x in _g10()["mat"])


def _system(order):
    """The cube in the caller's numbering (reorder=False) with its (lam, mu) operator object, once per order."""
    from diffsound_amd.modal_ops import HipModalOps, TetSystem

    if ("sys", order) not in _cache:
        v, t = dref.mesh_case("cube", order)
        mat = _mat()
        s = TetSystem(v.to(DEV), t.to(DEV), order, mat[0], reorder=False)
        lam, mu = fem.lame(mat[1], mat[2])
        _cache[("sys", order)] = (s, HipModalOps(s, lam, mu), lam, mu)
    return _cache[("sys", order)]


def _combine(s, C, k64=True, k32t=True):
    """Raw ds_combine_tangent into fresh buffers: (k64, k32, k32t, ms32, dinv)."""
    from diffsound_amd import _hip

    C = np.ascontiguousarray(C, dtype=np.float64)
    o64 = torch.full((s.nnzb, 9), float("nan"), dtype=torch.float64, device=DEV) if k64 else None
    o32 = torch.full((s.nnzb, 9), float("nan"), device=DEV)
    o32t = torch.full((s.nnzb, 9), float("nan"), device=DEV) if k32t else None
    ms32, dinv = torch.full((s.nnzb,), float("nan"), device=DEV), torch.full((s.nv, 9), float("nan"), device=DEV)
    p = _hip.ptr
    _hip.check(_hip.lib().ds_combine_tangent(p(s.klam), p(s.ms), s.nnzb, p(s.diagidx), s.nv, C.ctypes.data, p(o64), p(o32), p(o32t),
                                             p(ms32), p(dinv), _hip.stream_ptr()), "ds_combine_tangent")
    return o64, o32, o32t, ms32, dinv


def _dense(s, blocks):
    return torch.sparse_bsr_tensor(s.rowptr.long(), s.colidx.long(), blocks.reshape(-1, 3, 3), size=(s.n, s.n)).to_dense()


def _block_ulp(got, want):
    """max over blocks of |got - want| / (largest entry of the block of ``want``), in fp32 ulps."""
    got, want = got.double().reshape(got.shape[0], -1), want.double().reshape(want.shape[0], -1)
    return float(((got - want).abs().max(1).values / want.abs().max(1).values.clamp(min=1e-300)).max()) / ULP32


# ---------------------------------------------------------------------------------------------- (a) isotropic C
@pytest.mark.parametrize("order", [1, 2])
def test_isotropic_tangent_is_the_material_combine(order):
    s, ops, lam, mu = _system(order)
    if order == 2:  # more than one workgroup of the slot kernel, the last one partially filled
        assert s.nnzb > 256 and s.nnzb % 256 != 0
    C = fem.piola_jacobian(lam, mu)
    k64, k32, k32t, ms32, dinv = _combine(s, C)
    want = lam * s.klam + mu * s.kmu
    # nine fp64 products and eight additions per entry on terms bounded by max|C| max|H|: 81 units of roundoff at worst
    bound = 2e-14 * np.abs(C).max() * float(s.klam.abs().max())
    err = float((k64 - want).abs().max())
    print(f"order {order}: k64 against lam klam + mu kmu {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    for name, got, ref in (("k32", k32, ops.k32), ("k32t", k32t, ops.k32t), ("ms32", ms32[:, None], ops.ms32[:, None]),
                           ("dinv32", dinv, ops.dinv)):
        ulps = _block_ulp(got, ref)
        print(f"order {order}: {name} {ulps:.3f} ulp of the block's largest entry")
        assert ulps <= 1.0, name
    assert torch.equal(ms32, ops.ms32)


# ---------------------------------------------------------------------------------------------- (b) any C
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", tref.TANGENTS)
def test_outputs_are_consistent_for_any_tangent(name, order):
    s, _, _, _ = _system(order)
    C = _g10()[f"{name}_C"]
    k64, k32, k32t, ms32, dinv = _combine(s, C)
    assert torch.equal(k32, k64.float())
    assert torch.equal(k32t, k32.reshape(-1, 3, 3).transpose(1, 2).reshape(-1, 9))
    assert torch.equal(ms32, s.ms.float())
    want = torch.linalg.inv(k64[s.diagidx.long()].reshape(-1, 3, 3))
    assert dref.relmax(dinv.reshape(-1, 3, 3).cpu(), want.cpu()) < 1e-5  # as tests/test_hip_kernels.py checks dinv
    # the optional outputs may be left out, and two calls give the same bits
    again = _combine(s, C, k64=False, k32t=False)
    assert again[0] is None and torch.equal(again[1], k32) and torch.equal(again[4], dinv)


# ---------------------------------------------------------------------------------------------- (c) the reference's K
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", tref.TANGENTS)
def test_k64_is_the_references_stiffness_matrix(name, order):
    s, _, _, _ = _system(order)
    g = _g10()
    k64 = _combine(s, g[f"{name}_C"])[0]
    err = dref.relmax(_dense(s, k64).cpu(), g[f"{name}_o{order}_K"])
    print(f"order {order} {name}: k64 against the reference's stiff_matrix {err:.3e} (tolerance {K_RTOL:.1e}; the "
          f"reference's fp32 tables against fp64 {REF_TABLES:.3e})")
    assert err <= K_RTOL


# ---------------------------------------------------------------------------------------------- (d) ds_tangent_forms
def _solved(order):
    """A solved FixedLinear object on the cube, once per order."""
    from src.diffelastic.diff_model import DiffSoundObj, FixedLinear

    if ("solved", order) not in _cache:
        m = load_golden("g2_cube2.npz")
        v, t = torch.from_numpy(m["verts"]).to(DEV), torch.from_numpy(m["tets"]).long().to(DEV)
        obj = DiffSoundObj(vertices=v, tets=t, mode_num=8, mat=_mat(), order=order, mat_model=FixedLinear, task="gt")
        obj.eigen_decomposition()
        _cache[("solved", order)] = obj
    return _cache[("solved", order)]


def _forms_case(order):
    obj = _solved(order)
    ops, s = obj._ops, obj.system
    wide = torch.randn((s.n, 8), generator=torch.Generator().manual_seed(10 + order)).to(DEV)
    return obj, ops, s, (("modes", obj.last_result.vectors), ("random", wide[:, :5]))  # (the second: ldu = 8 > m = 5)


def _quad_and_bound(s, blocks, U):
    """(u^T K u, nnzb 2^-52 S) per column in torch fp64, S = sum_ab |u_a|^T |K_ab| |u_b|: the worst case of recursive summation."""
    K = _dense(s, blocks)
    U = U.double()
    return ((K @ U) * U).sum(0), s.nnzb * U64 * ((K.abs() @ U.abs()) * U.abs()).sum(0)


@pytest.mark.parametrize("order", [1, 2])
def test_forms_contract_to_the_quadratic_forms(order):
    obj, ops, s, blocks = _forms_case(order)
    g = _g10()
    if order == 2:
        assert s.nv > 64  # more than one row range: the second stage sums partial results
    for what, U in blocks:
        assert U.dtype == torch.float32 and U.shape[0] == s.n
        Q = ops.tangent_forms(U)
        assert Q.shape == (U.shape[1], 9, 9) and Q.dtype == torch.float64
        assert torch.equal(Q, ops.tangent_forms(U))  # two calls, the same bits
        for j in (0, U.shape[1] - 1):  # a column's Q does not depend on the other columns of the block
            assert torch.equal(ops.tangent_forms(U[:, j:j + 1].contiguous())[0], Q[j])
        assert torch.equal(ops.tangent_forms(U[:, 1:4])[1], Q[2])
        tangents = [(n_, g[f"{n_}_C"]) for n_ in tref.TANGENTS] + [("klam", fem.piola_jacobian(1.0, 0.0)),
                                                                   ("kmu", fem.piola_jacobian(0.0, 1.0))]
        for name, C in tangents:
            k64 = _combine(s, C)[0]
            want, bound = _quad_and_bound(s, k64, U)
            got = (torch.from_numpy(C).to(DEV) * Q).sum((-1, -2))
            worst = float(((got - want).abs() / bound).max())
            print(f"order {order} {what} {name}: |<C, Q> - u^T k64c u| / (nnzb 2^-52 S) = {worst:.3e}")
            assert worst <= 1.0
        # Q[c] is a symmetric 9 x 9 matrix to the same bound, entry by entry: S[3i+j][3k+l] = sum_ab |u_a,i| |H_ab[j][l]| |u_b,k|
        Habs = _dense(s, s.klam).abs().reshape(s.nv, 3, s.nv, 3)
        Uabs = U.double().abs().reshape(s.nv, 3, -1)
        S = torch.einsum("aic,ajbl,bkc->cijkl", Uabs, Habs, Uabs).reshape(-1, 9, 9)
        ratio = (Q - Q.transpose(1, 2)).abs() / (s.nnzb * U64 * torch.maximum(S, S.transpose(1, 2))).clamp(min=1e-300)
        print(f"order {order} {what}: asymmetry of Q / (nnzb 2^-52 S) = {float(ratio.max()):.3e}")
        assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize("order", [1, 2])
def test_forms_reproduce_the_solvers_quadratic_forms(order):
    """Q contracted with piola_jacobian(1, 0) / (0, 1) against the solver's own a_lambda / b_mu under nnzb 2^-52 S: the
    object's solver returns the forms of the fp32 vectors it returns (ModalSolver.vector_forms), and Q walks the same klam."""
    obj, ops, s, _ = _forms_case(order)
    res = obj.last_result
    Q = ops.tangent_forms(res.vectors)
    for name, C, blocks, own in (("a_lambda", fem.piola_jacobian(1.0, 0.0), s.klam, res.a_lambda),
                                 ("b_mu", fem.piola_jacobian(0.0, 1.0), s.kmu, res.b_mu)):
        _, bound = _quad_and_bound(s, blocks, res.vectors)
        got = (torch.from_numpy(C).to(DEV) * Q).sum((-1, -2))
        worst = float(((got - own).abs() / bound).max())
        print(f"order {order} {name}: |<C, Q> - {name}| / (nnzb 2^-52 S) = {worst:.3e}, relative {float(((got - own).abs() / own.abs()).max()):.3e}")
        assert worst <= 1.0, name


# ---------------------------------------------------------------------------------------------- (e) end to end
def _obj(name, order, mat_model, task="material", mode_num=8, mat=None, solver_config=None, requires_grad=False):
    from src.diffelastic.diff_model import DiffSoundObj

    m = load_golden({"cube": "g2_cube2.npz", "bowl": "g0_bowl_mesh.npz"}[name])
    v, t = torch.from_numpy(m["verts"]).to(DEV), torch.from_numpy(m["tets"]).long().to(DEV)
    if requires_grad:
        v.requires_grad_(True)
    return DiffSoundObj(vertices=v, tets=t, mode_num=mode_num, mat=mat or _mat(), order=order, mat_model=mat_model, task=task,
                        solver_config=solver_config)


def _check_modes(obj, what):
    """U_hat M-orthonormal (tests/test_api_gpu.py), the rigid block annihilated by K relative to ||K|| (tests/test_modal_gpu.py)."""
    U, K, M = obj.U_hat, obj.stiff_matrix, obj.mass_matrix
    assert obj.U_hat_full.shape == (U.shape[0], U.shape[1] + 6) and U.dtype == torch.float64
    gdef = float((U.T @ torch.sparse.mm(M, U) - torch.eye(U.shape[1], device=DEV, dtype=U.dtype)).abs().max())
    probe = torch.randn((U.shape[0], 8), generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(DEV)
    knorm = float(torch.linalg.vector_norm(torch.sparse.mm(K, probe)) / torch.linalg.vector_norm(probe))
    kdef = float(torch.linalg.vector_norm(torch.sparse.mm(K, obj.U_hat_full[:, :6]), dim=0).max()) / knorm
    print(f"{what}: U^T M U - I {gdef:.3e}, ||K Y|| / ||K|| {kdef:.3e}")
    assert gdef < 1e-4 and kdef < 1e-4
    Kd = K.to_dense()
    assert float((Kd - Kd.T).abs().max()) <= 1e-12 * float(Kd.abs().max())


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("name", tref.TANGENTS)
def test_eigendecomposition_with_a_fixed_tangent(name, order):
    from src.diffelastic.diff_model import fixed_tangent

    g = _g10()
    obj = _obj("cube", order, fixed_tangent(g[f"{name}_C"]))
    assert obj._tangent_model and not hasattr(obj.material_model, "lame")
    obj.eigen_decomposition()
    assert obj._ops.lame is None and obj.last_result.b_mu is None
    err = float(np.abs(obj.eigenvalues.cpu().numpy() / g[f"{name}_o{order}_eigenvalues"] - 1).max())
    print(f"cube order {order} {name}: eigenvalues against the reference's {err:.3e} (tolerance {EIG_TOL:.0e})")
    assert err < EIG_TOL
    assert dref.relmax(obj.stiff_matrix.to_dense().cpu(), g[f"{name}_o{order}_K"]) <= K_RTOL
    _check_modes(obj, f"cube order {order} {name}")
    f = obj.get_undamped_freqs()
    assert f.shape == (8, 1) and f.dtype == torch.float32
    assert dref.relmax(f.cpu(), np.sqrt(g[f"{name}_o{order}_eigenvalues"])[:, None] / 2 / np.pi) < EIG_TOL
    vals = obj.get_vals()
    assert vals.shape == (8, 1) and dref.relmax(vals.cpu(), g[f"{name}_o{order}_eigenvalues"][:, None]) < EIG_TOL
    e0 = obj.eigenvalues.clone()
    obj.eigen_decomposition()  # the warm start of a second call
    assert float(((obj.eigenvalues - e0).abs() / e0).max()) < 1e-6


def test_fp64_refinement_with_a_tangent():
    from diffsound_amd.lobpcg.modal_solver import tuned_config
    from src.diffelastic.diff_model import fixed_tangent

    g = _g10()
    obj = _obj("cube", 2, fixed_tangent(g["tri_C"]), solver_config=tuned_config(2, refine_tol=1e-10))
    obj.eigen_decomposition()
    assert obj.last_result.refine_iterations >= 0 and obj._ops._k64 is None
    assert float(np.abs(obj.eigenvalues.cpu().numpy() / g["tri_o2_eigenvalues"] - 1).max()) < EIG_TOL


def test_bowl_with_the_orthotropic_tangent():
    from src.diffelastic.diff_model import fixed_tangent

    mat = _mat()
    C = dref.orthotropic_tangent(*fem.lame(mat[1], mat[2])).numpy()
    v, t = dref.mesh_case("bowl", 1)
    ev, _ = tref.eigsh_modes(tref.assemble_general(v, t, 1, C), fem.assemble_mass(v, t, 1, mat[0])[0], 8)
    obj = _obj("bowl", 1, fixed_tangent(C))
    obj.eigen_decomposition()
    err = float(np.abs(obj.eigenvalues.cpu().numpy() / ev - 1).max())
    print(f"bowl order 1 orthotropic: eigenvalues against eigsh on the restatement {err:.3e} (tolerance {EIG_TOL:.0e})")
    assert err < EIG_TOL
    _check_modes(obj, "bowl order 1 orthotropic")


# ---------------------------------------------------------------------------------------------- (f) read-out
def _bracket_freqs(obj):
    """The reference's matrix-free bracket lambda + diag(U^T stiff_func(U)) - lambda m of the same object."""
    U = obj.U_hat.float()
    pred = obj.eigenvalues + (U * obj.stiff_func(U)).sum(0) - obj.eigenvalues * obj._m
    return (torch.sqrt(pred) / 2 / np.pi).float().unsqueeze(1)


@pytest.mark.parametrize("order", [1, 2])
def test_readout_matches_the_matrix_free_bracket(order):
    """get_undamped_freqs (lambda + <C, Q> - lambda m) and its gradient on log_scale against the matrix-free bracket of the
    same object, at 4x the reference's fp32 error."""
    from src.diffelastic.diff_model import TrainableOrthotropic

    obj = _obj("cube", order, TrainableOrthotropic)
    with torch.no_grad():
        obj.material_model.log_scale.copy_(torch.tensor(tref.READOUT_LOG_SCALE, dtype=torch.float64))
    assert [tuple(p.shape) for p in obj.parameters()] == [(9,)]
    obj.eigen_decomposition()
    f = obj.get_undamped_freqs()
    assert f.shape == (8, 1) and f.dtype == torch.float32
    f.sum().backward()
    grad = obj.material_model.log_scale.grad.clone()
    obj.material_model.zero_grad()
    fb = _bracket_freqs(obj)
    fb.sum().backward()
    gb = obj.material_model.log_scale.grad.clone()
    ef, eg = dref.relmax(f.detach().cpu(), fb.detach().cpu()), dref.relmax(grad, gb)
    print(f"cube order {order}: freqs {ef:.3e} (tolerance {4 * REF_TANGENT_FREQS:.3e}), d/d log_scale {eg:.3e} "
          f"(tolerance {4 * REF_SCALE_GRAD:.3e})")
    assert ef <= 4 * REF_TANGENT_FREQS and eg <= 4 * REF_SCALE_GRAD
    assert float(grad.abs().min()) > 0  # every engineering constant moves the frequencies


def test_zero_log_scale_is_the_trainable_linear_model():
    """At zero log_scale the orthotropic model IS the isotropic one: the same pencil to 1e-12 through two routes, so the
    eigenvalues and the frequencies agree at EIG_RTOL (the argument of tests/test_deform_gpu.py).  The frequencies are
    compared in fp64 - the brackets both read-outs take the square root of - and the returned float32 tensors are their
    roundings: a relative 2e-8 cannot be asked of float32 numbers."""
    from src.diffelastic.diff_model import MatSet, TrainableLinear, TrainableOrthotropic

    base = _obj("cube", 2, TrainableLinear, mat=MatSet.Ceramic)
    with torch.no_grad():  # (the bins' start, not the table's values)
        E, nu = float(base.material_model.youngs()), float(base.material_model.poisson())
    twin = _obj("cube", 2, TrainableOrthotropic, mat=(MatSet.Ceramic[0], E, nu) + tuple(MatSet.Ceramic[3:]))
    for o in (base, twin):
        o.eigen_decomposition()
    eb, et = base.eigenvalues, twin.eigenvalues
    err = float(((et - eb).abs() / eb).max())
    print(f"eigenvalues: largest relative difference of a pair {err:.3e} (tolerance {EIG_RTOL:.1e})")
    assert err <= EIG_RTOL
    lam, mu = (x.detach().to(DEV) for x in base.material_model.lame())
    fb64 = torch.sqrt(eb + (lam * base._a + mu * base._b) - eb * base._m) / 2 / np.pi
    C = twin.material_model.tangent().detach().to(DEV)
    ft64 = torch.sqrt(et + (C * twin._Q).sum((-1, -2)) - et * twin._m) / 2 / np.pi
    errf = float(((ft64 - fb64).abs() / fb64).max())
    print(f"frequencies: largest relative difference of a pair {errf:.3e} (tolerance {EIG_RTOL:.1e})")
    assert errf <= EIG_RTOL
    assert torch.equal(base.get_undamped_freqs().detach(), fb64.float().unsqueeze(1))
    assert torch.equal(twin.get_undamped_freqs().detach(), ft64.float().unsqueeze(1))


# ---------------------------------------------------------------------------------------------- (g) switching
@pytest.mark.parametrize("order", [1, 2])
def test_one_operator_switches_between_material_and_tangent(order):
    from diffsound_amd.lobpcg.modal_solver import ModalSolver, tuned_config
    from diffsound_amd.modal_ops import HipModalOps, TetSystem

    g = _g10()
    v, t = dref.mesh_case("cube", order)
    mat = _mat()
    lam, mu = fem.lame(mat[1], mat[2])
    s = TetSystem(v.to(DEV), t.to(DEV), order, mat[0])
    ops = HipModalOps(s, lam, mu)
    solve = lambda: ModalSolver(ops, tuned_config(order)).solve(8).eigenvalues.clone()
    k32, dinv, e0 = ops.k32.clone(), ops.dinv.clone(), solve()
    assert ops.lame == (lam, mu) and ops.k64c is None
    ops.set_tangent(g["tri_C"])
    assert ops.lame is None and ops.k64c is not None and (ops.coarse is None or ops.coarse.lame is None)
    assert ops.polish_terms()[0][0][1] is ops.k64c and len(ops.polish_terms()[0]) == 1
    assert not torch.equal(ops.k32, k32)
    et = solve()
    # (the fixture's eigenvalues: the object built with tangent=C from the start gives them too)
    assert float(np.abs(et.cpu().numpy() / g[f"tri_o{order}_eigenvalues"] - 1).max()) < EIG_TOL
    fresh = HipModalOps(s, tangent=g["tri_C"])
    assert torch.equal(fresh.k32, ops.k32) and torch.equal(fresh.dinv, ops.dinv) and torch.equal(fresh.k64c, ops.k64c)
    ops.set_material(lam, mu)
    assert ops.lame == (lam, mu) and ops.k64c is None
    assert torch.equal(ops.k32, k32) and torch.equal(ops.dinv, dinv)
    e2 = solve()
    err = float(((e2 - e0).abs() / e0).max())
    print(f"order {order}: eigenvalues after material -> tangent -> material {err:.3e} (tolerance {EIG_RTOL:.1e})")
    assert err <= EIG_RTOL
    with pytest.raises(ValueError):
        HipModalOps(s)
    with pytest.raises(ValueError):
        HipModalOps(s, lam, mu, tangent=g["tri_C"])


def test_limits_are_named():
    from src.diffelastic.diff_model import fixed_tangent

    g = _g10()
    obj = _obj("cube", 1, fixed_tangent(g["ortho_C"]), requires_grad=True)
    obj.eigen_decomposition()
    with pytest.raises(NotImplementedError, match="geometry gradient"):
        obj.get_vals()
    bad = g["ortho_C"].copy()
    bad[1, 3] = bad[3, 1] = 0.0
    obj = _obj("cube", 1, fixed_tangent(bad))
    with pytest.raises(ValueError, match="minor symmetry"):
        obj.eigen_decomposition()
    assert obj._ops is None  # refused on the host, before any launch


# ---------------------------------------------------------------------------------------------- (h) argument checks
def test_operands_are_checked():
    from diffsound_amd import _hip

    s, ops, lam, mu = _system(1)
    L, p = _hip.lib(), _hip.ptr
    C = np.ascontiguousarray(fem.piola_jacobian(lam, mu))
    k32, ms32, dinv = torch.empty((s.nnzb, 9), device=DEV), torch.empty((s.nnzb,), device=DEV), torch.empty((s.nv, 9), device=DEV)
    before = (ops.k32.clone(), ops.dinv.clone())

    def combine(nnzb=s.nnzb, nv=s.nv, c=C, out=k32):
        return L.ds_combine_tangent(p(s.klam), p(s.ms), nnzb, p(s.diagidx), nv, None if c is None else c.ctypes.data, None, p(out),
                                    None, p(ms32), p(dinv), _hip.stream_ptr())

    assert combine() == 0
    nan = C.copy()
    nan[4, 4] = np.nan
    for bad in (dict(nnzb=0), dict(nv=0), dict(c=None), dict(out=None), dict(c=nan)):
        assert combine(**bad) != 0, bad
        assert L.ds_last_error()
    U = torch.randn((s.n, 8), generator=torch.Generator().manual_seed(0)).to(DEV)
    Q = torch.empty((8, 81), dtype=torch.float64, device=DEV)
    need = L.ds_tangent_forms_workspace_bytes(s.nv, 8)
    assert need == -(-s.nv // 64) * 8 * 81 * 8 and L.ds_tangent_forms_workspace_bytes(s.nv, 0) == 0
    work = torch.empty((need,), dtype=torch.uint8, device=DEV)

    def forms(m=8, u=U.data_ptr(), ldu=8, work_bytes=need, q=Q):
        return L.ds_tangent_forms(p(s.rowptr), p(s.colidx), p(s.klam), s.nv, u, ldu, m, p(q), p(work), work_bytes, _hip.stream_ptr())

    assert forms() == 0
    for bad in (dict(m=0), dict(u=U.data_ptr() + 2), dict(work_bytes=need - 1), dict(ldu=4), dict(q=None), dict(u=None)):
        assert forms(**bad) != 0, bad
        assert L.ds_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ops.k32, before[0]) and torch.equal(ops.dinv, before[1])
    with pytest.raises(ValueError):
        ops.tangent_forms(U.double())
    with pytest.raises(RuntimeError, match="HIP"):
        ops.tangent_forms(U.cpu())
