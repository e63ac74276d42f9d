"""Shape gradients for a general tangent: ds_geometry_grad_tangent (csrc/geomgrad.hip), TetSystem.geometry_grad_tangent,
HipModalOps.geometry_grad and DiffSoundObj.get_vals_differentiable / get_undamped_freqs, against the fp64 restatement
tests/_geomgrad_ref.py (checked on the CPU by tests/test_geomgrad_tangent_cpu.py) and the fixture made from the
reference (tests/golden/g12_aniso_geometry.npz, make_golden_aniso_geometry.py).

The kernel-level mesh is the 2^3 cube of g2_cube2.npz (48 elements) with every node moved by a fixed seed, at most 0.1 of
the shortest grid edge per axis."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _geomgrad_ref as gref  # noqa: E402
import test_tangent_cpu as tref  # noqa: E402
from conftest import load_golden  # noqa: E402
from diffsound_amd import fem_tables  # noqa: E402
from oracle import fem  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
JITTER_SEED = 1207
# (a), (b): both sides are fp64 on identical inputs: 2^-52 times about 300 operations per element-mode-point, times 65
# modes, times at most 32 incident elements, with a factor 10 (1.4e-9 rounded down)
KERNEL_RTOL = 1e-9

_cache = {}


def _g10():
    return load_golden("g10_aniso_cube2.npz")


def _density():
    return float(_g10()["mat"][0])


def _tangent(name):
    g = _g10()
    if name != "asym":
        return np.ascontiguousarray(g[f"{name}_C"], dtype=np.float64)
    C = np.array(g["tri_C"], dtype=np.float64)  # symmetric only to a tolerance, as elastic_tangent admits
    return C + 1e-6 * np.abs(C).max() * np.random.default_rng(3).uniform(-1.0, 1.0, (9, 9))


def _mesh(order, T):
    """(vertices (nv, 3) fp32, tets (T, N) long) on the host: the jittered cube, its last element dropped for T = 47."""
    if ("mesh", order, T) not in _cache:
        m = load_golden("g2_cube2.npz")
        v0, t0 = m["verts"], m["tets"]
        assert t0.shape[0] == 48
        edge = float(((v0.max(0) - v0.min(0)) / 2).min())  # two cells per axis
        v = (v0.astype(np.float64) + 0.1 * edge * np.random.default_rng(JITTER_SEED).uniform(-1.0, 1.0, v0.shape)).astype(np.float32)
        v, t = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t0[:T]).long(), order)
        assert bool((gref.signed_dets(v.double(), t, order) > 0).all())
        _cache[("mesh", order, T)] = (v, t)
    return _cache[("mesh", order, T)]


def _system(order, T, reorder):
    from diffsound_amd.modal_ops import TetSystem

    if ("sys", order, T, reorder) not in _cache:
        v, t = _mesh(order, T)
        _cache[("sys", order, T, reorder)] = TetSystem(v.to(DEV), t.to(DEV), order, _density(), reorder=reorder)
    return _cache[("sys", order, T, reorder)]


def _operands(order, T, m):
    """(U (n, m + 3) fp32 in the caller's numbering, gk, gm (m,) fp64) on the host; gk positive, gm = gk * (an eigenvalue's
    size), so that the stiffness and the mass term are of one magnitude."""
    v, _ = _mesh(order, T)
    gen = torch.Generator().manual_seed(100 * order + m + T)
    U = torch.randn((3 * v.shape[0], m + 3), generator=gen)
    gk = torch.rand((m,), generator=gen, dtype=torch.float64) + 0.5
    gm = gk * (torch.rand((m,), generator=gen, dtype=torch.float64) + 0.5) * 1e10
    return U, gk, gm


def _want(order, T, m, name):
    """The restatement's gradient, once per case (shared by the reorder variants)."""
    key = ("want", order, T, m, name)
    if key not in _cache:
        v, t = _mesh(order, T)
        U, gk, gm = _operands(order, T, m)
        _cache[key] = gref.grad_of_s(v, t, order, U[:, :m], gk, gm, _tangent(name), _density())
    return _cache[key]


def _relmax(got, want):
    return float((got.cpu() - want).abs().max() / want.abs().max())


# ---------------------------------------------------------------------------------------------- (a) the restatement
@pytest.mark.parametrize("reorder", [True, False])
@pytest.mark.parametrize("T", [48, 47])
@pytest.mark.parametrize("m", [1, 8, 65])
@pytest.mark.parametrize("name", ["ortho", "tri", "asym"])
@pytest.mark.parametrize("order", [1, 2])
def test_kernel_matches_the_restatement(order, name, m, T, reorder):
    s = _system(order, T, reorder)
    assert s.T == T
    U, gk, gm = _operands(order, T, m)
    Ui = s.rows_to_internal(U.to(DEV))[:, :m]
    assert Ui.stride(0) == m + 3 and Ui.stride(1) == 1  # ldu = m + 3
    got = s.geometry_grad_tangent(Ui, gk.to(DEV), gm.to(DEV), _tangent(name))
    assert got.shape == (s.nv, 3) and got.dtype == torch.float64
    want = _want(order, T, m, name)
    err = _relmax(got, want)
    print(f"order {order} {name} m {m} T {T} reorder {reorder}: max|got - want| / max|want| = {err:.3e} (bound {KERNEL_RTOL:.0e})")
    assert err <= KERNEL_RTOL


# ---------------------------------------------------------------------------------------------- (b) isotropic C
@pytest.mark.parametrize("order", [1, 2])
def test_isotropic_tangent_agrees_with_the_lame_kernel(order):
    from diffsound_amd.modal_ops import HipModalOps, isotropic_tangent

    s = _system(order, 48, True)
    mat = _g10()["mat"]
    lam, mu = fem.lame(float(mat[1]), float(mat[2]))
    assert np.array_equal(isotropic_tangent(lam, mu), fem.piola_jacobian(lam, mu))
    U, gk, gm = _operands(order, 48, 8)
    Ui = s.rows_to_internal(U.to(DEV))[:, :8].contiguous()
    want = s.geometry_grad(Ui, gk.to(DEV), gm.to(DEV), lam, mu)
    got = s.geometry_grad_tangent(Ui, gk.to(DEV), gm.to(DEV), fem.piola_jacobian(lam, mu))
    err = _relmax(got, want.cpu())
    print(f"order {order}: tangent kernel with piola_jacobian(lam, mu) against ds_geometry_grad {err:.3e} (bound {KERNEL_RTOL:.0e})")
    assert err <= KERNEL_RTOL
    # the operator's own entry point: its current tangent, and after set_material the tangent of (lam, mu)
    ops = HipModalOps(s, tangent=_tangent("tri"))
    assert torch.equal(ops.geometry_grad(Ui, gk.to(DEV), gm.to(DEV)), s.geometry_grad_tangent(Ui, gk.to(DEV), gm.to(DEV), _tangent("tri")))
    ops.set_material(lam, mu)
    assert torch.equal(ops.geometry_grad(Ui, gk.to(DEV), gm.to(DEV)), got)


# ---------------------------------------------------------------------------------------------- raw calls
def _raw_args(s, U, gk, gm, C, grad, work):
    from diffsound_amd import _hip

    gt, gw = fem_tables.minimal_gradient_rule(s.order)
    gtab, gwt = torch.from_numpy(gt).to(DEV), torch.from_numpy(gw).to(DEV)
    cptr, cinc = s.corner_incidence()
    p = _hip.ptr
    keep = (gtab, gwt, cptr, cinc, C)  # (the caller keeps these alive)
    args = dict(tets=p(s.tets), T=s.T, N=s.N, nv=s.nv, tetgeo=p(s._tetgeo), U=p(U), ldu=U.stride(0), m=U.shape[1], gk=p(gk),
                gm=p(gm), C=C.ctypes.data, gtab=p(gtab), gw=p(gwt), ng=gt.shape[0], mtab=p(s.mtab), cinc_ptr=p(cptr),
                cinc=p(cinc), elem_work=p(work), grad=p(grad))
    return args, keep


def _raw_call(args, **over):
    from diffsound_amd import _hip

    a = dict(args, **over)
    order = ("tets", "T", "N", "nv", "tetgeo", "U", "ldu", "m", "gk", "gm", "C", "gtab", "gw", "ng", "mtab", "cinc_ptr", "cinc",
             "elem_work", "grad")
    return _hip.lib().ds_geometry_grad_tangent(*[a[k] for k in order], _hip.stream_ptr())


# ---------------------------------------------------------------------------------------------- (c) written, repeatable
@pytest.mark.parametrize("order,T", [(1, 48), (2, 48), (2, 47)])
def test_output_is_written_and_repeatable(order, T):
    s = _system(order, T, False)
    U, gk, gm = _operands(order, T, 65)
    Ui = U.to(DEV)[:, :65].contiguous()
    C = _tangent("asym")
    outs = []
    for _ in range(2):
        grad = torch.full((s.nv, 3), float("nan"), dtype=torch.float64, device=DEV)
        work = torch.full((s.T, 12), float("nan"), dtype=torch.float64, device=DEV)
        args, keep = _raw_args(s, Ui, gk.to(DEV), gm.to(DEV), C, grad, work)
        assert _raw_call(args) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(work).all())
        outs.append(grad)
    assert torch.equal(outs[0], outs[1])  # two calls, the same bits
    assert _relmax(outs[0], _want(order, T, 65, "asym")) <= KERNEL_RTOL
    corner = torch.zeros(s.nv, dtype=torch.bool, device=DEV)
    corner[s.tets[:, list(fem_tables.CORNER_SLOTS[order])].long().reshape(-1)] = True
    if order == 2:
        assert int((~corner).sum()) > 0
    assert bool((outs[0][~corner] == 0).all())  # mid-edge nodes (and nodes no element references): exactly 0
    assert bool((outs[0][corner].abs().amax(1) > 0).all())
    # the incidence list: a stable sort of the corner columns by node
    cptr, cinc = (x.cpu().long() for x in s.corner_incidence())
    nodes = s.tets[:, list(fem_tables.CORNER_SLOTS[order])].long().reshape(-1).cpu()
    assert cptr.shape[0] == s.nv + 1 and cinc.shape[0] == 4 * s.T and int(cptr[-1]) == 4 * s.T
    for n_ in range(s.nv):
        mine = cinc[cptr[n_]:cptr[n_ + 1]]
        assert bool((nodes[mine] == n_).all()) and bool((mine[1:] > mine[:-1]).all())


# ---------------------------------------------------------------------------------------------- (d) argument checks
def test_operands_are_checked():
    from diffsound_amd import _hip

    s = _system(1, 48, False)
    U, gk, gm = _operands(1, 48, 8)
    Ui, gk, gm = U.to(DEV)[:, :8], gk.to(DEV), gm.to(DEV)
    C = _tangent("tri")
    grad = torch.full((s.nv, 3), 7.0, dtype=torch.float64, device=DEV)
    work = torch.empty((s.T, 12), dtype=torch.float64, device=DEV)
    args, keep = _raw_args(s, Ui, gk, gm, C, grad, work)
    nan, inf = C.copy(), C.copy()
    nan[4, 4], inf[8, 0] = np.nan, np.inf
    bad = [{k: None} for k in ("tets", "tetgeo", "U", "gk", "gm", "C", "gtab", "gw", "mtab", "cinc_ptr", "cinc", "elem_work", "grad")]
    bad += [dict(N=5), dict(N=10, ng=0), dict(ng=0), dict(ng=5), dict(T=0), dict(nv=0), dict(m=0), dict(ldu=7), dict(T=1 << 29),
            dict(C=nan.ctypes.data), dict(C=inf.ctypes.data), dict(U=args["U"] + 2)]
    bad += [{k: args[k] + 4} for k in ("tetgeo", "gk", "gm", "gtab", "gw", "mtab", "elem_work", "grad")]
    for b in bad:
        assert _raw_call(args, **b) != 0, b
        assert _hip.lib().ds_last_error(), b
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all())  # refused on the host, before any launch
    assert _raw_call(args) == 0
    torch.cuda.synchronize()
    assert bool((grad != 7.0).all())
    with pytest.raises(ValueError):
        s.geometry_grad_tangent(Ui.double(), gk, gm, C)
    with pytest.raises(ValueError):
        s.geometry_grad_tangent(Ui, gk[:3], gm, C)
    with pytest.raises(ValueError):
        s.geometry_grad_tangent(Ui, gk, gm, nan)
    with pytest.raises(RuntimeError, match="HIP"):
        s.geometry_grad_tangent(Ui.cpu(), gk, gm, C)


# ---------------------------------------------------------------------------------------------- (e) the reference
@pytest.mark.parametrize("order", [1, 2])
def test_shape_gradient_matches_the_reference(order):
    """get_vals_differentiable() of a fixed triclinic tangent and its gradient on the vertices against the reference's
    get_vals() and autograd (g12 fixture): vals at 1e-4, d sum(vals) / dx and d sum(w vals) / dx at 2e-3 of the norm - the
    figures tests/test_api_gpu.py::test_geometry_backward_matches_reference uses for the same quantity."""
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, fixed_tangent

    g = load_golden("g12_aniso_geometry.npz")
    assert float(g["min_gap"]) >= 1e-2  # simple eigenvalues: the weighted gradient belongs to individual eigenvectors
    mat = tuple(float(x) for x in g["mat"])
    v = torch.from_numpy(g["verts"]).to(DEV).requires_grad_(True)
    obj = DiffSoundObj(vertices=v, tets=torch.from_numpy(g["tets"]).to(DEV), mode_num=int(g["mode_num"]), mat=mat, order=order,
                       mat_model=fixed_tangent(g["C"]), task="material")
    obj.eigen_decomposition()
    vals = obj.get_vals_differentiable()
    assert vals.shape == (8, 1) and vals.dtype == torch.float64
    ev = float(np.abs(vals.detach().cpu().numpy() / g[f"o{order}_vals"] - 1).max())
    print(f"order {order}: vals against the reference's get_vals() {ev:.3e} (tolerance 1e-4)")
    assert ev < 1e-4
    w = torch.linspace(0.5, 1.5, 8, device=DEV, dtype=torch.float64).reshape(8, 1)
    for what, loss, key in (("sum", vals.sum(), "grad_vertices"), ("weighted", (vals * w).sum(), "grad_vertices_weighted")):
        v.grad = None
        loss.backward(retain_graph=True)
        got, want = v.grad.cpu().numpy(), g[f"o{order}_{key}"]
        assert got.shape == want.shape
        err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"order {order}: d {what}(vals) / dx against the reference's autograd {err:.3e} (tolerance 2e-3)")
        assert err < 2e-3


# ---------------------------------------------------------------------------------------------- (f) joint gradient
def _cube_obj(order, mat_model, requires_grad, mat=None):
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj

    m = load_golden("g2_cube2.npz")
    v, t = torch.from_numpy(m["verts"]).to(DEV), torch.from_numpy(m["tets"]).long().to(DEV)
    if requires_grad:
        v.requires_grad_(True)
    mat = mat or tuple(float(x) for x in _g10()["mat"])
    return v, DiffSoundObj(vertices=v, tets=t, mode_num=8, mat=mat, order=order, mat_model=mat_model, task="material")


def _joint_case(order, mat_model, prepare, params, closed_form):
    """The checks of (f) for one model class.  ``prepare(model, first)`` puts the model into its state; ``params(model)``
    lists the parameters whose gradients are compared; ``closed_form(obj)`` is the fp64 bracket from the kept forms."""
    v, obj = _cube_obj(order, mat_model, True)
    prepare(obj.material_model, None)
    obj.eigen_decomposition()
    lifted = obj.tetmesh.vertices
    if not lifted.is_leaf:
        lifted.retain_grad()
    f = obj.get_undamped_freqs()
    assert f.shape == (8, 1) and f.dtype == torch.float32
    f.sum().backward()
    pg = [p.grad.clone() for p in params(obj.material_model)]
    assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0
    for g_ in pg:
        assert bool(torch.isfinite(g_).all()) and float(g_.abs().max()) > 0
    # the vertex gradient IS the kernel's, with gk = d sum(f) / d bracket through the same operations
    bracket = obj.get_vals_differentiable().detach().requires_grad_(True)
    (torch.sqrt(bracket.squeeze(1)) / 2 / np.pi).float().unsqueeze(1).sum().backward()
    gk = bracket.grad.reshape(-1)
    C = closed_form(obj)[1]
    direct = obj.system.geometry_grad_tangent(obj.last_result.vectors.float().contiguous(), gk, gk * obj.eigenvalues, C)
    assert torch.equal(lifted.grad, direct.to(lifted.dtype))
    # the material gradient: the same object on vertices without requires_grad, today's path
    _, plain = _cube_obj(order, mat_model, False)
    prepare(plain.material_model, obj.material_model)
    plain.eigen_decomposition()
    fp = plain.get_undamped_freqs()
    fp.sum().backward()
    for name, a, b in zip(("first", "second"), pg, [p.grad for p in params(plain.material_model)]):
        err = float((a - b).abs().max() / b.abs().max())
        print(f"order {order} {mat_model.__name__}: {name} parameter gradient, joint against material-only {err:.3e} (bound 1e-12)")
        assert err <= 1e-12
    # without requires_grad the read-out is what it was: the closed form of the kept quadratic forms, bit for bit
    want = (torch.sqrt(closed_form(plain)[0]) / 2 / np.pi).float().unsqueeze(1)
    assert torch.equal(fp.detach(), want)
    assert torch.equal(f.detach(), (torch.sqrt(closed_form(obj)[0]) / 2 / np.pi).float().unsqueeze(1))  # the joint path too


@pytest.mark.parametrize("order", [1, 2])
def test_joint_gradient_orthotropic(order):
    from diffsound_amd.diffelastic.diff_model import TrainableOrthotropic

    def prepare(model, first):
        with torch.no_grad():
            model.log_scale.copy_(torch.tensor(tref.READOUT_LOG_SCALE, dtype=torch.float64))

    def closed_form(o):
        C = o.material_model.tangent().detach()
        e = o.eigenvalues
        return e + (C.to(DEV) * o._Q).sum((-1, -2)) - e * o._m, C

    _joint_case(order, TrainableOrthotropic, prepare, lambda mm: [mm.log_scale], closed_form)


@pytest.mark.parametrize("order", [1, 2])
def test_joint_gradient_trainable_linear(order):
    from diffsound_amd.diffelastic.diff_model import TrainableLinear
    from diffsound_amd.modal_ops import isotropic_tangent

    def prepare(model, first):  # (the bin logits start at random values: the second object takes the first one's)
        if first is not None:
            model.load_state_dict(first.state_dict())

    def closed_form(o):
        lam, mu = (x.detach() for x in o.material_model.lame())
        e = o.eigenvalues
        return e + (lam.to(DEV) * o._a + mu.to(DEV) * o._b) - e * o._m, isotropic_tangent(float(lam), float(mu))

    _joint_case(order, TrainableLinear, prepare, lambda mm: [mm.youngs.probablity, mm.poisson.probablity], closed_form)


def test_plain_custom_model_is_named():
    """A custom model with neither lame() nor tangent(): the limit is named, and get_undamped_freqs keeps its path."""
    import test_deform_cpu as dref

    class Plain(torch.nn.Module):
        def __init__(self, mat):
            super().__init__()
            self.mat = mat
            self.lam, self.mu = fem.lame(mat.youngs, mat.poisson)

        def forward(self, F):
            return dref.linear_stress(F, self.lam, self.mu)

        def jacobian_F(self):
            return torch.from_numpy(fem.piola_jacobian(self.lam, self.mu)).reshape(1, 3, 3, 1, 3, 3)

    v, obj = _cube_obj(1, Plain, True)
    obj.eigen_decomposition()
    with pytest.raises(NotImplementedError, match="get_vals_differentiable"):
        obj.get_vals_differentiable()
    assert obj.get_undamped_freqs().shape == (8, 1)


# ---------------------------------------------------------------------------------------------- (g) shape loop
def test_shape_loop_end_to_end():
    """kuhn_grid -> sphere SDF -> marching tets -> largest component -> an orthotropic object -> frequencies -> a loss:
    one backward reaches the SDF and the material parameters."""
    from diffsound_amd import dmtet
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, TrainableOrthotropic
    from diffsound_amd.diffelastic.mesh import largest_connected_component

    pos, tets = (torch.from_numpy(x).to(DEV) for x in dmtet.kuhn_grid(8))
    sdf = (0.37 - pos.norm(dim=1)).detach().requires_grad_(True)  # positive inside the sphere
    verts, tet_out = dmtet.marching_tets(pos, sdf, tets)
    verts, tet_out = largest_connected_component(verts, tet_out)
    assert verts.requires_grad and tet_out.shape[0] > 100
    obj = DiffSoundObj(vertices=verts, tets=tet_out, mode_num=4, order=1, mat_model=TrainableOrthotropic, task="material")
    obj.eigen_decomposition()
    f = obj.get_undamped_freqs()
    target = f.detach() * torch.tensor([[1.05], [0.95], [1.04], [0.97]], device=DEV)
    loss = (((f - target) / target) ** 2).sum()
    loss.backward()
    for name, g_ in (("sdf", sdf.grad), ("log_scale", obj.material_model.log_scale.grad)):
        assert g_ is not None and bool(torch.isfinite(g_).all()) and float(g_.abs().max()) > 0, name
