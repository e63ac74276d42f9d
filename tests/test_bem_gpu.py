"""Helmholtz BEM on the device (csrc/bem.hip via diffsound_amd/diffelastic/bem.py): kernel parity with the fp64
restatement of tests/test_bem_cpu.py, the point-source solution, determinism, the mesh helpers and the public API."""
import os
import re
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bem_cpu as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _bem():
    from diffsound_amd.diffelastic import bem

    return bem


def _box_surface(n=3):
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic.mesh import TetMesh

    v, t = meshgen.kuhn_box(n)
    mesh = TetMesh(torch.from_numpy(v).to(DEV), torch.from_numpy(t).long().to(DEV))
    tri, _ = _bem().surface_of(mesh)
    return v, tri.cpu().numpy(), mesh


def _meshes():
    from diffsound_amd import meshgen

    v, f = meshgen.icosphere(2)
    bv, bf, _ = _box_surface(3)
    return {"icosphere2": (v, f, 2.0), "kuhn_box3": (bv, bf, 25.0)}


@pytest.mark.parametrize("name", ["icosphere2", "kuhn_box3"])
def test_assembly_and_potential_match_restatement(name):
    v, f, k = _meshes()[name]
    model = _bem().BEMModel(v, f)
    m = model.m
    perm = model._perm.cpu().numpy()
    g = ref.geometry(v, f[perm])  # the restatement on the model's internal (Morton) face order
    rng = np.random.default_rng(3)
    gv = (rng.normal(size=m) + 1j * rng.normal(size=m)).astype(np.complex64)
    A, rhs, V = model.assemble(k, torch.from_numpy(gv).to(DEV), want_V=True)
    A, rhs, V = A[:, :m].cpu().numpy(), rhs.cpu().numpy(), V[:, :m].cpu().numpy()
    Ar, Vr, rhsr, near = ref.assemble(g, k, gv.astype(np.complex128))
    assert near.sum() > m and (~near).sum() > 0
    for got, want in ((A, Ar), (V, Vr)):
        scale = np.abs(want).max()
        err = np.abs(got - want)
        assert err[~near].max() <= 1e-5 * scale, (name, err[~near].max() / scale)
        assert err[near].max() <= 1e-4 * scale, (name, err[near].max() / scale)
    assert np.all(np.diag(A).real == -0.5 * model.area.cpu().numpy())  # K_ii = 0 exactly: A_ii = -area / 2
    assert np.abs(rhs - rhsr).max() <= 1e-4 * np.abs(rhsr).max()
    # potential: far points and points near the surface (0.3 h off the centroids, on both sides of the faces)
    c, n, h = g["c"], g["n"], g["h"]
    near_pts = np.concatenate([c[:40] + 0.3 * h[:40, None] * n[:40], c[40:60] - 0.2 * h[40:60, None] * n[40:60]])
    pts = np.concatenate([ref.listener_points(np.abs(v).max()), near_pts])
    uv = (rng.normal(size=m) + 1j * rng.normal(size=m)).astype(np.complex64)
    out = model._potential(k, torch.from_numpy(gv).to(DEV), torch.from_numpy(uv).to(DEV), pts).cpu().numpy()
    want = ref.potential(g, k, gv.astype(np.complex128), uv.astype(np.complex128), pts)
    scale = np.abs(want).max()
    assert np.abs(out - want).max() <= 1e-4 * scale, np.abs(out - want).max() / scale


def test_cgemv_matches_torch_mv():
    bem = _bem()
    from diffsound_amd import meshgen

    v, f = meshgen.icosphere(1)
    model = bem.BEMModel(v, f)
    gen = torch.Generator().manual_seed(5)
    for n in (model.m,):
        A = torch.randn((n, n + (n & 1)), dtype=torch.complex64, generator=gen).to(DEV)
        x = torch.randn(n + (n & 1), dtype=torch.complex64, generator=gen).to(DEV)
        s = torch.rand(n, generator=gen).to(DEV) + 0.5
        y = model.cgemv(A, x, s)
        want = s.double() * torch.mv(A[:, :n].to(torch.complex128), x[:n].to(torch.complex128))
        bound = 4 * n * 6e-8 * float((A[:, :n].abs().double() @ x[:n].abs().double() * s.double()).max())
        assert float((y.to(torch.complex128) - want).abs().max()) <= bound


def test_cgemv_odd_size_and_long_rows():
    from diffsound_amd import _hip

    gen = torch.Generator().manual_seed(9)
    for n in (1, 63, 1001, 3001):
        lda = n + (n & 1)
        A = torch.randn((n, lda), dtype=torch.complex64, generator=gen).to(DEV)
        x = torch.randn(lda, dtype=torch.complex64, generator=gen).to(DEV)
        y = torch.empty(n, dtype=torch.complex64, device=DEV)
        _hip.check(_hip.lib().ds_bem_cgemv(A.data_ptr(), lda, x.data_ptr(), n, None, y.data_ptr(), _hip.stream_ptr()),
                   "ds_bem_cgemv")
        want = torch.mv(A[:, :n].to(torch.complex128), x[:n].to(torch.complex128))
        bound = 4 * n * 6e-8 * float((A[:, :n].abs().double() @ x[:n].abs().double()).max())
        assert float((y.to(torch.complex128) - want).abs().max()) <= bound, n


def _point_source_gpu(v, f, ka, radius):
    """(boundary error, potential error, gmres_info) of the device solve of the point-source problem."""
    model = _bem().BEMModel(v, f)
    g = ref.geometry(v, f)
    k = ka / radius
    x0 = ref.X0 * radius
    gvec, u_ex = ref.point_source_data(g, k, x0)
    model.boundary_equation_solve(gvec, k)
    u = model.dirichlet_fun.coefficients
    pts = ref.listener_points(radius)
    p = model.potential_solve(pts)
    p_ex = ref.exact_field(pts, k, x0)
    return (np.linalg.norm(u - u_ex) / np.linalg.norm(u_ex), np.linalg.norm(p - p_ex) / np.linalg.norm(p_ex),
            model.gmres_info)


@pytest.mark.parametrize("ka", [0.1, 1.0, 2.5])
def test_point_source_on_icospheres(ka):
    from diffsound_amd import meshgen

    errs = {}
    for level in (3, 4):
        v, f = meshgen.icosphere(level, radius=0.5)
        eu, ep, info = _point_source_gpu(v, f, ka, 0.5)
        assert info["converged"] and info["residual"] <= 1e-5, info
        errs[level] = (eu, ep)
    bu, bp = ref.POINT_SOURCE_BOUNDS[(3, ka)]  # the fp64 restatement's level-3 bounds
    assert errs[3][0] <= bu and errs[3][1] <= bp, errs
    assert errs[4][0] < 0.6 * errs[3][0] and errs[4][1] < 0.6 * errs[3][1], errs


def test_point_source_in_a_box():
    v, f, _ = _box_surface(6)
    center = v.mean(0).astype(np.float64)
    size = float(np.linalg.norm(v.max(0) - v.min(0)))
    model = _bem().BEMModel(v, f)
    g = ref.geometry(v, f)
    k = 1.0 / size
    x0 = center + np.array([0.01, -0.005, 0.004])
    gvec, u_ex = ref.point_source_data(g, k, x0)
    model.boundary_equation_solve(gvec, k)
    u = model.dirichlet_fun.coefficients
    pts = center + ref.listener_points(size)
    p = model.potential_solve(pts)
    p_ex = ref.exact_field(pts, k, x0)
    eu = np.linalg.norm(u - u_ex) / np.linalg.norm(u_ex)
    ep = np.linalg.norm(p - p_ex) / np.linalg.norm(p_ex)
    assert model.gmres_info["converged"], model.gmres_info
    assert eu < 2e-2 and ep < 2e-2, (eu, ep)


def test_bitwise_deterministic():
    from diffsound_amd import meshgen

    v, f = meshgen.icosphere(3)
    g = ref.geometry(v, f)
    gvec, _ = ref.point_source_data(g, 3.0, ref.X0)
    pts = ref.listener_points(1.0)
    runs = []
    for _ in range(2):
        model = _bem().BEMModel(v, f)
        A, rhs, V = model.assemble(3.0, model._to_internal(gvec, "g"), want_V=True)
        model.boundary_equation_solve(gvec, 3.0)
        runs.append((A.cpu(), rhs.cpu(), V.cpu(), model.dirichlet_fun.coefficients, model.potential_solve(pts)))
    for a, b in zip(*runs):
        a, b = np.asarray(a), np.asarray(b)
        assert a.tobytes() == b.tobytes()


def test_surface_of_box_is_closed_and_outward():
    from diffsound_amd import meshgen

    for n in (3, 4):
        v, f, mesh = _box_surface(n)
        g = ref.geometry(v, f)
        assert len(f) == 2 * 2 * (n * n * 3)
        an = g["area"][:, None] * g["n"]
        assert np.abs(an.sum(0)).max() <= 1e-6 * g["area"].sum()
        vol = (an * g["c"]).sum() / 3
        assert abs(vol / (0.10 * 0.08 * 0.06) - 1) < 1e-5, vol
        for order in (1, 2):
            m2 = mesh.to_high_order(order)
            tri, mids = _bem().surface_of(m2)
            assert tri.shape == (len(f), 3) and (mids is None) == (order == 1)
            x = m2.vertices.double()
            g2 = ref.geometry(x.cpu().numpy(), tri.cpu().numpy())
            assert abs((g2["area"][:, None] * g2["n"] * g2["c"]).sum() / 3 / (0.10 * 0.08 * 0.06) - 1) < 1e-5
            if order == 2:  # the mid-edge nodes sit on the midpoints of (a,b), (b,c), (c,a)
                for e in range(3):
                    mid = (x[tri[:, e]] + x[tri[:, (e + 1) % 3]]) / 2
                    assert float((x[mids[:, e]] - mid).abs().max()) < 1e-6


@pytest.mark.parametrize("order", [1, 2])
def test_mode_neumann_of_synthetic_fields(order):
    bem = _bem()
    _, _, mesh1 = _box_surface(3)
    mesh = mesh1.to_high_order(order)
    surf = bem.surface_of(mesh)
    x = mesh.vertices.double()
    nv = x.shape[0]
    U = torch.zeros((nv, 3, 2), dtype=torch.float64, device=DEV)
    U[:, 2, 0] = 1.0  # u = e_z
    U[:, :, 1] = x    # u = x
    obj = SimpleNamespace(tetmesh=mesh, U_hat=U.reshape(3 * nv, 2))
    un = bem.mode_neumann(obj, surf).cpu().numpy()
    g = ref.geometry(x.cpu().numpy(), surf[0].cpu().numpy())
    assert np.abs(un[:, 0] - g["n"][:, 2]).max() < 1e-12
    assert np.abs(un[:, 1] - (g["c"] * g["n"]).sum(1)).max() < 1e-12


def test_modal_transfer_decays_as_one_over_r():
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, FixedLinear

    v, t = meshgen.kuhn_box(3)
    obj = DiffSoundObj(vertices=torch.from_numpy(v).to(DEV), tets=torch.from_numpy(t).long().to(DEV), mode_num=4,
                       mat=(1070.0, 1.4e9, 0.35, 30.0, 1e-6), order=1, mat_model=FixedLinear, task="gt")
    obj.eigen_decomposition()
    size = float(np.linalg.norm(v.max(0) - v.min(0)))
    center = v.mean(0).astype(np.float64)
    dirs = np.array([[1.0, 0.3, 0.2], [-0.2, 1.0, 0.4], [0.1, -0.3, 1.0], [-0.6, -0.6, -0.5]])
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    R = 20 * size
    pts = np.concatenate([center + R * dirs, center + 2 * R * dirs])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        p = _bem().modal_transfer(obj, pts)
    assert p.shape == (8, 4) and np.isfinite(p).all()
    near_amp = np.abs(p[:4]) * R
    far_amp = np.abs(p[4:]) * 2 * R
    big = near_amp > 1e-3 * near_amp.max()
    assert np.abs(far_amp[big] / near_amp[big] - 1).max() < 0.05, far_amp / near_amp


def _read_element_data(path):
    text = open(path).read()
    views = {}
    for blk in re.findall(r"\$ElementData\n(.*?)\$EndElementData", text, re.S):
        lines = blk.strip().split("\n")
        name = lines[1].strip('"')
        count = int(lines[7])  # 1 string tag, 1 real tag, 3 integer tags (step, components, count)
        vals = np.array([float(l.split()[1]) for l in lines[8:8 + count]])
        views[name] = vals
    nodes = int(text.split("$Nodes\n")[1].split("\n")[0])
    elems = text.split("$Elements\n")[1].split("$EndElements")[0].strip().split("\n")
    tris = np.array([[int(x) for x in l.split()[5:8]] for l in elems[1:]]) - 1
    return nodes, tris, views


def test_api_round_trip_and_loud_errors(tmp_path, monkeypatch):
    bem = _bem()
    from diffsound_amd import meshgen

    v, f = meshgen.icosphere(2)
    model = bem.BEMModel(v.astype(np.float64), f.astype(np.int64))
    g = ref.geometry(v, f)
    gvec, _ = ref.point_source_data(g, 1.5, ref.X0)
    model.boundary_equation_solve(gvec, 1.5)
    assert model.k == 1.5 and model.neumann_fun.coefficients.shape == (len(f),)
    assert model.dirichlet_fun.coefficients.shape == (len(f),) and np.iscomplexobj(model.dirichlet_fun.coefficients)
    assert model.gmres_info["iterations"] > 0 and model.gmres_info["residual"] <= 1e-5
    p = model.potential_solve(np.array([[3.0, 0.0, 0.0], [0.0, -4.0, 1.0]]))
    assert p.shape == (2,) and np.isfinite(p).all()
    for which in ("dirichlet", "neumann"):
        path = str(tmp_path / f"{which}.msh")
        getattr(model, f"export_{which}")(path)
        nodes, tris, views = _read_element_data(path)
        coef = getattr(model, f"{which}_fun").coefficients
        assert nodes == len(v) and np.array_equal(tris, f)
        assert np.array_equal(views[f"{which}.real"], coef.real.astype(np.float64))
        assert np.array_equal(views[f"{which}.imag"], coef.imag.astype(np.float64))
    with pytest.raises(ValueError, match="wave_number"):
        model.boundary_equation_solve(gvec, -1.0)
    with pytest.raises(ValueError, match="neumann_coeff"):
        model.boundary_equation_solve(gvec[:-1], 1.0)
    with pytest.raises(ValueError, match="points"):
        model.potential_solve(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="degenerate"):
        bem.BEMModel(v, np.concatenate([f, [[1, 2, 1]]]))
    with pytest.raises(ValueError, match="out of range"):
        bem.BEMModel(v, np.concatenate([f, [[1, 2, -1]]]))
    monkeypatch.setattr(bem, "BEM_MEMORY_BUDGET_BYTES", 8 * 100 * 100)
    with pytest.raises(MemoryError, match="budget"):
        bem.BEMModel(v, f)
