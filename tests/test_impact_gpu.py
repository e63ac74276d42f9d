"""diffsound_amd.impact.ContactSurface on the device: the gains of a strike on the surface of a small ord-1 box with 8
modes, their gradients with respect to where it is struck, and the ``mode_gain`` keyword of the oscillator modules."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mode_sample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

MAT = (2700.0, 5e10, 0.25, 6.0, 1e-7)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


@functools.lru_cache(maxsize=None)
def _surface():
    """The object, its eigendecomposition and its contact surface: built once, never modified."""
    from diffsound_amd import meshgen
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, FixedLinear
    from diffsound_amd.impact import ContactSurface

    v, t = meshgen.kuhn_box(R.RECOVER_CELLS)
    obj = DiffSoundObj(vertices=torch.from_numpy(v).to(_dev()), tets=torch.from_numpy(t).long().to(_dev()),
                       mode_num=R.RECOVER_MODES, mat=MAT, order=1, mat_model=FixedLinear, task="gt")
    obj.eigen_decomposition()
    return obj, ContactSurface(obj)


def _host_reference(surf, face, bary3, direction):
    """The restatement on the surface's own tables: (out, vec) fp64 for fp32-rounded bary3 and direction."""
    obj = surf.obj
    tets = obj.tetmesh.tets.int().cpu().numpy()
    U = obj.U_hat.cpu().numpy()
    elem, corner = surf._elem32[face].cpu().numpy(), surf._corner[face].cpu().numpy()
    L = np.zeros((len(elem), 4), dtype=np.float32)
    np.put_along_axis(L, corner, bary3.detach().float().cpu().numpy(), 1)
    return R.forward(tets, U, U.shape[1], elem, L, direction.float().cpu().numpy(), with_abs=True)


def test_owners_and_normals_describe_the_surface():
    obj, surf = _surface()
    tets, x = obj.tetmesh.tets.long(), obj.tetmesh.vertices.double()
    nodes = torch.gather(tets[surf._elem32.long()], 1, surf._corner)
    assert torch.equal(nodes, surf.triangles)  # the owner's local corners are the triangle's nodes, in its order
    assert surf.num_faces == 2 * 6 * R.RECOVER_CELLS ** 2
    center = x.mean(0)
    assert bool((((surf._corners.mean(1) - center) * surf.normals).sum(1) > 0).all())  # outward, on a convex body
    assert float((torch.linalg.vector_norm(surf.normals, dim=1) - 1).abs().max()) < 1e-14


def test_amplitude_map_rows_are_the_gains_at_the_centroids():
    _, surf = _surface()
    amap = surf.amplitude_map()
    face = torch.arange(surf.num_faces, device=_dev())
    third = torch.full((surf.num_faces, 3), 1.0 / 3.0, dtype=torch.float64, device=_dev())
    assert amap.shape == (surf.num_faces, R.RECOVER_MODES) and amap.dtype == torch.float64
    assert torch.equal(amap, surf.amplitudes(face, third))
    out, _, aout, _ = _host_reference(surf, face, third, surf.normals)
    K = 2 * 4 + 10  # K_out of tests/test_mode_sample_kernels_gpu.py for N = 4
    assert np.all(np.abs(amap.cpu().numpy() - out) <= R.gamma(K) * aout)
    assert float(amap.abs().max()) > 1e-3  # mass-orthonormal modes of a 1.3 kg box: gains of order 1


def test_normal_is_the_explicit_normal_and_displacement_carries_the_gains():
    _, surf = _surface()
    g = torch.Generator(device="cpu").manual_seed(3)
    face = torch.randint(0, surf.num_faces, (37,), generator=g).to(_dev())
    b = torch.distributions.Dirichlet(torch.ones(3, dtype=torch.float64)).sample((37,)).to(_dev())
    by_name = surf.amplitudes(face, b, "normal")
    assert torch.equal(by_name, surf.amplitudes(face, b, surf.normals[face]))
    one = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=_dev())
    vec = surf.displacement(face, b)
    assert vec.shape == (37, R.RECOVER_MODES, 3)
    assert torch.equal(surf.amplitudes(face, b, one), vec[:, :, 2])  # d = e_z: the products with 0 and 1 are exact
    _, ref_vec, _, avec = _host_reference(surf, face, b, surf.normals[face])
    assert np.all(np.abs(vec.cpu().numpy() - ref_vec) <= R.gamma(2 * 4 + 4) * avec)


def test_locate_finds_the_face_under_a_point_off_the_surface():
    _, surf = _surface()
    cent = surf._corners.mean(1)
    face, b = surf.locate(cent + 1e-3 * surf.normals)
    assert torch.equal(face, torch.arange(surf.num_faces, device=_dev()))
    assert float((b - 1.0 / 3.0).abs().max()) < 1e-9
    # outside the triangle the barycentrics are clamped onto it: far beyond corner 0 along the face, corner 0 itself
    far = surf._corners[:, 0] + 10.0 * (surf._corners[:, 0] - 0.5 * (surf._corners[:, 1] + surf._corners[:, 2]))
    c = surf._corners
    from diffsound_amd.impact import _closest_barycentrics

    clamped = _closest_barycentrics(far, c[:, 0], c[:, 1], c[:, 2])
    assert torch.allclose(clamped, torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=_dev()).expand_as(clamped))


def test_gradient_in_points_against_central_differences():
    """The gains of an ord-1 face are affine in the point while it stays over the face (P1 shape functions, a plane
    projection), so a central difference has no truncation error.  What is left is the kernel's fp32 rounding of L: each
    coordinate moves by at most 2^-24 (L <= 1), a gain by at most 2^-24 W_i with W_i = sum over the face's nodes of
    |n . U[node, :, i]|, and a difference quotient of two such values by 2^-24 W_i / h.  The fp64 roundings are 2^-29
    of that and covered by the factor 1.01.  The analytic gradient carries no fp32 rounding: dN/dL is constant on P1."""
    obj, surf = _surface()
    g = torch.Generator(device="cpu").manual_seed(5)
    face = torch.randint(0, surf.num_faces, (12,), generator=g).to(_dev())
    b = torch.tensor([0.3, 0.3, 0.4], dtype=torch.float64, device=_dev()) + 0.1 * (torch.rand((12, 3), generator=g).double().to(_dev()) - 0.5)
    b = b / b.sum(1, keepdim=True)  # strictly inside: every coordinate in [0.2, 0.5]
    pts = (torch.einsum("pk,pkx->px", b, surf._corners[face]) + 2e-4 * surf.normals[face]).requires_grad_(True)
    r = torch.randn((12, R.RECOVER_MODES), generator=g).double().to(_dev())
    (surf.amplitudes_at(pts) * r).sum().backward()
    assert torch.equal(surf.locate(pts.detach())[0], face)
    h = 1e-3  # the faces' edges are 0.02 to 0.04 long: a coordinate moves by at most 0.05
    Un = torch.einsum("pkcm,pc->pkm", obj.U_hat.reshape(-1, 3, R.RECOVER_MODES)[surf.triangles[face]], surf.normals[face].float().double())
    tol = 1.01 * 2.0 ** -24 * (Un.abs().sum(1) * r.abs()).sum(1) / h
    for c in range(3):
        e = torch.zeros(3, dtype=torch.float64, device=_dev())
        e[c] = h
        with torch.no_grad():
            assert torch.equal(surf.locate(pts + e)[0], face) and torch.equal(surf.locate(pts - e)[0], face)
            fd = ((surf.amplitudes_at(pts + e) - surf.amplitudes_at(pts - e)) * r).sum(1) / (2 * h)
        err = (fd - pts.grad[:, c]).abs()
        print(f"component {c}: worst error / tolerance = {float((err / tol).max()):.3g}; |gradient| up to {float(pts.grad[:, c].abs().max()):.3g}")
        assert bool((err <= tol).all()), (c, float((err / tol).max()))
    assert float(pts.grad.abs().max()) > 100 * float(tol.max())  # the comparison resolves the gradient
    # a displacement along the normal changes nothing: the gradient lies in the face's plane
    assert float(((pts.grad * surf.normals[face]).sum(1)).abs().max()) <= 1e-9 * float(pts.grad.abs().max())


def test_gradient_in_direction_is_the_displacement():
    _, surf = _surface()
    face = torch.tensor([0, 5, surf.num_faces - 1], device=_dev())
    b = torch.tensor([[0.2, 0.3, 0.5]] * 3, dtype=torch.float64, device=_dev())
    d = torch.tensor([0.3, -0.5, 0.8], dtype=torch.float64, device=_dev()).requires_grad_(True)
    r = torch.randn((3, R.RECOVER_MODES), generator=torch.Generator().manual_seed(2)).double().to(_dev())
    (surf.amplitudes(face, b, d) * r).sum().backward()
    vec = surf.displacement(face, b)
    want = torch.einsum("pm,pmc->c", r, vec)
    assert d.grad.shape == (3,) and torch.allclose(d.grad, want, rtol=1e-12, atol=1e-12 * float(want.abs().max()))


def test_position_recovery():
    """Gains at a known interior point of a known face; Adam on bary3 from another point of that face brings the loss
    |c - c*|^2 / |c*|^2 below RECOVER_MARGIN of its start value (the margin's derivation: tests/_mode_sample_ref.py)."""
    _, surf = _surface()
    spot = torch.tensor(R.RECOVER_SPOT, dtype=torch.float64, device=_dev())
    f = int(((surf._corners.mean(1) - spot) ** 2).sum(1).argmin())
    face = torch.tensor([f], device=_dev())
    rank = torch.argsort(torch.argsort(surf.triangles[f]))  # R.RECOVER_* are in the order of ascending node ids
    gains = lambda b: surf.amplitudes(face, b.to(_dev())[:, rank])
    first, last, b = R.recover(gains)
    print(f"recovery on the device: face {f}, start {first:.3g}, end {last:.3g}, ratio {last / first:.3g}, bary3 {b}")
    assert first > 0.1
    assert last <= R.RECOVER_MARGIN * first
    assert np.abs(b - np.array(R.RECOVER_TARGET)).max() < 0.05


def test_errors_come_before_device_work():
    from diffsound_amd.diffelastic.diff_model import DiffSoundObj, FixedLinear
    from diffsound_amd.impact import ContactSurface
    from diffsound_amd import meshgen

    obj, surf = _surface()
    v, t = meshgen.kuhn_box(1)
    fresh = DiffSoundObj(vertices=torch.from_numpy(v).to(_dev()), tets=torch.from_numpy(t).long().to(_dev()), mode_num=2,
                         mat=MAT, order=1, mat_model=FixedLinear, task="gt")
    with pytest.raises(ValueError, match="U_hat"):
        ContactSurface(fresh)
    face = torch.tensor([0, 1], device=_dev())
    b = torch.tensor([[0.2, 0.3, 0.5]] * 2, dtype=torch.float64, device=_dev())
    with pytest.raises(ValueError, match="bary3 must be"):
        surf.amplitudes(face, b[:1])
    with pytest.raises(ValueError, match="out of range"):
        surf.amplitudes(face + surf.num_faces - 1, b)
    with pytest.raises(ValueError, match="out of range"):
        surf.amplitudes(face - 1, b)
    with pytest.raises(ValueError, match="non-finite"):
        surf.amplitudes(face, b * float("nan"))
    with pytest.raises(ValueError, match="sum to 1"):
        surf.amplitudes(face, b * 1.001)
    surf.amplitudes(face, b * (1 + 5e-5))  # inside the 1e-4 tolerance
    with pytest.raises(ValueError, match="direction"):
        surf.amplitudes(face, b, torch.ones((5, 3), device=_dev()))
    with pytest.raises(ValueError, match="direction"):
        surf.amplitudes(face, b, "tangent")
    with pytest.raises(ValueError, match="non-finite"):
        surf.amplitudes(face, b, torch.tensor([0.0, float("inf"), 1.0], device=_dev()))
    with pytest.raises(ValueError, match="points must be"):
        surf.locate(torch.zeros((4, 2), device=_dev()))
    with pytest.raises(RuntimeError, match="HIP"):
        surf.amplitudes(face.cpu(), b.cpu())
    with pytest.raises(RuntimeError, match="HIP"):
        surf.amplitudes(face, b, torch.ones(3))
    with pytest.raises(RuntimeError, match="HIP"):
        surf.locate(torch.zeros((4, 3)))


def _modules():
    from diffsound_amd.ddsp.oscillator import DampedOscillator, GTDampedOscillator, TraditionalDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material

    A, m, S, sr = 2, R.RECOVER_MODES, 800, 32000
    forces = torch.zeros((A, 16), device=_dev())
    forces[:, 0] = 1
    torch.manual_seed(4)
    mat = Material(MAT)
    freq = torch.linspace(400.0, 4000.0, m, device=_dev()).reshape(m, 1)
    trad = TraditionalDampedOscillator(forces, A, m, S, sr, mat).cuda()
    damp = DampedOscillator(forces, A, m, S, sr, [20, 16000], mat).cuda()
    gt = GTDampedOscillator(forces, A, m, S, sr, [20, 16000], mat).cuda()
    return A, m, (("traditional", lambda **k: trad(freq, **k)), ("damped", lambda **k: damp(freq, **k)),
                  ("gt", lambda **k: gt(**k)), ("gt time-varying", lambda **k: gt(non_linear_rate=0.01, **k)))


def test_mode_gain_none_and_ones_keep_the_bits():
    A, m, calls = _modules()
    ones = torch.ones((A, m), dtype=torch.float64, device=_dev())
    for name, call in calls:
        with torch.no_grad():
            plain = call()
            assert torch.equal(call(mode_gain=None), plain), name
            assert torch.equal(call(mode_gain=ones), plain), name
            assert not torch.equal(call(mode_gain=2 * ones), plain), name
        with pytest.raises(ValueError, match="mode_gain"):
            call(mode_gain=ones[:, :-1])


def test_a_strike_renders_and_its_position_gets_a_gradient():
    _, surf = _surface()
    A, m, calls = _modules()
    face = torch.tensor([3, 11], device=_dev())
    b = torch.tensor([[0.2, 0.3, 0.5], [0.4, 0.4, 0.2]], dtype=torch.float64, device=_dev(), requires_grad=True)
    gain = surf.amplitudes(face, b)
    for name, call in calls[:3]:
        b.grad = None
        sig = call(mode_gain=gain)
        assert sig.shape[0] == A and bool(torch.isfinite(sig).all())
        (sig ** 2).mean().backward(retain_graph=True)
        assert b.grad is not None and bool(torch.isfinite(b.grad).all()) and float(b.grad.abs().max()) > 0, name
