"""The kernels of diffsound_amd/csrc/bem.hip behind ds_bem_geometry, ds_bem_assemble and ds_bem_potential, entry by entry
against the fp64 restatement of tests/_bem_ref.py evaluated from the kernel's own inputs (the fp32 vertices and points
cast up), up to kr = 100.

Every error is a complex error divided by the scale of its own entry (_bem_ref.pair_scales / point_scales: the magnitude
of what the entry sums), never by a matrix maximum.  No tolerance is fixed here: for each case and each quantity (V, K,
regular and near pairs apart; rhs; the potential) the restatement is run in fp32 on the same inputs, its largest scaled
error against the fp64 run is that case's fp32 level, and the kernel's bound is MARGIN = 4 times it (another summation
order, the hardware rsq, the hardware sine and cosine in revolutions).  Each case prints level, bound and kernel error
(``pytest -s``).  A pair within 1e-5 of the near threshold may be classified either way and is left out; the cases are
chosen so that there is none (tests/test_bem_ref_cpu.py), and a case may leave out at most 0.5 %.

Cases (_bem_ref.mesh): A, the 80-face icosphere of radius 0.1 at k = 0, 1, 30, 300, 500 (kr up to 0, 0.2, 6, 60, 100) and
translated off the origin at k = 300; B, a 0.1 x 0.03 x 0.005 plate (stretched faces, stacked near-parallel near pairs,
axis-aligned planes: points exactly in a face's plane and on an edge's line) at k = 0, 30, 300; C, the first n face
records of the 320-face icosphere through the C ABI with n = 1, 7, 9, 255, 256, 257 (row band and column tile edges),
lda = ldv = n + 3 in NaN-filled buffers, with and without V."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bem_ref as R  # noqa: E402
from _guarded import PAD, Guarded, _lib, _up  # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a HIP device")]

SURFACES = [("A", False), ("A", True), ("B", False), ("C", False)]
AB = R.CASES_A + R.CASES_B
AB_IDS = [R.case_id(c) for c in AB]


@functools.lru_cache(maxsize=None)
def _model(name, shifted):
    """(model, fp32 vertices, faces in the model's internal order)."""
    from diffsound_amd.diffelastic import bem

    v, f = R.mesh(name, shifted)
    model = bem.BEMModel(v, f)
    return model, v, f[model._perm.cpu().numpy()]


def _coefficients(m, k):
    gv, uv = R.coefficients(m, 3)
    if k == 0:  # the static problem with real data: every imaginary part must be exactly zero
        gv, uv = gv.real.astype(np.complex64), uv.real.astype(np.complex64)
    return gv, uv


@functools.lru_cache(maxsize=None)
def _truth(name, k, shifted):
    model, v, f = _model(name, shifted)
    if name == "C":
        f = f[:max(R.C_SIZES)]
    gv, uv = _coefficients(len(f), k)
    return gv, uv, R.assembly_truth(v, f, k, gv)


def _report(case, what, level, err, count):
    bound = R.MARGIN * level
    print(f"LEVEL bem {case} {what}: fp32 level {level:.3g} bound {bound:.3g} kernel {err:.3g} ({count} entries)")
    return err <= bound


def _check_entries(case, t, n, A, V, area32):
    """V and K = A + diag(area) / 2 of the kernel against the leading n x n block of the truth ``t``."""
    s = np.s_[:n, :n]
    near, skip = t["near"][s], t["skip"][s]
    assert skip.sum() == 0 and skip.sum() <= 0.005 * n * n
    assert np.all(np.diag(A).real == -0.5 * area32) and np.all(np.diag(A).imag == 0)  # K_ii = 0 exactly
    K = A + np.diag(0.5 * area32).astype(np.complex64)
    levels = R.assembly_levels(t, n)
    ok = True
    for cat, mask in R._categories(near, skip).items():
        ok &= _report(case, f"V/{cat}", levels["V", cat], R.worst(V, t["V"][s], t["sV"][s], mask), int(mask.sum()))
        ok &= _report(case, f"K/{cat}", levels["K", cat], R.worst(K, t["K"][s], t["sK"][s], mask), int(mask.sum()))
    return ok


def _check_rhs(case, t, n, gv, rhs):
    s = np.s_[:n, :n]
    want = t["V"][s] @ gv[:n].astype(np.complex128)
    scale = t["sV"][s] @ np.abs(gv[:n])
    level = R.worst(t["V32"][s] @ gv[:n], want, scale)
    return _report(case, "rhs", level, R.worst(rhs, want, scale), n)


@pytest.mark.parametrize("name,shifted", SURFACES, ids=["A", "A-shifted", "B", "C"])
def test_geometry_record(name, shifted):
    """All 48 floats of every face record against the fp64 record of the same fp32 vertices, at the counted bounds of
    _bem_ref.record_bounds (in units of the fp32 rounding of the face's largest coordinate, or of its diameter where
    only edge vectors enter); the vertices and the zero tail exact."""
    model, v, f = _model(name, shifted)
    g = R.geometry(v, f)
    rec = model.rec.cpu().numpy().astype(np.float64)
    assert rec.shape == (len(f), 48)
    want, bound = R.face_records(g), R.record_bounds(g)
    err = np.abs(rec - want)
    fields = dict(q=np.s_[:, 0:18], w=np.s_[:, 18:24], n=np.s_[:, 24:27], c=np.s_[:, 27:30], h=np.s_[:, 30], area=np.s_[:, 31])
    print("RATIO bem geometry", name, "shifted" if shifted else "", " ".join(f"{k} {(err[s] / bound[s]).max():.3g}" for k, s in fields.items()))
    assert np.all(err <= bound), np.argwhere(err > bound)[:5]
    assert np.all(rec[:, 32:41] == want[:, 32:41]) and np.all(rec[:, 41:] == 0)


@pytest.mark.parametrize("case", AB, ids=AB_IDS)
def test_assembly_per_entry(case):
    name, k, shifted = case
    model, v, f = _model(name, shifted)
    gv, uv, t = _truth(*case)
    m = model.m
    A, rhs, V = model.assemble(k, _up(gv), want_V=True)
    A, rhs, V = A[:, :m].cpu().numpy(), rhs.cpu().numpy(), V[:, :m].cpu().numpy()
    area32 = model.area.cpu().numpy()
    ok = _check_entries(R.case_id(case), t, m, A, V, area32)
    ok &= _check_rhs(R.case_id(case), t, m, gv, rhs)
    if k == 0:
        assert np.all(A.imag == 0) and np.all(V.imag == 0) and np.all(rhs.imag == 0)
    assert ok


@functools.lru_cache(maxsize=None)
def _point_truth(case):
    name, k, shifted = case
    gv, uv, t = _truth(*case)
    g = t["g"]
    pts, kinds = R.potential_points(g, k)
    d2, t2 = R._point_d2_t2(g, pts)
    near = d2 < t2
    model, v, f = _model(name, shifted)
    want = R.potential(g, k, gv, uv, pts)
    p32 = R.potential(R.geometry(v, f, np.float32), k, gv, uv, pts, near=near)
    return pts, kinds, want, p32, R.point_scales(g, k, pts, gv, uv, near), R.borderline_points(g, pts)


@pytest.mark.parametrize("case", AB, ids=AB_IDS)
def test_potential_per_point(case):
    """257 points (two workgroups, the second with one point), then one point of every kind alone (np = 1)."""
    name, k, shifted = case
    model, *_ = _model(name, shifted)
    gv, uv, _ = _truth(*case)
    pts, kinds, want, p32, scale, skip = _point_truth(case)
    assert skip.sum() == 0 and len(pts) == 257
    level = R.worst(p32, want, scale)
    g_d, u_d = _up(gv), _up(uv)
    out = Guarded((257, 2))
    _hip, lib = _lib()
    pd = _up(pts.astype(np.float32))
    _hip.check(lib.ds_bem_potential(model.rec.data_ptr(), model.m, k, g_d.data_ptr(), u_d.data_ptr(), pd.data_ptr(), 257,
                                    out.ptr, _hip.stream_ptr()), "ds_bem_potential")
    out.check("potential")
    got = out.numpy()[:, 0] + 1j * out.numpy()[:, 1]
    err = np.abs(got - want) / scale
    print("RATIO bem potential by kind", R.case_id(case),
          " ".join(f"{kd} {err[kinds == kd].max() / (R.MARGIN * level):.3g}" for kd in sorted(set(kinds))))
    ok = _report(R.case_id(case), "potential np=257", level, float(err.max()), 257)
    if k == 0:
        assert np.all(got.imag == 0)
    for kd in sorted(set(kinds)):
        p = int(np.nonzero(kinds == kd)[0][-1])
        one = model._potential(k, g_d, u_d, pts[p:p + 1]).cpu().numpy()
        assert one.shape == (1,) and one[0] == got[p].astype(np.complex64), (kd, one, got[p])  # same point, same bits
    assert ok


@functools.lru_cache(maxsize=None)
def _raw_assemble(n, with_V):
    """ds_bem_assemble on the first n records of case C: A (and V) with lda = ldv = n + 3 inside NaN-filled buffers."""
    model, *_ = _model("C", False)
    gv, _, _ = _truth("C", R.C_K, False)
    _hip, lib = _lib()
    ld = n + 3
    nbytes = lib.ds_bem_assemble_workspace_bytes(n)
    assert nbytes == 8 * n * ((n + 255) // 256)
    bufs = dict(A=Guarded((n, ld, 2)), V=Guarded((n, ld, 2)), rhs=Guarded((n, 2)), work=Guarded((nbytes // 4,)))
    g_d = _up(gv[:n])
    _hip.check(lib.ds_bem_assemble(model.rec.data_ptr(), n, R.C_K, g_d.data_ptr(), bufs["A"].ptr, ld,
                                   bufs["V"].ptr if with_V else None, ld, bufs["rhs"].ptr, bufs["work"].ptr,
                                   _hip.stream_ptr()), "ds_bem_assemble")
    torch.cuda.synchronize()
    return bufs


def _matrix(buf, n):
    """The n x n complex part of a guarded (n, n + 3, 2) buffer, after checking that nothing else was written."""
    whole = buf.buf.cpu().numpy()
    assert np.isnan(whole[:PAD]).all() and np.isnan(whole[PAD + buf.n:]).all(), "written outside the buffer"
    a = buf.numpy()
    assert np.isnan(a[:, n:]).all(), "padding columns written"
    assert np.isfinite(a[:, :n]).all(), "not every entry written"
    return a[:, :n, 0] + 1j * a[:, :n, 1]


@pytest.mark.parametrize("n", R.C_SIZES)
def test_leading_records_padding_and_null_V(n):
    model, *_ = _model("C", False)
    gv, _, t = _truth("C", R.C_K, False)
    first, second = _raw_assemble(n, True), _raw_assemble(n, False)
    A, V = _matrix(first["A"], n), _matrix(first["V"], n)
    for b in (first, second):
        b["rhs"].check("rhs")
        b["work"].check("workspace")
    assert second["V"].untouched()
    for key in ("A", "rhs"):  # A and rhs do not depend on whether V is asked for
        assert torch.equal(first[key].buf[PAD:-PAD].view(torch.int32), second[key].buf[PAD:-PAD].view(torch.int32)), key
    rhs = first["rhs"].numpy()
    case = f"C-n{n}"
    ok = _check_entries(case, t, n, A.astype(np.complex64), V, model.area.cpu().numpy()[:n])
    ok &= _check_rhs(case, t, n, gv, rhs[:, 0] + 1j * rhs[:, 1])
    assert ok
