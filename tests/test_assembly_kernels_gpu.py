"""The numeric assembly (ds_assemble_kml: tet_geometry_kernel, assemble_blocks_kernel<4|10>) and ds_combine_material, per
entry against the fp64 references of tests/_assembly_ref.py (anchored without a GPU in tests/test_assembly_ref_cpu.py).
Run with  pytest -m gpu -s  to see the measured err / bound of every case.

Measured on the MI355X when these tests were written (worst err / bound over the case; (b), (c): the largest of K_lambda,
K_mu, M_s) - what a rewrite of the assembly is held to:

  case              nnzb  % 256  longest list   (a)     (b)     (c)
  single-o1           16     16       1         0       0       0
  single-o2          100    100       1         0       0.026   0.011
  islands-16         256      0       1         0.095   0.039   0.046
  islands-17         272     16       1         0.086   0.042   0.073
  islands-32         512      0       1         0.108   0.041   0.103
  box2-o2           2441    137      24         0.118   0.193   0.074
  box3-o2           7525    101      24         0.107   0.197   0.086
  box3-o1            622    110      24         0.107   0.162   0.063
  graded            2441    137      24         0.055   0.097   0.035
  flipped-box2-o2   2441    137      24         0.118   0.193   0.099
  flipped-box3-o1    622    110      24         0.107   0.156   0.081
  unused             223    223      24         0.118   0.174   0.068

(d) flipped against twin 0.069, reorder 0 (the same bits); (e) 0.19; (f) k32 0.995 (the bound is half an fp32 ulp), dinv 0.485."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _assembly_ref as R  # noqa: E402
from diffsound_amd import fem_tables, meshgen  # noqa: E402
from oracle import fem  # noqa: E402  (mesh lifting and the Lame constants only)

pytestmark = pytest.mark.gpu

RHO = 2700.0
LAM, MU = fem.lame(5e10, 0.25)
MATERIALS = {"steel-like": (LAM, MU), "no-lambda": (0.0, MU), "soft-shear": (LAM, 1e-3 * MU)}
PAD = 9 * 256  # doubles behind the last slot of the raw entry point's buffers

CASES = ["single-o1", "single-o2", "islands-16", "islands-17", "islands-32", "box2-o2", "box3-o2", "box3-o1", "graded",
         "flipped-box2-o2", "flipped-box3-o1", "unused"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    return torch.device("cuda:0")


def _box(cells, order):
    v, t = meshgen.kuhn_box(cells)
    v, t = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), order)
    return v.numpy().astype(np.float32), t.numpy()


def _mesh(name):
    """(verts float32, tets int64, order) of a case."""
    if name.startswith("single"):
        order = int(name[-1])
        v = (np.array([[1, 0, 0], [1, 2, 0], [0.5, 1, 4], [0, 0, 0]]) + np.array([0.25, -0.5, 2.0])).astype(np.float32)
        v, t = fem.to_high_order(torch.from_numpy(v), torch.tensor([[0, 1, 2, 3]]), order)
        return v.numpy().astype(np.float32), t.numpy(), order
    if name.startswith("islands"):
        n = int(name.split("-")[1])
        return R.islands(n, seed=n) + (1,)
    if name.startswith("box"):
        order = int(name[-1])
        return _box(int(name[3]), order) + (order,)
    if name == "graded":
        v, t = _box(2, 2)
        return R.graded_vertices(v), t, 2
    if name.startswith("flipped-"):
        v, t, order = _mesh(name[len("flipped-"):])
        return v, R.flip_tets(t, order), order
    if name == "unused":
        v, t = _box(2, 1)
        v, t, _ = R.with_unused_nodes(v, t)
        return v, t, 1
    raise KeyError(name)


def _tables(order):
    return fem_tables.stiffness_table(order), fem_tables.mass_table(order, RHO)


def _host(sysd):
    """The kernel's arrays on the host: (rowptr, colidx, dense dict Kl / Km / Ms, tetgeo)."""
    rp, ci = sysd.rowptr.cpu().numpy(), sysd.colidx.cpu().numpy()
    assert rp.size == sysd.nv + 1 and ci.size == sysd.nnzb and R.pattern_is_clean(rp, ci)
    got = dict(Kl=R.bsr_to_dense(rp, ci, sysd.klam.cpu().numpy()), Km=R.bsr_to_dense(rp, ci, sysd.kmu.cpu().numpy()),
               Ms=R.bsr_to_dense(rp, ci, sysd.ms.cpu().numpy()))
    return rp, ci, got, sysd._tetgeo.cpu().numpy()


def _own_reference(sysd, t, order, tables=None):
    """assemble_from_geometry on the kernel's own geometry."""
    dtab, mtab = _tables(order) if tables is None else tables
    return R.assemble_from_geometry(sysd._tetgeo.cpu().numpy(), t, order, dtab, mtab, nv=sysd.nv)


def _geometry_ratio(sysd, v, t, order):
    """(worst |tetgeo - exact| / (16 2^-53 bound), where, exact geometry, its bound)."""
    geo, gb = R.tet_geometry_exact(v, t, order)
    r = R.worst_ratio(sysd._tetgeo.cpu().numpy(), geo, R.GEO_FACTOR * R.U53 * gb)
    return r, geo, gb


_CACHE = {}


def _case(name, dev):
    """One TetSystem per case (caller's numbering), with its references; built once per module and left unchanged."""
    if name not in _CACHE:
        from diffsound_amd.modal_ops import TetSystem

        v, t, order = _mesh(name)
        sysd = TetSystem(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), order, RHO, reorder=False)
        torch.cuda.synchronize()
        dtab, mtab = _tables(order)
        # the tables the kernel read are the documented ones, bit for bit
        assert np.array_equal(sysd.dtab.cpu().numpy(), dtab) and np.array_equal(sysd.mtab.cpu().numpy(), mtab)
        assert np.array_equal(sysd.vertices.cpu().numpy(), v) and np.array_equal(sysd.tets.cpu().numpy(), t)
        rp, ci, got, tetgeo = _host(sysd)
        own = _own_reference(sysd, t, order)
        geo, gb = R.tet_geometry_exact(v, t, order)
        exact = R.assemble_from_geometry(geo, t, order, dtab, mtab, nv=sysd.nv, dgeo=R.GEO_FACTOR * R.U53 * gb)
        _CACHE[name] = dict(v=v, t=t, order=order, sys=sysd, rp=rp, ci=ci, got=got, tetgeo=tetgeo, own=own, geo=geo, gb=gb,
                            exact=exact)
    return _CACHE[name]


@pytest.fixture(scope="module", params=CASES)
def case(request, dev):
    return dict(_case(request.param, dev), name=request.param)


# ---------------------------------------------------------------------------------------------------------------- a. geometry

def test_geometry_against_exact(case):
    """sys._tetgeo per tet and per scalar against exact rational arithmetic on the same fp32 coordinates:
    |got - exact| <= 16 * 2^-53 * bound, bound the running-error magnitude of the cofactor formulas (_assembly_ref.GEO_FACTOR
    derives the 16).  On ``graded`` the bound is large where cond(A) is."""
    r, at = R.worst_ratio(case["tetgeo"], case["geo"], R.GEO_FACTOR * R.U53 * case["gb"])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.nanmax(np.where(case["geo"] != 0, R.U53 * case["gb"] / np.abs(case["geo"]), 0.0))
    print(f"(a) {case['name']}: worst err / bound {r:.3f} at tet, scalar {at}; largest 2^-53 bound / |value| {rel:.2e}")
    assert r <= 1
    assert (case["tetgeo"][:, 12] > 0).all()  # |det|, also on the negatively oriented elements


# ---------------------------------------------------------------------------------------------------------------- b. blocks

def test_blocks_against_own_geometry(case):
    """klam, kmu, ms per entry against the reference on the kernel's OWN geometry: |got - ref| <= (nterms + 8) 2^-53 mag
    (_assembly_ref.block_bounds).  No conditioning in it: a lost, doubled or misplaced slot, a wrong (a, b) decode or a wrong
    transpose is an error of order mag."""
    sysd, own, got = case["sys"], case["own"], case["got"]
    nc = own["ncontrib"]
    cptr = sysd.cptr.cpu().numpy().astype(np.int64)
    rows = R.bsr_rows(case["rp"])
    print(f"(b) {case['name']}: nv {sysd.nv} T {sysd.T} nnzb {sysd.nnzb} nnzb % 256 {sysd.nnzb % 256} "
          f"longest contribution list {int(np.diff(cptr).max())}")
    # the pattern covers every block that has a contribution; its contribution lists are as long as the reference's
    mask = np.zeros_like(nc, dtype=bool)
    mask[rows, case["ci"]] = True
    assert mask[nc > 0].all()
    assert np.array_equal(np.diff(cptr), nc[rows, case["ci"]])
    for k in ("Kl", "Km", "Ms"):  # a structural block without a contribution holds zeros
        assert (got[k][mask & (nc == 0)] == 0).all()
    ratios = R.block_ratios(got, own)
    print(f"(b) {case['name']}: worst err / bound {({k: (round(v[0], 4), v[1]) for k, v in ratios.items()})}")
    assert all(np.isfinite(got[k]).all() for k in got)
    assert all(r[0] <= 1 for r in ratios.values()), ratios


# ---------------------------------------------------------------------------------------------------------------- c. end to end

def test_blocks_end_to_end(case):
    """The same arrays against the reference on the EXACT geometry: the bound of (b) plus the geometry bound of (a) propagated
    through H to first order, term by term (sum |D| (dG |G| + |G| dG) J + sum |D| |G| |G| dJ - never more than
    2 relerr(G) mag + relerr(J) mag)."""
    exact, got = case["exact"], case["got"]
    bb = R.block_bounds(exact)
    bounds = {k: bb[k] + exact[k + "_dgeo"] for k in bb}
    ratios = R.block_ratios(got, exact, bounds)
    with np.errstate(divide="ignore", invalid="ignore"):
        width = {k: float(np.nanmax(np.where(exact[k + "_mag"] > 0, bounds[k] / exact[k + "_mag"], 0.0))) for k in bb}
    print(f"(c) {case['name']}: worst err / bound {({k: (round(v[0], 4), v[1]) for k, v in ratios.items()})}; "
          f"largest bound / mag {({k: f'{w:.1e}' for k, w in width.items()})}")
    assert all(r[0] <= 1 for r in ratios.values()), ratios


# ---------------------------------------------------------------------------------------------------------------- d. metamorphic

@pytest.mark.parametrize("name", ["box2-o2", "box3-o1"])
def test_flipped_against_twin(name, dev):
    """A mesh with every third tet's local order swapped v1 <-> v2 (det changes sign) against its unflipped twin, kernel against
    kernel, per entry within the sum of their (b) bounds plus what the two geometry kernels may differ by on the swapped tets
    (_assembly_ref.flip_geometry_allowance: without it an entry whose exact value is 0 fails - measured on box3-o1, block
    (61, 56): 5.5e-21 in one order, -5.5e-21 in the other, from a cofactor that vanishes exactly and leaves a residue of the
    fused multiply-add in one corner order only; the (b) bounds there are 1e-34).  The twin is the unflipped tets with the tables relabelled on the
    swapped ones (_assembly_ref.flip_twin says why the same tables cannot do): two assemblies of the unflipped sub-meshes, one
    with the tables as they are, one with the swapped tables, added.  The P1 stiffness table IS symmetric under the swap: there
    the flipped mesh is also compared with the plain unflipped case."""
    from diffsound_amd.modal_ops import TetSystem

    flipped, plain = _case("flipped-" + name, dev), _case(name, dev)
    v, t, order = plain["v"], plain["t"], plain["order"]
    mask = R.flip_mask(t.shape[0])
    assert (np.sign(R.signed_dets(v, flipped["t"], order)) == np.where(mask, -1, 1) * np.sign(R.signed_dets(v, t, order))).all()
    dtab, mtab = _tables(order)
    s, p = list(R.FLIP_SLOTS[order]), [1, 0, 2, 3]
    dsw = np.ascontiguousarray(dtab[s][:, p][:, :, s][:, :, :, p])
    msw = np.ascontiguousarray(mtab[s][:, s])
    vd = torch.from_numpy(v).to(dev)
    twin = {k: 0.0 for k in ("Kl", "Km", "Ms")}
    bounds = R.block_bounds(flipped["own"])
    allow = R.flip_geometry_allowance((plain["geo"], plain["gb"], t), (flipped["geo"], flipped["gb"], flipped["t"]), order, dtab,
                                      mtab, mask, plain["sys"].nv)
    bounds = {k: bounds[k] + allow[k] for k in bounds}
    for sel, tabs in ((~mask, (dtab, mtab)), (mask, (dsw, msw))):
        sub = TetSystem(vd, torch.from_numpy(t[sel]).to(dev), order, RHO, reorder=False)
        sub.dtab, sub.mtab = torch.from_numpy(tabs[0]).to(dev), torch.from_numpy(tabs[1]).to(dev)
        sub.assemble()
        torch.cuda.synchronize()
        assert sub.nv == plain["sys"].nv
        _, _, got, _ = _host(sub)
        b = R.block_bounds(_own_reference(sub, t[sel], order, tabs))
        for k in twin:
            twin[k] = twin[k] + got[k]
            bounds[k] = bounds[k] + b[k]
    ratios = R.block_ratios(flipped["got"], twin, bounds)
    print(f"(d) flipped-{name} against its twin: worst err / bound {({k: (round(r[0], 4), r[1]) for k, r in ratios.items()})}")
    assert all(r[0] <= 1 for r in ratios.values()), ratios
    if order == 1:
        assert np.array_equal(dsw, dtab)
        bp = R.block_bounds(plain["own"])
        bf = R.block_bounds(flipped["own"])
        direct = {k: R.worst_ratio(flipped["got"][k], plain["got"][k], bp[k] + bf[k] + allow[k]) for k in ("Kl", "Km")}
        print(f"(d) flipped-{name} against {name}, same tables: {({k: (round(r[0], 4), r[1]) for k, r in direct.items()})}")
        assert all(r[0] <= 1 for r in direct.values()), direct


@pytest.mark.parametrize("name", ["box2-o2", "box3-o2", "graded", "unused"])
def test_reorder_is_transparent_per_entry(name, dev):
    """reorder=True against reorder=False through to_scipy(), per entry within the sum of the two (b) bounds."""
    from diffsound_amd.modal_ops import TetSystem

    c = _case(name, dev)
    nv = c["sys"].nv
    s1 = TetSystem(torch.from_numpy(c["v"]).to(dev), torch.from_numpy(c["t"]).to(dev), c["order"], RHO, reorder=True)
    perm = s1.perm.cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(nv))
    Kl, Km, Ms = s1.to_scipy()
    blocks = lambda A: A.toarray().reshape(nv, 3, nv, 3).transpose(0, 2, 1, 3)
    got1 = dict(Kl=blocks(Kl), Km=blocks(Km), Ms=Ms.toarray())
    bb = R.block_bounds(c["own"])
    ratios = R.block_ratios(got1, c["got"], {k: 2 * bb[k] for k in bb})
    print(f"(d) {name} reorder=True against reorder=False: moved {int((perm != np.arange(nv)).sum())} of {nv} nodes; "
          f"worst err / bound {({k: (round(r[0], 4), r[1]) for k, r in ratios.items()})}")
    assert all(r[0] <= 1 for r in ratios.values()), ratios


# ---------------------------------------------------------------------------------------------------------------- e. refresh

def _check_system(sysd, v, t, order, what):
    """(a) and (b) on a system: its geometry against exact arithmetic, its blocks against the reference on its geometry."""
    assert np.array_equal(sysd.vertices.cpu().numpy(), v) and np.array_equal(sysd.tets.cpu().numpy(), t)
    (ra, at), _, _ = _geometry_ratio(sysd, v, t, order)
    _, _, got, _ = _host(sysd)
    ratios = R.block_ratios(got, _own_reference(sysd, t, order))
    print(f"(e) {what}: geometry err / bound {ra:.3f} at {at}; blocks {({k: (round(r[0], 4), r[1]) for k, r in ratios.items()})}")
    assert ra <= 1 and all(r[0] <= 1 for r in ratios.values()), (ra, ratios)
    return got


def test_refresh_and_corner_level(dev):
    """assemble(new_vertices) on box2-o2 with the vertices jittered by 1 % of a cell: the fine level and the corner-node level
    (P1 on the corner sub-mesh) match their references on the NEW coordinates per entry; P^T K P of the fine level's blocks
    matches, per entry, the P1 assembly with the P2 tables restricted to the corner functions (the Galerkin identity; with the
    project's own P1 table it holds to the tables' fp32 rounding only, printed); with_own_values() gives the same bits."""
    from diffsound_amd.modal_ops import TetSystem

    v, t, order = _mesh("box2-o2")
    sysd = TetSystem(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), order, RHO, reorder=False)
    lvl = sysd.coarse_level()
    assert lvl is not None
    before = sysd.klam.clone()
    h = np.array([0.10, 0.08, 0.06]) / 2
    v2 = (v.astype(np.float64) + 0.01 * h * np.random.default_rng(11).uniform(-1, 1, v.shape)).astype(np.float32)
    sysd.assemble(torch.from_numpy(v2).to(dev))
    torch.cuda.synchronize()
    assert not torch.equal(before, sysd.klam)
    got = _check_system(sysd, v2, t, order, "box2-o2 refreshed")
    # the corner sub-mesh, built here
    cs = list(fem_tables.CORNER_SLOTS[2])
    corners = np.unique(t[:, cs])
    cid = np.full(v.shape[0], -1, dtype=np.int64)
    cid[corners] = np.arange(corners.size)
    tc = cid[t[:, cs]]
    csys = lvl["sys"]
    assert np.array_equal(lvl["corners"].cpu().numpy(), corners)
    gotc = _check_system(csys, v2[corners], tc, 1, "corner-node level after the refresh")
    # P^T K P: P copies a corner's value and averages a mid-edge node's end points
    nv, nvc = v.shape[0], corners.size
    P = np.zeros((nv, nvc))
    P[corners, np.arange(nvc)] = 1.0
    for slot, (p_, q_) in fem_tables._MID.items():
        P[t[:, slot], cid[t[:, cs[p_]]]] = 0.5
        P[t[:, slot], cid[t[:, cs[q_]]]] = 0.5
    assert np.array_equal(P.sum(1), np.ones(nv))
    Ploc = np.zeros((10, 4))
    for slot, k in fem_tables._CORNER.items():
        Ploc[slot, k] = 1.0
    for slot, (p_, q_) in fem_tables._MID.items():
        Ploc[slot, p_] = Ploc[slot, q_] = 0.5
    d2, m2 = _tables(2)
    d1r = np.einsum("ac,akbl,bd->ckdl", Ploc, d2, Ploc)
    m1r = np.einsum("ac,ab,bd->cd", Ploc, m2, Ploc)
    print(f"(e) restricted P2 mass table against the P1 mass table: {np.abs(m1r - _tables(1)[1]).max() / np.abs(m1r).max():.2e}")
    fine_own = _own_reference(sysd, t, 2)
    restricted = R.assemble_from_geometry(sysd._tetgeo.cpu().numpy(), tc, 1, d1r, m1r, nv=nvc)
    bfine = R.block_bounds(fine_own)
    ptkp = lambda A: np.einsum("pa,pq...,qb->ab...", P, A, P)
    # (every product with P is exact - its entries are 1 and 1/2 - so P^T . P carries the fine bounds over; the sum behind a
    # coarse block has at most nsum terms and rounds that often relative to the same magnitudes)
    nsum = int((P > 0).sum(0).max()) ** 2
    ratios = {}
    for k in ("Kl", "Km", "Ms"):
        bound = ptkp(bfine[k]) + nsum * R.U53 * ptkp(fine_own[k + "_mag"]) + 8 * R.U53 * restricted[k + "_mag"]
        ratios[k] = R.worst_ratio(ptkp(got[k]), restricted[k], bound)
    print(f"(e) P^T K P against the restricted P1 assembly: {({k: (round(r[0], 4), r[1]) for k, r in ratios.items()})}")
    assert all(r[0] <= 1 for r in ratios.values()), ratios
    # ... and against the corner-node level itself to the tables' rounding
    gap = max(float(np.abs(ptkp(got[k]) - gotc[k]).max() / np.abs(gotc[k]).max()) for k in ("Kl", "Km", "Ms"))
    print(f"(e) P^T K P against the corner-node level's own arrays (relative to the largest entry): {gap:.2e}")
    assert gap < 1e-6
    own = sysd.with_own_values()
    torch.cuda.synchronize()
    for a in ("klam", "kmu", "ms", "_tetgeo"):
        assert torch.equal(getattr(own, a), getattr(sysd, a)) and getattr(own, a).data_ptr() != getattr(sysd, a).data_ptr()
    oc = own.coarse_level()["sys"]
    assert torch.equal(oc.klam, csys.klam) and torch.equal(oc.kmu, csys.kmu) and torch.equal(oc.ms, csys.ms)


# ---------------------------------------------------------------------------------------------------------------- f. material

def _f32_bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("material", list(MATERIALS))
@pytest.mark.parametrize("name", ["box2-o2", "graded", "unused", "islands-17"])
def test_combine_material(name, material, dev):
    """ds_combine_material (and ds_pack_groups behind it, as HipModalOps calls them) on the case's assembled arrays:
    k32 one fp32 rounding of lam klam + mu kmu (fused or not), k32t / ms32 / kgrp bit for bit, dinv against numpy's inverse of
    the fp64 diagonal block."""
    from diffsound_amd import _hip

    c = _case(name, dev)
    s = c["sys"]
    lam, mu = MATERIALS[material]
    f32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    k32, k32t, ms32, dinv, kgrp = f32(s.nnzb, 9), f32(s.nnzb, 9), f32(s.nnzb), f32(s.nv, 9), f32(s.nnzb, 9)
    p = _hip.ptr
    L = _hip.lib()
    _hip.check(L.ds_combine_material(p(s.klam), p(s.kmu), p(s.ms), s.nnzb, p(s.diagidx), s.nv, float(lam), float(mu), p(k32),
                                     p(k32t), p(ms32), p(dinv), _hip.stream_ptr()), "ds_combine_material")
    assert s.groups is not None
    _hip.check(L.ds_pack_groups(p(k32t), p(s.groups["kperm"]), s.nnzb, p(kgrp), _hip.stream_ptr()), "ds_pack_groups")
    torch.cuda.synchronize()
    klam, kmu = s.klam.cpu().numpy(), s.kmu.cpu().numpy()
    r = lam * klam + mu * kmu
    bound = 2.0 ** -24 * np.abs(r) + 2.0 ** -52 * (np.abs(lam * klam) + np.abs(mu * kmu))
    rk, at = R.worst_ratio(k32.cpu().numpy().astype(np.float64), r, bound)
    assert rk <= 1, (rk, at)
    assert torch.equal(_f32_bits(k32t), _f32_bits(k32.reshape(-1, 3, 3).transpose(1, 2).reshape(-1, 9)))
    assert torch.equal(_f32_bits(ms32), _f32_bits(s.ms.float()))
    kperm = s.groups["kperm"].long()
    assert np.array_equal(np.sort(kperm.cpu().numpy()), np.arange(s.nnzb))
    assert torch.equal(_f32_bits(kgrp), _f32_bits(k32t[kperm]))
    # block-Jacobi blocks
    diag = s.diagidx.cpu().numpy()
    used = np.flatnonzero(diag >= 0)
    B = r[diag[used]].reshape(-1, 3, 3)
    inv = np.linalg.inv(B)
    n1 = lambda A: np.abs(A).sum(1).max(1)  # 1-norm per block
    cond = n1(B) * n1(inv)
    dbound = 2.0 ** -23 * np.abs(inv).max(axis=(1, 2)) * (1 + cond * 2.0 ** -29)
    dgot = dinv.cpu().numpy().astype(np.float64).reshape(-1, 3, 3)
    rd, atd = R.worst_ratio(dgot[used], inv, dbound[:, None, None])
    print(f"(f) {name} {material}: k32 err / bound {rk:.3f}; dinv err / bound {rd:.3f} at node {used[atd[0]]}, "
          f"largest cond_1 of a diagonal block {cond.max():.2e}")
    assert rd <= 1, (rd, atd)
    unused = np.flatnonzero(diag < 0)
    if name == "unused":
        assert unused.size == 2
    else:
        assert unused.size == 0
    rp = c["rp"]
    for i in unused:  # identity, and an empty pattern row
        assert rp[i + 1] == rp[i]
        assert np.array_equal(dgot[i], np.eye(3))


# ---------------------------------------------------------------------------------------------------------------- g. raw entry

@pytest.mark.parametrize("name", ["islands-17", "single-o1", "single-o2"])
def test_raw_entry_point_stays_inside(name, dev):
    """ds_assemble_kml into buffers pre-filled with NaN and padded by 9 * 256 doubles behind nnzb: no NaN is left inside, the
    padding is untouched (the staged store writes whole rows of 256 x 9, the last workgroup only nslot x 9), and the values
    are those of TetSystem.assemble bit for bit."""
    from diffsound_amd import _hip

    c = _case(name, dev)
    s = c["sys"]
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    klam, kmu, ms, geo = nan(s.nnzb * 9 + PAD), nan(s.nnzb * 9 + PAD), nan(s.nnzb + PAD), nan(s.T * 13 + PAD)
    p = _hip.ptr
    _hip.check(_hip.lib().ds_assemble_kml(p(s.vertices), p(s.tets), s.T, s.N, s.nv, p(s.cptr), p(s.clist), s.nnzb, p(s.dtab),
                                          p(s.mtab), p(geo), p(klam), p(kmu), p(ms), _hip.stream_ptr()), "ds_assemble_kml")
    torch.cuda.synchronize()
    for buf, n, want in ((klam, s.nnzb * 9, s.klam), (kmu, s.nnzb * 9, s.kmu), (ms, s.nnzb, s.ms), (geo, s.T * 13, s._tetgeo)):
        assert not torch.isnan(buf[:n]).any()
        assert torch.isnan(buf[n:]).all() and buf[n:].numel() == PAD
        assert torch.equal(buf[:n], want.reshape(-1))
