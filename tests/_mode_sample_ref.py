"""fp64 NumPy restatement of csrc/modesample.hip: the modal gains of a strike and both of their gradients.

  out[p, i]    = sum_a N_a(L_p) sum_c dir[p, c] U[3 tets[elem_p, a] + c, i]
  vec[p, i, c] = sum_a N_a(L_p) U[3 tets[elem_p, a] + c, i]
  gL[p, j]     = sum_i gout[p, i] sum_a dN_a/dL_j(L_p) sum_c dir[p, c] U[3 node_a + c, i]
  gdir[p, c]   = sum_i gout[p, i] vec[p, i, c]

The shape functions and their derivatives are those of ``fem_tables.shape_values`` / ``shape_gradients``, evaluated in
fp64 on whatever L is given (the GPU tests hand over the fp64 image of the kernel's fp32 L and dir, so that only fp64
summation error separates the two).  Every function also returns, on request, the sum of the absolute values of the
terms of each output element: what an error bound of the form gamma_k * sum |terms| is built on.
"""
import numpy as np

from diffsound_amd import fem_tables

U64 = 2.0 ** -53  # unit roundoff of fp64


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u) for fp64."""
    return k * U64 / (1.0 - k * U64)


def _gather(tets, U, m, elem):
    """U at the nodes of each point's element: (P, N, 3, m) fp64."""
    nodes = np.asarray(tets, dtype=np.int64)[np.asarray(elem, dtype=np.int64)]  # (P, N)
    U = np.asarray(U, dtype=np.float64)[:, :m]
    return U.reshape(-1, 3, m)[nodes]


def _order(tets):
    return {4: 1, 10: 2}[np.asarray(tets).shape[1]]


def forward(tets, U, m, elem, L, dirs, with_abs=False):
    """(out (P, m), vec (P, m, 3)), and with ``with_abs`` also the sums of |terms| of both."""
    L = np.asarray(L, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    Ug = _gather(tets, U, m, elem)
    Nv = fem_tables.shape_values(L, _order(tets))  # (P, N)
    vec = np.einsum("pa,pacm->pmc", Nv, Ug)
    out = np.einsum("pmc,pc->pm", vec, d)
    if not with_abs:
        return out, vec
    avec = np.einsum("pa,pacm->pmc", np.abs(Nv), np.abs(Ug))
    aout = np.einsum("pmc,pc->pm", avec, np.abs(d))
    return out, vec, aout, avec


def backward(tets, U, m, elem, L, dirs, gout, with_abs=False):
    """(gL (P, 4), gdir (P, 3)), and with ``with_abs`` also the sums of |terms| of both."""
    L = np.asarray(L, dtype=np.float64)
    d = np.asarray(dirs, dtype=np.float64)
    g = np.asarray(gout, dtype=np.float64)
    Ug = _gather(tets, U, m, elem)
    order = _order(tets)
    Nv = fem_tables.shape_values(L, order)
    dN = fem_tables.shape_gradients(L, order)  # (P, N, 4)
    w = np.einsum("pacm,pc->pam", Ug, d)  # dir . U[node_a, :, i]
    gL = np.einsum("pm,paj,pam->pj", g, dN, w)
    gdir = np.einsum("pm,pa,pacm->pc", g, Nv, Ug)
    if not with_abs:
        return gL, gdir
    aw = np.einsum("pacm,pc->pam", np.abs(Ug), np.abs(d))
    agL = np.einsum("pm,paj,pam->pj", np.abs(g), np.abs(dN), aw)
    agdir = np.einsum("pm,pa,pacm->pc", np.abs(g), np.abs(Nv), np.abs(Ug))
    return gL, gdir, agL, agdir


def element_frame(verts, tets, elem):
    """Corner coordinates (P, 4, 3) of each point's element (corner slots of fem_tables): x(L) = sum_k L_k X_k."""
    order = _order(tets)
    c = np.asarray(tets, dtype=np.int64)[np.asarray(elem, dtype=np.int64)][:, list(fem_tables.CORNER_SLOTS[order])]
    return np.asarray(verts, dtype=np.float64)[c]


# ----------------------------------------------------------------------------------------------- shared test inputs
def mesh(order, cells=2):
    """(verts (nv, 3) fp64, tets (T, N) int32) of ``meshgen.kuhn_box(cells)`` lifted to ``order``; the coordinates of
    the mid-edge nodes are the exact fp64 midpoints of their corners (the element map is affine)."""
    import torch

    from diffsound_amd import meshgen
    from oracle import fem

    v, t = meshgen.kuhn_box(cells)
    v2, t2 = fem.to_high_order(torch.from_numpy(v), torch.from_numpy(t).long(), order)
    tets = t2.numpy().astype(np.int32)
    verts = v2.numpy().astype(np.float64)
    if order == 2:
        for slot, (p, q) in fem_tables._MID.items():
            cp, cq = fem_tables.CORNER_SLOTS[2][p], fem_tables.CORNER_SLOTS[2][q]
            verts[tets[:, slot]] = 0.5 * (verts[tets[:, cp]] + verts[tets[:, cq]])
    return verts, tets


SPECIAL_L = np.array([[0, 0, 1, 0],              # a corner
                      [0.25, 0, 0, 0.75],        # on an edge: two zero coordinates
                      [0.5, 0.5, 0, 0],          # an edge midpoint (a node of the P2 element)
                      [1 / 3, 1 / 3, 0, 1 / 3],  # a face centroid
                      [0.1, 0.2, 0.3, 0.4]],     # the interior
                     dtype=np.float64)


def sample_points(T, P, seed):
    """(elem (P,) int32, L (P, 4) fp32, dir (P, 3) fp32): the special points of SPECIAL_L first (as many as fit, in
    elements spread over the mesh, the last element among them), then Dirichlet-distributed interior points."""
    rng = np.random.default_rng(seed)
    elem = rng.integers(0, T, size=P).astype(np.int32)
    L = rng.dirichlet(np.ones(4), size=P)
    ns = min(P, len(SPECIAL_L))
    L[:ns] = SPECIAL_L[P % len(SPECIAL_L):][:ns] if P < len(SPECIAL_L) else SPECIAL_L
    elem[0] = T - 1
    dirs = rng.standard_normal((P, 3))
    return elem, L.astype(np.float32), dirs.astype(np.float32)


def random_modes(nv, m, ldu, seed):
    """(3 nv, ldu) fp64 with NaN in the padding columns m..ldu: a kernel that reads them shows it."""
    rng = np.random.default_rng(seed)
    U = np.full((3 * nv, ldu), np.nan)
    U[:, :m] = rng.standard_normal((3 * nv, m))
    return U


def check_refusals(lib):
    """Every host-side refusal of ds_mode_sample_fwd / _bwd: a non-zero status and a message, in front of any launch
    (the pointers are fakes that a launch would fault on, the call needs no device)."""
    ok = 1 << 20  # never dereferenced: the checks come first
    # (tets, T, N, nv, U, ldu, m, elem, L, dir, P)
    good = dict(tets=ok, T=6, N=4, nv=9, U=ok, ldu=8, m=5, elem=ok, L=ok, dir=ok, P=3)
    order = ("tets", "T", "N", "nv", "U", "ldu", "m", "elem", "L", "dir", "P")
    bad = [(dict(tets=None), b"null pointer"), (dict(U=None), b"null pointer"), (dict(elem=None), b"null pointer"),
           (dict(L=None), b"null pointer"), (dict(dir=None), b"null pointer"),
           (dict(N=5), b"N must be 4 or 10"), (dict(N=0), b"N must be 4 or 10"),
           (dict(P=0), b"bad sizes"), (dict(P=-1), b"bad sizes"), (dict(m=0), b"bad sizes"), (dict(T=0), b"bad sizes"),
           (dict(nv=0), b"bad sizes"), (dict(ldu=4), b"less than m"), (dict(U=ok + 4), b"8-byte aligned")]
    seen = 0
    for change, text in bad:
        a = [dict(good, **change)[k] for k in order]
        assert lib.ds_mode_sample_fwd(*a, ok, ok, None) != 0 and text in lib.ds_last_error(), (change, lib.ds_last_error())
        assert lib.ds_mode_sample_bwd(*a, ok, ok, ok, None) != 0 and text in lib.ds_last_error(), (change, lib.ds_last_error())
        seen += 2
    a = [good[k] for k in order]
    for outs, text in (((None, None), b"null pointer"), ((ok + 4, ok), b"8-byte aligned"), ((ok, ok + 12), b"8-byte aligned")):
        assert lib.ds_mode_sample_fwd(*a, *outs, None) != 0 and text in lib.ds_last_error(), (outs, lib.ds_last_error())
        seen += 1
    for outs, text in (((None, ok, ok), b"null pointer"), ((ok, None, None), b"null pointer"),
                       ((ok + 4, ok, ok), b"8-byte aligned"), ((ok, ok + 4, None), b"8-byte aligned"),
                       ((ok, None, ok + 4), b"8-byte aligned")):
        assert lib.ds_mode_sample_bwd(*a, *outs, None) != 0 and text in lib.ds_last_error(), (outs, lib.ds_last_error())
        seen += 1
    return seen


# ----------------------------------------------------------------------------------------------- position recovery
RECOVER_TARGET = (0.2, 0.3, 0.5)   # barycentrics of the struck point, in the order of the face's ascending node ids
RECOVER_START = (0.6, 0.25, 0.15)  # where the search starts, on the same face
RECOVER_STEPS, RECOVER_LR = 120, 0.05
RECOVER_CELLS, RECOVER_MODES = 3, 8  # meshgen.kuhn_box(3), order 1, the 8 lowest elastic modes
# The loop on this restatement with ARPACK's modes of that box (tests/test_mode_sample_ref_cpu.py runs it) ends at
# 8.5e-7 from a start of 0.342: a ratio of 2.5e-6.  The gains are linear in bary3 on a P1 face, so the loss is a fixed
# convex quadratic and Adam at this step size is still oscillating into the minimum after 120 steps; the device's modes
# differ from ARPACK's by the eigensolver's tolerance (1e-4 relative), which moves that late trajectory but not its
# envelope.  The margin leaves a factor 400 for that: the loss has to fall to 1e-3 of its start value.  A gradient with
# a wrong sign or a wrong component does not descend this quadratic at all (ratio >= 1 after the clamp and renormalise).
RECOVER_MARGIN = 1e-3
RECOVER_MEASURED = 2.5e-6
RECOVER_SPOT = (0.05, 0.04, 0.06)  # the face whose centroid is nearest to this point of the default kuhn_box's top side


def boundary_faces(verts, tets4):
    """NumPy restatement of bem.surface_of + impact.face_owners for corner tets (T, 4): (elem (F,), corner (F, 3)
    local corners with ascending node ids, normal (F, 3) outward unit)."""
    loc = np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])
    t = np.asarray(tets4, dtype=np.int64)
    faces = t[:, loc]  # (T, 4, 3)
    keys = np.sort(faces.reshape(-1, 3), axis=1)
    _, inv, cnt = np.unique(keys, axis=0, return_inverse=True, return_counts=True)
    idx = np.nonzero(cnt[inv.reshape(-1)] == 1)[0]
    elem, opp = idx // 4, idx % 4
    corner = loc[opp]
    corner = np.take_along_axis(corner, np.argsort(np.take_along_axis(t[elem], corner, 1), axis=1), 1)
    x = np.asarray(verts, dtype=np.float64)
    p = x[np.take_along_axis(t[elem], corner, 1)]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= np.where(((x[t[elem, opp]] - p[:, 0]) * n).sum(1) > 0, -1.0, 1.0)[:, None]
    return elem, corner, n


def recover(gains, steps=RECOVER_STEPS, lr=RECOVER_LR):
    """The position-recovery loop: Adam on bary3 from RECOVER_START towards the gains at RECOVER_TARGET, clamped to the
    triangle and renormalised after every step, loss |c - c*|^2 / |c*|^2.  ``gains``: differentiable map from a (1, 3)
    fp64 tensor to (1, m).  Returns (loss at the start, loss after the last step, final bary3)."""
    import torch

    b = torch.tensor([RECOVER_START], dtype=torch.float64)
    probe = gains(b)
    b = b.to(probe.device).requires_grad_(True)
    with torch.no_grad():
        target = gains(torch.tensor([RECOVER_TARGET], dtype=torch.float64, device=probe.device))
    loss_of = lambda: ((gains(b) - target) ** 2).sum() / (target ** 2).sum()
    opt = torch.optim.Adam([b], lr=lr)
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_of()
        first = float(loss.detach()) if first is None else first
        loss.backward()
        opt.step()
        with torch.no_grad():
            b.clamp_(min=0.0)
            b /= b.sum()
    with torch.no_grad():
        last = float(loss_of())
    return first, last, b.detach().cpu().numpy()[0]


def numpy_gains(tets, U, m, elem, corner, direction):
    """The restatement as a differentiable torch map bary3 (1, 3) -> (1, m) on the CPU, on one face."""
    import torch

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, b):
            L = np.zeros((1, 4))
            L[0, corner] = b.detach().numpy()[0]
            ctx.L = L
            return torch.from_numpy(forward(tets, U, m, [elem], L, direction[None])[0])

        @staticmethod
        def backward(ctx, g):
            gL, _ = backward(tets, U, m, [elem], ctx.L, direction[None], g.numpy())
            return torch.from_numpy(gL[:, corner])

    return Fn.apply
