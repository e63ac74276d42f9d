"""An fp64 torch restatement, on the CPU, of the function ds_geometry_grad_tangent differentiates (csrc/geomgrad.hip):

    s(x) = sum_i gk_i u_i^T K(C, x) u_i - gm_i u_i^T M(x) u_i ,     u_i constant,

element by element: the affine map A = [p0 - p3, p1 - p3, p2 - p3] of the corner nodes through torch.linalg.inv / det,
F = sum_k c_k (x) grad L_k at the points of ``fem_tables.minimal_gradient_rule`` (or a rule handed in), the energy
|det A| sum_g w_g vec(F)^T C vec(F) with vec(F) row 3i+j, and the element mass table.  Differentiable in x by autograd;
U may be the same fp32 block the kernel reads (promoted to fp64 here), x the same fp32 coordinates promoted to fp64."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diffsound_amd import fem_tables  # noqa: E402


def element_geometry(x, tets, order):
    """(G (T, 4, 3): rows grad L_1..4, J (T,) = |det A|) of the corner nodes, fp64."""
    p = x[tets[:, list(fem_tables.CORNER_SLOTS[order])]]  # (T, 4, 3)
    A = torch.stack([p[:, 0] - p[:, 3], p[:, 1] - p[:, 3], p[:, 2] - p[:, 3]], dim=2)  # columns
    Ainv = torch.linalg.inv(A)
    return torch.cat([Ainv, -Ainv.sum(1, keepdim=True)], dim=1), torch.abs(torch.linalg.det(A))


def signed_dets(x, tets, order):
    """det [p1 - p0, p2 - p0, p3 - p0] of every element: six times its signed volume in the reference's orientation (the
    triple product of src/diffelastic/diff_model.py:272-288; the element map A above has the opposite sign)."""
    p = x[tets[:, list(fem_tables.CORNER_SLOTS[order])]]
    return torch.linalg.det(torch.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]], dim=2))


def s_of_x(x, tets, order, U, gk, gm, C, density, rule=None):
    """x (nv, 3) fp64, tets (T, N) long, U (3 nv, m), gk / gm (m,), C (9, 9): the scalar s(x), fp64.
    ``rule``: (dN/dL (ng, N, 4), weights (ng,)) in the place of the minimal rule."""
    x = x.double()
    nv, m = x.shape[0], U.shape[1]
    gt, gw = fem_tables.minimal_gradient_rule(order) if rule is None else rule
    gt, gw = torch.as_tensor(np.asarray(gt), dtype=torch.float64), torch.as_tensor(np.asarray(gw), dtype=torch.float64)
    mtab = torch.from_numpy(fem_tables.mass_table(order, density))
    C = torch.as_tensor(np.asarray(C), dtype=torch.float64)
    gk, gm = torch.as_tensor(gk).double().cpu(), torch.as_tensor(gm).double().cpu()
    G, J = element_geometry(x, tets, order)
    ue = U.double().reshape(nv, 3, m)[tets]  # (T, N, 3, m)
    c = torch.einsum("gak,tarm->tgkrm", gt, ue)
    F = torch.einsum("tgkrm,tkj->tgmrj", c, G).reshape(tets.shape[0], gt.shape[0], m, 9)
    W = torch.einsum("tgmp,pq,tgmq->tgm", F, C, F)
    stiff = torch.einsum("tgm,g,t,m->", W, gw, J, gk)
    mass = torch.einsum("ab,tarm,tbrm->tm", mtab, ue, ue)
    return stiff - torch.einsum("tm,t,m->", mass, J, gm)


def grad_of_s(x, tets, order, U, gk, gm, C, density):
    """ds/dx (nv, 3) fp64 by autograd."""
    x = x.detach().double().clone().requires_grad_(True)
    s_of_x(x, tets, order, U, gk, gm, C, density).backward()
    return x.grad
