#!/usr/bin/env python3
"""G12 (shape gradients with an anisotropic tangent): the REFERENCE's DiffSoundObj with the fixed triclinic tangent of
g10_aniso_cube2.npz (``tri_C``) on the 4^3 Kuhn cube of g4_cube4_geometry.npz, every node jittered by at most 0.1 of the
shortest grid edge with a recorded seed, ``vertices.requires_grad``, orders 1 and 2, 8 modes; run once on the CPU
through ``_ref_harness`` like make_golden_aniso.py (needs the reference checkout; the fixture holds recorded results and
settings only):

    python tests/golden/make_golden_aniso_geometry.py

Per order the file records ``get_vals()`` (reference src/diffelastic/diff_model.py:390-399), d sum(vals) / d vertices
and d sum(w * vals) / d vertices with w = linspace(0.5, 1.5, 8), by the reference's autograd through ``stiff_matrix``
(:184-220), ``mass_matrix`` (:222-312) and torch.inverse / det of the element maps.

The weighted gradient uses individual eigenvectors, so the eigenvalues must be simple: the generator computes NINE
elastic eigenvalues per order and requires every relative gap among them, (l_{i+1} - l_i) / l_{i+1}, to be at least
MIN_GAP; otherwise it takes the next jitter seed.  The seed used and the smallest gap are recorded."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_harness  # noqa: E402

_ref_harness.install()

from src.diffelastic.diff_model import DiffSoundObj  # noqa: E402  (the reference's)

from make_golden_aniso import fixed_model  # noqa: E402

FIRST_SEED = 20241017
MODE_NUM = 8
MIN_GAP = 1e-2
JITTER = 0.1  # of the shortest grid edge
CELLS = 4  # of the cube per axis


def jittered(verts, seed):
    edge = float(((verts.max(0) - verts.min(0)) / CELLS).min())
    rng = np.random.default_rng(seed)
    return (verts.astype(np.float64) + JITTER * edge * rng.uniform(-1.0, 1.0, verts.shape)).astype(np.float32)


def solved(verts, tets, mat, C, order, mode_num, grad):
    v = torch.from_numpy(verts).clone().requires_grad_(grad)
    obj = DiffSoundObj(vertices=v, tets=torch.from_numpy(tets), mode_num=mode_num, mat=mat, order=order,
                       mat_model=fixed_model(C), task="material")
    obj.eigen_decomposition()
    return v, obj


def main():
    g4 = np.load(os.path.join(HERE, "g4_cube4_geometry.npz"))
    C = np.load(os.path.join(HERE, "g10_aniso_cube2.npz"))["tri_C"]
    verts0, tets, mat = g4["verts"], g4["tets"], tuple(float(x) for x in g4["mat"])
    seed = FIRST_SEED
    while True:
        verts = jittered(verts0, seed)
        gaps = []
        for order in (1, 2):
            with torch.no_grad():
                ev = solved(verts, tets, mat, C, order, MODE_NUM + 1, False)[1].eigenvalues.numpy()
            gaps.append(float(((ev[1:] - ev[:-1]) / ev[1:]).min()))
        print("seed", seed, "smallest relative gaps of nine eigenvalues (order 1, 2):", gaps)
        if min(gaps) >= MIN_GAP:
            break
        seed += 1
    out = {"verts": verts, "tets": tets, "mat": np.asarray(mat), "C": C, "mode_num": MODE_NUM, "seed": seed,
           "min_gap": min(gaps), "jitter": JITTER}
    w = torch.linspace(0.5, 1.5, MODE_NUM, dtype=torch.float64).reshape(MODE_NUM, 1)
    for order in (1, 2):
        v, obj = solved(verts, tets, mat, C, order, MODE_NUM, True)
        vals = obj.get_vals()
        out[f"o{order}_eigenvalues"] = obj.eigenvalues.numpy()
        out[f"o{order}_vals"] = vals.detach().numpy()
        vals.sum().backward(retain_graph=True)
        out[f"o{order}_grad_vertices"] = v.grad.numpy().copy()
        v.grad = None
        (vals * w).sum().backward()
        out[f"o{order}_grad_vertices_weighted"] = v.grad.numpy().copy()
        print(order, out[f"o{order}_vals"][:3, 0], np.abs(out[f"o{order}_grad_vertices"]).max())
    path = os.path.join(HERE, "g12_aniso_geometry.npz")
    np.savez_compressed(path, **out)
    print("g12 aniso geometry done", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
