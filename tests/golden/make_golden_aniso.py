#!/usr/bin/env python3
"""G10 (anisotropic tangents): the REFERENCE's DiffSoundObj with a material model whose ``jacobian_F()`` is a fixed 9x9
tangent, on the 2^3 cube of g2_cube2.npz at orders 1 and 2, run once on the CPU through ``_ref_harness`` like
make_golden.py (needs the reference checkout; the fixture holds recorded results and settings only):

    python tests/golden/make_golden_aniso.py

Two tangents: ``ortho``, the one of tests/test_deform_cpu.py::orthotropic_tangent (the x axis 1.5 times as stiff), and
``tri``, fully triclinic - a random symmetric positive definite 6x6 Voigt matrix (seed TRI_SEED) scaled to the material's
Young's modulus and expanded with both minor symmetries.  Per tangent and order the file records C, the dense
``stiff_matrix`` (reference src/diffelastic/diff_model.py:184-220), the eigenvalues of eigsh(K, M=M, k=mode_num+6,
sigma=20000) with the six rigid ones dropped (:335-369) and ``get_undamped_freqs()`` of task "material" (:371-388)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _ref_harness  # noqa: E402

_ref_harness.install()

from src.diffelastic.diff_model import DiffSoundObj  # noqa: E402  (the reference's)

sys.path.append(ROOT)
from oracle import fem  # noqa: E402

TRI_SEED = 20240610
MODE_NUM = 8
VOIGT_OF = (0, 5, 4, 5, 1, 3, 4, 3, 2)  # the Voigt index (11, 22, 33, 23, 13, 12) of 3i+j


def tangents(E, nu):
    lam, mu = fem.lame(E, nu)
    ortho = fem.piola_jacobian(lam, mu)
    ortho[0, 0] *= 1.5
    rng = np.random.default_rng(TRI_SEED)
    A = rng.standard_normal((6, 6))
    voigt = A @ A.T + 6.0 * np.eye(6)
    voigt *= E / np.mean(np.diag(voigt))
    idx = np.asarray(VOIGT_OF)
    return {"ortho": ortho, "tri": np.ascontiguousarray(voigt[idx][:, idx])}


def fixed_model(C):
    C = torch.from_numpy(C)

    class Fixed(torch.nn.Module):
        def __init__(self, mat):
            super().__init__()
            self.mat = mat

        def forward(self, F):
            return (F.reshape(*F.shape[:-2], 9) @ C.to(F.dtype).T).reshape(F.shape)

        def jacobian_F(self):
            return C.reshape(1, 3, 3, 1, 3, 3)

    return Fixed


def main():
    g = np.load(os.path.join(HERE, "g2_cube2.npz"))
    verts, tets, mat = g["verts"], g["tets"], tuple(float(x) for x in g["mat"])
    out = {"mat": np.asarray(mat), "mode_num": MODE_NUM, "tri_seed": TRI_SEED}
    for name, C in tangents(mat[1], mat[2]).items():
        out[f"{name}_C"] = C
        for order in (1, 2):
            obj = DiffSoundObj(vertices=torch.from_numpy(verts), tets=torch.from_numpy(tets), mode_num=MODE_NUM, mat=mat,
                               order=order, mat_model=fixed_model(C), task="material")
            obj.eigen_decomposition()
            out[f"{name}_o{order}_K"] = obj.stiff_matrix.to_dense().numpy()
            out[f"{name}_o{order}_eigenvalues"] = obj.eigenvalues.numpy()
            with torch.no_grad():
                out[f"{name}_o{order}_freqs"] = obj.get_undamped_freqs().numpy()
            print(name, order, out[f"{name}_o{order}_K"].shape, out[f"{name}_o{order}_eigenvalues"][:3])
    path = os.path.join(HERE, "g10_aniso_cube2.npz")
    np.savez_compressed(path, **out)
    print("g10 aniso done", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
