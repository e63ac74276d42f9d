#!/usr/bin/env python3
"""Generate tests/golden/g10_dmtet.npz by running the REFERENCE's three DMTet classes on CPU.

Run only in the build container (needs the reference tree, see _ref_harness.py):

    python tests/golden/make_golden_dmtet.py

The reference hard-codes device="cuda" in its lookup tables; that is mapped to the CPU here.  ``render``, ``open3d``
and ``torch.utils.tensorboard`` (imported at module level by the thickness / interpolation modules, never called on
these paths) are stubbed in sys.modules.  Stored (data only):

* the reference's 16^3 tet grid (data/tets/16_tets.npz: vertices as float32, indices);
* SDF cases on it: a sphere, a noisy torus, a sphere with values exactly 0 and exactly t, a deformed grid, all
  outside; per case the thickness t and a second SDF for the interpolation variant;
* per case and variant the fp32 outputs (plain: verts, tets; thickness / interpolation: verts, faces, all_verts,
  all_tets) and, for fixed random cotangents, the VJPs w.r.t. pos, sdf, t (thickness) and sdf2 / c (interpolation)
  from the same reference code run in fp64 (same topology: the fp32 inputs are exact in fp64);
* the key names, shapes and checksums of DMTetGeometry(16).state_dict() under torch.manual_seed(0).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_harness  # noqa: E402

_ref_harness.install()


def _stub_modules():
    render = types.ModuleType("render")
    for sub in ("mesh", "render"):
        m = types.ModuleType("render." + sub)
        setattr(render, sub, m)
        sys.modules["render." + sub] = m
    sys.modules["render"] = render
    sys.modules["open3d"] = types.ModuleType("open3d")
    tb = types.ModuleType("torch.utils.tensorboard")

    class SummaryWriter:
        def __init__(self, *a, **k):
            pass

    tb.SummaryWriter = SummaryWriter
    sys.modules["torch.utils.tensorboard"] = tb


def _cuda_to_cpu():
    """device="cuda" -> cpu for the factory functions the reference's DMTet tables use."""
    def wrap(fn):
        def f(*a, **k):
            if str(k.get("device", "")).startswith("cuda"):
                k["device"] = "cpu"
            return fn(*a, **k)
        return f

    for name in ("tensor", "ones", "zeros", "arange", "full"):
        setattr(torch, name, wrap(getattr(torch, name)))


_stub_modules()
_cuda_to_cpu()

from src.dmtet.geometry import dmtet_geometry as ref_plain  # noqa: E402
from src.dmtet.geometry import dmtet_thickness as ref_thick  # noqa: E402
from src.dmtet.geometry import dmtet_interpolate as ref_interp  # noqa: E402


def sphere(p, r=0.35):
    return r - np.linalg.norm(p, axis=1)


def torus(p, R=0.25, r=0.12):
    q = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R
    return r - np.sqrt(q ** 2 + p[:, 2] ** 2)


def make_cases(pos, rng):
    n = len(pos)
    cases = {}
    s = sphere(pos).astype(np.float32)
    cases["sphere"] = (pos, s, np.float32(0.12))
    tn = (torus(pos) + 0.01 * rng.standard_normal(n)).astype(np.float32)
    cases["torus"] = (pos, tn, np.float32(0.05))
    t = np.float32(0.15)
    se = s.copy()
    se[rng.choice(np.flatnonzero(s > 0), 25, replace=False)] = 0.0
    se[rng.choice(np.flatnonzero(s > 0), 25, replace=False)] = t
    se[rng.choice(np.flatnonzero(s < 0), 10, replace=False)] = 0.0
    cases["exact"] = (pos, se, t)
    interior = np.abs(pos).max(axis=1) < 0.49
    pd = (pos + interior[:, None] * rng.uniform(-0.02, 0.02, size=pos.shape)).astype(np.float32)
    cases["deformed"] = (pd, (sphere(pd, 0.3) + 0.05 * np.sin(9 * pd[:, 0])).astype(np.float32), np.float32(0.1))
    cases["outside"] = (pos, (-0.1 - rng.uniform(0, 1, n)).astype(np.float32), np.float32(0.1))
    return cases


def plain(pos, sdf, tets, dtype):
    return ref_plain.DMTet()(pos.to(dtype), sdf.to(dtype), tets)


def main():
    g = np.load(os.path.join(_ref_harness.REFERENCE_ROOT, "data/tets/16_tets.npz"))
    verts = g["vertices"].astype(np.float32)
    tets = g["indices"].astype(np.int64)
    rng = np.random.default_rng(2024)
    out = {"grid_vertices": verts, "grid_indices": tets}
    T = torch.from_numpy(tets)
    names = []
    for name, (pos, sdf, t) in make_cases(verts, rng).items():
        names.append(name)
        n = len(pos)
        s2 = torus(pos, 0.2, 0.15).astype(np.float32) if name != "outside" else (-0.2 - rng.uniform(0, 1, n)).astype(np.float32)
        c = np.float32(0.3)
        out.update({f"{name}/pos": pos, f"{name}/sdf": sdf, f"{name}/t": t, f"{name}/sdf2": s2, f"{name}/c": c})
        P32, S32 = torch.from_numpy(pos), torch.from_numpy(sdf)

        # plain (dmtet_geometry.DMTet)
        v, tt = ref_plain.DMTet()(P32, S32, T)
        out[f"{name}/plain/verts"], out[f"{name}/plain/tets"] = v.numpy(), tt.numpy()
        gv = rng.standard_normal(v.shape).astype(np.float32)
        out[f"{name}/plain/cot"] = gv
        P, S = P32.double().requires_grad_(True), S32.double().requires_grad_(True)
        v64, _ = ref_plain.DMTet()(P, S, T)
        if v64.shape[0]:
            (v64 * torch.from_numpy(gv).double()).sum().backward()
        out[f"{name}/plain/dpos"] = np.zeros((n, 3)) if P.grad is None else P.grad.numpy()
        out[f"{name}/plain/dsdf"] = np.zeros(n) if S.grad is None else S.grad.numpy()

        # thickness band (dmtet_thickness.DMTet), t = thickness_coef * max_thickness with max_thickness = 1
        m = ref_thick.DMTet()
        m.max_thickness = 1.0
        ve, f, va, ta = m(P32, S32, T, torch.tensor(t))
        for k, x in zip(("verts", "faces", "all_verts", "all_tets"), (ve, f, va, ta)):
            out[f"{name}/thick/{k}"] = x.numpy()
        g1 = rng.standard_normal(va.shape).astype(np.float32)
        g2 = rng.standard_normal(ve.shape).astype(np.float32)
        out[f"{name}/thick/cot_all"], out[f"{name}/thick/cot_surf"] = g1, g2
        P, S = P32.double().requires_grad_(True), S32.double().requires_grad_(True)
        tc = torch.tensor(float(t), dtype=torch.float64, requires_grad=True)
        ve64, _, va64, _ = m(P, S, T, tc)
        if va64.shape[0]:
            ((va64 * torch.from_numpy(g1).double()).sum() + (ve64 * torch.from_numpy(g2).double()).sum()).backward()
        out[f"{name}/thick/dpos"] = np.zeros((n, 3)) if P.grad is None else P.grad.numpy()
        out[f"{name}/thick/dsdf"] = np.zeros(n) if S.grad is None else S.grad.numpy()
        out[f"{name}/thick/dt"] = np.float64(0.0 if tc.grad is None else tc.grad.item())

        # interpolation (dmtet_interpolate.DMTet): c * sdf1 + (1 - c) * sdf2
        m = ref_interp.DMTet()
        ve, f, va, ta = m(P32, S32, torch.from_numpy(s2), T, torch.tensor(c))
        for k, x in zip(("verts", "faces", "all_verts", "all_tets"), (ve, f, va, ta)):
            out[f"{name}/interp/{k}"] = x.numpy()
        g1 = rng.standard_normal(va.shape).astype(np.float32)
        out[f"{name}/interp/cot_all"] = g1
        P, S = P32.double().requires_grad_(True), S32.double().requires_grad_(True)
        S2 = torch.from_numpy(s2).double().requires_grad_(True)
        cc = torch.tensor(float(c), dtype=torch.float64, requires_grad=True)
        _, _, va64, _ = m(P, S, S2, T, cc)
        if va64.shape[0]:
            (va64 * torch.from_numpy(g1).double()).sum().backward()
        out[f"{name}/interp/dpos"] = np.zeros((n, 3)) if P.grad is None else P.grad.numpy()
        out[f"{name}/interp/dsdf"] = np.zeros(n) if S.grad is None else S.grad.numpy()
        out[f"{name}/interp/dsdf2"] = np.zeros(n) if S2.grad is None else S2.grad.numpy()
        out[f"{name}/interp/dc"] = np.float64(0.0 if cc.grad is None else cc.grad.item())
        print(name, {k: out[f"{name}/{k}/all_tets" if k != "plain" else f"{name}/plain/tets"].shape
                     for k in ("plain", "thick", "interp")})
    out["cases"] = np.array(names)

    # DMTetGeometry(16) parameters under a fixed seed (the reference loads data/tets/ from the working directory)
    cwd = os.getcwd()
    os.chdir(_ref_harness.REFERENCE_ROOT)
    try:
        torch.manual_seed(0)
        geo = ref_plain.DMTetGeometry(16)
    finally:
        os.chdir(cwd)
    sd = geo.state_dict()
    out["state/keys"] = np.array(list(sd.keys()))
    out["state/shapes"] = np.array([",".join(map(str, v.shape)) for v in sd.values()])
    out["state/sum"] = np.array([v.double().sum().item() for v in sd.values()])
    out["state/abs_sum"] = np.array([v.double().abs().sum().item() for v in sd.values()])
    path = os.path.join(HERE, "g10_dmtet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
