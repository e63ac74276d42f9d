"""The kernels of diffsound_amd/csrc/friction.hip behind ds_friction_fwd / ds_friction_bwd, element by element against the
longdouble restatement of tests/_friction_ref.py, at bounds measured from the float64 restatement's own error (there;
tests/test_friction_ref_cpu.py vouches for the restatement without a GPU and holds every case to E64 <= 1e-10).

Every output and the workspace (sized exactly to ds_friction_workspace_bytes) live inside NaN-filled guard zones; each case
is run twice and every output and the workspace must come out with the same bits.  Each case prints its largest
error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _friction_ref as Fr  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
IDS = [Fr.case_id(c) + "-" + str(i) for i, c in enumerate(Fr.CASES)]
F64 = torch.float64
GROUPS = dict(modes=("gd", "gw"), gain=("gc",), gesture=("gvb", "gN"), peak=("gvs",))


def _call(case, inputs, modes=True, gain=True, gesture=True, peak=True):
    """One forward and one backward call on fresh guarded buffers; a gradient group that is switched off gets NULL."""
    _hip, L = _lib()
    A, m, F, R = case[:4]
    d, w, c, vb, N, vs, g = inputs
    ops = [_up(x) for x in (d, w, c, vb, N, vs)]
    d_g = _up(g)
    ptr = _hip.ptr
    nbytes = L.ds_friction_workspace_bytes(A, m, F, R)
    assert nbytes == 16 * (A * F * m + A * R * m + A * m)
    out = dict(work=Guarded((nbytes // 8,), F64), force=Guarded((A, F)), gd=Guarded((m,), F64), gw=Guarded((m,), F64),
               gc=Guarded((A, m), F64), gvb=Guarded((A, F), F64), gN=Guarded((A, F), F64), gvs=Guarded((A,), F64))
    on = lambda k, flag: out[k].ptr if flag else None  # noqa: E731
    _hip.check(L.ds_friction_fwd(*map(ptr, ops), A, m, F, R, Fr.SR, out["force"].ptr, _hip.stream_ptr()), "ds_friction_fwd")
    _hip.check(L.ds_friction_bwd(ptr(d_g), *map(ptr, ops), A, m, F, R, Fr.SR, out["work"].ptr, nbytes, on("gd", modes),
                                 on("gw", modes), on("gc", gain), on("gvb", gesture), on("gN", gesture), on("gvs", peak),
                                 _hip.stream_ptr()), "ds_friction_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(i):
    inputs = Fr.inputs(Fr.CASES[i])
    return inputs, _call(Fr.CASES[i], inputs), _call(Fr.CASES[i], inputs)


@functools.lru_cache(maxsize=None)
def _refs(i):
    """(float64, longdouble) restatements of case i: forward and adjoint, computed once."""
    case = Fr.CASES[i]
    d, w, c, vb, N, vs, g = Fr.inputs(case)
    out = []
    for dt in (np.float64, LD):
        fw = Fr.forward(d, w, c, vb, N, vs, case[3], dtype=dt, keep=True)
        adj = Fr.adjoint(g, d, w, c, vb, N, vs, case[3], dtype=dt)
        out.append(dict(adj, force=fw["force"], vr=fw["vr"], s=fw["s"]))
    return out


@pytest.mark.parametrize("i", range(len(Fr.CASES)), ids=IDS)
def test_forward(i):
    case = Fr.CASES[i]
    (d, w, c, vb, N, vs, g), out, again = _run(i)
    r64, rld = _refs(i)
    assert set(case[4]) | set(case[5]) <= Fr.properties(case, rld)
    assert Fr.e64(r64["force"], rld["force"])[0] <= Fr.E64_MAX
    out["force"].check("force")
    assert _same_bits(out["force"], again["force"])
    got = out["force"].numpy()
    truth = np.asarray(rld["force"], dtype=np.float64)
    assert _ratio("friction.force", (IDS[i],), got, truth, Fr.bound(r64["force"], rld["force"], stored32=True)) <= 1.0
    assert not got[~N.any(-1)].any(), "a clip without normal force gets exact zeros"


@pytest.mark.parametrize("i", range(len(Fr.CASES)), ids=IDS)
def test_backward(i):
    case = Fr.CASES[i]
    A, m, F, R = case[:4]
    (d, w, c, vb, N, vs, g), out, again = _run(i)
    r64, rld = _refs(i)
    for k in Fr.GRADS:
        out[k].check(k)
        assert _same_bits(out[k], again[k]), k
    assert _same_bits(out["work"], again["work"])
    # the workspace: written inside only and all of it; the checkpoints are the states that enter the samples, and the
    # segment is left holding the first sample's substeps, the last one the reverse sweep re-ran
    out["work"].check("work")
    work = out["work"].numpy()
    ckpt = work[:2 * A * F * m].reshape(A, F, m, 2)
    seg = work[2 * A * F * m:2 * A * (F + R) * m].reshape(A, R, m, 2)
    for name, got, rows in (("checkpoints", ckpt, slice(0, None, R)), ("segment", seg, slice(0, R))):
        pick = lambda r: np.moveaxis(np.asarray(r["s"], dtype=np.clongdouble)[rows], 0, 1)  # noqa: E731
        for part, col in ((np.real, 0), (np.imag, 1)):
            r, truth = part(pick(r64)), part(pick(rld))
            assert Fr.e64(r, truth)[0] <= Fr.E64_MAX
            assert _ratio(f"friction.{name}.{'ri'[col]}", (IDS[i],), got[..., col], np.asarray(truth, dtype=np.float64),
                          Fr.bound(r, truth)) <= 1.0, name
    for k in Fr.GRADS:
        assert Fr.e64(r64[k], rld[k])[0] <= Fr.E64_MAX, k
        truth = np.asarray(rld[k], dtype=np.float64)
        assert _ratio("friction." + k, (IDS[i],), out[k].numpy(), truth, Fr.bound(r64[k], rld[k])) <= 1.0, k
    idle = ~N.any(-1)
    for k in ("gc", "gvb", "gvs"):
        assert not out[k].numpy()[idle].any(), f"{k}: a clip without normal force gets exact zeros"
    if idle.any():
        assert out["gN"].numpy()[idle].any()


def test_gradients_not_asked_for_are_not_written():
    """Each NULL group: it stays unwritten, the rest keeps its bits."""
    i = 3
    inputs, out, _ = _run(i)
    for off in GROUPS:
        flags = dict.fromkeys(GROUPS, True)
        flags[off] = False
        bare = _call(Fr.CASES[i], inputs, **flags)
        for name, keys in GROUPS.items():
            for k in keys:
                if name == off:
                    assert bare[k].untouched(), k
                else:
                    bare[k].check(k)
                    assert _same_bits(bare[k], out[k]), k
    none = _call(Fr.CASES[i], inputs, **dict.fromkeys(GROUPS, False))
    assert all(none[k].untouched() for keys in GROUPS.values() for k in keys)
    assert _same_bits(none["force"], out["force"])


def test_every_clip_without_normal_force():
    """All clips with N = 0: every output but gN is exact zeros (the bound of an all-zero output admits nothing else)."""
    case = (3, 70, 33, 4, ("idle",) * 3, ())
    inputs = Fr.inputs(case)
    out = _call(case, inputs)
    for k in ("force",) + Fr.GRADS:
        out[k].check(k)
        assert out[k].numpy().any() == (k == "gN"), k
    ref = Fr.adjoint(inputs[6], *inputs[:6], 4, dtype=LD)["gN"]
    r64 = Fr.adjoint(inputs[6], *inputs[:6], 4)["gN"]
    assert _ratio("friction.idle.gN", None, out["gN"].numpy(), np.asarray(ref, dtype=np.float64), Fr.bound(r64, ref)) <= 1.0


def test_more_than_one_gesture_chunk_and_eight_modes_a_lane():
    """F = 130: three chunks of the gesture, the last one partly filled; m = 257: NM = 8, the widest instantiation, with its
    last round holding one mode.  Slipping, so that the reference is well conditioned at this length too."""
    case = (2, 257, 130, 2, ("slip", "reversal"), ("mixed",))
    inputs = Fr.inputs(case)
    d, w, c, vb, N, vs, g = inputs
    out = _call(case, inputs)
    fw64, fwld = (Fr.forward(d, w, c, vb, N, vs, 2, dtype=dt) for dt in (np.float64, LD))
    a64, ald = (Fr.adjoint(g, d, w, c, vb, N, vs, 2, dtype=dt) for dt in (np.float64, LD))
    assert Fr.properties(case, fwld) >= {"slip", "reversal"} and (Fr.stability(case) < 0.1).all()
    out["force"].check("force")
    assert Fr.e64(fw64["force"], fwld["force"])[0] <= Fr.E64_MAX
    truth = np.asarray(fwld["force"], dtype=np.float64)
    assert _ratio("friction.long.force", None, out["force"].numpy(), truth, Fr.bound(fw64["force"], fwld["force"], True)) <= 1.0
    for k in Fr.GRADS:
        out[k].check(k)
        assert Fr.e64(a64[k], ald[k])[0] <= Fr.E64_MAX, k
        assert _ratio("friction.long." + k, None, out[k].numpy(), np.asarray(ald[k], dtype=np.float64), Fr.bound(a64[k], ald[k])) <= 1.0, k
