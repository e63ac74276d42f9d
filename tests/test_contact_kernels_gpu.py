"""The kernels of diffsound_amd/csrc/contact.hip behind ds_contact_fwd / ds_contact_bwd, element by element against the
longdouble restatement of tests/_contact_ref.py, at bounds measured from the float64 restatement's own error (there;
tests/test_contact_ref_cpu.py vouches for the restatement without a GPU).

Every output and the workspace (sized exactly to ds_contact_workspace_bytes) live inside NaN-filled guard zones; each case
is run twice and every output and the workspace must come out with the same bits.  Each case prints its largest
error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _contact_ref as C  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
IDS = [C.case_id(c) + "-" + str(i) for i, c in enumerate(C.CASES)]
F64 = torch.float64


def _call(case, inputs, modes=True, gain=True, hammer=True):
    """One forward and one backward call on fresh guarded buffers; a gradient group that is switched off gets NULL."""
    _hip, L = _lib()
    A, m, F, R, p = case[:5]
    d, w, c, M, v0, kH, g = inputs
    ops = [_up(x) for x in (d, w, c, M, v0, kH)]
    d_g = _up(g)
    ptr = _hip.ptr
    nbytes = L.ds_contact_workspace_bytes(A, m, F, R)
    assert nbytes == 16 * (A * F * R * (1 + m) + A * m)
    out = dict(work=Guarded((nbytes // 8,), F64), force=Guarded((A, F)), gd=Guarded((m,), F64), gw=Guarded((m,), F64),
               gc=Guarded((A, m), F64), gM=Guarded((A,), F64), gv0=Guarded((A,), F64), gkH=Guarded((A,), F64))
    on = lambda k, flag: out[k].ptr if flag else None  # noqa: E731
    _hip.check(L.ds_contact_fwd(*map(ptr, ops), A, m, F, R, p, C.SR, out["force"].ptr, _hip.stream_ptr()), "ds_contact_fwd")
    _hip.check(L.ds_contact_bwd(ptr(d_g), *map(ptr, ops), A, m, F, R, p, C.SR, out["work"].ptr, nbytes, on("gd", modes),
                                on("gw", modes), on("gc", gain), on("gM", hammer), on("gv0", hammer), on("gkH", hammer),
                                _hip.stream_ptr()), "ds_contact_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(i):
    inputs = C.inputs(C.CASES[i])
    return inputs, _call(C.CASES[i], inputs), _call(C.CASES[i], inputs)


@functools.lru_cache(maxsize=None)
def _refs(i):
    """(float64, longdouble) restatements of case i: forward and adjoint, computed once."""
    case = C.CASES[i]
    d, w, c, M, v0, kH, g = C.inputs(case)
    A, m, F, R, p = case[:5]
    out = []
    for dt in (np.float64, LD):
        fw = C.forward(d, w, c, M, v0, kH, F, p, R, dtype=dt)
        adj = C.adjoint(g, d, w, c, M, v0, kH, p, R, dtype=dt)
        out.append(dict(adj, force=fw["force"], f=fw["f"]))
    return out


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=IDS)
def test_forward(i):
    case = C.CASES[i]
    (d, w, c, M, v0, kH, g), out, again = _run(i)
    r64, rld = _refs(i)
    assert set(case[8]) <= C.properties(case, rld)
    out["force"].check("force")
    assert _same_bits(out["force"], again["force"])
    got = out["force"].numpy()
    truth = np.asarray(rld["force"], dtype=np.float64)
    assert _ratio("contact.force", (IDS[i],), got, truth, C.bound(r64["force"], rld["force"], stored32=True)) <= 1.0
    assert not got[v0 <= 0].any(), "a clip the hammer never reaches gets exact zeros"


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=IDS)
def test_backward(i):
    case = C.CASES[i]
    A, m, F, R, p = case[:5]
    (d, w, c, M, v0, kH, g), out, again = _run(i)
    r64, rld = _refs(i)
    hit = v0 > 0
    for k in C.GRADS:
        out[k].check(k)
        assert _same_bits(out[k], again[k]), k
    assert _same_bits(out["work"], again["work"])
    # the workspace: written inside only, every record of a clip that is hit, none of a clip that is not
    whole, N = out["work"].buf.cpu().numpy(), F * R
    assert np.isnan(whole[:64]).all() and np.isnan(whole[-64:]).all(), "workspace: written outside"
    work = out["work"].numpy()
    traj, state, part = work[:2 * A * N].reshape(A, N, 2), work[2 * A * N:2 * A * N * (1 + m)].reshape(A, N, m, 2), work[-2 * A * m:]
    assert np.isfinite(traj[hit]).all() and np.isfinite(state[hit]).all() and np.isfinite(part).all()
    assert np.isnan(traj[~hit]).all() and np.isnan(state[~hit]).all()
    for k in C.GRADS:
        truth = np.asarray(rld[k], dtype=np.float64)
        assert _ratio("contact." + k, (IDS[i],), out[k].numpy(), truth, C.bound(r64[k], rld[k])) <= 1.0, k
    for k in ("gc", "gM", "gv0", "gkH"):
        assert not out[k].numpy()[~hit].any(), f"{k}: a clip the hammer never reaches gets exact zeros"


def test_gradients_not_asked_for_are_not_written():
    i = 3
    inputs, out, _ = _run(i)
    for off in ("modes", "gain", "hammer"):
        flags = dict(modes=True, gain=True, hammer=True)
        flags[off] = False
        bare = _call(C.CASES[i], inputs, **flags)
        groups = dict(modes=("gd", "gw"), gain=("gc",), hammer=("gM", "gv0", "gkH"))
        for name, keys in groups.items():
            for k in keys:
                if name == off:
                    assert bare[k].untouched(), k
                else:
                    bare[k].check(k)
                    assert _same_bits(bare[k], out[k]), k


def test_every_clip_without_contact():
    """All clips with v0 <= 0: every output is exact zeros (the bound of an all-zero output admits nothing else)."""
    case = (3, 70, 33, 4, 1.5, (1e7,) * 3, (0.01,) * 3, (0.0, -1.0, -0.0), ("none",))
    out = _call(case, C.inputs(case))
    for k in ("force",) + C.GRADS:
        out[k].check(k)
        assert not out[k].numpy().any(), k
