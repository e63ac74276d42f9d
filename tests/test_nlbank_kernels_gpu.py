"""The kernels of diffsound_amd/csrc/nlbank.hip behind ds_nlbank_fwd / ds_nlbank_bwd, element by element against the
longdouble restatement of tests/_nlbank_ref.py, at bounds measured from the float64 restatement's own error (there;
tests/test_nlbank_ref_cpu.py vouches for the restatement without a GPU and holds every case to E64 <= 1e-10).

Every output and the workspace (sized exactly to ds_nlbank_workspace_bytes) live inside NaN-filled guard zones; each case
is run twice and every output and the workspace must come out with the same bits.  Each case prints its largest
error / bound ratio per output (``pytest -s``)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _nlbank_ref as Nl  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
IDS = [Nl.case_id(c) + "-" + str(i) for i, c in enumerate(Nl.CASES)]
F64 = torch.float64
GROUPS = dict(modes=("gd", "gw"), gain=("gc",), amp=("gamp",), force=("gf",), stretch=("gC",), coupling=("ggamma",))


def _call(case, inputs, **groups):
    """One forward and one backward call on fresh guarded buffers; a gradient group that is switched off gets NULL."""
    _hip, L = _lib()
    A, m, K, R, F, S = case[:6]
    ops = [_up(x) for x in inputs[:7]]
    d_g = _up(inputs[7])
    ptr = _hip.ptr
    nbytes = L.ds_nlbank_workspace_bytes(A, m, K, S, R)
    assert nbytes == 16 * (A * S * m + A * R * m + A * m) + 8 * A * K * m
    out = dict(work=Guarded((nbytes // 8,), F64), y=Guarded((A, S)), gd=Guarded((m,), F64), gw=Guarded((m,), F64),
               gc=Guarded((A, m), F64), gamp=Guarded((A, m), F64), gf=Guarded((A, F), F64), gC=Guarded((K, m), F64),
               ggamma=Guarded((A, K), F64))
    on = lambda k, group: out[k].ptr if groups.get(group, True) else None  # noqa: E731
    _hip.check(L.ds_nlbank_fwd(*map(ptr, ops), A, m, K, F, S, R, Nl.SR, out["y"].ptr, _hip.stream_ptr()), "ds_nlbank_fwd")
    _hip.check(L.ds_nlbank_bwd(ptr(d_g), *map(ptr, ops), A, m, K, F, S, R, Nl.SR, out["work"].ptr, nbytes, on("gd", "modes"),
                               on("gw", "modes"), on("gc", "gain"), on("gamp", "amp"), on("gf", "force"), on("gC", "stretch"),
                               on("ggamma", "coupling"), _hip.stream_ptr()), "ds_nlbank_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(i):
    inputs = Nl.inputs(Nl.CASES[i])
    return inputs, _call(Nl.CASES[i], inputs), _call(Nl.CASES[i], inputs)


@functools.lru_cache(maxsize=None)
def _refs(i):
    """(float64, longdouble) restatements of case i: forward and adjoint, computed once."""
    case = Nl.CASES[i]
    d, w, c, amp, f, C, gamma, gy = Nl.inputs(case)
    out = []
    for dt in (np.float64, LD):
        fw = Nl.forward(d, w, c, amp, f, C, gamma, case[5], case[3], dtype=dt, keep=True)
        adj = Nl.adjoint(gy, d, w, c, amp, f, C, gamma, case[3], dtype=dt, per_clip=True)
        out.append(dict(adj, y=fw["y"], s=fw["s"]))
    return out


def _within(tag, i, got, r64, rld, stored32=False):
    """``got`` against the longdouble truth in units of the bound, every element; the case is admitted only if the reference
    alone is well conditioned."""
    assert Nl.e64(r64, rld)[0] <= Nl.E64_MAX, tag
    truth = np.asarray(rld, dtype=np.float64)
    assert _ratio("nlbank." + tag, (IDS[i],), got, truth, Nl.bound(r64, rld, stored32=stored32)) <= 1.0, tag


@pytest.mark.parametrize("i", range(len(Nl.CASES)), ids=IDS)
def test_forward(i):
    case = Nl.CASES[i]
    inputs, out, again = _run(i)
    r64, rld = _refs(i)
    out["y"].check("y")
    assert _same_bits(out["y"], again["y"])
    got = out["y"].numpy()
    _within("y", i, got, r64["y"], rld["y"], stored32=True)
    for a, kind in enumerate(case[6]):
        assert got[a].any() == (kind != "idle"), "a clip without force gets exact zeros, and only that one"


@pytest.mark.parametrize("i", range(len(Nl.CASES)), ids=IDS)
def test_backward(i):
    case = Nl.CASES[i]
    A, m, K, R, F, S = case[:6]
    inputs, out, again = _run(i)
    r64, rld = _refs(i)
    for k in Nl.GRADS:
        out[k].check(k)
        assert _same_bits(out[k], again[k]), k
    assert _same_bits(out["work"], again["work"])
    # the workspace: written inside only and all of it; the checkpoints are the states that enter the samples, the segment is
    # left holding the first sample's substeps (the last one the reverse sweep re-ran), then the per-clip partials
    out["work"].check("work")
    work = out["work"].numpy()
    n_ck, n_seg, n_part = 2 * A * S * m, 2 * A * R * m, 2 * A * m
    ckpt = work[:n_ck].reshape(A, S, m, 2)
    seg = work[n_ck:n_ck + n_seg].reshape(A, R, m, 2)
    part = work[n_ck + n_seg:n_ck + n_seg + n_part].reshape(A, m, 2)
    partC = work[n_ck + n_seg + n_part:].reshape(A, K, m)
    for name, got, rows in (("checkpoints", ckpt, slice(0, None, R)), ("segment", seg, slice(0, R))):
        pick = lambda r: np.moveaxis(np.asarray(r["s"], dtype=np.clongdouble)[rows], 0, 1)  # noqa: E731
        for take, col in ((np.real, 0), (np.imag, 1)):
            _within(f"{name}.{'ri'[col]}", i, got[..., col], take(pick(r64)), take(pick(rld)))
    _within("part.gd", i, part[..., 0], r64["gd_a"], rld["gd_a"])
    _within("part.gw", i, part[..., 1], r64["gw_a"], rld["gw_a"])
    _within("part.gC", i, partC, r64["gC_a"], rld["gC_a"])
    for k in Nl.GRADS:
        _within(k, i, out[k].numpy(), r64[k], rld[k])
    assert not out["gf"].numpy()[:, S:].any(), "force samples behind the output: an exact zero"
    for a, kind in enumerate(case[6]):
        if kind == "idle":
            for k, got in (("gc", out["gc"].numpy()), ("gamp", out["gamp"].numpy()), ("ggamma", out["ggamma"].numpy()),
                           ("part", part), ("partC", partC)):
                assert not got[a].any(), f"{k}: a clip without force gets exact zeros"
            assert out["gf"].numpy()[a, :min(F, S)].all()
        if kind == "linear":
            assert not partC[a].any(), "a clip with gamma = 0 adds exact zeros to gC"
            assert out["ggamma"].numpy()[a].all() and part[a].any()
        if kind == "hard":
            assert partC[a].any()


def test_gradients_not_asked_for_are_not_written():
    """Each NULL group: it stays unwritten, the rest keeps its bits."""
    i = 5
    inputs, out, _ = _run(i)
    for off in GROUPS:
        bare = _call(Nl.CASES[i], inputs, **{off: False})
        for name, keys in GROUPS.items():
            for k in keys:
                if name == off:
                    assert bare[k].untouched(), k
                else:
                    bare[k].check(k)
                    assert _same_bits(bare[k], out[k]), k
    none = _call(Nl.CASES[i], inputs, **dict.fromkeys(GROUPS, False))
    assert all(none[k].untouched() for keys in GROUPS.values() for k in keys)
    assert _same_bits(none["y"], out["y"])


def test_every_clip_without_force():
    """All clips idle: every output but gf is exact zeros (the bound of an all-zero output admits nothing else)."""
    case = (3, 70, 2, 4, 33, 33, ("idle",) * 3)
    d, w, c, amp, f, C, gamma, gy = Nl.inputs(case)
    gamma = np.full_like(gamma, 1e9)  # (an idle clip takes the first clip's gamma, which is idle too here)
    inputs = (d, w, c, amp, f, C, gamma, gy)
    out = _call(case, inputs)
    for k in ("y",) + Nl.GRADS:
        out[k].check(k)
        assert out[k].numpy().any() == (k == "gf"), k
    r64, rld = (Nl.adjoint(gy, d, w, c, amp, f, C, gamma, 4, dtype=dt)["gf"] for dt in (np.float64, LD))
    assert _ratio("nlbank.idle.gf", None, out["gf"].numpy(), np.asarray(rld, dtype=np.float64), Nl.bound(r64, rld)) <= 1.0
