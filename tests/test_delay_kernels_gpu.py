"""The kernels of diffsound_amd/csrc/delay.hip behind ds_delay_fwd / ds_delay_bwd, element by element against the dense fp64
references of tests/_delay_ref.py at the bounds derived there (tests/test_delay_ref_cpu.py anchors both without a GPU).

Every output and the workspace (sized exactly to ds_delay_workspace_bytes) live inside NaN-filled guard zones; each case is
run twice and every output must come out with the same bits.  Each case prints its largest error / bound ratio per output
(``pytest -s``); every element must be <= 1 and none is left out."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _delay_ref as DL  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [DL.case_id(c) for c in DL.CASES]
R = DL.R


def _call(case, inputs, with_gs=True, with_gtau=True):
    """One forward and one backward call on fresh guarded buffers."""
    _hip, L = _lib()
    B, S, K, hop, _ = case
    s, tau, gy = inputs
    p = _hip.ptr
    d_s, d_tau, d_gy = map(_up, (s, tau, gy))
    nbytes = L.ds_delay_workspace_bytes(B, S, K, hop)
    assert nbytes == 8 * B * S
    out = dict(work=Guarded((nbytes // 8,), torch.float64), y=Guarded((B, S)), gs=Guarded((B, S)),
               gtau=Guarded((B, K), torch.float64))
    _hip.check(L.ds_delay_fwd(p(d_s), p(d_tau), B, S, K, hop, out["y"].ptr, _hip.stream_ptr()), "ds_delay_fwd")
    _hip.check(L.ds_delay_bwd(p(d_gy), p(d_s), p(d_tau), B, S, K, hop, out["work"].ptr, nbytes,
                              out["gs"].ptr if with_gs else None, out["gtau"].ptr if with_gtau else None, _hip.stream_ptr()),
               "ds_delay_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(case):
    inputs = DL.inputs(case)
    return inputs, _call(case, inputs), _call(case, inputs)


@pytest.mark.parametrize("case", DL.CASES, ids=IDS)
def test_forward(case):
    B, S, K, hop, kind = case
    (s, tau, gy), out, again = _run(case)
    out["y"].check("y")
    assert _same_bits(out["y"], again["y"])
    y = out["y"].numpy()
    f = DL.forward(s, tau, hop)
    assert _ratio("delay.y", case, y, f["y"], DL.bound_y(f)) <= 1.0
    if kind in ("zero", "int"):                      # an exact shift, bit for bit; the leading samples exactly 0
        N = DL.int_delay(S) if kind == "int" else 0
        assert np.array_equal(y[:, N:].view(np.uint32), s[:, :S - N].view(np.uint32)) and not y[:, :N].any()
        assert not np.signbit(y[:, :N]).any()
    if kind == "far":
        assert np.array_equal(y.view(np.uint32), np.zeros((B, S), dtype=np.uint32))


@pytest.mark.parametrize("case", DL.CASES, ids=IDS)
def test_backward(case):
    B, S, K, hop, kind = case
    (s, tau, gy), out, again = _run(case)
    for k in ("gs", "gtau", "work"):
        out[k].check(k)
    assert _same_bits(out["gs"], again["gs"]) and _same_bits(out["gtau"], again["gtau"])
    b = DL.backward(gy, s, tau, hop)
    gs, gtau = out["gs"].numpy(), out["gtau"].numpy()
    assert not gtau[:, DL.frames_needed(S, hop):].any(), "frames no sample touches must get exactly 0"
    assert _ratio("delay.gs", case, gs, b["gs"], DL.bound_gs(b)) <= 1.0
    assert _ratio("delay.gtau", case, gtau, b["gtau"], b["gtau_bound"]) <= 1.0
    if kind in ("zero", "int"):                      # the adjoint of a shift is the shift back, bit for bit
        N = DL.int_delay(S) if kind == "int" else 0
        assert np.array_equal(gs[:, :S - N].view(np.uint32), gy[:, N:].view(np.uint32)) and not gs[:, S - N:].any()
    if kind == "far":
        assert not gs.any() and not gtau.any()


@pytest.mark.parametrize("which", ["gs", "gtau"])
def test_backward_without_an_optional_output_leaves_it_alone(which):
    """gs = NULL or gtau = NULL: nothing is computed for it, and the other output has the bits of the call with both."""
    case = DL.CASES[17]
    inputs, out, _ = _run(case)
    bare = _call(case, inputs, with_gs=which != "gs", with_gtau=which != "gtau")
    assert bare[which].untouched()
    other = "gtau" if which == "gs" else "gs"
    bare[other].check(other)
    assert _same_bits(bare[other], out[other])
    if which == "gtau":
        assert bare["work"].untouched()
    neither = _call(case, inputs, with_gs=False, with_gtau=False)
    assert neither["gs"].untouched() and neither["gtau"].untouched() and neither["work"].untouched()


def test_unsafe_delays_read_nothing_out_of_range():
    """What the header promises for EVERY tau: non-finite frames give NaN in y over the samples they weigh on and nothing
    elsewhere; huge delays of either sign give 0; the backward of the same input writes only its own outputs."""
    case = (2, DL.TILE + 1, 4, 48, "unsafe")
    B, S, K, hop, _ = case
    rng = np.random.default_rng(5)
    s = rng.standard_normal((B, S)).astype(np.float32)
    gy = rng.standard_normal((B, S)).astype(np.float32)
    tau = np.array([[2.0, np.nan, 1e300, -1e300], [np.inf, 3.0, 5.5, 4.0]])
    out = _call(case, (s, tau, gy))
    y = out["y"].numpy()
    p, _ = DL.positions(tau, hop, S)
    bad = ~np.isfinite(p)
    assert np.isnan(y[bad]).all() and np.isfinite(y[~bad]).all()
    assert bad[0, :96].all() and not bad[0, 96:].any() and bad[1, :48].all() and not bad[1, 48:].any()   # (0 * NaN is NaN)
    big = ~bad & (np.abs(p) > 1e100)
    assert big.any() and not y[big].any()
    whole = lambda g: g.buf.cpu().numpy()
    for k in ("y", "gs", "gtau", "work"):
        w = whole(out[k])
        assert np.isnan(w[:64]).all() and np.isnan(w[-64:]).all(), f"{k}: written outside"
    f = DL.forward(s[1:, :], tau[1:, :], hop)
    ok = ~bad[1]
    assert _ratio("delay.unsafe.y", case, y[1][ok], f["y"][0][ok], DL.bound_y(f)[0][ok]) <= 1.0


def test_workspace_bytes():
    _, L = _lib()
    for a in [(0, 1, 1, 16), (65536, 1, 1, 16), (1, 0, 1, 16), (1, 1, 0, 16), (1, 1, 1, 0), (1, 1, 1, -3)]:
        assert L.ds_delay_workspace_bytes(*a) == 0
    for B, S in [(1, 1), (3, DL.TILE + 1), (16, 32000), (65535, 2 ** 20)]:
        assert L.ds_delay_workspace_bytes(B, S, 3, 48) == 8 * B * S
