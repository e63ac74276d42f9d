"""csrc/modesample.hip on the device, every output element against the fp64 restatement of tests/_mode_sample_ref.py.

The only fp32 quantities are L and dir; the reference is handed the same fp32 values, so kernel and reference evaluate
the same real number and differ by fp64 rounding alone.  Each of them is within gamma_k * sum |terms| of that number,
k the number of roundings the worst-placed term goes through, and gamma_a + gamma_b <= gamma_(a + b): the bound is
gamma_K * sum |terms| with K = k_kernel + k_reference.  With N nodes per element, m modes and c = ceil(m / 64):

  shape functions   at most 2 roundings (P2 corner: 2 L - 1, then times L; 2 L, 4 L are exact), on both sides.
  vec   kernel      a chain of N fused multiply-adds on top of N_a: N + 2.
        reference   N products and N - 1 additions on top of N_a: at most N + 2.               K_vec  = 2 N + 4
  out   kernel      vec, then d_0 v_0 and two fused multiply-adds: N + 5.
        reference   vec, then 3 products and 2 additions: N + 5.                               K_out  = 2 N + 10
  gdir  kernel      vec (N + 2), a lane's c fused multiply-adds over its own modes, 6 butterfly additions.
        reference   one einsum over (a, m): N_a, two products, at most N m - 1 additions.      K_gdir = N + 8 + c + N m + 3
  gL    kernel      w_a = dir . U_a (3), the shape-gradient dot (P2: 4 L - 1 and its product, then three fused
                    multiply-adds by the exact 4 L: 5), the lane's c, the butterfly's 6.
        reference   w_a (3), dN (1), two products, at most N m - 1 additions.                   K_gL   = 14 + c + N m + 6
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mode_sample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS, MODES, POINTS = (1, 2), (1, 5, 64, 70), (1, 63, 130)
CASES = [(o, m, P) for o in ORDERS for m in MODES for P in POINTS]


def k_bounds(N, m):
    c = -(-m // 64)
    return dict(vec=2 * N + 4, out=2 * N + 10, gdir=N + 8 + c + N * m + 3, gL=14 + c + N * m + 6)


@functools.lru_cache(maxsize=None)
def _mesh(order):
    verts, tets = R.mesh(order)
    tets.setflags(write=False)
    return verts.shape[0], tets


@functools.lru_cache(maxsize=None)
def _case(order, m, P):
    """Inputs and references of one case, computed once and left unchanged."""
    nv, tets = _mesh(order)
    elem, L, dirs = R.sample_points(tets.shape[0], P, seed=1000 * order + 10 * m + P)
    U = R.random_modes(nv, m, m + 3, seed=7 * m + order)
    gout = np.random.default_rng(m + P).standard_normal((P, m))
    out, vec, aout, avec = R.forward(tets, U, m, elem, L, dirs, with_abs=True)
    gL, gdir, agL, agdir = R.backward(tets, U, m, elem, L, dirs, gout, with_abs=True)
    ref = dict(out=out, vec=vec, gL=gL, gdir=gdir)
    mag = dict(out=aout, vec=avec, gL=agL, gdir=agdir)
    for a in (elem, L, dirs, U, gout, *ref.values(), *mag.values()):
        a.setflags(write=False)
    return nv, tets, elem, L, dirs, U, gout, ref, mag


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(order, m, P, outs=("out", "vec", "gL", "gdir")):
    from diffsound_amd import _hip

    nv, tets, elem, L, dirs, U, gout, _, _ = _case(order, m, P)
    lib, p = _hip.lib(), _hip.ptr
    t, u, e, l, d, g = (_dev(a) for a in (tets, U, elem, L, dirs, gout))
    new = lambda name, shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda") if name in outs else None
    res = dict(out=new("out", (P, m)), vec=new("vec", (P, m, 3)), gL=new("gL", (P, 4)), gdir=new("gdir", (P, 3)))
    common = (p(t), tets.shape[0], tets.shape[1], nv, p(u), U.shape[1], m, p(e), p(l), p(d), P)
    if res["out"] is not None or res["vec"] is not None:
        _hip.check(lib.ds_mode_sample_fwd(*common, p(res["out"]), p(res["vec"]), _hip.stream_ptr()), "ds_mode_sample_fwd")
    if res["gL"] is not None or res["gdir"] is not None:
        _hip.check(lib.ds_mode_sample_bwd(*common, p(g), p(res["gL"]), p(res["gdir"]), _hip.stream_ptr()), "ds_mode_sample_bwd")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if v is not None}


def _compare(order, m, P, got):
    _, tets, *_, ref, mag = _case(order, m, P)
    K = k_bounds(tets.shape[1], m)
    for name, g in got.items():
        err, bound = np.abs(g - ref[name]), R.gamma(K[name]) * mag[name]
        assert np.isfinite(g).all(), (name, "an element was not written, or a padding column was read")
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print(f"ord {order} m {m} P {P} {name}: worst error / bound = {worst:.3g} (K = {K[name]})")
        assert np.all(err <= bound), (name, order, m, P, float(err.max()), worst)


@pytest.mark.parametrize("order,m,P", CASES)
def test_every_element_within_the_derived_bound(order, m, P):
    _compare(order, m, P, _run(order, m, P))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("outs", [("gL",), ("gdir",), ("out",), ("vec",)])
def test_null_outputs_are_skipped(order, outs):
    """gL alone, gdir alone (and out alone, vec alone): the other output is NULL, the one asked for has the same bits
    as in the call that writes both."""
    m, P = 70, 63
    alone, both = _run(order, m, P, outs), _run(order, m, P)
    _compare(order, m, P, alone)
    assert list(alone) == list(outs) and np.array_equal(alone[outs[0]], both[outs[0]])


@pytest.mark.parametrize("order", ORDERS)
def test_two_calls_give_identical_bits(order):
    a, b = _run(order, 70, 130), _run(order, 70, 130)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def test_host_side_refusals_launch_nothing():
    from diffsound_amd import _hip

    assert R.check_refusals(_hip.lib()) >= 30
    torch.cuda.synchronize()  # nothing was enqueued: a launch on the fake pointers would have faulted here
