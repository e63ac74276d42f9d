"""The kernels of diffsound_amd/csrc/fdn.hip behind ds_fdn_fwd / ds_fdn_bwd, element by element against the fp64 recursion of
tests/_fdn_ref.py at the bounds derived there (tests/test_fdn_ref_cpu.py anchors both without a GPU).

Every output, the state and the workspace (sized exactly to ds_fdn_workspace_bytes) live inside NaN-filled guard zones; each
case is run twice and every output must come out with the same bits, and an output must keep its bits when another one is
not asked for.  Each case prints its largest error / bound ratio per output (``pytest -s``); every element must be <= 1 and
none is left out."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fdn_ref as F  # noqa: E402
from _guarded import Guarded, _lib, _ratio, _up, outside_untouched as _outside_untouched, same_bits as _same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [F.case_id(c) for c in F.CASES]
OUTS = ("gx",) + F.GRADS


def _call(i, want=("y",) + OUTS):
    """One forward and (where a gradient is wanted) one backward call on fresh guarded buffers; ``i``: the dict of
    F.inputs; ``want``: the outputs asked for (NULL for the others; y and the state are always made)."""
    _hip, L = _lib()
    (B, N), (H, n) = i["x"].shape, i["delays"].shape
    p = _hip.ptr
    d_x, d_gy = _up(i["x"]), _up(i["gy"])
    par = [_up(None if i[k] is None else np.asarray(i[k], dtype=np.int32 if k == "delays" else np.float64)) for k in F.PARAMS]
    out = dict(y=Guarded((B, N)), state=Guarded((B, n, N), torch.float64))
    _hip.check(L.ds_fdn_fwd(p(d_x), *map(p, par), B, H, N, n, out["state"].ptr, out["y"].ptr, _hip.stream_ptr()), "ds_fdn_fwd")
    if any(k in want for k in OUTS):
        nbytes = L.ds_fdn_workspace_bytes(B, H, N, n)
        assert nbytes == 8 * B * (n * N + -(-N // F.CHUNK) * (n * n + 3 * n + 1))
        out["work"] = Guarded((nbytes // 8,), torch.float64)
        shapes = dict(gx=(B, N), gA=(H, n, n), gb=(H, n), gc=(H, n), gd=(H,), gp=(H, n))
        for k in OUTS:
            if k in want:
                out[k] = Guarded(shapes[k], torch.float32 if k == "gx" else torch.float64)
        ptr = lambda k: out[k].ptr if k in out else None
        _hip.check(L.ds_fdn_bwd(p(d_gy), p(d_x), *map(p, par), B, H, N, n, out["state"].ptr, out["work"].ptr, nbytes,
                                *map(ptr, OUTS), _hip.stream_ptr()), "ds_fdn_bwd")
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _run(case):
    i, f, b = F.reference(case)
    return i, f, b, _call(i), _call(i)


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_forward(case):
    _, f, _, out, again = _run(case)
    for k in ("y", "state"):
        out[k].check(k)
        assert _same_bits(out[k], again[k]), k
    assert _ratio("fdn.y", (F.case_id(case),), out["y"].numpy(), f["y"], f["y_bound"]) <= 1.0
    assert _ratio("fdn.state", (F.case_id(case),), out["state"].numpy(), f["state"], f["state_bound"]) <= 1.0


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_backward(case):
    _, _, b, out, again = _run(case)
    _outside_untouched(out["work"], "work")
    for k in OUTS:
        out[k].check(k)
        assert _same_bits(out[k], again[k]), k
        assert _ratio("fdn." + k, (F.case_id(case),), out[k].numpy(), b[k], b[k + "_bound"]) <= 1.0, k


@pytest.mark.parametrize("case", F.NULL_CASES, ids=F.case_id)
def test_each_output_null_in_turn(case):
    """What is NULL is not computed, and the rest keeps its bits."""
    i, _, _, out, _ = _run(case)
    for gone in OUTS:
        rest = tuple(k for k in OUTS if k != gone)
        got = _call(i, ("y",) + rest)
        for k in rest:
            got[k].check(k)
            assert _same_bits(got[k], out[k]), (gone, k)
    alone = _call(i, ("y", "gx"))
    assert _same_bits(alone["gx"], out["gx"])


def test_a_null_damping_has_the_bits_of_zeros():
    null, zero = _run((4, 2, 317, F.D3, "null"))[3], _run((4, 2, 317, F.D3, "zero"))[3]
    for k in ("y", "state") + OUTS:
        assert _same_bits(null[k], zero[k]), k


def _plain(B, H, N, delays, seed):
    """Inputs of a hand-made network: x, gy random, the coefficients for the caller to fill."""
    rng = np.random.default_rng(seed)
    n = np.shape(delays)[1]
    x = F.spread(rng, (B, N), -3, 1).astype(np.float32)
    x.reshape(-1)[::7] = 0.0
    return dict(x=x, gy=F.spread(rng, (B, N), -3, 1).astype(np.float32), delays=np.asarray(delays, dtype=np.int32),
                A=np.zeros((H, n, n)), b=np.ones((H, n)), c=np.ones((H, n)), d=np.zeros(H), p=np.zeros((H, n)))


def _shifted(x, m):
    out = np.zeros_like(x)
    if m < x.shape[1]:
        out[:, m:] = x[:, :x.shape[1] - m]
    return out


@pytest.mark.parametrize("m", [64, 65, 100, 256, 257, 300])
def test_a_pure_delay_shifts_bit_for_bit(m):
    """A = 0, b = c = 1, d = 0, p = 0, one line a set: y is x shifted by m with exact zeros in front, and gx is gy advanced."""
    N = 3 * m + 17
    i = _plain(3, 3, N, [[m], [m + 1], [N + 1]], m)
    out = _call(i, ("y", "gx"))
    out["y"].check("y"), out["gx"].check("gx")
    y, gx = out["y"].numpy(), out["gx"].numpy()
    for row, lag in enumerate((m, m + 1, N + 1)):
        assert np.array_equal(y[row:row + 1].view(np.uint32), _shifted(i["x"][row:row + 1], lag).view(np.uint32)), lag
        back = _shifted(i["gy"][row:row + 1, ::-1], lag)[:, ::-1]
        assert np.array_equal(gx[row:row + 1].view(np.uint32), np.ascontiguousarray(back).view(np.uint32)), lag


@pytest.mark.parametrize("delays", [(64, 65, 100), (100, 127, 128, 129), F.D16], ids=lambda d: f"{len(d)}lines")
def test_a_permutation_sends_an_impulse_round(delays):
    """A the cyclic permutation (line j feeds line j + 1), the input into line 0 alone, unit gains: an impulse comes out as
    exact impulses at m_0, m_0 + m_1, ... round and round."""
    n, N = len(delays), 3 * sum(delays) // 2 + 17
    i = _plain(1, 1, N, [delays], n)
    i["A"][0] = np.roll(np.eye(n), 1, axis=0)
    i["b"][0, 1:] = 0.0
    i["x"][:] = 0.0
    i["x"][0, 3] = np.float32(0.37)
    want, t, j = np.zeros((1, N), np.float32), 3, 0
    while t + delays[j % n] < N:
        t, j = t + delays[j % n], j + 1
        want[0, t] = np.float32(0.37)
    assert j > n   # more than one round
    out = _call(i, ("y",))
    out["y"].check("y")
    assert np.array_equal(out["y"].numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("case", [(4, 2, 317, F.D3, "damp"), (2, 1, 209, F.D16, "damp")], ids=F.case_id)
def test_no_wet_path_returns_the_bits_of_x(case):
    i = dict(F.inputs(case))
    i["c"], i["d"] = np.zeros_like(i["c"]), np.ones_like(i["d"])
    out = _call(i, ("y",))
    out["y"].check("y")
    assert np.array_equal(out["y"].numpy().view(np.uint32), (i["x"] + np.float32(0)).view(np.uint32))


def test_a_nan_stays_in_its_row():
    case = (4, 2, 317, F.D3, "damp")
    i, _, _, clean, _ = _run(case)
    bad = dict(i, x=i["x"].copy(), gy=i["gy"].copy())
    bad["x"][1, 5] = np.nan
    bad["gy"][1, 300] = np.nan
    out = _call(bad)
    for k in ("y", "state", "gx") + F.GRADS:
        _outside_untouched(out[k], k)
    rest = [0, 2, 3]
    for k in ("y", "state", "gx"):
        got, want = out[k].numpy(), clean[k].numpy()
        assert got[rest].tobytes() == want[rest].tobytes(), k
    assert np.isnan(out["y"].numpy()[1, 5]) and np.isfinite(out["y"].numpy()[1, :5]).all() and np.isnan(out["gx"].numpy()[1]).any()
    for k in F.GRADS:   # row 1 belongs to set 1: set 0 keeps its bits, set 1 is lost
        got, want = out[k].numpy(), clean[k].numpy()
        assert got[0].tobytes() == want[0].tobytes() and np.isnan(got[1]).all(), k


def test_zero_gradient_gives_exact_zeros():
    i = dict(F.inputs((4, 2, 317, F.D3, "damp")))
    i["gy"] = np.zeros_like(i["gy"])
    out = _call(i)
    for k in OUTS:
        out[k].check(k)
        assert not out[k].numpy().any(), k


def test_more_than_one_chunk_of_the_parameter_sums():
    """N = 2 FDN_CHUNK + 1 with long delays (three circulations): the chunked sums and their join."""
    case = (4, 2, 2 * F.CHUNK + 1, (700, 811, 1001), "damp")
    i, f, b = F.reference(case)
    out, again = _call(i), _call(i)
    for k in ("y", "state"):
        out[k].check(k)
        assert _ratio("fdn.chunks." + k, None, out[k].numpy(), f[k], f[k + "_bound"]) <= 1.0
    for k in OUTS:
        out[k].check(k)
        assert _same_bits(out[k], again[k]), k
        assert _ratio("fdn.chunks." + k, None, out[k].numpy(), b[k], b[k + "_bound"]) <= 1.0, k


def test_workspace_bytes():
    _, L = _lib()
    for a in [(0, 1, 1, 1), (65536, 1, 1, 1), (1, 0, 1, 1), (2, 3, 1, 1), (3, 2, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 17)]:
        assert L.ds_fdn_workspace_bytes(*a) == 0
    for B, H, N, n in [(1, 1, 1, 1), (6, 3, 5000, 5), (64, 1, 32000, 16)]:
        assert L.ds_fdn_workspace_bytes(B, H, N, n) == 8 * B * (n * N + -(-N // F.CHUNK) * (n * n + 3 * n + 1))
