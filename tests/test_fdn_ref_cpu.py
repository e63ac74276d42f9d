"""The reference of tests/_fdn_ref.py is anchored without a GPU: against a sample-by-sample numpy.longdouble loop inside its
own bound, against the closed-form comb, every gradient formula against central differences in fp64, the energy an
orthogonal loop keeps, and the module's closed-form ``response`` against the FFT of the reference's impulse response."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fdn_ref as F  # noqa: E402

LD = np.longdouble
LOOP_CASES = [(2, 1, 102, F.D3, "damp"), (4, 2, 317, F.D3, "damp"), (4, 2, 317, F.D3, "null"), (2, 1, 209, F.D16, "damp"),
              (2, 1, 200, (64, 198, 199, 200, 201), "damp"), (1, 1, 150, (149,), "damp")]


def _longdouble(i):
    """state, y, r, gx and the five parameter sums, one sample at a time in longdouble."""
    x, gy = i["x"].astype(LD), i["gy"].astype(LD)
    B, N = x.shape
    m, A, b, c, d, p = F._sets(B, *[i[k] for k in F.PARAMS])
    A, b, c, d, p = (a.astype(LD) for a in (A, b, c, d, p))
    H, n = i["delays"].shape
    bi, ji = np.arange(B)[:, None], np.arange(n)[None, :]

    def at(a, u, lo, hi):
        return np.where((u >= lo) & (u < hi), a[bi, ji, np.clip(u, 0, N - 1)], LD(0))

    s, q, y = np.zeros((B, n, N), LD), np.zeros((B, n, N), LD), np.zeros((B, N), LD)
    for t in range(N):
        q[:, :, t] = (1 - p) * at(s, t - m, 0, N) + p * at(s, t - m - 1, 0, N)
        s[:, :, t] = b * x[:, t:t + 1] + np.einsum("bij,bj->bi", A, q[:, :, t])
        y[:, t] = d * x[:, t] + (c * q[:, :, t]).sum(1)
    r, l, gx = np.zeros((B, n, N), LD), np.zeros((B, n, N), LD), np.zeros((B, N), LD)
    for t in range(N - 1, -1, -1):
        l[:, :, t] = (1 - p) * at(r, t + m, 0, N) + p * at(r, t + m + 1, 0, N)
        r[:, :, t] = c * gy[:, t:t + 1] + np.einsum("bij,bi->bj", A, l[:, :, t])
        gx[:, t] = d * gy[:, t] + (b * l[:, :, t]).sum(1)
    u = np.arange(N)[None, None, :] - m[:, :, None]
    along = lambda v: np.where(v >= 0, np.take_along_axis(s, np.maximum(v, 0), 2), LD(0))
    D = along(u - 1) - along(u)
    fold = lambda a: a.reshape((B // H, H) + a.shape[1:]).sum(0)
    sums = dict(gA=np.einsum("bit,bjt->bij", l, q), gb=np.einsum("bit,bt->bi", l, x), gc=np.einsum("bt,bjt->bj", gy, q),
                gd=np.einsum("bt,bt->b", gy, x), gp=np.einsum("bjt,bjt->bj", r, D))
    return dict(state=s, y=y, r=r, gx=gx, **{k: fold(v) for k, v in sums.items()})


@pytest.mark.parametrize("case", LOOP_CASES, ids=F.case_id)
def test_reference_against_longdouble(case):
    """The blocked fp64 reference against the plain loop, every element inside the reference's own bound (without the fp32
    store): the bound's derivation grants the kernel no more."""
    i, f, b = F.reference(case)
    ld = _longdouble(i)
    for name, ref, bound in [("state", f["state"], f["state_bound"]), ("y", f["y"], f["y_bound64"]), ("r", b["r"], b["r_bound"]),
                             ("gx", b["gx"], b["gx_bound64"])] + [(k, b[k], b[k + "_bound"]) for k in F.GRADS]:
        err = np.abs((ref.astype(LD) - ld[name]).astype(np.float64))
        assert (err <= bound).all(), (name, float((err / np.where(bound > 0, bound, 1)).max()))
        assert np.isfinite(bound).all() and (bound[np.abs(ref) > 0] > 0).all(), name
    # the bound still says something: at most 1e-12 of the largest magnitude
    assert f["state_bound"].max() <= 1e-12 * np.abs(f["state"]).max() and b["gA_bound"].max() <= 1e-11 * np.abs(b["gA"]).max()


def test_cases_cover_the_block_loop():
    ids = [F.case_id(c) for c in F.CASES]
    assert len(set(ids)) == len(ids)
    for delays in (F.D3, F.D3_LONG):
        T, mn = F.block_length(delays), min(delays)
        assert {1, T - 1, T, T + 1, mn, mn + 1, mn + 2, 3 * mn + 17} <= {c[2] for c in F.CASES if c[3] == delays}
    assert F.block_length(F.D3) == 100 and F.block_length(F.D3_LONG) == F.THREADS and min(F.D3) % 64
    assert {64, 65, 100, 127, 128, 129} <= {c[3][0] for c in F.CASES if len(c[3]) == 1}
    assert {1, 2, 3, 16} <= {len(c[3]) for c in F.CASES} and {(1, 1), (3, 1), (4, 2), (3, 3)} <= {c[:2] for c in F.CASES}
    assert {"null", "zero", "damp"} == {c[4] for c in F.CASES}
    assert {c[3][0] - c[2] for c in F.CASES if len(c[3]) == 1 and c[2] == 150} == {-2, -1, 0, 1}
    assert max(c[2] / min(c[3]) for c in F.CASES) < 3.3
    i = F.inputs((4, 2, 317, F.D3, "damp"))
    assert i["p"].max() == 0.5 and i["p"].min() > 0 and (i["delays"][1] == i["delays"][0] + 3).all()
    a = np.abs(i["x"][i["x"] != 0])
    assert a.max() / a.min() > 1e3 and (i["x"] == 0).any()


@pytest.mark.parametrize("m,N", [(64, 300), (100, 100), (7, 50)])
def test_one_line_is_the_comb(m, N):
    """n = 1, p = 0: y[t] = d x[t] + c sum_k A^k x[t - (k + 1) m]."""
    rng = np.random.default_rng(m)
    x = rng.standard_normal((2, N))
    A, c, d = 0.8, -1.3, 0.7
    f = F.forward(x, [[m]], [[[A]]], [[1.0]], [[c]], [d])
    want = d * x
    for k in range(N // m + 1):
        lag = (k + 1) * m
        if lag < N:
            want[:, lag:] += c * A ** k * x[:, :N - lag]
    assert np.abs(f["y"] - want).max() <= 1e-14 * np.abs(want).max()


@pytest.mark.parametrize("case", [(2, 1, 230, (64, 71, 90), "damp"), (4, 2, 150, (64, 70), "damp"), (1, 1, 150, (148,), "damp")],
                         ids=F.case_id)
def test_every_gradient_against_central_differences(case):
    """L = sum gy y.  Every entry of A, b, c, d, p and eight samples of x, perturbed by +-h in fp64."""
    i = F.inputs(case)
    par = {k: (None if i[k] is None else np.array(i[k], dtype=np.float64 if k != "delays" else np.int32)) for k in F.PARAMS}
    x, gy = i["x"].astype(np.float64), i["gy"].astype(np.float64)
    loss = lambda x_, par_: float((gy * F.forward(x_, *[par_[k] for k in F.PARAMS])["y"]).sum())
    b = F.backward(gy, x, *[par[k] for k in F.PARAMS])
    scale = np.abs(gy).max() * np.abs(x).max()

    def check(name, got, perturb):
        for idx in np.ndindex(got.shape):
            h = 1e-6
            fd = (loss(*perturb(idx, +h)) - loss(*perturb(idx, -h))) / (2 * h)
            assert abs(fd - got[idx]) <= 1e-7 * max(abs(got[idx]), scale), (name, idx, fd, got[idx])

    def shifted(key):
        def f(idx, h):
            q = dict(par)
            q[key] = par[key].copy()
            q[key][idx] += h
            return x, q
        return f

    for g, key in (("gA", "A"), ("gb", "b"), ("gc", "c"), ("gd", "d"), ("gp", "p")):
        check(g, b[g], shifted(key))
    B, N = x.shape
    picks = [(r, t) for r in range(B) for t in (0, 1, N // 3, N - 1)][:8]

    def xshift(idx, h):
        x_ = x.copy()
        x_[picks[idx[0]]] += h
        return x_, par
    check("gx", np.array([b["gx"][pk] for pk in picks]), xshift)


def test_an_orthogonal_loop_keeps_the_energy_of_an_impulse():
    """p = 0 and A orthogonal: what the lines hold, sum_j sum_{u in (t - m_j, t]} s_j[u]^2, stays |b|^2 for ever."""
    rng = np.random.default_rng(5)
    delays = np.array([[64, 71, 97, 130]])
    n, N = 4, 1200   # nine circulations of the longest line
    x = np.zeros((1, N))
    x[0, 0] = 1.0
    b = rng.standard_normal((1, n))
    f = F.forward(x, delays, F.orthogonal(rng, n)[None], b, np.zeros((1, n)), [0.0], None)
    s2 = np.cumsum(f["state"][0] ** 2, 1)
    for t in range(int(delays.max()), N):
        held = sum(s2[j, t] - s2[j, t - delays[0, j]] for j in range(n))
        assert abs(held - (b ** 2).sum()) <= 1e-13 * (b ** 2).sum(), t


def test_response_is_the_transform_of_the_impulse_response():
    """The module's closed form at the DFT frequencies against the FFT of the reference's impulse response, run until it is
    below 1e-12 of its peak: rt60 = 0.1 s at 8 kHz is 800 samples for 60 dB, 4096 samples are 307 dB."""
    from diffsound_amd.ddsp.fdn import FeedbackDelayNetwork

    sr, N = 8000.0, 4096
    net = FeedbackDelayNetwork(2, 4, sr, [0.1, 0.08], delays=[[67, 89, 113, 149], [64, 90, 121, 160]], damp=0.2, wet_db=-3.0,
                               init="wet")
    with torch.no_grad():
        net.S.copy_(0.3 * torch.randn((2, 4, 4), dtype=torch.float64, generator=torch.Generator().manual_seed(3)))
    A, b, c, d, p = (t.detach().numpy() for t in net.coefficients())
    U = net.mixing().detach().numpy()
    assert np.abs(U @ U.transpose(0, 2, 1) - np.eye(4)).max() <= 1e-14
    x = np.zeros((2, N))
    x[:, 0] = 1.0
    ir = F.forward(x, net.delays.numpy(), A, b, c, d, p)["y"]
    assert np.abs(ir[:, -200:]).max() <= 1e-12 * np.abs(ir[:, 1:]).max()
    freqs = np.arange(N // 2 + 1) * sr / N
    got = net.response(freqs)
    assert got.dtype == torch.complex128 and got.shape == (2, N // 2 + 1) and got.requires_grad
    assert np.abs(got.detach().numpy() - np.fft.rfft(ir, axis=1)).max() <= 1e-10


def test_default_delays_are_what_the_docstring_says():
    from diffsound_amd.ddsp.fdn import _is_prime, default_delays

    for n, sr in ((1, 32000), (8, 32000), (16, 16000), (16, 48000)):
        got = default_delays(n, sr)
        assert len(set(got)) == n and all(_is_prime(k) for k in got) and got == sorted(got)
        for j, k in enumerate(got):
            target = sr * 0.02 * 5.0 ** (j / max(n - 1, 1))
            assert abs(k - target) <= 0.01 * target    # primes are dense enough here
    assert default_delays(8, 32000)[0] == 641 and default_delays(8, 32000) == default_delays(8, 32000)
