"""The Sinkhorn divergence's fp64 oracle (tests/_sinkhorn_ref.py) on its own - closed forms and finite differences -
and the front end's checks that need no device: SamplesLoss options, shapes, and the compat/geomloss shim."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sinkhorn_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clouds(seed, B, N, D, scale=1.0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((B, N, D)) * scale


def test_two_diracs():
    x = np.array([[0.3, -1.2, 0.5]])
    y = np.array([[1.1, 0.4, -0.7]])
    S, gx, gy, _, _ = ref.oracle(x, y, blur=0.05)
    want = ((x - y) ** 2).sum() / 2
    assert abs(S[0] - want) <= 1e-12 * want
    np.testing.assert_allclose(gx, x - y, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gy, y - x, rtol=1e-12, atol=1e-12)


def test_translated_copy():
    """S(x, x + t) = |t|^2 / 2 exactly (translation equivariance of every step), without convergence."""
    x = _clouds(0, 2, 129, 4)
    t = np.array([0.7, -0.3, 0.2, 1.1])
    S, _, _, eps, _ = ref.oracle(x, x + t, blur=0.05)
    want = (t ** 2).sum() / 2
    print("translated copy: S", S, "want", want, "steps", len(eps))
    np.testing.assert_allclose(S, want, rtol=1e-8)


def test_identical_clouds():
    x = _clouds(1, 2, 129, 4)
    S, gx, gy, _, _ = ref.oracle(x, x.copy(), blur=0.05)
    assert np.abs(S).max() <= 1e-8 * (x ** 2).sum(-1).max()
    assert np.abs(gx).max() <= 1e-8 and np.abs(gy).max() <= 1e-8


def test_schedule_follows_numpy_arange():
    eps = ref.eps_schedule(2.0, 0.01, 0.5)
    assert eps[0] == 4.0 and eps[-1] == 0.01 ** 2
    inner = np.exp(np.arange(2 * np.log(2.0), 2 * np.log(0.01), 2 * np.log(0.5)))
    assert np.array_equal(np.array(eps[1:-1]), inner)
    from diffsound_amd.ddsp.sinkhorn import eps_schedule

    assert eps_schedule(2.0, 0.01, 0.5) == eps


@pytest.mark.parametrize("debias", [True, False])
def test_gradient_formula_matches_finite_differences(debias):
    """At convergence (averaged updates at blur^2 until the last change < 1e-12) S is stationary in the potentials,
    so the last step's gradient formula is the derivative of S: central differences agree."""
    rng = np.random.default_rng(3)
    B, N, M, D = 1, 6, 5, 2
    x, y = rng.standard_normal((B, N, D)), rng.standard_normal((B, M, D))
    a = rng.uniform(0.5, 1.5, (B, N))
    b = rng.uniform(0.5, 1.5, (B, M))
    a /= a.sum(1, keepdims=True)
    b /= b.sum(1, keepdims=True)
    kw = dict(blur=0.5, diameter_=4.0, debias=debias, converge=True)
    S, gx, gy, _, res = ref.oracle(x, y, a, b, **kw)
    assert res.max() < 1e-12
    h = 1e-5
    for arr, g in ((x, gx), (y, gy)):
        fd = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            old = arr[idx]
            arr[idx] = old + h
            sp = ref.oracle(x, y, a, b, **kw)[0].sum()
            arr[idx] = old - h
            sm = ref.oracle(x, y, a, b, **kw)[0].sum()
            arr[idx] = old
            fd[idx] = (sp - sm) / (2 * h)
        err = np.abs(fd - g).max() / np.abs(g).max()
        print(f"debias={debias}: max |fd - formula| / max |formula| = {err:.2e}")
        assert err < 1e-6


# ---- front end: checks that happen before any device work ----

def test_samplesloss_refuses_options_outside_the_contract():
    from diffsound_amd.ddsp.sinkhorn import SamplesLoss

    for kw, word in ((dict(loss="gaussian"), "loss"), (dict(loss="energy"), "loss"), (dict(p=1), "p"),
                     (dict(reach=1.0), "reach"), (dict(potentials=True), "potentials"),
                     (dict(cost=lambda x, y: x), "cost"), (dict(kernel=lambda x, y: x), "kernel"),
                     (dict(backend="multiscale"), "multiscale")):
        with pytest.raises(ValueError, match=word) as ei:
            SamplesLoss(**kw)
        assert "geomloss" in str(ei.value)
    for kw in (dict(blur=0.0), dict(blur=-1.0), dict(scaling=1.0), dict(scaling=0.0), dict(diameter=0.0)):
        with pytest.raises(ValueError):
            SamplesLoss(**kw)
    L = SamplesLoss(loss="sinkhorn", p=2, blur=0.01)  # what the reference's spectral loss constructs
    assert (L.blur, L.scaling, L.debias) == (0.01, 0.5, True)


def test_samplesloss_refuses_bad_input_before_device_work():
    from diffsound_amd.ddsp.sinkhorn import SamplesLoss, sinkhorn_divergence

    L = SamplesLoss(blur=0.01)
    x = torch.zeros(5, 3)
    with pytest.raises(ValueError, match="HIP device"):
        L(x, torch.zeros(4, 3))  # CPU tensors: no CPU path
    with pytest.raises(ValueError, match="D"):
        L(x, torch.zeros(4, 2))
    with pytest.raises(ValueError, match="batched"):
        L(x, torch.zeros(1, 4, 3))
    with pytest.raises(ValueError, match="batch size"):
        L(torch.zeros(2, 5, 3), torch.zeros(3, 4, 3))
    with pytest.raises(ValueError, match="weights a"):
        L(torch.ones(4), x, torch.ones(4), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="loss\\(x, y\\)"):
        L(x)
    with pytest.raises(ValueError, match="D <="):
        sinkhorn_divergence(torch.zeros(2, 33), torch.zeros(2, 33))
    big = torch.empty(10001, 3)
    with pytest.raises(ValueError, match="multiscale"):
        L(big, torch.empty(10001, 3))


def test_compat_shim_is_opt_in(monkeypatch):
    """``import geomloss`` with compat/ in front of sys.path yields the native class; the directory holds only it."""
    from diffsound_amd.ddsp.sinkhorn import SamplesLoss

    assert sorted(os.listdir(os.path.join(ROOT, "compat"))) == ["geomloss"]
    saved = sys.modules.pop("geomloss", None)
    try:
        monkeypatch.syspath_prepend(os.path.join(ROOT, "compat"))
        import geomloss

        assert geomloss.SamplesLoss is SamplesLoss
        assert os.path.dirname(geomloss.__file__) == os.path.join(ROOT, "compat", "geomloss")
    finally:  # leave the process as it was: the shim stays opt-in for the tests that follow
        sys.modules.pop("geomloss", None)
        if saved is not None:
            sys.modules["geomloss"] = saved
