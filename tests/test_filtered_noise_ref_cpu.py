"""Anchors of tests/_filtered_noise_ref.py (no GPU), at the shapes of tests/test_filtered_noise_kernels_gpu.py: the fp64
direct-sum references against the oracle's FFT restatement, the imported reference's saved outputs and fp64 autograd of
the torch.fft formulation; every bound against a CPU model of the kernels' roundings; and the same model with one fault
planted at a time - a bound that holds must also see a wrong kernel.

Tolerances, as measured on the CPU (printed by each test, ``pytest -s``), relative to the largest element:
  reference vs oracle.oscillator.filtered_noise, vs the fp64 torch.fft formulation, backward vs its fp64 autograd:
      at most 1.8e-15 over all cases and both gains -> FP64_TOL = 1e-13.  Both sides are fp64; the FFT side carries
      O(log2(T + F)) 2^-53 per element and the direct sums O(sqrt(L)) 2^-53, so 1e-13 leaves a factor 50 and is still
      six orders of magnitude below the fp32 effects the bounds are about.
  reference vs fn_signal / fn_grad_bank of g7_real_audio.npz (fp32 outputs of the imported reference's fp32 FFT chain):
      3.2e-7 for either (rel-L2 1.9e-7 / 2.3e-7) -> GOLDEN_TOL = 2e-6, the tolerance tests/test_oracle_golden.py gives
      the oracle for the same array: a few fp32 roundings in pocketfft's butterflies.
The single-sample case is exactly 0 in the direct-sum form (out[0] = noise[0] h[0] and w_0 = 0) and ~1e-16 through the
FFTs, whose frames hold elements of size |h| before the cut; errors are therefore taken relative to the largest element or,
if that is larger, to the size of one term of the sum: |gain| max |h| for the output (|noise| <= 1) and |gain| max |gy|
max (dmag) / T for the gradient.
Largest error / bound ratio of the rounding model over all cases: h 0.40, out 0.17, gc 0.42."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filtered_noise_ref as R  # noqa: E402
from _guarded import _id  # noqa: E402
from oracle import oscillator as oosc  # noqa: E402

FP64_TOL = 1e-13
GOLDEN_TOL = 2e-6
CASES = [(c, g) for c in R.SHAPES for g in R.GAINS]


def _cid(p):
    return f"{_id(p[0])}-gain{p[1]}"


def _rel(got, ref, term=0.0):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), term))


def _terms(c, gy, gain):
    """Size of one term of an output sample's and of a gradient element's sum (see the module docstring)."""
    return (abs(gain) * np.abs(R.impulse(c)).max(),
            abs(gain) * np.abs(gy).max() * R.dmag(c).max() / (2 * c.shape[-1] - 1))


def _worst(err, bound):
    """Largest |err| / bound; a zero bound admits only an exact match."""
    err = np.abs(err)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)).max())


@functools.lru_cache(maxsize=None)
def _refs(case, gain):
    """References and bounds of one case, computed once and left unchanged."""
    B, L, F, S = case
    c, noise, gy = R.inputs(case)
    return dict(c=c, noise=noise, gy=gy, out=R.forward(c, noise, S, F, gain), gc=R.backward(gy, c, noise, S, F, gain),
                b_out=R.bound_forward(c, noise, S, F, gain), b_gc=R.bound_backward(gy, c, noise, S, F, gain))


# ------------------------------------------------------------------------------ references vs oracle and torch
@pytest.mark.parametrize("case,gain", CASES, ids=map(_cid, CASES))
def test_reference_matches_oracle_and_autograd(case, gain):
    B, L, F, S = case
    r = _refs(case, gain)
    c, noise, gy = r["c"], r["noise"], r["gy"]
    assert r["out"].shape == (B, S) and r["gc"].shape == c.shape == (B, R.n_frames(S, F), L)
    t_out, t_gc = _terms(c, gy, gain)
    e_oracle = _rel(r["out"], oosc.filtered_noise(c, noise, S, F, gain), t_out)
    ct = torch.from_numpy(c).double().requires_grad_(True)
    out = R.torch_formulation(ct, torch.from_numpy(noise).double(), S, F, gain)
    (out * torch.from_numpy(gy).double()).sum().backward()
    e_torch = _rel(r["out"], out.detach().numpy(), t_out)
    e_grad = _rel(r["gc"], ct.grad.numpy(), t_gc)
    print(f"reference {_cid((case, gain))}: oracle {e_oracle:.1e} torch {e_torch:.1e} autograd {e_grad:.1e}")
    assert max(e_oracle, e_torch, e_grad) <= FP64_TOL
    dead = np.arange(R.n_frames(S, F)) * F >= S  # the last frame when F divides S
    assert dead.any() == (S % F == 0) and not r["gc"][:, dead].any()


def test_reference_matches_the_imported_reference(golden):
    g = golden("g7_real_audio.npz")
    bank, noise = g["fn_bank"], g["fn_noise"]
    assert bank.shape == (3, 126, 65) and noise.shape == (3, 126, 64)
    out = R.forward(bank, noise, 8000, 64)
    e_sig = _rel(out, g["fn_signal"])
    gc = R.backward(2.0 * out / out.size, bank, noise, 8000, 64)  # tests/golden/make_golden.py: (y ** 2).mean().backward()
    e_grad = _rel(gc, g["fn_grad_bank"])
    print(f"reference vs golden: signal {e_sig:.1e} grad {e_grad:.1e}")
    assert e_sig <= GOLDEN_TOL and e_grad <= GOLDEN_TOL
    assert _rel(out, oosc.filtered_noise(bank, noise, 8000)) <= FP64_TOL


def test_backward_is_the_adjoint_in_noise_free_form():
    """<gy, forward> is linear in h: d / dh of it, chained through ``impulse`` by finite differences in fp64, is gc."""
    case = (2, 5, 3, 20)
    B, L, F, S = case
    c, noise, gy = R.inputs(case)
    c = c.astype(np.float64)
    gc = R.backward(gy, c, noise, S, F, 0.7)
    eps = 1e-6
    for idx in [(0, 0, 0), (1, 3, 2), (0, 6, 4), (1, 5, 1)]:
        cp, cm = c.copy(), c.copy()
        cp[idx] += eps
        cm[idx] -= eps
        fd = ((R.forward(cp, noise, S, F, 0.7) - R.forward(cm, noise, S, F, 0.7)) * gy).sum() / (2 * eps)
        assert abs(fd - gc[idx]) <= 1e-8 * max(1.0, abs(gc[idx]))  # central difference: eps^2 f''' ~ 1e-12, rounding 1e-10


# ------------------------------------------------------------------------------------ the model and the bounds
@pytest.mark.parametrize("case,gain", CASES, ids=map(_cid, CASES))
def test_rounding_model_stays_inside_the_bounds(case, gain):
    B, L, F, S = case
    r = _refs(case, gain)
    m = R.round_like_kernel(r["c"], r["noise"], S, F, gain, r["gy"])
    worst = dict(h=_worst(m["h"] - R.impulse(r["c"]), R.bound_impulse(r["c"])), out=_worst(m["out"] - r["out"], r["b_out"]),
                 gc=_worst(m["gc"] - r["gc"], r["b_gc"]))
    print(f"model {_cid((case, gain))}: " + " ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0
    assert (r["b_out"] >= 0).all() and (r["b_gc"] >= 0).all()
    # the bounds are rounding-sized: nowhere above 1e-3 of the largest element (at the upper limits gamma_M = 3e-5 for the
    # M = 514 products of a sample, whose absolute sum is about sqrt(M) = 20 times a typical |sum|)
    t_out, t_gc = _terms(r["c"], r["gy"], gain)
    assert r["b_out"].max() <= 1e-3 * max(np.abs(r["out"]).max(), t_out)
    assert r["b_gc"].max() <= 1e-3 * max(np.abs(r["gc"]).max(), t_gc)


def _shows(fault, case):
    """Whether ``fault`` changes any output of ``case`` at all.  The single sample is noise[0] h[0] with w_0 = 0: exactly 0
    whatever the window, roll or doubling, with zero gradient (only reading past S shows there).  The oldest frame is one
    of several only from sample reach F on."""
    B, L, F, S = case
    if fault == "tail":
        return True
    if S == 1:
        return False
    if fault == "oldest_frame":
        return S > ((2 * L - 1 + F - 2) // F) * F
    return True


_PLANTED = [(f, c) for f in R.FAULTS for c in R.SHAPES if _shows(f, c)]


@pytest.mark.parametrize("fault,case", _PLANTED, ids=[f"{f}-{_id(c)}" for f, c in _PLANTED])
def test_planted_fault_leaves_the_bounds(fault, case):
    B, L, F, S = case
    gain = R.GAINS[1]
    r = _refs(case, gain)
    m = R.round_like_kernel(r["c"], r["noise"], S, F, gain, r["gy"], fault=fault)
    seen = []
    if fault in R.FORWARD_FAULTS:
        seen.append(_worst(m["out"] - r["out"], r["b_out"]))
    if fault in R.BACKWARD_FAULTS:
        seen.append(_worst(m["gc"] - r["gc"], r["b_gc"]))
    print(f"fault {fault} {_id(case)}: " + " ".join(f"{v:.3g}" for v in seen))
    assert min(seen) > 1.0  # every output the fault touches, not just one of them


def test_every_fault_is_planted_somewhere():
    assert {f for f, _ in _PLANTED} == set(R.FAULTS)
    assert set(R.FORWARD_FAULTS) | set(R.BACKWARD_FAULTS) == set(R.FAULTS)
