"""The two kernels of diffsound_amd/csrc/filtered_noise.hip behind ds_filtered_noise_fwd / ds_filtered_noise_bwd, and the
FilteredNoise module on them, element by element against the fp64 references of tests/_filtered_noise_ref.py at the bounds
derived there (tests/test_filtered_noise_ref_cpu.py anchors both without a GPU and shows that the bounds see planted faults).

Every output lives 64 elements inside a NaN-filled buffer: after a call both guard zones must still be NaN and the output
finite, so every element is written and nothing else is.  A second call of either entry point must be bitwise equal.
Each case prints its largest error / bound ratio per output (``pytest -s``).

Worst error / bound ratio per output over all cases: MI355X as measured, and the CPU model of the kernels' roundings
(_filtered_noise_ref.round_like_kernel):

    output              MI355X   CPU model
    abi.out             0.173    0.173
    abi.gc              0.418    0.418
    golden.out          0.0643   0.0643
    golden.gc           0.0073   -
    module.out          0.0834   0.0834
    module.gc           0.0039   0.0047   (the model on another gy)
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _filtered_noise_ref as R  # noqa: E402
from _guarded import PAD, Guarded, _id, _lib, _ratio, _up, dev as _dev, same_on_other_device  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(c, g) for c in R.SHAPES for g in R.GAINS]


def _cid(p):
    return f"{_id(p[0])}-gain{p[1]}"


def _fwd_call(d_c, d_noise, B, L, F, S, gain):
    _hip, lib = _lib()
    out = Guarded((B, S))
    _hip.check(lib.ds_filtered_noise_fwd(_hip.ptr(d_c), _hip.ptr(d_noise), B, S, L, F, gain, out.ptr, _hip.stream_ptr()),
               "ds_filtered_noise_fwd")
    torch.cuda.synchronize()
    return out


def _bwd_call(d_gy, d_c, d_noise, B, L, F, S, gain):
    _hip, lib = _lib()
    gc = Guarded((B, R.n_frames(S, F), L))
    _hip.check(lib.ds_filtered_noise_bwd(_hip.ptr(d_gy), _hip.ptr(d_c), _hip.ptr(d_noise), B, S, L, F, gain, gc.ptr,
                                         _hip.stream_ptr()), "ds_filtered_noise_bwd")
    torch.cuda.synchronize()
    return gc


def _check_case(tag, case, gain, c, noise, gy):
    B, L, F, S = case
    d_c, d_noise = _up(c), _up(noise)
    # gy sits flush against the end of its allocation's payload inside a NaN-filled buffer: a read past S would be NaN
    g_gy = Guarded((B, S))
    g_gy.buf[PAD:PAD + B * S] = _up(gy).reshape(-1)
    d_gy = g_gy.buf[PAD:PAD + B * S]
    out, again = (_fwd_call(d_c, d_noise, B, L, F, S, gain) for _ in range(2))
    gc, gc_again = (_bwd_call(d_gy, d_c, d_noise, B, L, F, S, gain) for _ in range(2))
    for o, what in ((out, "out"), (again, "out, second call"), (gc, "gc"), (gc_again, "gc, second call")):
        o.check(what)
    assert np.array_equal(out.numpy(), again.numpy()) and np.array_equal(gc.numpy(), gc_again.numpy())  # deterministic
    assert torch.equal(d_c, _up(c)) and torch.equal(d_noise, _up(noise))  # inputs are read only
    worst = [_ratio(tag + ".out", (*case, gain), out.numpy(), R.forward(c, noise, S, F, gain), R.bound_forward(c, noise, S, F, gain)),
             _ratio(tag + ".gc", (*case, gain), gc.numpy(), R.backward(gy, c, noise, S, F, gain),
                    R.bound_backward(gy, c, noise, S, F, gain))]
    assert max(worst) <= 1.0
    dead = np.arange(R.n_frames(S, F)) * F >= S  # a frame that starts at or after S: exact zero gradient
    assert dead.any() == (S % F == 0) and not gc.numpy()[:, dead].any()


@pytest.mark.parametrize("case,gain", CASES, ids=map(_cid, CASES))
def test_kernels_against_fp64_reference(case, gain):
    _check_case("abi", case, gain, *R.inputs(case))


def test_kernels_on_the_golden_bank(golden):
    """S = 8000, B = 3: the bank and the draw of the imported reference; also its saved fp32 outputs, at the tolerances of
    tests/test_api_gpu.py::test_filtered_noise_matches_reference."""
    g = golden("g7_real_audio.npz")
    c, noise = g["fn_bank"], g["fn_noise"]
    gy = (2.0 * R.forward(c, noise, 8000, 64) / (3 * 8000)).astype(np.float32)  # d mean(y^2) / dy
    _check_case("golden", (3, 65, 64, 8000), 1.0, c, noise, gy)


_OK = dict(B=2, L=65, F=64, S=200)
_REFUSALS = [(fn, bad) for fn in ("ds_filtered_noise_fwd", "ds_filtered_noise_bwd") for bad in R.REFUSED]


@pytest.mark.parametrize("fn,bad", _REFUSALS, ids=[f"{f}-{b}" for f, b in _REFUSALS])
def test_refusals_name_the_argument_and_write_nothing(fn, bad):
    _hip, lib = _lib()
    a = dict(_OK)
    a.update(R.REFUSED[bad])
    ones = lambda *s: torch.ones(s, device=_dev())
    c, noise, gy = ones(2, 8, 130), ones(2, 8, 257), ones(2, 200)  # large enough for every shape tried
    p, st = _hip.ptr, _hip.stream_ptr()
    if fn == "ds_filtered_noise_fwd":
        out = Guarded((2, 200))
        rc = lib.ds_filtered_noise_fwd(p(c), p(noise), a["B"], a["S"], a["L"], a["F"], 1.0, out.ptr, st)
    else:
        out = Guarded((2, 8, 130))
        rc = lib.ds_filtered_noise_bwd(p(gy), p(c), p(noise), a["B"], a["S"], a["L"], a["F"], 1.0, out.ptr, st)
    torch.cuda.synchronize()
    assert rc != 0
    msg = lib.ds_last_error().decode()
    name = bad.split("=")[0]
    assert fn in msg and f"{name} (" in msg and bad.replace("=", " = ").split(" = ")[1] in msg, msg
    assert out.untouched()
    with pytest.raises(RuntimeError, match=fn):
        _hip.check(rc, fn)


# ------------------------------------------------------------------------------------------ through the module
def _kernel_names(fn):
    """Names of the device activities of one call of ``fn`` from torch's kernel tracer; [] where the tracer gives none."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower()]


def test_module_launches_no_fft(monkeypatch):
    """FilteredNoise(3, 8000) on the device calls no FFT, forward or backward; its device work is the uniform draw, ONE
    filtered-noise kernel forward and ONE backward."""
    from diffsound_amd.ddsp.oscillator import FilteredNoise

    fnz = FilteredNoise(3, 8000).to(_dev())

    def step():
        fnz.zero_grad()
        fnz().pow(2).mean().backward()

    step()  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    names = _kernel_names(step)
    print("device activities:", [n[:60] for n in names])
    if names:  # the tracer is not available under an outer profiler
        assert sum("filtered_noise_fwd_kernel" in n for n in names) == 1
        assert sum("filtered_noise_bwd_kernel" in n for n in names) == 1
        assert not any(w in n.lower() for n in names for w in ("fft", "col2im", "im2col")), names

    def refuse(*a, **k):
        raise AssertionError("FilteredNoise on the device called torch.fft")

    for name in ("rfft", "irfft", "fft", "ifft"):
        monkeypatch.setattr(torch.fft, name, refuse)
    step()
    assert torch.isfinite(fnz.coefficient_bank.grad).all() and float(fnz.coefficient_bank.grad.abs().max()) > 0


def test_module_matches_reference_and_is_deterministic(golden):
    from diffsound_amd.ddsp.oscillator import FilteredNoise

    g = golden("g7_real_audio.npz")
    c, noise = g["fn_bank"], g["fn_noise"]
    fnz = FilteredNoise(3, 8000, attenuate_gain=0.7).to(_dev())
    assert list(fnz.state_dict()) == ["coefficient_bank"] and fnz.coefficient_bank.shape == (3, 126, 65)
    with torch.no_grad():
        fnz.coefficient_bank.copy_(torch.from_numpy(c))
    d_noise = _up(noise)
    out = fnz(d_noise)
    assert out.shape == (3, 8000) and out.dtype == torch.float32
    gy = np.random.default_rng(23).standard_normal((3, 8000)).astype(np.float32)
    (out * _up(gy)).sum().backward()
    grad = fnz.coefficient_bank.grad
    worst = [_ratio("module.out", (3, 65, 64, 8000), out.detach().cpu().numpy(), R.forward(c, noise, 8000, 64, 0.7),
                    R.bound_forward(c, noise, 8000, 64, 0.7)),
             _ratio("module.gc", (3, 65, 64, 8000), grad.cpu().numpy(), R.backward(gy, c, noise, 8000, 64, 0.7),
                    R.bound_backward(gy, c, noise, 8000, 64, 0.7))]
    assert max(worst) <= 1.0
    assert torch.equal(fnz(d_noise), out)  # deterministic
    # the internal draw is torch.rand(B, nf, F) * 2 - 1 on the generator: a seeded call equals the injected same draw
    torch.manual_seed(5)
    drawn = fnz()
    torch.manual_seed(5)
    assert torch.equal(drawn, fnz(torch.rand(3, 126, 64, device=_dev()) * 2 - 1))
    # an injected noise that requires grad takes the torch formulation and gets its gradient
    nz = d_noise.clone().requires_grad_(True)
    slow = fnz(nz)
    slow.sum().backward()
    assert nz.grad is not None and float((slow.detach() - out.detach()).norm() / out.detach().norm()) < 1e-5


def test_sizes_outside_the_native_range_keep_working():
    """filter_coeff_length = 140 (> 129) and a CPU module: the torch formulation, as before."""
    from diffsound_amd.ddsp.oscillator import FilteredNoise

    big = FilteredNoise(2, 300, filter_coeff_length=140, frame_length=32).to(_dev())
    noise = torch.rand(2, 10, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1
    out = big(noise.to(_dev()))
    ref = R.forward(big.coefficient_bank.detach().cpu().numpy(), noise.numpy(), 300, 32)
    assert out.shape == (2, 300) and np.linalg.norm(out.detach().cpu().numpy() - ref) / np.linalg.norm(ref) < 1e-5
    out.sum().backward()
    assert torch.isfinite(big.coefficient_bank.grad).all()
    cpu = FilteredNoise(2, 300)
    o = cpu(noise[:, :5].repeat(1, 1, 2))
    ref = R.forward(cpu.coefficient_bank.detach().numpy(), noise[:, :5].repeat(1, 1, 2).numpy(), 300, 64)
    assert o.device.type == "cpu" and np.linalg.norm(o.detach().numpy() - ref) / np.linalg.norm(ref) < 1e-5


def test_gradient_reaches_the_bank_through_gt_oscillator():
    from diffsound_amd.ddsp.oscillator import GTDampedOscillator
    from diffsound_amd.diffelastic.material_model import Material

    forces = torch.zeros((2, 16), device=_dev())
    forces[:, 0] = 1
    torch.manual_seed(1)
    osc = GTDampedOscillator(forces, 2, 6, 1000, 32000, [20, 16000], Material((2700.0, 6.0e10, 0.25, 6.0, 1e-7))).cuda()
    clean = osc(noise_rate=0.0)
    assert osc.noise.coefficient_bank.grad is None
    torch.manual_seed(2)
    noisy = osc(noise_rate=1e-2)
    torch.manual_seed(2)
    branch = osc.noise()
    assert noisy.shape == (2, 1000) and torch.allclose(noisy - clean, branch * 1e-2, rtol=0, atol=1e-6)
    (noisy ** 2).mean().backward()
    g = osc.noise.coefficient_bank.grad
    assert g is not None and g.shape == (2, 1000 // 64 + 1, 65) and torch.isfinite(g).all()
    assert float(g.abs().max()) > 0 and float(osc.amp.value.grad.abs().max()) > 0
    # d mean(noisy^2) / d bank = backward(rate 2 noisy / n) on the same draw, at the gradient tolerance (rel-L2 1e-4) that
    # tests/test_api_gpu.py::test_filtered_noise_matches_reference gives the module
    torch.manual_seed(2)
    draw = (torch.rand(2, 16, 64, device=_dev()) * 2 - 1).cpu().numpy()
    gy = 2.0 * noisy.detach().double().cpu().numpy() / noisy.numel() * 1e-2
    ref = R.backward(gy, osc.noise.coefficient_bank.detach().cpu().numpy(), draw, 1000, 64)
    assert np.linalg.norm(g.cpu().numpy() - ref) / np.linalg.norm(ref) < 1e-4


def test_module_runs_on_its_parameters_device():
    """The smallest native clip (one sample, a 2-bin response, 1-sample frames), forward and backward, with the module off
    the current device."""
    from diffsound_amd.ddsp.filtered_noise import FilteredNoise

    bank, noise = torch.tensor([[[0.5, -0.25], [0.125, 1.0]]]), torch.tensor([[[0.75], [-0.5]]])

    def run(device):
        mod = FilteredNoise(1, 1, filter_coeff_length=2, frame_length=1).to(device)
        with torch.no_grad():
            mod.coefficient_bank.copy_(bank)
        y = mod(noise.to(device))
        return y.detach(), torch.autograd.grad(y.sum(), mod.coefficient_bank)[0]

    same_on_other_device(run)
