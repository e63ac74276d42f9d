"""What the kernel tests share (not a test module).  Guard zones for kernel outputs: an output placed PAD elements inside a
NaN-filled device buffer, so that a write before its start or past its end, or an element left unwritten, is seen after the
call.  And the small helpers: the library handle, uploads, case ids, the printed error / bound ratio and the comparisons of
two guarded outputs."""
import numpy as np
import pytest
import torch

PAD = 64


def dev():
    assert torch.cuda.is_available(), "needs a HIP device"
    return torch.device("cuda:0")


def _lib():
    from diffsound_amd import _hip

    return _hip, _hip.lib()


def _up(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _id(case):
    """A case tuple, with any shape tuple inside it spread out, joined by dashes: ((1, 5), "base") -> 1-5-base."""
    return "-".join(str(v) for c in case for v in (c if isinstance(c, tuple) else (c,)))


def _ratio(tag, case, got, ref, bound):
    """Largest |got - ref| / bound, printed as ``RATIO <tag> <case> <value>`` (no case: None); a zero bound admits only an
    exact match."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    worst = float(r.max())
    print(f"RATIO {tag} {_id(case)} {worst:.4g}" if case is not None else f"RATIO {tag} {worst:.4g}")
    return worst


def same_bits(a, b):
    """Two Guarded outputs hold the same bytes, guard zones included."""
    return np.array_equal(a.buf.cpu().numpy().view(np.uint8), b.buf.cpu().numpy().view(np.uint8))


def outside_untouched(g, what):
    """The guard zones of the Guarded ``g`` are still NaN, whatever the output itself holds."""
    whole = g.buf.cpu().numpy()
    assert np.isnan(whole[:PAD]).all() and np.isnan(whole[PAD + g.n:]).all(), f"{what}: written outside"


def same_on_other_device(run):
    """``run(device)`` builds its operands on ``device`` and returns a tuple of results.  Made with device 0 current and the
    operands on device 1, it gives what it gives with device 1 current, bit for bit, on device 1.  Skips on one device."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip(f"needs two HIP devices, {n} visible")
    other = torch.device("cuda:1")
    with torch.cuda.device(1):
        want = run(other)
    with torch.cuda.device(0):
        got = run(other)
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert g.device == other and g.dtype == w.dtype and g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()


class Guarded:
    """An output of ``shape`` placed PAD elements inside a NaN-filled buffer."""

    def __init__(self, shape, dtype=torch.float32):
        self.shape = tuple(shape)
        self.n = int(np.prod(self.shape))
        self.buf = torch.full((self.n + 2 * PAD,), float("nan"), dtype=dtype, device=dev())

    @property
    def ptr(self):
        return self.buf.data_ptr() + PAD * self.buf.element_size()

    def numpy(self):
        return self.buf[PAD:PAD + self.n].cpu().numpy().reshape(self.shape)

    def check(self, what):
        whole = self.buf.cpu().numpy()
        assert np.isnan(whole[:PAD]).all(), f"{what}: written before its start"
        assert np.isnan(whole[PAD + self.n:]).all(), f"{what}: written past its end"
        assert np.isfinite(whole[PAD:PAD + self.n]).all(), f"{what}: not every element written / finite"

    def untouched(self):
        """True if the whole buffer, output included, is still NaN (a refused call wrote nothing)."""
        return bool(torch.isnan(self.buf).all())
